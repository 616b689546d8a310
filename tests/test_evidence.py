"""CPU: the finalisation of the importance-sampling accumulator (``EvidenceEstimate.from_state``) against float64 numpy on
synthetic log-weights, the argument errors of the two log-weight entry points (no GPU is touched: every call below fails its
checks before a launch), and the refusal of a CPU posterior."""
import ctypes

import numpy as np
import pytest
import torch


def _state(log_w, chunk=7):
    """The accumulator state ``[M, S1, S2, sum lw, n, n_nonfinite]`` as csrc/vsde_elbo.hip builds it: chunk max, chunk sums,
    merged into the running state by rescaling to the new max (float64)."""
    st = np.array([-np.inf, 0.0, 0.0, 0.0, 0.0, 0.0])
    lw = np.asarray(log_w, dtype=np.float32).astype(np.float64)
    for c in range(0, lw.size, chunk):
        v = lw[c:c + chunk]
        ok = ~np.isnan(v) & (v != np.inf)
        mc = v[ok].max() if ok.any() else -np.inf
        e = np.exp(v[ok] - mc) if mc > -np.inf else np.zeros(0)
        mn = max(st[0], mc)
        a, b = (np.exp(st[0] - mn), np.exp(mc - mn)) if mn > -np.inf else (0.0, 0.0)
        st = np.array([mn, st[1] * a + e.sum() * b, st[2] * a * a + (e * e).sum() * b * b, st[3] + v[ok].sum(), st[4] + v.size,
                       st[5] + (~ok).sum()])
    return st


def _direct(log_w):
    """log Z, ESS, standard error and mean log w straight from the definitions (float64)."""
    lw = np.asarray(log_w, dtype=np.float32).astype(np.float64)
    n, m = lw.size, lw.max()
    w = np.exp(lw - m)
    ess = w.sum() ** 2 / (w * w).sum()
    return m + np.log(w.sum()) - np.log(n), ess, np.sqrt(max(1.0 / ess - 1.0 / n, 0.0)), lw.mean()


def _check(log_w, **kw):
    from viforsdes_amd import EvidenceEstimate
    est = EvidenceEstimate.from_state(_state(log_w, **kw))
    le, ess, se, elbo = _direct(log_w)
    assert est.n_samples == len(log_w) and est.n_nonfinite == 0
    assert abs(est.log_evidence - le) <= 1e-12 * max(1.0, abs(le))
    assert abs(est.effective_sample_size - ess) <= 1e-12 * ess
    assert abs(est.standard_error - se) <= 1e-12 * max(se, 1e-300) + 1e-15
    assert abs(est.evidence_lower_bound - elbo) <= 1e-12 * max(1.0, abs(elbo))
    assert est.log_evidence >= est.evidence_lower_bound - 1e-12 * max(1.0, abs(elbo))
    assert 0.0 < est.effective_sample_size <= len(log_w) * (1 + 1e-12)
    return est


def test_finalisation_matches_float64_definitions():
    rng = np.random.default_rng(0)
    _check(rng.normal(-50.0, 3.0, size=1000))
    _check(rng.normal(-50.0, 3.0, size=1000), chunk=1000)


def test_dynamic_range_of_1e4_in_log_space():
    rng = np.random.default_rng(1)
    lw = rng.uniform(-1.0e4, 0.0, size=4096)
    lw[[5, 77]] = [-3.0, -4.5]                 # the weight is carried by a few draws far above the bulk
    est = _check(lw, chunk=256)
    assert 1.0 <= est.effective_sample_size < 3.0


def test_standard_error_is_delta_method_on_the_log_scale():
    from viforsdes_amd import EvidenceEstimate
    lw = np.log(np.array([1.0, 1.0, 2.0, 4.0]))                  # weights 1, 1, 2, 4 (to float32 rounding of their logs)
    est = EvidenceEstimate.from_state(_state(lw, chunk=3))
    ess = 8.0 ** 2 / 22.0
    assert est.effective_sample_size == pytest.approx(ess, rel=1e-6)
    assert est.standard_error == pytest.approx(np.sqrt(1.0 / ess - 1.0 / 4.0), rel=1e-6)
    flat = EvidenceEstimate.from_state(_state(np.full(10, -2.0)))
    assert flat.effective_sample_size == pytest.approx(10.0) and flat.standard_error < 1e-6
    assert flat.log_evidence == pytest.approx(-2.0, abs=1e-12)


def test_single_sample():
    from viforsdes_amd import EvidenceEstimate
    est = EvidenceEstimate.from_state(_state([-3.25]))
    assert (est.log_evidence, est.effective_sample_size, est.standard_error, est.evidence_lower_bound) == (-3.25, 1.0, 0.0, -3.25)
    assert est.n_samples == 1


def test_minus_infinity_weights_are_zero_weights():
    from viforsdes_amd import EvidenceEstimate
    lw = np.array([-1.0, -np.inf, -2.0, -np.inf, -0.5, -1.5, -3.0, -np.inf, -0.25])
    est = EvidenceEstimate.from_state(_state(lw, chunk=4))
    fin = lw[np.isfinite(lw)]
    m = fin.max()
    assert est.n_samples == 9 and est.n_nonfinite == 0
    assert est.log_evidence == pytest.approx(m + np.log(np.exp(fin - m).sum()) - np.log(9), abs=1e-12)
    w = np.exp(fin - m)
    assert est.effective_sample_size == pytest.approx(w.sum() ** 2 / (w * w).sum(), rel=1e-12)
    assert est.evidence_lower_bound == -np.inf
    # a chunk of only -inf between finite chunks changes nothing but n
    est2 = EvidenceEstimate.from_state(_state(np.concatenate([fin[:3], [-np.inf] * 5, fin[3:]]), chunk=3))
    assert est2.log_evidence == pytest.approx(m + np.log(w.sum()) - np.log(11), abs=1e-12)


def test_all_minus_infinity():
    from viforsdes_amd import EvidenceEstimate
    est = EvidenceEstimate.from_state(_state(np.full(20, -np.inf), chunk=6))
    assert est.log_evidence == -np.inf and est.effective_sample_size == 0.0 and est.n_samples == 20 and est.n_nonfinite == 0


def test_nan_weights_make_the_estimate_nan_and_are_counted():
    from viforsdes_amd import EvidenceEstimate
    lw = np.array([-1.0, np.nan, -2.0, -0.5, np.nan, -np.inf, -1.0])
    est = EvidenceEstimate.from_state(_state(lw, chunk=3))
    assert est.n_nonfinite == 2 and est.n_samples == 7
    assert np.isnan(est.log_evidence) and np.isnan(est.effective_sample_size) and np.isnan(est.standard_error)


def test_evidence_estimate_is_exported_and_frozen():
    import dataclasses

    import viforsdes_amd
    from viforsdes_amd.posterior.variational_posterior import EvidenceEstimate
    assert viforsdes_amd.EvidenceEstimate is EvidenceEstimate and "EvidenceEstimate" in viforsdes_amd.__all__
    est = EvidenceEstimate.from_state([0.0, 1.0, 1.0, 0.0, 1.0, 0.0])
    with pytest.raises(dataclasses.FrozenInstanceError):
        est.log_evidence = 1.0


# ------------------------------------------------------------------------------------------------------------ C ABI
_FAKE = ctypes.c_void_p(0x1000)   # never dereferenced: each call below is rejected by its argument checks


def _log_weights(lib, kind=0, S=2, O=2, P=3, z=_FAKE, n_mask=None):
    mask = (ctypes.c_uint8 * 32)()
    return lib.vsde_log_weights(
        ctypes.c_int(kind), ctypes.c_int(8), ctypes.c_int(10), ctypes.c_int(S), ctypes.c_int(3), ctypes.c_int(O), ctypes.c_int(P),
        z, _FAKE, _FAKE, _FAKE, _FAKE, _FAKE, _FAKE, _FAKE, None, ctypes.c_double(0.1), ctypes.c_int(0), ctypes.c_double(0.0),
        ctypes.c_double(1.0), _FAKE, _FAKE, mask, mask, ctypes.c_double(0.05), _FAKE, None)


def test_log_weight_entry_points_reject_bad_arguments_without_gpu():
    from viforsdes_amd import _hip
    lib = _hip.load()
    assert _log_weights(lib, S=17, O=17) == -5                    # VSDE_E_STATE
    assert b"state_dim 17" in lib.vsde_last_error()
    assert _log_weights(lib, S=2, O=2, P=17) == -1                # P beyond the kernel's 16
    assert b"<= 16" in lib.vsde_last_error()
    assert _log_weights(lib, z=ctypes.c_void_p(None)) == -1
    assert b"NULL" in lib.vsde_last_error()
    assert _log_weights(lib, kind=2, S=1, O=1) == -1              # Lotka-Volterra is two-dimensional
    assert b"Lotka-Volterra" in lib.vsde_last_error()
    assert _log_weights(lib, kind=7) == -1
    for n in (0, -3):
        assert lib.vsde_log_weight_accumulate(ctypes.c_int(n), _FAKE, _FAKE, None) == -1
        assert b"positive" in lib.vsde_last_error()
    assert lib.vsde_log_weight_accumulate(ctypes.c_int(4), ctypes.c_void_p(None), _FAKE, None) == -1
    assert lib.vsde_log_weight_accumulate(ctypes.c_int(4), _FAKE, ctypes.c_void_p(None), None) == -1
    assert b"NULL" in lib.vsde_last_error()


def test_log_evidence_on_a_cpu_posterior_raises():
    from viforsdes_amd import EncoderConfig, GaussianObservationLikelihood, HeadConfig, _hip
    from viforsdes_amd.examples.sdes import ou_problem
    from viforsdes_amd.inference.exponential_moving_average import ExponentialMovingAverage
    from viforsdes_amd.inference.state_space import StateSpace
    from viforsdes_amd.models.variational_sde_posterior import VariationalSDEPosterior
    from viforsdes_amd.posterior.variational_posterior import VariationalPosterior
    sde, obs, like, prior, horizon, dt, _, theta_pos = ou_problem()
    model = VariationalSDEPosterior(1, 1, 3, EncoderConfig(hidden_dim=32, cond_dim=16, num_heads=4, depth=1),
                                    HeadConfig(hidden_dim=16, num_layers=1), theta_pos)
    vp = VariationalPosterior(model=model, exponential_moving_average=ExponentialMovingAverage(model), prior=prior,
                              observations=obs, time_horizon=horizon, time_step=dt, state_space=StateSpace(1, []),
                              evidence_lower_bound_history=[], device=torch.device("cpu"))
    before = {k: v.clone() for k, v in model.state_dict().items()}
    with pytest.raises(_hip.HipLibraryError):
        vp.log_evidence(sde, like, n_samples=8, chunk_size=4)
    for bad in ({"n_samples": 0}, {"chunk_size": 0}):
        with pytest.raises(ValueError):
            vp.log_evidence(sde, GaussianObservationLikelihood(variance=0.1), **bad)
    for k, v in model.state_dict().items():
        assert torch.equal(v, before[k]), k
