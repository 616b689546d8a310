"""GPU: the guided (bridge) variant of the particle-filter kernel (csrc/vsde_filter.hip, ``_hip.guided_particle_filter``) through the
public ``particle_filter(..., proposal="bridge")``.

Stage by stage against float64 on the kernel's own previous stage, as tests/test_particle_filter_gpu.py does and for its reason.

* propagation and log-ratio: particles and ``log_weights`` at observation k against the float64 reference segment
  (tests/guided_filter_reference.py) started from the kernel's particles at k - 1 gathered through the kernel's ancestors.
  Particles: 2e-4 of the largest magnitude.  ``log_weights``: the ratio cancels large terms when the observation variance is small,
  so its bound is measured, per segment: E32 = the error of the SAME reference run in fp32 against float64 on the same starts; the
  kernel gets 4 E32 + 1e-5 max(1, largest finite |lw|) (the 4 allows for fused multiply-adds and another summation order);
* increments, ESS, mean, std from the kernel's own log_weights and particles in float64: 1e-5 / 1e-4 as for the bootstrap kernel;
* ancestors against float64 systematic resampling of those weights: at most 1e-3 differ, each by exactly 1, never decreasing in
  j, the float64 ESS above N / 20 at every observation -- with the Lotka-Volterra case at its own observation variance 1.0;
* the n = 1 identity, unbiasedness against the Kalman likelihood, kernel route against torch route, routing, and the bootstrap
  call through the public function against ``_hip.particle_filter`` called directly."""
import math

import numpy as np
import pytest
import torch

import guided_filter_reference as gref
import particle_filter_reference as ref
from philox_reference import forecast_noise

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
# observed dims O: ou 1, lv 2, lv_prey 1, sir 2, chain4 2, autoreg 2 take the kernels built for O <= 2; chain4_full (O = 4, H absent)
# and lindiag3 (O = 4 through a dense [4, 3] H; the linear-diagonal kind) take those built for O <= 4
CASES = ["ou", "lv", "lv_prey", "sir", "chain4", "autoreg", "chain4_full", "lindiag3"]
KIND = {"ou": "ornstein_uhlenbeck", "lv": "lotka_volterra", "lv_prey": "lotka_volterra", "sir": "reaction_network",
        "chain4": "reaction_network", "autoreg": "reaction_network", "chain4_full": "reaction_network", "lindiag3": "linear_diagonal"}
STATE_DIM = {"ou": 1, "chain4": 4, "chain4_full": 4, "lindiag3": 3}


def _key(k0, k1, dev=DEV):
    return torch.from_numpy(np.array([k0, k1], dtype=np.uint32).view(np.int32)).to(dev)


def _max_n(name):
    from viforsdes_amd import _hip
    return _hip.particle_filter_max_particles(KIND[name], STATE_DIM.get(name, 2), proposal="bridge")


def _sizes(name):
    return [64, _max_n(name)]


def _counted(fn):
    """(result of fn(), number of guided kernel calls, number of bootstrap kernel calls it made)."""
    from viforsdes_amd import _hip
    calls = {"guided": 0, "bootstrap": 0}
    real_g, real_b = _hip.guided_particle_filter, _hip.particle_filter
    _hip.guided_particle_filter = lambda *a, **k: (calls.__setitem__("guided", calls["guided"] + 1), real_g(*a, **k))[1]
    _hip.particle_filter = lambda *a, **k: (calls.__setitem__("bootstrap", calls["bootstrap"] + 1), real_b(*a, **k))[1]
    try:
        out = fn()
    finally:
        _hip.guided_particle_filter, _hip.particle_filter = real_g, real_b
    return out, calls["guided"], calls["bootstrap"]


_RUNS = {}


def _cached(name, N, rows=None, interior=False):
    """One kernel-route run of the case (M = 64), shared by the stage tests and left unchanged."""
    tag = (name, N, None if rows is None else tuple(rows), interior)
    if tag not in _RUNS:
        from viforsdes_amd import particle_filter
        sde, obs, like, th, x0, dt, pos = gref.case(name, 64, rows, interior)
        key = (0x9E3779B9 ^ N, 0x7F4A7C15 + len(name))
        res, guided, bootstrap = _counted(lambda: particle_filter(
            sde, obs.to(DEV), like, th.to(DEV), dt, n_particles=N, initial_state=x0.to(DEV), positive_dims=pos, return_particles=True,
            key=_key(*key), proposal="bridge"))
        assert (guided, bootstrap) == (1, 0)                      # the public function took the guided kernel, exactly once
        _RUNS[tag] = (sde, obs, like, th, x0, dt, pos, res, key)
    return _RUNS[tag]


def _params():
    return [pytest.param(name, big, id=f"{name}-{'max' if big else '64'}") for name in CASES for big in (False, True)]


def _n(name, big):
    return _sizes(name)[1 if big else 0]


def _gauss32(y, x, variance, H):
    x = x.astype(np.float32)
    pred = x if H is None else x @ H.astype(np.float32).T
    r = y.astype(np.float32) - pred
    lw = (np.float32(-0.5) * r * r / np.float32(variance) - np.float32(0.5 * math.log(2.0 * math.pi * variance))).sum(axis=-1)
    return lw.astype(np.float32)


def _segment_references(sde, like, th, dt, pos, start, z, y, N):
    """(x64, lw64, lw32): the reference segment from ``start`` in float64, and its log-weights when run in fp32."""
    H = None if like.obs_matrix is None else like.obs_matrix.double().numpy()
    theta = np.repeat(th.double().numpy(), N, axis=0)
    x64, lr64 = gref.guided_segment(gref.sde_coefficients(sde), start, theta, z, y, H, like.variance, dt, pos)
    lw64 = lr64 + ref.gaussian_log_weights(y, x64, like.variance, H)
    x32, lr32 = gref.guided_segment(gref.sde_coefficients(sde, np.float32), start, theta, z, y, H, like.variance, dt, pos, np.float32)
    with np.errstate(all="ignore"):
        lw32 = (lr32 + _gauss32(y, x32, like.variance, H)).astype(np.float64)
    return x64, lw64, np.where(np.isnan(lw32), -np.inf, lw32)


def _lw_errors(got, lw64, lw32):
    """(kernel error, fp32 reference error, bound) over the entries finite in float64."""
    ok = np.isfinite(lw64)
    assert ok.any() and np.isfinite(got[ok]).all()
    e_k, e_32 = float(np.abs(got[ok] - lw64[ok]).max()), float(np.abs(lw32[ok] - lw64[ok]).max())
    return e_k, e_32, 4.0 * e_32 + 1e-5 * max(1.0, float(np.abs(lw64[ok]).max()))


# ------------------------------------------------------------------------------------------------- propagation and log-ratio
@pytest.mark.parametrize("name,big", _params())
def test_propagation_and_log_ratio_match_the_float64_segment(name, big):
    N = _n(name, big)
    sde, obs, like, th, x0, dt, pos, res, key = _cached(name, N)
    M, K, S, rows = th.shape[0], obs.values.shape[0], sde.state_dim, gref.rows_of(name)
    parts, anc = res.particles.double().cpu().numpy(), res.ancestors.long().cpu().numpy()
    lw = res.log_weights.double().cpu().numpy()
    assert np.isfinite(parts).all() and lw.shape == (M, K, N)
    assert np.array_equal(parts[:, 0], np.broadcast_to(x0.double().numpy()[:, None, :], (M, N, S)))
    H = None if like.obs_matrix is None else like.obs_matrix.double().numpy()
    noise = forecast_noise(M * N, rows[-1], S, key)
    worst_x = 0.0
    for k in range(K):
        y = obs.values[k].double().numpy()
        if k == 0 or rows[k] == rows[k - 1]:          # no step since the last observation: the plain Gaussian weight
            if k > 0:
                start = np.take_along_axis(parts[:, k - 1], anc[:, k - 1, :, None], axis=1)
                assert np.array_equal(parts[:, k], start)
            want = ref.gaussian_log_weights(y, parts[:, k], like.variance, H)
            ok = np.isfinite(want)
            e = float(np.abs(lw[:, k][ok] - want[ok]).max())
            print(f"{name} N={N} k={k} (no step): log-weight error {e:.2e}")
            assert e <= 1e-5 * max(1.0, float(np.abs(want[ok]).max()))
            continue
        start = np.take_along_axis(parts[:, k - 1], anc[:, k - 1, :, None], axis=1).reshape(M * N, S)
        x64, lw64, lw32 = _segment_references(sde, like, th, dt, pos, start, noise[:, rows[k - 1]:rows[k]], y, N)
        e_x = float(np.abs(parts[:, k].reshape(M * N, S) - x64).max() / np.abs(x64).max())
        e_k, e_32, bound = _lw_errors(lw[:, k].reshape(M * N), lw64, lw32)
        print(f"{name} N={N} k={k} (n = {rows[k] - rows[k - 1]}): particles {e_x:.2e} of the largest magnitude; log-weights: kernel "
              f"{e_k:.2e}, fp32 reference {e_32:.2e}, bound {bound:.2e}")
        worst_x = max(worst_x, e_x)
        assert e_k <= bound
    assert worst_x < 2e-4
    if pos:
        assert (parts[..., list(pos)] >= gref.STATE_FLOOR).all()
    if pos:
        assert (parts[:, 1:][..., list(pos)] == gref.STATE_FLOOR).any()    # the clamp was exercised


# ----------------------------------------------------------------------------------------------------- weights and summaries
@pytest.mark.parametrize("name,big", _params())
def test_summaries_match_float64_on_the_kernels_weights_and_particles(name, big):
    N = _n(name, big)
    sde, obs, like, th, x0, dt, pos, res, key = _cached(name, N)
    M, K = th.shape[0], obs.values.shape[0]
    parts, lws = res.particles.double().cpu().numpy(), res.log_weights.double().cpu().numpy()
    got = [t.double().cpu().numpy() for t in (res.increments, res.effective_sample_size, res.filtered_mean, res.filtered_std)]
    e_inc = e_ess = e_mean = e_std = 0.0
    for m in range(M):
        for k in range(K):
            lw = lws[m, k]
            inc, ess, mean, std, w = ref.observation_stage(lw, parts[m, k])
            size = (w[:, None] * np.abs(parts[m, k])).sum(axis=0) / w.sum()
            e_inc = max(e_inc, abs(got[0][m, k] - inc) / max(1.0, np.abs(lw[np.isfinite(lw)]).max()))
            e_ess = max(e_ess, abs(got[1][m, k] - ess) / ess)
            e_mean = max(e_mean, float((np.abs(got[2][m, k] - mean) / np.maximum(size, 1e-30)).max()))
            e_std = max(e_std, float((np.abs(got[3][m, k] - std) / (std + 1e-2 * size + 1e-30)).max()))
    print(f"{name} N={N}: increments {e_inc:.2e} (of max(1, |lw|)), ESS {e_ess:.2e}, mean {e_mean:.2e}, std {e_std:.2e} (relative)")
    assert e_inc < 1e-5
    assert e_ess < 1e-4 and e_mean < 1e-4 and e_std < 1e-4
    total = res.increments.double().sum(dim=1)
    assert torch.allclose(res.log_likelihood.double(), total, rtol=1e-6, atol=1e-5 * float(res.increments.abs().max()))


# ----------------------------------------------------------------------------------------------------------------- ancestors
@pytest.mark.parametrize("name,big", _params())
def test_ancestors_match_float64_systematic_resampling(name, big):
    N = _n(name, big)
    sde, obs, like, th, x0, dt, pos, res, key = _cached(name, N)
    M, K = th.shape[0], obs.values.shape[0]
    lws = res.log_weights.double().cpu().numpy()
    anc = res.ancestors.cpu().numpy().astype(np.int64)
    assert anc.min() >= 0 and anc.max() < N
    assert (np.diff(anc, axis=-1) >= 0).all()
    u = ref.resampling_uniforms(M, K, key)
    differ, low = 0, float("inf")
    for m in range(M):
        for k in range(K):
            w = np.exp(lws[m, k] - lws[m, k].max())
            low = min(low, w.sum() ** 2 / (w * w).sum())
            d = np.abs(anc[m, k] - ref.systematic_ancestors(w, u[m, k]))
            assert d.max() <= 1, (m, k, int(d.max()))
            differ += int((d != 0).sum())
    print(f"{name} N={N}: {differ} of {anc.size} ancestors differ from float64 ({differ / anc.size:.1e}); smallest float64 ESS {low:.1f}")
    assert low > N / 20
    assert differ <= 1e-3 * anc.size


# ---------------------------------------------------------------------------------------------------------- the n = 1 identity
@pytest.mark.parametrize("name", ["ou", "lv", "lv_prey", "chain4", "chain4_full", "lindiag3"])
def test_one_step_segments_give_the_fully_adapted_weight_on_the_device(name):
    N, rows = 64, [0, 1, 2, 3, 4]
    sde, obs, like, th, x0, dt, pos, res, key = _cached(name, N, rows, interior=True)              # no clamp binds
    M, S = th.shape[0], sde.state_dim
    parts, anc = res.particles.double().cpu().numpy(), res.ancestors.long().cpu().numpy()
    lw = res.log_weights.double().cpu().numpy()
    if pos:
        assert (parts[..., list(pos)] > gref.STATE_FLOOR).all()
    Hm = np.eye(S) if like.obs_matrix is None else like.obs_matrix.double().numpy()
    theta = np.repeat(th.double().numpy(), N, axis=0)
    noise = forecast_noise(M * N, rows[-1], S, key)
    coef = gref.sde_coefficients(sde)
    for k in range(1, len(rows)):
        y = obs.values[k].double().numpy()
        prev = np.take_along_axis(parts[:, k - 1], anc[:, k - 1, :, None], axis=1).reshape(M * N, S)
        f, L = coef(prev, theta)
        HL = np.einsum("ok,bki->boi", Hm, L)
        cov = dt * np.einsum("boi,bqi->boq", HL, HL) + like.variance * np.eye(Hm.shape[0])
        want = gref.gaussian_log_density(y, (prev + f * dt) @ Hm.T, cov)
        _, lw64, lw32 = _segment_references(sde, like, th, dt, pos, prev, noise[:, rows[k - 1]:rows[k]], y, N)
        assert np.abs(lw64 - want).max() <= 1e-9 * max(1.0, np.abs(want).max())          # the identity itself, in float64
        e_k, e_32, bound = _lw_errors(lw[:, k].reshape(-1), want, lw32)
        print(f"{name} k={k}: n = 1 identity: kernel {e_k:.2e}, fp32 reference {e_32:.2e}, bound {bound:.2e}")
        assert e_k <= bound


# ---------------------------------------------------------------------------------------------------------------- statistics
def test_bridge_likelihood_is_unbiased_on_the_device():
    from viforsdes_amd import GaussianObservationLikelihood, particle_filter
    from viforsdes_amd.examples.sdes import ou_problem
    M, N = 4096, 64
    sde, obs, _, _, _, dt, _, _ = ou_problem()
    rows = np.round(obs.times.numpy() / dt).astype(int)
    for theta, variance in [((0.8, 1.0, 0.5), 0.01), ((1.5, 0.5, 1.0), 0.1), ((0.3, 2.0, 0.3), 0.01)]:
        like = GaussianObservationLikelihood(variance=variance)
        exact = gref.ou_kalman(theta, dt, variance, obs.values[0].numpy(), rows, obs.values.numpy())
        res, guided, _ = _counted(lambda: particle_filter(sde, obs.to(DEV), like, torch.tensor([theta], device=DEV).expand(M, 3), dt,
                                                          n_particles=N, key=_key(11, int(theta[0] * 100)), proposal="bridge"))
        assert guided == 1
        ll = res.log_likelihood.double().cpu().numpy()
        r = np.exp(ll - exact)
        z = abs(r.mean() - 1.0) / (r.std(ddof=1) / math.sqrt(M))
        print(f"OU theta {theta}, variance {variance}: exact {exact:.4f}, std of log p^ {ll.std(ddof=1):.4f}, z {z:.2f}")
        assert z < 5.0


def test_linear_diagonal_bridge_likelihood_is_unbiased_on_the_device():
    """The linear-diagonal kind's guided kernels against the Kalman likelihood: S = 2 with a dense [2, 2] H (built for O <= 2) and
    S = 4 with a dense [3, 4] H (built for O <= 4, the 512-thread ones)."""
    from viforsdes_amd import GaussianObservationLikelihood, Observations, particle_filter
    from viforsdes_amd.examples.sdes import LinearDiagonalSDE
    M, N, dt, rows = 4096, 64, 0.05, [0, 1, 7, 20]
    g = torch.Generator().manual_seed(17)
    for S, O in ((2, 2), (4, 3)):
        H = torch.randn(O, S, generator=g)
        theta = tuple((0.4 + 0.3 * torch.arange(S)).tolist()) + tuple((-1.2 + 0.4 * torch.arange(S)).tolist())
        x0 = 0.5 * torch.randn(S, generator=g)
        obs = Observations(times=torch.tensor(rows) * dt, values=0.3 * torch.randn(len(rows), O, generator=g))
        like = GaussianObservationLikelihood(variance=0.01, obs_matrix=H)
        exact = ref.linear_diagonal_kalman(theta, dt, 0.01, H.numpy(), x0.numpy(), rows, obs.values.numpy())
        res, guided, _ = _counted(lambda: particle_filter(LinearDiagonalSDE(S), obs.to(DEV), like,
                                                          torch.tensor([theta], device=DEV).expand(M, 2 * S), dt, n_particles=N,
                                                          initial_state=x0.to(DEV), key=_key(41, S), proposal="bridge"))
        assert guided == 1
        ll = res.log_likelihood.double().cpu().numpy()
        r = np.exp(ll - exact)
        z = abs(r.mean() - 1.0) / (r.std(ddof=1) / math.sqrt(M))
        print(f"linear-diagonal S={S}, O={O}: exact {exact:.4f}, std of log p^ {ll.std(ddof=1):.4f}, z {z:.2f}")
        assert z < 5.0


def test_kernel_route_and_torch_route_agree_on_the_sir_network(monkeypatch):
    from viforsdes_amd import particle_filter
    from viforsdes_amd.inference import particle_filter as pf
    M, N = 512, 128
    sde, obs, like, th, x0, dt, pos = gref.case("sir", M)
    th, x0 = th[1:2].expand(M, 2).contiguous(), x0[1:2].expand(M, 2).contiguous()
    run = lambda k: particle_filter(sde, obs.to(DEV), like, th.to(DEV), dt, n_particles=N, initial_state=x0.to(DEV),
                                    positive_dims=pos, key=_key(*k), proposal="bridge").log_likelihood.double().cpu().numpy()
    a, guided, _ = _counted(lambda: run((31, 32)))
    monkeypatch.setattr(pf, "HIP_FILTER", False)
    b, guided_off, _ = _counted(lambda: run((33, 34)))
    assert (guided, guided_off) == (1, 0)
    z = abs(a.mean() - b.mean()) / math.sqrt(a.var(ddof=1) / M + b.var(ddof=1) / M)
    print(f"SIR, bridge: mean log p^ kernel {a.mean():.4f}, torch {b.mean():.4f}, two-sample z {z:.2f}")
    assert z < 5.0


# ------------------------------------------------------------------------------------------------------------------- routing
def test_five_dims_and_too_many_particles_take_the_torch_route():
    from viforsdes_amd import GaussianObservationLikelihood, Observations, particle_filter
    from viforsdes_amd.examples.sdes import LinearDiagonalSDE
    M, N, dt = 512, 64, 0.05
    g = torch.Generator().manual_seed(3)
    for S, O in ((5, 2), (2, 5)):
        sde = LinearDiagonalSDE(S)
        H = torch.randn(O, S, generator=g) / 2.0
        theta = tuple((0.3 + 0.1 * torch.arange(S)).tolist()) + tuple((-1.0 + 0.2 * torch.arange(S)).tolist())
        x0 = 0.3 * torch.randn(S, generator=g)
        obs = Observations(times=torch.tensor([0.0, 0.05, 0.25]), values=0.3 * torch.randn(3, O, generator=g))
        like = GaussianObservationLikelihood(variance=0.04, obs_matrix=H)
        exact = ref.linear_diagonal_kalman(theta, dt, 0.04, H.numpy(), x0.numpy(), [0, 1, 5], obs.values.numpy())
        res, guided, bootstrap = _counted(lambda: particle_filter(sde, obs.to(DEV), like, torch.tensor([theta], device=DEV).expand(M, 2 * S),
                                                                  dt, n_particles=N, initial_state=x0.to(DEV), key=_key(5, S),
                                                                  proposal="bridge"))
        assert (guided, bootstrap) == (0, 0)
        r = np.exp(res.log_likelihood.double().cpu().numpy() - exact)
        z = abs(r.mean() - 1.0) / (r.std(ddof=1) / math.sqrt(M))
        print(f"linear-diagonal S={S}, O={O} (torch route): exact {exact:.4f}, z {z:.2f}")
        assert z < 5.0
    # the guided route's own limit: 512 particles at S = 4, where the bootstrap kernel takes 1024
    from viforsdes_amd import _hip
    assert _hip.particle_filter_max_particles("reaction_network", 4, proposal="bridge") == 512
    assert _hip.particle_filter_max_particles("reaction_network", 4) == 1024
    sde, obs, like, th, x0, dt, pos = gref.case("chain4", 2)
    run = lambda proposal: _counted(lambda: particle_filter(sde, obs.to(DEV), like, th.to(DEV), dt, n_particles=1024,
                                                            initial_state=x0.to(DEV), positive_dims=pos, key=_key(1, 2),
                                                            proposal=proposal))
    res, guided, bootstrap = run("bridge")
    assert (guided, bootstrap) == (0, 0) and bool(torch.isfinite(res.log_likelihood).all())
    assert run("bootstrap")[1:] == (0, 1)


def test_guided_entry_point_refuses_what_it_cannot_take():
    from viforsdes_amd import _hip
    key, rows = _key(1, 2), torch.tensor([0, 2], dtype=torch.int32, device=DEV)
    z = lambda *s: torch.zeros(*s, device=DEV)
    out = _hip.guided_particle_filter("linear_diagonal", z(4, 4), z(4, 8), rows, z(2, 4), None, 0.1, key, 0.05, 64, ())
    assert len(out) == 8 and out[0].shape == (4,) and out[7] is None and bool(torch.isfinite(out[0]).all())
    with pytest.raises(ValueError, match="state_dim"):
        _hip.guided_particle_filter("linear_diagonal", z(4, 5), z(4, 10), rows, z(2, 5), None, 0.1, key, 0.05, 64, ())
    with pytest.raises(ValueError, match="obs_dim"):
        _hip.guided_particle_filter("linear_diagonal", z(4, 2), z(4, 4), rows, z(2, 5), z(5, 2), 0.1, key, 0.05, 64, ())
    for N in (0, 32, 100, 2048):
        with pytest.raises(ValueError, match="particles"):
            _hip.guided_particle_filter("linear_diagonal", z(4, 2), z(4, 4), rows, z(2, 2), None, 0.1, key, 0.05, N, ())
    assert _hip.guided_particle_filter("linear_diagonal", z(4, 4), z(4, 8), rows, z(2, 4), None, 0.1, key, 0.05, 512, ())[0].shape == (4,)
    with pytest.raises(ValueError, match="particles"):                      # S = 4: 512 at most
        _hip.guided_particle_filter("linear_diagonal", z(4, 4), z(4, 8), rows, z(2, 4), None, 0.1, key, 0.05, 1024, ())
    assert _hip.guided_particle_filter("linear_diagonal", z(4, 3), z(4, 6), rows, z(2, 3), None, 0.1, key, 0.05, 1024, ())[0].shape == (4,)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------ the parent's behaviour
def test_bootstrap_through_the_public_function_is_the_direct_kernel_call():
    from viforsdes_amd import _hip, particle_filter
    sde, obs, like, th, x0, dt, pos = gref.case("lv", 16)
    th, x0, obs = th.to(DEV), x0.to(DEV), obs.to(DEV)
    key = _key(77, 78)
    rows = torch.round(obs.times / dt).to(torch.int32)
    for kw in ({}, {"proposal": "bootstrap"}):
        res, guided, bootstrap = _counted(lambda: particle_filter(sde, obs, like, th, dt, n_particles=128, initial_state=x0,
                                                                  positive_dims=pos, return_particles=True, key=key, **kw))
        assert (guided, bootstrap) == (0, 1)
        want = _hip.particle_filter("lotka_volterra", x0, th, rows, obs.values, None, like.variance, key, dt, 128, pos,
                                    return_particles=True)
        got = (res.log_likelihood, res.increments, res.effective_sample_size, res.filtered_mean, res.filtered_std, res.particles,
               res.ancestors)
        for a, b in zip(got, want):
            assert torch.equal(a, b)
        lw = like.log_prob(obs.values[None, :, None, :].expand(16, -1, 128, -1).reshape(-1, 2), res.particles.reshape(-1, 2))
        assert torch.equal(res.log_weights, lw.reshape(16, -1, 128))
