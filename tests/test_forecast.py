"""CPU: the numpy Philox4x32-10 reference against the published Random123 known-answer vectors, the torch route of
``forecast_states`` against ``euler_maruyama`` on the same noise, ``PosteriorPredictive`` statistics against torch, the argument
errors of ``VariationalPosterior.predict`` on a CPU posterior and of the ``vsde_forecast`` entry point (no GPU is touched: each
call below fails its checks before a launch).

Largest errors observed: none -- every comparison here is exact (bitwise), including the quantiles."""
import ctypes
import dataclasses

import numpy as np
import pytest
import torch

from philox_reference import box_muller, forecast_noise, philox4x32_10

KNOWN_ANSWERS = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


@pytest.mark.parametrize("ctr,key,expected", KNOWN_ANSWERS)
def test_numpy_philox_reproduces_random123_known_answers(ctr, key, expected):
    out = philox4x32_10(*ctr, *key)
    assert tuple(int(v) for v in out) == expected


def test_box_muller_ends_and_stream_layout():
    za, zb = box_muller(np.array([0, 0xFFFFFFFF], np.uint32), np.array([0, 0], np.uint32))
    assert za[0] == pytest.approx(np.sqrt(50 * np.log(2.0)), rel=1e-12)       # the tail cut: u_a = 2^-25
    assert za[1] == 0.0                                                        # u_a rounds to 1 in fp32
    # normal (b, t, i) is word t % 4 of the counter (t // 4, i, b, 0)
    z = forecast_noise(3, 7, 2, (5, 9))
    w = philox4x32_10(1, 1, 2, 0, 5, 9)
    z2, z3 = box_muller(w[2], w[3])
    assert z[2, 6, 1] == z2 and z[2, 5, 1] == box_muller(w[0], w[1])[1]


def _problem(S=3):
    from viforsdes_amd import make_sde

    def drift(x, th):
        return th[:, :S] * (1.0 - x)

    def diffusion(x, th):
        return torch.diag_embed(torch.nn.functional.softplus(th[:, S:]) + 0.1 * x.abs())
    return make_sde(drift, diffusion, S, 2 * S)


@pytest.mark.parametrize("use_builtin", [False, True])
def test_torch_route_is_euler_maruyama_gathered(use_builtin):
    from viforsdes_amd.core.euler_maruyama import euler_maruyama
    from viforsdes_amd.core.forecast import forecast_states
    from viforsdes_amd.examples.sdes import LotkaVolterra
    g = torch.Generator().manual_seed(3)
    if use_builtin:   # a built-in SDE on CPU tensors: small populations, so rows hit the 1e-6 clamp
        sde, pos, B = LotkaVolterra(), [0, 1], 64
        x = torch.rand(B, 2, generator=g) * 0.5
        th = torch.rand(B, 3, generator=g) * 0.5 + 0.2
    else:
        sde, pos, B = _problem(), [1], 33
        x = torch.randn(B, 3, generator=g)
        x[:, 1] = x[:, 1].abs() * 0.05
        th = torch.randn(B, 6, generator=g)
    steps, dt = [1, 4, 4, 9, 17], 0.1
    torch.manual_seed(21)
    got = forecast_states(sde, x, th, 17, steps, dt, pos)
    torch.manual_seed(21)
    ref = euler_maruyama(sde, x, th, 17 * dt, dt, pos)[:, steps]
    assert got.shape == (B, len(steps), sde.state_dim)
    assert torch.equal(got, ref)
    assert bool((got[..., pos] == 1e-6).any())                 # the clamp was exercised
    assert bool((got[..., pos] >= 1e-6).all())


def test_forecast_states_argument_errors():
    from viforsdes_amd.core.forecast import forecast_states
    sde, x, th = _problem(), torch.zeros(4, 3), torch.zeros(4, 6)
    for bad in ([], [0, 1], [2, 1], [1, 6]):
        with pytest.raises(ValueError):
            forecast_states(sde, x, th, 5, bad, 0.1)
    with pytest.raises(ValueError):
        forecast_states(sde, x, th, 0, [1], 0.1)
    with pytest.raises(ValueError):
        forecast_states(sde, x, th[:3], 5, [1], 0.1)


def _predictive(obs=True):
    from viforsdes_amd import PosteriorPredictive
    g = torch.Generator().manual_seed(5)
    n, K, S = 1001, 4, 3
    states = torch.randn(n, K, S, generator=g) * torch.arange(1, S + 1)
    return PosteriorPredictive(times=torch.linspace(0, 1, K), sde_parameters=torch.randn(n, 2, generator=g), states=states,
                               observations=states[..., :2] + torch.randn(n, K, 2, generator=g) if obs else None)


def test_predictive_statistics_match_torch():
    from viforsdes_amd.posterior.variational_posterior import QUANTILE_LEVELS
    pp = _predictive()
    levels = torch.tensor(QUANTILE_LEVELS)
    for flag, v in ((False, pp.states), (True, pp.observations)):
        q = pp.quantiles(observations=flag)
        ref = torch.quantile(v, levels, dim=0)
        for k, name in enumerate(("q05", "q25", "q50", "q75", "q95")):
            assert torch.equal(getattr(q, name), ref[k]), name
        assert torch.equal(pp.mean(flag), v.mean(0)) and torch.equal(pp.std(flag), v.std(0))
    with pytest.raises(dataclasses.FrozenInstanceError):
        pp.states = pp.states
    with pytest.raises(ValueError):
        _predictive(obs=False).quantiles(observations=True)


def test_predictive_quantiles_in_column_blocks(monkeypatch):
    from viforsdes_amd.posterior import variational_posterior as vpm
    pp = _predictive()
    whole = pp.quantiles()
    monkeypatch.setattr(vpm, "_QUANTILE_MAX_ELEMENTS", 2 * pp.states.shape[0] + 1)   # 2 columns per torch.quantile call
    blocks = pp.quantiles()
    assert all(torch.equal(getattr(whole, f), getattr(blocks, f)) for f in ("q05", "q25", "q50", "q75", "q95"))


def test_gaussian_likelihood_sample():
    from viforsdes_amd import GaussianObservationLikelihood
    H = torch.tensor([[1.0, 0.5], [0.0, 2.0]])
    like = GaussianObservationLikelihood(variance=0.09, obs_matrix=H)
    x = torch.randn(4, 5, 2)
    torch.manual_seed(1)
    y = like.sample(x)
    torch.manual_seed(1)
    assert torch.equal(y, x @ H.T + 0.3 * torch.randn(4, 5, 2))


class _NoSample:
    def log_prob(self, observations, state):
        return state.sum(-1)


def test_predict_on_a_cpu_posterior_raises():
    from viforsdes_amd import EncoderConfig, GaussianObservationLikelihood, HeadConfig, _hip
    from viforsdes_amd.examples.sdes import LotkaVolterra, ou_problem
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
    rng = torch.get_rng_state()
    with pytest.raises(_hip.HipLibraryError):
        vp.predict(sde, [1.0, 6.0], n_samples=8, chunk_size=4)
    for bad in ({"times": []}, {"times": [[1.0]]}, {"times": [2.0, 1.0]}, {"times": [-0.5, 1.0]}, {"times": [1.0, float("nan")]},
                {"n_samples": 0}, {"chunk_size": 0}, {"sde": LotkaVolterra()}):
        kw = {"sde": sde, "times": [1.0, 6.0], **bad}
        with pytest.raises(ValueError):
            vp.predict(kw.pop("sde"), kw.pop("times"), **kw)
    with pytest.raises(TypeError):
        vp.predict(sde, [6.0], observation_likelihood=_NoSample())
    with pytest.raises(_hip.HipLibraryError):   # a likelihood with sample() passes the checks
        vp.predict(sde, [6.0], observation_likelihood=GaussianObservationLikelihood(variance=0.1))
    assert torch.equal(torch.get_rng_state(), rng)             # nothing was drawn
    for k, v in model.state_dict().items():
        assert torch.equal(v, before[k]), k
    assert vp._captured == {} and vp._calls == {}


# ------------------------------------------------------------------------------------------------------------ C ABI
_FAKE = ctypes.c_void_p(0x1000)   # never dereferenced: each call below is rejected by its argument checks


def _forecast(lib, kind=1, B=8, T=10, S=1, P=3, K=2, x=_FAKE, th=_FAKE, steps=_FAKE, key=_FAKE, out=_FAKE, dt=0.1):
    mask = (ctypes.c_uint8 * 64)()
    return lib.vsde_forecast(ctypes.c_int(kind), ctypes.c_int(B), ctypes.c_int(T), ctypes.c_int(S), ctypes.c_int(P),
                             ctypes.c_int(K), x, th, steps, key, ctypes.c_double(dt), mask, out, None)


def test_forecast_entry_point_rejects_bad_arguments_without_gpu():
    from viforsdes_amd import _hip
    lib = _hip.load()
    lib.vsde_forecast.restype = ctypes.c_int

    def rejected(fragment, **kw):
        assert _forecast(lib, **kw) == -1, kw
        assert fragment in lib.vsde_last_error(), (kw, lib.vsde_last_error())

    for kind in (0, 4, -1):
        rejected(b"kind", kind=kind)
    for dims in ({"B": 0}, {"T": 0}, {"B": -3}):
        rejected(b"dims", **dims)
    rejected(b"K=0", K=0)
    rejected(b"K=-2", K=-2)
    rejected(b"Ornstein-Uhlenbeck", S=2)
    rejected(b"Ornstein-Uhlenbeck", P=2)
    rejected(b"Lotka-Volterra", kind=2, S=1)
    rejected(b"Lotka-Volterra", kind=2, S=2, P=4)
    rejected(b"linear-diagonal", kind=3, S=33, P=66)
    rejected(b"linear-diagonal", kind=3, S=4, P=7)
    for name in ("x", "th", "steps", "key", "out"):
        rejected(b"NULL", **{name: ctypes.c_void_p(None)})
    rejected(b"time_step", dt=0.0)


def test_forecast_binding_refuses_cpu_tensors():
    from viforsdes_amd import _hip
    with pytest.raises(_hip.HipLibraryError):
        _hip.forecast("ornstein_uhlenbeck", torch.zeros(4, 1), torch.ones(4, 3), 3, torch.tensor([1, 3], dtype=torch.int32),
                      torch.zeros(2, dtype=torch.int32), 0.1)
