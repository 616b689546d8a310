"""GPU: the forecast kernel (csrc/vsde_sde.hip: forecast_kernel, vsde_forecast), ``forecast_states`` and
``VariationalPosterior.predict``.

* The kernel's normals, recovered from its outputs, equal the numpy Philox / Box-Muller reference (tests/philox_reference.py)
  within 1e-5 absolute.  Observed on an MI355X: 5.2e-7.
* The forecast against a float64 Euler-Maruyama run on the reference noise: 2e-5 of the largest magnitude at T <= 3, 2e-4 at
  T = 400 (the bound the simulator's own float64 test allows).  Observed: 1.7e-7 (T <= 3), 3.3e-6 (T = 400, Lotka-Volterra).
* Moments and two-sample comparisons: z-scores below 5.  Observed: at most 2.4."""
import math

import numpy as np
import pytest
import torch

from philox_reference import forecast_noise

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FLOOR = float(np.float32(1e-6))      # the clamp bound as the fp32 kernels hold it


def _key(k0, k1):
    return torch.from_numpy(np.array([k0, k1], dtype=np.uint32).view(np.int32)).to(DEV)


def _forecast(kind, x, th, T, steps, key, dt, pos=()):
    from viforsdes_amd import _hip
    steps = torch.tensor(steps, dtype=torch.int32, device=DEV)
    return _hip.forecast(kind, x.to(DEV), th.to(DEV), T, steps, key, dt, pos)


# --------------------------------------------------------------------------------------------------- 1. the noise stream
def test_noise_stream_is_the_specified_one_element_by_element():
    B, T, key = 300, 9, (0x1234ABCD, 0xDEADBEEF)
    ref = forecast_noise(B, T, 5, key)
    # OU with kappa = 0, sigma = 1, dt = 1, x_start = 0: x_{t+1} - x_t = z_t
    th = torch.tensor([[0.0, 0.0, 1.0]]).expand(B, 3)
    out = _forecast("ornstein_uhlenbeck", torch.zeros(B, 1), th, T, list(range(1, T + 1)), _key(*key), 1.0)
    x = torch.cat([torch.zeros(B, 1, 1, device=DEV), out], 1).double().cpu().numpy()
    err_ou = np.abs(np.diff(x, axis=1) - ref[:, :, :1]).max()
    # linear-diagonal, a = 0, S = 5: x_{t+1} - x_t = g z_t with g = softplus(b) + 1e-3 (b > 20: softplus(b) = b in fp32)
    g = np.float32(np.float32(21.0) + np.float32(1e-3))
    th3 = torch.cat([torch.zeros(B, 5), torch.full((B, 5), 21.0)], 1)
    out3 = _forecast("linear_diagonal", torch.zeros(B, 5), th3, T, list(range(1, T + 1)), _key(*key), 1.0)
    x3 = torch.cat([torch.zeros(B, 1, 5, device=DEV), out3], 1).double().cpu().numpy()
    err_ld = np.abs(np.diff(x3, axis=1) / float(g) - ref).max()
    print(f"noise stream: max |z - z_ref| OU {err_ou:.2e}, linear-diagonal {err_ld:.2e}")
    assert err_ou < 1e-5 and err_ld < 1e-5


# --------------------------------------------------------------------------------------- 2. against float64 Euler-Maruyama
def _case(name, B):
    from viforsdes_amd.examples.sdes import LinearDiagonalSDE, LotkaVolterra, OrnsteinUhlenbeck
    g = torch.Generator().manual_seed(17)
    if name == "ou":
        th = torch.stack([0.5 + 1.5 * torch.rand(B, generator=g), torch.randn(B, generator=g), 0.2 + torch.rand(B, generator=g)], 1)
        return OrnsteinUhlenbeck(), "ornstein_uhlenbeck", torch.randn(B, 1, generator=g), th, 0.05, []
    if name == "lv":   # around the classical parameters; every 4th row starts from small populations and hits the 1e-6 floor
        th = torch.tensor([0.5, 0.0025, 0.3]) * (1.0 + 0.1 * torch.rand(B, 3, generator=g))
        x = torch.tensor([[71.0, 79.0]]).repeat(B, 1)
        x[::4] = torch.rand(len(x[::4]), 2, generator=g) * 0.05
        return LotkaVolterra(), "lotka_volterra", x, th, 0.1, [0, 1]
    S = 32
    th = torch.cat([torch.rand(B, S, generator=g), torch.randn(B, S, generator=g)], 1)
    x = torch.randn(B, S, generator=g)
    pos = [0, 3, 17, 31]
    x[:, pos] = x[:, pos].abs() * 0.05
    return LinearDiagonalSDE(S), "linear_diagonal", x, th, 0.05, pos


STEPS = {1: [1, 1], 3: [1, 3, 3], 400: [1, 2, 50, 50, 257, 399, 400]}


@pytest.mark.parametrize("T", [1, 3, 400])
@pytest.mark.parametrize("name", ["ou", "lv", "lindiag"])
def test_forecast_matches_float64_euler_maruyama(name, T):
    from viforsdes_amd.core.euler_maruyama import euler_maruyama
    B = 257
    sde, kind, x, th, dt, pos = _case(name, B)
    x[7] = float("nan")                                          # poisons its own path only
    key = (0x9E3779B9 ^ T, 0x7F4A7C15)
    out = _forecast(kind, x, th, T, STEPS[T], _key(*key), dt, pos).double().cpu()
    noise = torch.from_numpy(forecast_noise(B, T, sde.state_dim, key))
    ref = euler_maruyama(sde, x.double(), th.double(), T * dt, dt, pos, noise=noise)[:, STEPS[T]]
    assert bool(out[7].isnan().all())
    keep = torch.arange(B) != 7
    o, r = out[keep], ref[keep]
    assert bool(torch.isfinite(o).all())
    err = float((o - r).abs().max() / r.abs().max())
    print(f"{name} T={T}: max error {err:.2e} of the largest magnitude")
    assert err < (2e-4 if T > 3 else 2e-5), err
    if pos:
        assert bool((o[..., pos] >= FLOOR).all())
        if name == "lv":
            assert bool((o == FLOOR).any())                    # the clamp was exercised


# --------------------------------------------------------------------------------------------------------------- 3. keys
def test_keys_and_seeds():
    from viforsdes_amd.core.forecast import forecast_states
    from viforsdes_amd.examples.sdes import LotkaVolterra
    sde, kind, x, th, dt, pos = _case("lv", 300)
    a = _forecast(kind, x, th, 50, [10, 50], _key(1, 2), dt, pos)
    b = _forecast(kind, x, th, 50, [10, 50], _key(1, 2), dt, pos)
    c = _forecast(kind, x, th, 50, [10, 50], _key(1, 3), dt, pos)
    d = _forecast(kind, x, th, 50, [10, 50], _key(2, 2), dt, pos)
    assert torch.equal(a, b)
    assert not bool((a == c).all()) and not bool((a == d).all())
    x, th = x.to(DEV), th.to(DEV)
    torch.manual_seed(5)
    e = forecast_states(LotkaVolterra(), x, th, 50, [10, 50], dt, pos)
    torch.manual_seed(5)
    f = forecast_states(LotkaVolterra(), x, th, 50, [10, 50], dt, pos)
    g = forecast_states(LotkaVolterra(), x, th, 50, [10, 50], dt, pos)
    assert torch.equal(e, f) and not torch.equal(f, g)


# ------------------------------------------------------------------------------------------------------ 4. graph capture
def test_graph_replays_take_a_fresh_key():
    from viforsdes_amd import _hip
    sde, kind, x, th, dt, pos = _case("lindiag", 300)
    x, th = x.to(DEV), th.to(DEV)
    steps = torch.tensor([1, 7, 20], dtype=torch.int32, device=DEV)

    def launch():
        key = torch.randint(-2 ** 31, 2 ** 31, (2,), device=DEV, dtype=torch.int32)
        return key, _hip.forecast(kind, x, th, 20, steps, key, dt, pos)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        key_s, out_s = launch()
    replays = []
    for _ in range(2):
        graph.replay()
        replays.append((key_s.clone(), out_s.clone()))
    torch.cuda.synchronize()
    (k1, o1), (k2, o2) = replays
    assert not torch.equal(k1, k2) and not torch.equal(o1, o2)
    for k, o in replays:
        assert torch.equal(_hip.forecast(kind, x, th, 20, steps, k, dt, pos), o)


# ------------------------------------------------------------------------------------------------------------ 5. moments
def test_ou_moments_and_increment_statistics():
    n = 1 << 20
    kappa, mu, sigma, dt, T = 0.8, 1.5, 0.6, 0.1, 20
    steps = [1, 2, 5, 10, 20]
    th = torch.tensor([[kappa, mu, sigma]]).expand(n, 3)
    out = _forecast("ornstein_uhlenbeck", torch.zeros(n, 1), th, T, steps, _key(7, 11), dt)[..., 0].double()
    a, m, v, exact = 1.0 - kappa * dt, 0.0, 0.0, {}
    for t in range(1, T + 1):
        m, v = a * m + kappa * mu * dt, a * a * v + sigma * sigma * dt
        exact[t] = (m, v)
    worst = 0.0
    for k, t in enumerate(steps):
        m, v = exact[t]
        zm = (float(out[:, k].mean()) - m) / math.sqrt(v / n)
        zv = (float(out[:, k].var()) - v) / (v * math.sqrt(2.0 / (n - 1)))
        worst = max(worst, abs(zm), abs(zv))
    # increments: kappa = 0, sigma = 1, dt = 1
    Ti = 8
    th0 = torch.tensor([[0.0, 0.0, 1.0]]).expand(n, 3)
    x = _forecast("ornstein_uhlenbeck", torch.zeros(n, 1), th0, Ti, list(range(1, Ti + 1)), _key(3, 4), 1.0)[..., 0].double()
    z = torch.diff(torch.cat([torch.zeros(n, 1, device=DEV, dtype=torch.float64), x], 1), dim=1)   # [n, Ti]
    N = z.numel()
    zs = [float(z.mean()) / math.sqrt(1.0 / N), (float(z.var()) - 1.0) / math.sqrt(2.0 / N),
          (float((z ** 4).mean() / z.var() ** 2) - 3.0) / math.sqrt(24.0 / N)]
    lag_t = float((z[:, 1:] * z[:, :-1]).mean())                   # across steps
    lag_b = float((z[1:] * z[:-1]).mean())                         # across neighbouring paths
    print(f"moment z-scores: worst {worst:.2f}; increments {[round(v, 2) for v in zs]}; lag-1 {lag_t:.2e} {lag_b:.2e}")
    assert worst < 5.0 and all(abs(v) < 5.0 for v in zs)
    assert abs(lag_t) < 5.0 / math.sqrt(n) and abs(lag_b) < 5.0 / math.sqrt(n)
    assert float(z.abs().max()) <= math.sqrt(50.0 * math.log(2.0)) + 1e-4


# ------------------------------------------------------------------------------------------------------------- predict
_POSTERIORS = {}


def _posterior(name):
    """An untrained posterior on the GPU (the draws' distribution does not matter here, only how they are paired)."""
    if name in _POSTERIORS:
        return _POSTERIORS[name]
    from viforsdes_amd import EncoderConfig, GaussianObservationLikelihood, HeadConfig, Observations
    from viforsdes_amd.examples.sdes import LinearDiagonalSDE, ou_problem
    from viforsdes_amd.inference.exponential_moving_average import ExponentialMovingAverage
    from viforsdes_amd.inference.state_space import StateSpace
    from viforsdes_amd.models.variational_sde_posterior import VariationalSDEPosterior
    from viforsdes_amd.posterior.variational_posterior import VariationalPosterior
    torch.manual_seed(0)
    if name == "ou":
        sde, obs, like, prior, horizon, dt, _, theta_pos = ou_problem()
    else:
        sde, theta_pos, horizon, dt = LinearDiagonalSDE(2), [], 2.0, 0.05
        obs = Observations(times=torch.tensor([0.0, 1.0, 2.0]), values=torch.tensor([[0.5, -0.3], [0.2, 0.1], [-0.4, 0.6]]))
        like = GaussianObservationLikelihood(variance=0.09, obs_matrix=torch.tensor([[1.0, 0.5], [-0.3, 2.0]]))
        from viforsdes_amd import Prior, PriorType
        prior = Prior(type=PriorType.NORMAL, mean=0.0, std=1.0, dim=4)
    S, P = sde.state_dim, sde.sde_param_dim
    model = VariationalSDEPosterior(obs.values.shape[1], S, P, EncoderConfig(hidden_dim=32, cond_dim=32, num_heads=4, depth=1),
                                    HeadConfig(hidden_dim=32, num_layers=1), theta_pos)
    vp = VariationalPosterior(model=model, exponential_moving_average=ExponentialMovingAverage(model), prior=prior,
                              observations=obs, time_horizon=horizon, time_step=dt, state_space=StateSpace(S, []),
                              evidence_lower_bound_history=[], device=DEV)
    _POSTERIORS[name] = (sde, like, vp)
    return _POSTERIORS[name]


def test_predict_inside_the_horizon_equals_sample():
    sde, _, vp = _posterior("ou")
    times = vp.observations.times
    n = 256
    torch.manual_seed(123)
    pred = vp.predict(sde, times, n_samples=n, chunk_size=n)
    assert vp._captured == {} and vp._calls == {}
    torch.manual_seed(123)
    s = vp.sample(n)
    rows = torch.round(times / vp.time_step).long()
    assert pred.states.shape == (n, times.numel(), 1) and pred.observations is None
    assert torch.equal(pred.sde_parameters, s.sde_parameters)
    assert torch.equal(pred.states, s.diffusion_paths[:, rows])
    vp.release_graphs()


def test_forecast_continues_each_draws_own_path():
    sde, _, vp = _posterior("ou")
    n, dt = 8192, vp.time_step
    torch.manual_seed(9)
    pred = vp.predict(sde, [vp.time_horizon, vp.time_horizon + dt], n_samples=n, chunk_size=2048)
    assert vp._captured == {} and vp._calls == {}
    x0, x1 = pred.states[:, 0, 0].double(), pred.states[:, 1, 0].double()
    kappa, mu, sigma = pred.sde_parameters.double().unbind(1)
    z = (x1 - x0 - kappa * (mu - x0) * dt) / (sigma * math.sqrt(dt))
    zm, zv = float(z.mean()) * math.sqrt(n), (float(z.var()) - 1.0) / math.sqrt(2.0 / n)
    print(f"own-path continuation: mean z-score {zm:.2f}, variance z-score {zv:.2f}")
    assert abs(zm) < 5.0 and abs(zv) < 5.0
    # the path end is the sampled path's last state: the draws of the chunks beyond the first are the captured sampler's
    torch.manual_seed(9)
    ends = vp.predict(sde, [vp.time_horizon], n_samples=n, chunk_size=2048).states[:, 0]
    assert torch.equal(ends, pred.states[:, 0])


def _ou_functional():
    from viforsdes_amd import FunctionalSDE
    return FunctionalSDE(lambda x, th: th[:, 0:1] * (th[:, 1:2] - x), lambda x, th: th[:, 2:3].reshape(-1, 1, 1), 1, 3)


def test_user_sde_and_builtin_sde_agree_in_distribution():
    from viforsdes_amd.core.forecast import forecast_states
    from viforsdes_amd.examples.sdes import OrnsteinUhlenbeck
    n, T, dt, steps = 16384, 30, 0.05, [1, 10, 30]
    g = torch.Generator().manual_seed(2)
    x = torch.randn(n, 1, generator=g).to(DEV)
    th = torch.stack([0.5 + torch.rand(n, generator=g), torch.randn(n, generator=g), 0.3 + torch.rand(n, generator=g)], 1).to(DEV)
    torch.manual_seed(4)
    a = forecast_states(OrnsteinUhlenbeck(), x, th, T, steps, dt).double()
    b = forecast_states(_ou_functional(), x, th, T, steps, dt).double()
    worst = 0.0
    for k in range(len(steps)):
        ma, mb, va, vb = float(a[:, k].mean()), float(b[:, k].mean()), float(a[:, k].var()), float(b[:, k].var())
        worst = max(worst, abs(ma - mb) / math.sqrt((va + vb) / n), abs(va - vb) / math.sqrt(2.0 * (va * va + vb * vb) / n))
    print(f"user vs built-in SDE: worst two-sample z {worst:.2f}")
    assert worst < 5.0
    # predict() takes the torch route for the user SDE
    sde, _, vp = _posterior("ou")
    pred = vp.predict(_ou_functional(), [1.0, vp.time_horizon + 0.5], n_samples=300, chunk_size=128)
    assert pred.states.shape == (300, 2, 1) and bool(torch.isfinite(pred.states).all())


def test_observation_draws_and_shapes():
    sde, like, vp = _posterior("lindiag")
    times = [0.5, 2.0, 2.5, 3.0]
    n = 1000
    pred = vp.predict(sde, times, n_samples=n, observation_likelihood=like, chunk_size=384)
    assert vp._captured == {} and vp._calls == {}
    assert pred.sde_parameters.shape == (n, 4) and pred.states.shape == (n, 4, 2) and pred.observations.shape == (n, 4, 2)
    assert pred.times.shape == (4,)
    H = like.obs_matrix.to(DEV)
    r = (pred.observations - pred.states @ H.T).double()
    N = r.numel()
    zm, zv = float(r.mean()) / math.sqrt(like.variance / N), (float(r.var()) - like.variance) / (like.variance * math.sqrt(2.0 / N))
    print(f"observation residuals: mean z {zm:.2f}, variance z {zv:.2f}")
    assert abs(zm) < 5.0 and abs(zv) < 5.0
    q = pred.quantiles(observations=True)
    assert q.q50.shape == (4, 2) and bool((q.q05 <= q.q95).all())
