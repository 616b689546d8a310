"""GPU: the reaction-network kernels (kind 4: coef_*_kernel, em_*_kernel, forecast_kernel, log_weight_kernel in
csrc/vsde_sde.hip / csrc/vsde_elbo.hip, device functions in csrc/vsde_sde_coef.h) and every route that reaches them.

Bounds (fp32 kernels against float64 references, or against kind 2 on the same fp32 inputs):
* coefficients: per element |got - want| <= 2e-5 |want| + 2e-6 max|want|; VJP: 1e-4 of the largest entry;
* network-LV against kind 2 (the same model, other rounding order): 1e-5 of the largest entry for coefficients, VJP and
  log-weights, 1e-4 for the 400-step trajectory, its gradients and the 400-step forecast;
* simulator (400 steps) against float64 Euler-Maruyama: 1e-4 of the largest magnitude, its (x0, theta) gradient 1e-3;
* forecast against the float64 recursion on the Philox reference noise: 2e-5 (T <= 3), 2e-4 (T = 400), as
  tests/test_forecast_gpu.py;
* log-weights against the kind-0 route fed the float64 spec's coefficients: 5e-5 of the largest |log w|."""
import numpy as np
import pytest
import torch

from philox_reference import forecast_noise
from reaction_networks import BD, CHAIN8, ISOMER, LV, NET3, NET4, NETS, SIR  # noqa: F401
from viforsdes_amd import ReactionNetworkSDE

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")



def _rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-30))


def _spec_coefficients(sde, x, th, gf, gG):
    """float64 drift / diffusion of the spec on x [B, T+1, S] (rows 0..T-1) and their VJP for (gf, gG)."""
    x = x.detach().double().cpu().requires_grad_(True)
    th = th.detach().double().cpu().requires_grad_(True)
    B, T, S = x.shape[0], x.shape[1] - 1, x.shape[2]
    xf, tf = x[:, :-1].reshape(B * T, S), th.unsqueeze(1).expand(B, T, -1).reshape(B * T, -1)
    f, G = sde.drift(xf, tf).reshape(B, T, S), sde.diffusion(xf, tf).reshape(B, T, S, S)
    gx, gth = torch.autograd.grad((f * gf.double().cpu()).sum() + (G * gG.double().cpu()).sum(), [x, th])
    return f.detach(), G.detach(), gx, gth


def _coef_inputs(S, P, B=64, T=40, seed=0, lo=0.5, hi=3.0, tlo=0.2, thi=1.2):
    g = torch.Generator().manual_seed(seed)
    x = lo + (hi - lo) * torch.rand(B, T + 1, S, generator=g)
    th = tlo + (thi - tlo) * torch.rand(B, P, generator=g)
    return x, th, torch.randn(B, T, S, generator=g), torch.randn(B, T, S, S, generator=g)


def _kernel_coefficients(kind, sde, x, th, gf, gG):
    from viforsdes_amd import _hip
    net = sde.network_descriptor() if kind == "reaction_network" else None
    d = lambda t: t.to(DEV)
    f, G = _hip.sde_coefficients_fwd(kind, d(x), d(th), network=net)
    gx, gth = _hip.sde_coefficients_bwd(kind, d(x), d(th), d(gf), d(gG), network=net)
    return [t.double().cpu() for t in (f, G, gx, gth)]


# ------------------------------------------------------------------------------------------------------ 1. coefficients
@pytest.mark.parametrize("name", ["bd", "sir", "net3", "net4", "chain8"])
def test_coefficients_and_vjp_vs_float64_spec(name):
    sde = ReactionNetworkSDE(**NETS[name])
    x, th, gf, gG = _coef_inputs(sde.state_dim, sde.sde_param_dim, seed=len(name))
    f, G, gx, gth = _kernel_coefficients("reaction_network", sde, x, th, gf, gG)
    rf, rG, rgx, rgth = _spec_coefficients(sde, x, th, gf, gG)
    for got, want in ((f, rf), (G, rG)):
        assert bool(((got - want).abs() <= 2e-5 * want.abs() + 2e-6 * want.abs().max()).all()), (name, _rel(got, want))
    assert float(torch.diagonal(rG, dim1=-2, dim2=-1).min()) > 1e-2         # inputs clear of the floor
    for got, want in ((gx, rgx), (gth, rgth)):
        assert _rel(got, want) < 1e-4, (name, _rel(got, want))


def test_singular_network_binds_the_floor_like_the_spec():
    """A <-> B: rank-1 covariance, so L_11 is the 1e-6 floor's sqrt and passes no gradient; magnitudes keep the fp32
    cancellation error of Sigma_11 - L_10^2 (~1e-7) well below the floor."""
    sde = ReactionNetworkSDE(**ISOMER)
    x, th, gf, gG = _coef_inputs(2, 2, seed=11, lo=0.1, hi=1.0, tlo=0.1, thi=0.5)
    f, G, gx, gth = _kernel_coefficients("reaction_network", sde, x, th, gf, gG)
    rf, rG, rgx, rgth = _spec_coefficients(sde, x, th, gf, gG)
    assert bool((G[..., 1, 1] == float(np.sqrt(np.float32(1e-6)))).all())
    for got, want in ((f, rf), (G, rG)):
        assert bool(((got - want).abs() <= 2e-5 * want.abs() + 2e-6 * want.abs().max()).all())
    for got, want in ((gx, rgx), (gth, rgth)):
        assert _rel(got, want) < 1e-4


# ------------------------------------------------------------------------------------------- 2. network-LV against kind 2
def _lv_inputs(B, seed):
    g = torch.Generator().manual_seed(seed)
    th = torch.tensor([0.5, 0.0025, 0.3]) * (1.0 + 0.1 * torch.rand(B, 3, generator=g))
    x0 = torch.tensor([[71.0, 79.0]]) * (0.8 + 0.4 * torch.rand(B, 2, generator=g))
    return x0, th, g


def test_network_lv_kernels_equal_kind_2():
    from viforsdes_amd import _hip
    from viforsdes_amd.examples.sdes import LotkaVolterra
    net_sde, lv = ReactionNetworkSDE(**LV), LotkaVolterra()
    net = net_sde.network_descriptor()
    # coefficients and VJP on states along LV's orbit
    x, th, gf, gG = _coef_inputs(2, 3, B=128, T=50, seed=21, lo=5.0, hi=300.0)
    th = th * torch.tensor([0.5, 0.0025, 0.3])
    a = _kernel_coefficients("reaction_network", net_sde, x, th, gf, gG)
    b = _kernel_coefficients("lotka_volterra", lv, x, th, gf, gG)
    for u, v in zip(a, b):
        assert _rel(u, v) < 1e-5, _rel(u, v)
    # simulator forward / backward, 400 steps of the LV bench grid
    B, T, dt = 256, 400, 0.1
    x0, th, g = _lv_inputs(B, 22)
    noise, g_traj = torch.randn(B, T, 2, generator=g), torch.randn(B, T + 1, 2, generator=g)
    d = lambda t: t.to(DEV)
    tr = {k: _hip.euler_maruyama_fwd(k, d(x0), d(th), d(noise), dt, (0, 1), network=n)
          for k, n in (("reaction_network", net), ("lotka_volterra", None))}
    assert _rel(tr["reaction_network"], tr["lotka_volterra"]) < 1e-4
    gr = {k: _hip.euler_maruyama_bwd(k, d(th), d(noise), tr["lotka_volterra"], d(g_traj), dt, (0, 1), network=n)
          for k, n in (("reaction_network", net), ("lotka_volterra", None))}
    for u, v in zip(gr["reaction_network"], gr["lotka_volterra"]):
        assert _rel(u, v) < 1e-4, _rel(u, v)
    # forecast under one key
    key = torch.tensor([12345, -678], dtype=torch.int32, device=DEV)
    steps = torch.tensor([1, 7, 100, 400], dtype=torch.int32, device=DEV)
    fc = [_hip.forecast(k, d(x0), d(th), T, steps, key, dt, (0, 1), network=n)
          for k, n in (("reaction_network", net), ("lotka_volterra", None))]
    assert bool(torch.isfinite(fc[0]).all()) and _rel(fc[0], fc[1]) < 1e-4
    # log-weights
    lw = [_log_weights(k, n, _lw_case(2, 3, seed=23, theta_scale=torch.tensor([0.5, 0.0025, 0.3]), z_level=4.0))
          for k, n in (("reaction_network", net), ("lotka_volterra", None))]
    assert bool(torch.isfinite(lw[0]).all()) and _rel(lw[0], lw[1]) < 1e-5


# ------------------------------------------------------------------------------------------------------- 3. simulator
@pytest.mark.parametrize("name", ["sir", "chain8"])
def test_simulator_and_gradient_vs_float64(name):
    from viforsdes_amd.core.euler_maruyama import euler_maruyama
    sde = ReactionNetworkSDE(**NETS[name])
    S, P = sde.state_dim, sde.sde_param_dim
    B, T, dt = 128, 400, 0.01
    g = torch.Generator().manual_seed(31)
    if name == "sir":
        x0 = torch.tensor([[50.0, 10.0]]) * (0.8 + 0.4 * torch.rand(B, 2, generator=g))
        th = torch.tensor([0.01, 0.3]) * (0.8 + 0.4 * torch.rand(B, 2, generator=g))
    else:              # copy numbers ~ 100: the populations stay far from the floor
        x0 = 100.0 * (0.8 + 0.4 * torch.rand(B, S, generator=g))
        th = torch.cat([200.0 + 10.0 * torch.rand(B, 1, generator=g), 1.0 + torch.rand(B, P - 1, generator=g)], 1)
    noise, w = torch.randn(B, T, S, generator=g), torch.randn(B, T + 1, S, generator=g)
    pos = tuple(range(S))
    x0d, thd = x0.to(DEV).requires_grad_(True), th.to(DEV).requires_grad_(True)
    traj = euler_maruyama(sde, x0d, thd, T * dt, dt, pos, noise=noise.to(DEV))
    gx0, gth = torch.autograd.grad((traj * w.to(DEV)).sum(), [x0d, thd])
    x64, th64 = x0.double().requires_grad_(True), th.double().requires_grad_(True)
    ref = euler_maruyama(sde, x64, th64, T * dt, dt, pos, noise=noise.double())
    rgx0, rgth = torch.autograd.grad((ref * w.double()).sum(), [x64, th64])
    assert float(ref.detach().min()) > 0.1                               # no clamp on this grid
    assert _rel(traj.detach(), ref.detach()) < 1e-4
    assert _rel(gx0, rgx0) < 1e-3 and _rel(gth, rgth) < 1e-3, (_rel(gx0, rgx0), _rel(gth, rgth))


# -------------------------------------------------------------------------------------------------------- 4. forecast
STEPS = {3: [1, 3, 3], 400: [1, 2, 50, 257, 399, 400]}


@pytest.mark.parametrize("T", [3, 400])
@pytest.mark.parametrize("name", ["sir", "net3", "chain8"])
def test_forecast_vs_float64_recursion(name, T):
    from viforsdes_amd import _hip
    from viforsdes_amd.core.euler_maruyama import euler_maruyama
    sde = ReactionNetworkSDE(**NETS[name])
    S, P = sde.state_dim, sde.sde_param_dim
    B, dt = 257, 0.01
    g = torch.Generator().manual_seed(41)
    x = 10.0 * (0.8 + 0.4 * torch.rand(B, S, generator=g))
    th = 0.2 + torch.rand(B, P, generator=g)
    # rates that keep every population well above the floor over 400 steps
    if name == "sir":
        th[:, 0] *= 0.02
        th[:, 1] *= 0.1
    if name == "net3":         # copy numbers ~ 100
        x *= 10.0
        th *= torch.tensor([0.001, 0.05, 10.0, 10.0, 0.05])
    if name == "chain8":
        x *= 10.0
        th[:, 0] += 150.0
        th[:, 1:] += 1.0
    key = (0x9E3779B9 ^ T, 0x7F4A7C15)
    k = torch.from_numpy(np.array(key, dtype=np.uint32).view(np.int32)).to(DEV)
    steps = torch.tensor(STEPS[T], dtype=torch.int32, device=DEV)
    pos = tuple(range(S))
    out = _hip.forecast("reaction_network", x.to(DEV), th.to(DEV), T, steps, k, dt, pos,
                        network=sde.network_descriptor()).double().cpu()
    noise = torch.from_numpy(forecast_noise(B, T, S, key))
    ref = euler_maruyama(sde, x.double(), th.double(), T * dt, dt, pos, noise=noise)[:, STEPS[T]]
    assert bool(torch.isfinite(out).all())
    err = _rel(out, ref)
    print(f"{name} T={T}: max error {err:.2e} of the largest magnitude")
    assert err < (2e-4 if T > 3 else 2e-5), err


# ------------------------------------------------------------------------------------------------------ 5. log-weights
def _lw_case(S, P, seed, theta_scale=None, z_level=3.0, B=48, T=40):
    g = torch.Generator().manual_seed(seed)
    z = z_level + 0.05 * torch.randn(B, T + 1, S, generator=g).cumsum(1)
    means = z[:, :-1] + 0.02 * torch.randn(B, T, S, generator=g)
    chol = torch.tril(0.01 * torch.randn(B, T, S, S, generator=g), -1) + torch.diag_embed(0.2 + 0.1 * torch.rand(B, T, S, generator=g))
    th = 0.3 + 0.5 * torch.rand(B, P, generator=g)
    if theta_scale is not None:
        th = th * theta_scale
    rows = torch.tensor([0, 10, 20, 30, 40], dtype=torch.int32)
    vals = z[0, rows.long()] + 0.1 * torch.randn(5, S, generator=g)
    return dict(z=z, means=means, chol=chol, theta=th, obs_rows=rows, obs_values=vals, S=S, P=P)


def _log_weights(kind, network, c, drift=None, diffusion=None):
    from viforsdes_amd import _hip
    d = lambda t: None if t is None else t.to(DEV)
    S, P = c["S"], c["P"]
    return _hip.log_weights(kind, d(c["z"]), d(c["means"]), d(c["chol"]), d(drift), d(diffusion), d(c["theta"]), d(c["obs_rows"]),
                            d(c["obs_values"]), None, 1.0, 1, 0.0, 1.5, d(torch.zeros(P)), d(torch.zeros(P)), tuple(range(S)),
                            tuple(range(P)), 0.05, network=network).double().cpu()


@pytest.mark.parametrize("name", ["sir", "net4", "chain8"])
def test_log_weights_vs_kind_0_fed_the_spec(name):
    sde = ReactionNetworkSDE(**NETS[name])
    S, P = sde.state_dim, sde.sde_param_dim
    c = _lw_case(S, P, seed=51)
    x = torch.nn.functional.softplus(c["z"].double())
    B, T = x.shape[0], x.shape[1] - 1
    xf, tf = x[:, :-1].reshape(B * T, S), c["theta"].double().unsqueeze(1).expand(B, T, P).reshape(B * T, P)
    drift = sde.drift(xf, tf).reshape(B, T, S).float()
    diffusion = sde.diffusion(xf, tf).reshape(B, T, S, S).float()
    assert float(torch.diagonal(diffusion, dim1=-2, dim2=-1).min()) > 1e-2
    lw4 = _log_weights("reaction_network", sde.network_descriptor(), c)
    lw0 = _log_weights(None, None, c, drift, diffusion)
    assert bool(torch.isfinite(lw4).all())
    assert _rel(lw4, lw0) < 5e-5, _rel(lw4, lw0)


# ------------------------------------------------------------------------------------------------------------- 6. ELBO
def test_elbo_and_gradients_lotka_volterra_vs_network_lv():
    from viforsdes_amd import GaussianObservationLikelihood, Prior, PriorType
    from viforsdes_amd.examples.sdes import LotkaVolterra, lv_problem
    from viforsdes_amd.inference.evidence_lower_bound import compute_evidence_lower_bound
    from viforsdes_amd.inference.state_space import StateSpace
    from viforsdes_amd.inference.types import DiffusionPathSample
    from viforsdes_amd.models.sde_parameter_posterior import SDEParameterPosterior
    _, obs, like, prior, horizon, dt, state_pos, theta_pos = lv_problem()
    obs = type(obs)(times=obs.times.to(DEV), values=obs.values.to(DEV))
    T = round(horizon / dt)
    c = _lw_case(2, 3, seed=61, B=64, T=T, z_level=4.0)
    out = {}
    for name, sde in (("lv", LotkaVolterra()), ("net", ReactionNetworkSDE(**LV))):
        post = SDEParameterPosterior(3, theta_pos).to(DEV)
        z = c["z"].to(DEV).requires_grad_(True)
        theta = (c["theta"] * torch.tensor([0.5, 0.0025, 0.3])).to(DEV).requires_grad_(True)
        sample = DiffusionPathSample(z=z, transition_means=c["means"].to(DEV), transition_cholesky=c["chol"].to(DEV),
                                     state_space=StateSpace(2, state_pos))
        res = compute_evidence_lower_bound(sde, obs, like, prior, post, theta, sample, dt)
        gz, gth = torch.autograd.grad(res.evidence_lower_bound, [z, theta])
        out[name] = (res.evidence_lower_bound.detach().double().cpu(), gz.double().cpu(), gth.double().cpu())
    assert bool(torch.isfinite(out["net"][0]))
    for u, v in zip(out["net"], out["lv"]):
        assert _rel(u, v) < 1e-5, _rel(u, v)


# ------------------------------------------------------------------------------------------------------ 7. end to end
def test_sir_infer_predict_log_evidence_never_calls_python_propensities(monkeypatch):
    from viforsdes_amd import (EncoderConfig, GaussianObservationLikelihood, HeadConfig, InferenceConfig, Observations,
                               PretrainConfig, Prior, PriorType, TrainingConfig, infer)
    from viforsdes_amd.console import Console
    from viforsdes_amd.core import reaction_network
    from viforsdes_amd.core.euler_maruyama import euler_maruyama
    from viforsdes_amd.inference.trainer import VariationalInferenceTrainer

    sde = ReactionNetworkSDE(**SIR, species=["S", "I"], reactions=["infection", "removal"])
    horizon, dt = 20.0, 0.1
    g = torch.Generator().manual_seed(71)
    truth = euler_maruyama(sde, torch.tensor([[95.0, 5.0]], dtype=torch.float64), torch.tensor([[0.004, 0.15]], dtype=torch.float64),
                           horizon, dt, [0, 1], noise=torch.randn(1, round(horizon / dt), 2, generator=g, dtype=torch.float64))[0]
    times = torch.tensor([0.0, 5.0, 10.0, 15.0, 20.0])
    values = (truth[(times / dt).round().long()] + torch.randn(5, 2, generator=g, dtype=torch.float64)).float()
    obs = Observations(times=times, values=values)
    like = GaussianObservationLikelihood(variance=1.0)
    prior = Prior(type=PriorType.LOG_NORMAL, mean=-3.0, std=2.0, dim=2)

    calls = {"propensities": 0, "captured": []}
    real = reaction_network.propensities

    def counting(*a, **k):
        calls["propensities"] += 1
        return real(*a, **k)

    monkeypatch.setattr(reaction_network, "propensities", counting)
    capture = VariationalInferenceTrainer._capture_pretrain_step

    def recording(self, *a, **k):
        r = capture(self, *a, **k)
        calls["captured"].append(r is not None)
        return r

    monkeypatch.setattr(VariationalInferenceTrainer, "_capture_pretrain_step", recording)
    cfg = InferenceConfig(training=TrainingConfig(time_step=dt, batch_size=32, n_iterations=24),
                          encoder=EncoderConfig(hidden_dim=32, cond_dim=32, num_heads=4, depth=1),
                          head=HeadConfig(hidden_dim=32, num_layers=1), state_positive_dims=[0, 1], sde_param_positive_dims=[0, 1],
                          pretrain=PretrainConfig(n_iterations=30, batch_size=512), console=Console(enabled=False), seed=5)
    post = infer(sde, obs, like, prior, horizon, cfg)
    hist = post.evidence_lower_bound_history
    assert len(hist) == 24 and all(np.isfinite(hist))
    assert calls["captured"] == [True]                                    # the pre-training graph was captured
    pred = post.predict(sde, [horizon, horizon + 2.0, horizon + 5.0], n_samples=256, chunk_size=128)
    assert pred.states.shape == (256, 3, 2) and bool(torch.isfinite(pred.states).all())
    ev = post.log_evidence(sde, like, n_samples=256, chunk_size=128)
    assert np.isfinite(float(ev.log_evidence))
    assert calls["propensities"] == 0, calls                               # every GPU route ran the kernels
    # the same predict through the Python callables does call them (the counter sees the torch route)
    reaction_network.propensities(torch.ones(1, 2), torch.ones(1, 2), sde.reactants)
    assert calls["propensities"] == 1
