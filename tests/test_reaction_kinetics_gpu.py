"""GPU: reaction networks with rate laws and fixed / shared rate constants on the kernels (the KIN instantiations of kind 4:
coef_*_kernel, em_*_kernel, forecast_kernel, log_weight_kernel; device functions in csrc/vsde_sde_coef.h) and every route that
reaches them through the ``vsde_crn_kinetic_*`` entry points.

Bounds (fp32 kernels against float64 references, or against the mass-action entry points on the same fp32 inputs):
* coefficients: per element |got - want| <= 2e-5 |want| + 2e-6 max|want|; VJP: 1e-4 of the largest entry (observed on the
  MI355X, as a fraction of the largest entry: <= 7.8e-8 and <= 1.3e-7);
* simulator (400 steps) against float64 Euler-Maruyama: 1e-4 of the largest magnitude, its (x0, theta) gradient 1e-3
  (observed: <= 1.1e-6, <= 2.6e-6);
* forecast against the float64 recursion on the Philox reference noise: 2e-5 (T = 3), 2e-4 (T = 400) (observed: <= 1.4e-7,
  <= 1.4e-6);
* log-weights against the kind-0 route fed the float64 spec's coefficients: 5e-5 of the largest |log w| (observed: <= 1.4e-7);
* a mass-action network through the kinetic entry points against the mass-action ones: 1e-5 for coefficients, VJP and
  log-weights, 1e-4 for the trajectory, its gradients and the forecast, as tests/test_reaction_network_gpu.py (observed: 0,
  the same arithmetic);
* ELBO and its (theta, z) gradients with a shared and a fixed constant against the same ELBO whose coefficients are the float64
  spec and its autograd: 1e-5 of the value, 1e-4 of the largest gradient entry (observed: 0, <= 9.8e-8)."""
import numpy as np
import pytest
import torch

from philox_reference import forecast_noise
from reaction_networks import AUTOREG, CLAMP2, REPRESS3
from reaction_networks import KINETIC_CHAIN8 as CHAIN8
from viforsdes_amd import Hill, MichaelisMenten, ReactionNetworkSDE

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

# S = 1: self-repressed production (n = 2), linear decay, and a saturating (Michaelis-Menten) removal: R = 3, NR = 4
SELF1 = dict(reactants=[[0], [1], [1]], products=[[1], [0], [0]],
             rate_laws={0: Hill(0, "K", n=2, repression=True), 2: MichaelisMenten(0, "Km")}, rate_constants=["a", "d", "v"])
NETS = {"self1": SELF1, "autoreg": AUTOREG, "repress3": REPRESS3, "chain8": CHAIN8}


def _rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-30))


def _spec_coefficients(sde, x, th, gf, gG):
    """float64 drift / diffusion of the spec on x [B, T+1, S] (rows 0..T-1) and their VJP in (x, theta) for (gf, gG)."""
    x = x.detach().double().cpu().requires_grad_(True)
    th = th.detach().double().cpu().requires_grad_(True)
    B, T, S = x.shape[0], x.shape[1] - 1, x.shape[2]
    xf, tf = x[:, :-1].reshape(B * T, S), th.unsqueeze(1).expand(B, T, -1).reshape(B * T, -1)
    f, G = sde.drift(xf, tf).reshape(B, T, S), sde.diffusion(xf, tf).reshape(B, T, S, S)
    gx, gth = torch.autograd.grad((f * gf.double().cpu()).sum() + (G * gG.double().cpu()).sum(), [x, th])
    return f.detach(), G.detach(), gx, gth


def _kernel_coefficients(sde, x, th, gf, gG):
    """The kinetic entry points on the effective constants of theta; the theta gradient through the differentiable map."""
    from viforsdes_amd import _hip
    route = sde.kernel_descriptor()
    assert isinstance(route, _hip.CrnKineticRoute)
    d = lambda t: t.to(DEV)
    thd = d(th).requires_grad_(True)
    rates = sde.kernel_parameters(thd)
    f, G = _hip.sde_coefficients_fwd("reaction_network", d(x), rates.detach(), network=route)
    gx, grates = _hip.sde_coefficients_bwd("reaction_network", d(x), rates.detach(), d(gf), d(gG), network=route)
    (gth,) = torch.autograd.grad(rates, thd, grates)
    return [t.double().cpu() for t in (f, G, gx, gth)]


def _coef_inputs(sde, B=64, T=40, seed=0, lo=0.5, hi=3.0, tlo=0.2, thi=1.2):
    g = torch.Generator().manual_seed(seed)
    x = lo + (hi - lo) * torch.rand(B, T + 1, sde.state_dim, generator=g)
    th = tlo + (thi - tlo) * torch.rand(B, sde.sde_param_dim, generator=g)
    return x, th, torch.randn(B, T, sde.state_dim, generator=g), torch.randn(B, T, sde.state_dim, sde.state_dim, generator=g)


def _check_coefficients(name, got, want):
    f, G, gx, gth = got
    rf, rG, rgx, rgth = want
    for a, b in ((f, rf), (G, rG)):
        assert bool(((a - b).abs() <= 2e-5 * b.abs() + 2e-6 * b.abs().max()).all()), (name, _rel(a, b))
    for a, b in ((gx, rgx), (gth, rgth)):
        assert _rel(a, b) < 1e-4, (name, _rel(a, b))
    print(f"{name}: coefficients {max(_rel(f, rf), _rel(G, rG)):.1e}, VJP {max(_rel(gx, rgx), _rel(gth, rgth)):.1e}")


# ------------------------------------------------------------------------------------------------------ 1. coefficients
@pytest.mark.parametrize("name", ["self1", "autoreg", "repress3", "chain8"])
def test_coefficients_and_vjp_vs_float64_spec(name):
    sde = ReactionNetworkSDE(**NETS[name])
    kw = dict(lo=2.0, hi=40.0, tlo=1.0, thi=5.0) if name in ("repress3", "chain8") else {}
    x, th, gf, gG = _coef_inputs(sde, seed=len(name), **kw)
    spec = _spec_coefficients(sde, x, th, gf, gG)
    assert float(torch.diagonal(spec[1], dim1=-2, dim2=-1).min()) > 1e-2      # inputs clear of the floor
    _check_coefficients(name, _kernel_coefficients(sde, x, th, gf, gG), spec)


def test_modifier_at_the_clamp():
    """Both Hill laws with the modifier at 0 (gradient passes) and below 0 (h at u = 0, no gradient), as torch.clamp."""
    sde = ReactionNetworkSDE(**CLAMP2)
    x, th, gf, gG = _coef_inputs(sde, B=32, T=24, seed=5)
    x[:, :, 0] = torch.tensor([0.0, -0.7, 0.0, 1.3]).repeat(7)[:25]           # the modifier A: 0, negative, 0, positive
    spec = _spec_coefficients(sde, x, th, gf, gG)
    got = _kernel_coefficients(sde, x, th, gf, gG)
    _check_coefficients("clamp2", got, spec)
    gx = got[2][:, :-1, 0]
    assert bool((gx[:, 1::4] == 0).all()) and float(gx[:, 0::4].abs().max()) > 0   # no gradient below 0, a gradient at 0


# ------------------------------------------------------------------------------------------------------- 2. simulator
@pytest.mark.parametrize("name", ["autoreg", "repress3"])
def test_simulator_and_gradient_vs_float64(name):
    from viforsdes_amd.core.euler_maruyama import euler_maruyama
    sde = ReactionNetworkSDE(**NETS[name])
    S, P = sde.state_dim, sde.sde_param_dim
    B, T, dt = 128, 400, 0.01
    g = torch.Generator().manual_seed(31)
    x0 = 30.0 * (0.8 + 0.4 * torch.rand(B, S, generator=g))
    base = {"autoreg": [40.0, 1.0, 0.1, 10.0], "repress3": [60.0, 50.0, 0.2, 15.0]}[name]
    th = torch.tensor(base) * (0.8 + 0.4 * torch.rand(B, P, generator=g))
    noise, w = torch.randn(B, T, S, generator=g), torch.randn(B, T + 1, S, generator=g)
    pos = tuple(range(S))
    x0d, thd = x0.to(DEV).requires_grad_(True), th.to(DEV).requires_grad_(True)
    traj = euler_maruyama(sde, x0d, thd, T * dt, dt, pos, noise=noise.to(DEV))
    gx0, gth = torch.autograd.grad((traj * w.to(DEV)).sum(), [x0d, thd])
    x64, th64 = x0.double().requires_grad_(True), th.double().requires_grad_(True)
    ref = euler_maruyama(sde, x64, th64, T * dt, dt, pos, noise=noise.double())
    rgx0, rgth = torch.autograd.grad((ref * w.double()).sum(), [x64, th64])
    assert float(ref.detach().min()) > 0.1                               # no clamp on this grid
    e = (_rel(traj.detach(), ref.detach()), _rel(gx0, rgx0), _rel(gth, rgth))
    print(f"{name}: trajectory {e[0]:.1e}, gradients {e[1]:.1e} / {e[2]:.1e}")
    assert e[0] < 1e-4 and e[1] < 1e-3 and e[2] < 1e-3, e


# -------------------------------------------------------------------------------------------------------- 3. forecast
STEPS = {3: [1, 3, 3], 400: [1, 2, 50, 257, 399, 400]}


@pytest.mark.parametrize("T", [3, 400])
@pytest.mark.parametrize("name", ["self1", "autoreg", "chain8"])
def test_forecast_vs_float64_recursion(name, T):
    from viforsdes_amd.core.euler_maruyama import euler_maruyama
    from viforsdes_amd.core.forecast import forecast_states
    sde = ReactionNetworkSDE(**NETS[name])
    S, P = sde.state_dim, sde.sde_param_dim
    B, dt = 257, 0.01
    g = torch.Generator().manual_seed(41)
    x = 50.0 * (0.8 + 0.4 * torch.rand(B, S, generator=g))
    base = {"self1": [80.0, 0.5, 5.0, 30.0, 10.0], "autoreg": [40.0, 1.0, 0.1, 10.0], "chain8": [100.0, 20.0, 0.1, 30.0, 10.0]}
    th = torch.tensor(base[name][:P]) * (0.8 + 0.4 * torch.rand(B, P, generator=g))
    key = (0x9E3779B9 ^ T, 0x7F4A7C15)
    k = torch.from_numpy(np.array(key, dtype=np.uint32).view(np.int32)).to(DEV)
    pos = tuple(range(S))
    from viforsdes_amd import _hip
    route = sde.kernel_descriptor()
    steps = torch.tensor(STEPS[T], dtype=torch.int32, device=DEV)
    out = _hip.forecast("reaction_network", x.to(DEV), sde.kernel_parameters(th.to(DEV)), T, steps, k, dt, pos,
                        network=route).double().cpu()
    noise = torch.from_numpy(forecast_noise(B, T, S, key))
    ref = euler_maruyama(sde, x.double(), th.double(), T * dt, dt, pos, noise=noise)[:, STEPS[T]]
    assert bool(torch.isfinite(out).all()) and float(ref.min()) > 0.1
    err = _rel(out, ref)
    print(f"{name} T={T}: max error {err:.2e} of the largest magnitude")
    assert err < (2e-4 if T > 3 else 2e-5), err
    # the public route (forecast_states: Philox key from torch's generator) runs the same kernel
    fs = forecast_states(sde, x.to(DEV), th.to(DEV), T, STEPS[T], dt, pos)
    assert fs.shape == (B, len(STEPS[T]), S) and bool(torch.isfinite(fs).all())


# ----------------------------------------------------------------------------------------------------- 4. log-weights
def _lw_case(S, P, seed, B=48, T=40, z_level=3.0, theta_scale=None):
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


def _log_weights(kind, network, c, drift=None, diffusion=None, rates=None):
    from viforsdes_amd import _hip
    d = lambda t: None if t is None else t.to(DEV)
    S, P = c["S"], c["P"]
    return _hip.log_weights(kind, d(c["z"]), d(c["means"]), d(c["chol"]), d(drift), d(diffusion), d(c["theta"]), d(c["obs_rows"]),
                            d(c["obs_values"]), None, 1.0, 1, 0.0, 1.5, d(torch.zeros(P)), d(torch.zeros(P)), tuple(range(S)),
                            tuple(range(P)), 0.05, network=network, rates=d(rates)).double().cpu()


@pytest.mark.parametrize("name", ["self1", "autoreg", "repress3", "chain8"])
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
    lw4 = _log_weights("reaction_network", sde.kernel_descriptor(), c, rates=sde.kernel_parameters(c["theta"]))
    lw0 = _log_weights(None, None, c, drift, diffusion)
    assert bool(torch.isfinite(lw4).all())
    print(f"{name}: log-weights {_rel(lw4, lw0):.1e}")
    assert _rel(lw4, lw0) < 5e-5, _rel(lw4, lw0)


# ------------------------------------------------------------------------------- 5. mass action through the new entry points
def test_mass_action_network_through_kinetic_entry_points_equals_the_mass_action_ones():
    from viforsdes_amd import _hip
    net4 = dict(reactants=[[0, 0, 0, 0], [2, 0, 0, 0], [1, 1, 1, 0], [0, 0, 0, 1], [0, 1, 0, 0], [0, 0, 3, 0]],
                products=[[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 1], [0, 0, 0, 0], [0, 0, 1, 0], [0, 0, 1, 1]])
    plain = ReactionNetworkSDE(**net4)
    net = plain.network_descriptor()
    route = _hip.CrnKineticRoute(net, _hip.crn_kinetics([None] * 6), plain.kernel_parameters)
    x, th, gf, gG = _coef_inputs(plain, B=96, T=30, seed=61)
    d = lambda t: t.to(DEV)
    rates = plain.kernel_parameters(d(th))
    a = [*_hip.sde_coefficients_fwd("reaction_network", d(x), d(th), network=net),
         *_hip.sde_coefficients_bwd("reaction_network", d(x), d(th), d(gf), d(gG), network=net)]
    b = [*_hip.sde_coefficients_fwd("reaction_network", d(x), rates, network=route),
         *_hip.sde_coefficients_bwd("reaction_network", d(x), rates, d(gf), d(gG), network=route)]
    b[3] = b[3][:, :6]
    for u, v in zip(b, a):
        assert _rel(u, v) < 1e-5, _rel(u, v)
    B, T, dt = 128, 400, 0.005
    g = torch.Generator().manual_seed(62)
    x0 = 20.0 * (0.8 + 0.4 * torch.rand(B, 4, generator=g))
    th = torch.tensor([20.0, 0.01, 0.001, 0.5, 0.5, 0.001]) * (0.8 + 0.4 * torch.rand(B, 6, generator=g))
    noise, g_traj = torch.randn(B, T, 4, generator=g), torch.randn(B, T + 1, 4, generator=g)
    pos = (0, 1, 2, 3)
    ta = _hip.euler_maruyama_fwd("reaction_network", d(x0), d(th), d(noise), dt, pos, network=net)
    tb = _hip.euler_maruyama_fwd("reaction_network", d(x0), plain.kernel_parameters(d(th)), d(noise), dt, pos, network=route)
    assert _rel(tb, ta) < 1e-4
    ga = _hip.euler_maruyama_bwd("reaction_network", d(th), d(noise), ta, d(g_traj), dt, pos, network=net)
    gb = _hip.euler_maruyama_bwd("reaction_network", plain.kernel_parameters(d(th)), d(noise), ta, d(g_traj), dt, pos,
                                 network=route)
    assert _rel(gb[0], ga[0]) < 1e-4 and _rel(gb[1][:, :6], ga[1]) < 1e-4 and float(gb[1][:, 6:].abs().max()) == 0.0
    key = torch.tensor([12345, -678], dtype=torch.int32, device=DEV)
    steps = torch.tensor([1, 7, 100, 400], dtype=torch.int32, device=DEV)
    fa = _hip.forecast("reaction_network", d(x0), d(th), T, steps, key, dt, pos, network=net)
    fb = _hip.forecast("reaction_network", d(x0), plain.kernel_parameters(d(th)), T, steps, key, dt, pos, network=route)
    assert bool(torch.isfinite(fa).all()) and _rel(fb, fa) < 1e-4
    c = _lw_case(4, 6, seed=63)
    la = _log_weights("reaction_network", net, c)
    lb = _log_weights("reaction_network", route, c, rates=plain.kernel_parameters(c["theta"]))
    assert bool(torch.isfinite(la).all()) and _rel(lb, la) < 1e-5
    print("mass action, kinetic vs mass-action entry points:", _rel(b[0], a[0]), _rel(tb, ta), _rel(fb, fa), _rel(lb, la))


# ------------------------------------------------------------------------------------------------------------- 6. ELBO
class _SpecCoefficients64(torch.autograd.Function):
    """The spec's drift / diffusion evaluated in float64 on the host, its VJP by float64 autograd: the reference ELBO."""

    @staticmethod
    def forward(ctx, x, theta, sde):
        ctx.sde, ctx.dev = sde, x.device
        ctx.save_for_backward(x, theta)
        f, G, _, _ = _spec64(sde, x, theta, None, None)
        return f.float().to(ctx.dev), G.float().to(ctx.dev)

    @staticmethod
    def backward(ctx, gf, gG):
        x, theta = ctx.saved_tensors
        _, _, gx, gth = _spec64(ctx.sde, x, theta, gf, gG)
        return gx.float().to(ctx.dev), gth.float().to(ctx.dev), None


def _spec64(sde, x, theta, gf, gG):
    with torch.enable_grad():
        x = x.detach().double().cpu().requires_grad_(True)
        th = theta.detach().double().cpu().requires_grad_(True)
        B, T, S = x.shape[0], x.shape[1] - 1, x.shape[2]
        xf, tf = x[:, :-1].reshape(B * T, S), th.unsqueeze(1).expand(B, T, -1).reshape(B * T, -1)
        f, G = sde.drift(xf, tf).reshape(B, T, S), sde.diffusion(xf, tf).reshape(B, T, S, S)
        if gf is None:
            return f.detach(), G.detach(), None, None
        gx, gth = torch.autograd.grad((f * gf.double().cpu()).sum() + (G * gG.double().cpu()).sum(), [x, th])
    return f.detach(), G.detach(), gx, gth


def test_elbo_theta_gradients_with_shared_and_fixed_constants_vs_float64(monkeypatch):
    from viforsdes_amd import GaussianObservationLikelihood, Observations, Prior, PriorType
    from viforsdes_amd.inference import evidence_lower_bound as elbo_mod
    from viforsdes_amd.inference.state_space import StateSpace
    from viforsdes_amd.inference.types import DiffusionPathSample
    from viforsdes_amd.models.sde_parameter_posterior import SDEParameterPosterior
    sde = ReactionNetworkSDE(**REPRESS3)                              # alpha shared by two reactions, a fixed K and decay d x3
    S, P, B, T, dt = 3, sde.sde_param_dim, 64, 40, 0.05
    c = _lw_case(S, P, seed=71, B=B, T=T, z_level=3.0, theta_scale=torch.tensor([20.0, 20.0, 0.5, 10.0]))
    obs = Observations(times=torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0], device=DEV), values=c["obs_values"].to(DEV))
    like = GaussianObservationLikelihood(variance=1.0)
    prior = Prior(type=PriorType.LOG_NORMAL, mean=0.0, std=2.0, dim=P)
    out = {}
    for name in ("kernels", "float64 spec"):
        if name == "float64 spec":
            monkeypatch.setattr(elbo_mod, "sde_coefficients", lambda s, x, th: _SpecCoefficients64.apply(x, th, s))
        post = SDEParameterPosterior(P, list(range(P))).to(DEV)
        z = c["z"].to(DEV).requires_grad_(True)
        theta = c["theta"].to(DEV).requires_grad_(True)
        sample = DiffusionPathSample(z=z, transition_means=c["means"].to(DEV), transition_cholesky=c["chol"].to(DEV),
                                     state_space=StateSpace(S, list(range(S))))
        res = elbo_mod.compute_evidence_lower_bound(sde, obs, like, prior, post, theta, sample, dt)
        gz, gth = torch.autograd.grad(res.evidence_lower_bound, [z, theta])
        out[name] = (res.evidence_lower_bound.detach().double().cpu(), gz.double().cpu(), gth.double().cpu())
    (e, gz, gth), (re, rgz, rgth) = out["kernels"], out["float64 spec"]
    assert bool(torch.isfinite(e)) and float(rgth.abs().max()) > 0
    errs = (_rel(e, re), _rel(gz, rgz), _rel(gth, rgth))
    print(f"ELBO {errs[0]:.1e}, z gradient {errs[1]:.1e}, theta gradient {errs[2]:.1e}")
    assert errs[0] < 1e-5 and errs[1] < 1e-4 and errs[2] < 1e-4, errs


# ------------------------------------------------------------------------------------------------------ 7. end to end
def test_autoregulation_infer_predict_log_evidence_never_calls_python_propensities(monkeypatch):
    from viforsdes_amd import (EncoderConfig, GaussianObservationLikelihood, HeadConfig, InferenceConfig, Observations,
                               PretrainConfig, Prior, PriorType, TrainingConfig, infer)
    from viforsdes_amd.console import Console
    from viforsdes_amd.core import reaction_network
    from viforsdes_amd.core.euler_maruyama import euler_maruyama
    from viforsdes_amd.inference.trainer import VariationalInferenceTrainer

    sde = ReactionNetworkSDE(**AUTOREG)
    horizon, dt = 20.0, 0.1
    g = torch.Generator().manual_seed(81)
    truth = euler_maruyama(sde, torch.tensor([[5.0, 20.0]], dtype=torch.float64),
                           torch.tensor([[20.0, 0.5, 0.1, 15.0]], dtype=torch.float64), horizon, dt, [0, 1],
                           noise=torch.randn(1, round(horizon / dt), 2, generator=g, dtype=torch.float64))[0]
    times = torch.tensor([0.0, 5.0, 10.0, 15.0, 20.0])
    values = (truth[(times / dt).round().long()] + torch.randn(5, 2, generator=g, dtype=torch.float64)).float()
    obs = Observations(times=times, values=values)
    like = GaussianObservationLikelihood(variance=1.0)
    prior = Prior(type=PriorType.LOG_NORMAL, mean=0.0, std=2.0, dim=4)

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
                          head=HeadConfig(hidden_dim=32, num_layers=1), state_positive_dims=[0, 1],
                          sde_param_positive_dims=[0, 1, 2, 3],
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
    reaction_network.propensities(torch.ones(1, 2), torch.ones(1, 8), sde.reactants, [None] * 4)
    assert calls["propensities"] == 1
