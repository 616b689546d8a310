"""GPU: the count observation terms (Poisson, negative binomial) on the ELBO tail, log-weight and particle-filter kernels
(csrc/vsde_elbo.hip, csrc/vsde_filter.hip: the CNT instantiations), against float64 torch / numpy on the same inputs.  The bounds
are the project's own for the same quantities under the Gaussian term (tests/test_elbo_gpu.py, tests/test_evidence_gpu.py,
tests/test_particle_filter_gpu.py).

The filter is compared STAGE BY STAGE against float64 on its own previous stage (the kernel's particles), never as a whole.  A
species that sits at the 1e-6 floor must not be observed on its own under a count likelihood (y log(1e-6) differs by hundreds
between a clamped particle and its neighbour: the particle ESS collapses, which is the model's doing, not the kernel's), so the
positive-state cases observe it through an H row that adds a populated species.

Observed on an MI355X: tail values <= 5.7e-7 (bound 2e-5), gradients <= 3.9e-7 (1e-5); log-weights <= 6.3e-7 of the largest
component (1e-5); filter increments <= 1.1e-6 (1e-5), ESS / mean / std <= 2.0e-6 / 6.8e-6 / 2.7e-5 (1e-4), <= 4.9e-5 of the ancestors
off by one (1e-3), smallest float64 particle ESS 16.6 of 64 and 291 of 1024; kernel against torch route z = 0.21."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import count_likelihood_reference as cref
import particle_filter_reference as ref
from helpers import rel_err

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FLOOR = float(np.float32(1e-6))
SIR = dict(reactants=[[1, 1], [0, 1]], products=[[0, 2], [0, 0]])
AUTOREG_KW = dict(reactants=[[0, 0], [1, 0], [1, 0], [0, 1]], products=[[1, 0], [1, 1], [0, 0], [0, 0]], species=["M", "P"],
                  reactions=["transcription", "translation", "mRNA decay", "protein decay"],
                  rate_constants=["k_tx", "k_tl", 0.1, "d_P"])
SIR_TIMES = [0.0, 5.0, 10.0, 15.0, 20.0]
SIR_VALUES = [[95.0, 5.0], [85.0, 8.0], [72.0, 11.0], [60.0, 12.0], [50.0, 11.0]]


def _key(k0, k1, dev=DEV):
    return torch.from_numpy(np.array([k0, k1], dtype=np.uint32).view(np.int32)).to(dev)


def _like(kind, scale=1.0, H=None):
    from viforsdes_amd import NegativeBinomialObservationLikelihood, PoissonObservationLikelihood
    if kind == "poisson":
        return PoissonObservationLikelihood(scale=scale, obs_matrix=H)
    return NegativeBinomialObservationLikelihood(dispersion=10.0, scale=scale, obs_matrix=H)


def _like64(like):
    kw = dict(scale=like.scale, obs_matrix=None if like.obs_matrix is None else like.obs_matrix.double())
    if hasattr(like, "dispersion"):
        kw["dispersion"] = like.dispersion
    return type(like)(**kw)


def _sir():
    from viforsdes_amd import ReactionNetworkSDE
    return ReactionNetworkSDE(**SIR, species=["S", "I"], reactions=["infection", "removal"])


def _autoreg():
    from viforsdes_amd import Hill, ReactionNetworkSDE
    return ReactionNetworkSDE(**AUTOREG_KW, rate_laws={"transcription": Hill("P", K="K", n=2, repression=True)})


# ----------------------------------------------------------------------------------------------------- 1. tail, forward / backward
THETA_VARIANTS = [("normal", []), ("log_normal", [0, 2]), ("log_normal", [0, 1, 2]), ("normal", [1])]   # tests/test_elbo_gpu.py


def _tail_inputs(kind, B, S, O, with_matrix):
    """x_obs [B, K, S], y [K, O], the likelihood.  Rates from a few to about 1000, counts of 0 and 1000 among the observations; the
    state row (b, k) = (0, 0) sits at the 1e-6 floor where every rate is floored: scale * x = 5e-7 without H, scale * H x < 0 with
    the H below (first column -10, the rest in 0.1 .. 0.5)."""
    g = torch.Generator().manual_seed(100 * S + O + B)
    K, scale = 3, 0.5
    level = torch.tensor([8.0, 400.0, 30.0])
    if with_matrix:
        H = 0.1 + 0.4 * torch.rand(O, S, generator=g)
        H[:, 0] = -10.0
        xbar = level[:, None].expand(K, S).clone()
        xbar[:, 0] = 0.05
    else:
        H = None
        xbar = level[:, None].expand(K, S).clone()
    x = xbar[None] * (1.0 + 0.2 * torch.randn(B, K, S, generator=g)).abs()
    x[0, 0] = 1e-6
    pred = xbar if H is None else xbar @ H.T
    if S == 1 and with_matrix:
        raise AssertionError("the S = 1 case has no matrix")
    y = torch.round(scale * pred).clamp(min=0.0)
    y[0, 0] = 0.0
    y[1, O - 1] = 1000.0
    like = _like(kind, scale, None if H is None else H.to(DEV))
    return x, y, like


def _tail_reference(x, y, like, th, prior, mean, log_std, tpos, paths, w):
    """float64 torch: out6 and the gradients of sum(w * out6) w.r.t. x, theta, mean, log_std."""
    from viforsdes_amd.models.sde_parameter_posterior import SDEParameterPosterior
    xr, tr = x.double().requires_grad_(True), th.double().requires_grad_(True)
    post = SDEParameterPosterior(th.shape[1], list(tpos)).double()
    with torch.no_grad():
        post.mean.copy_(mean.double()); post.log_std.copy_(log_std.double())
    B = x.shape[0]
    obs = _like64(like).log_prob(y.double().unsqueeze(0).expand(B, -1, -1), xr).sum(-1)
    pr = prior.log_prob(tr)
    pr = pr.sum(-1) if pr.ndim > 1 else pr
    po = post.log_prob(tr)
    s, gn, j = (p.double() for p in paths)
    out = torch.stack([(obs + s - gn + j + pr - po).mean(), obs.mean(), s.mean(), gn.mean(), pr.mean(), po.mean()])
    grads = torch.autograd.grad((out * w.double()).sum(), [xr, tr, post.mean, post.log_std])
    return out.detach(), grads


@pytest.mark.parametrize("dims", [(1, 1, False), (2, 2, False), (3, 2, True), (16, 16, True)], ids=lambda d: f"S{d[0]}O{d[1]}")
@pytest.mark.parametrize("B", [5, 130])
@pytest.mark.parametrize("kind", ["poisson", "negbin"])
def test_tail_forward_and_backward_match_float64(kind, B, dims):
    from viforsdes_amd import Prior, PriorType, _hip
    S, O, with_matrix = dims
    P = 3
    x, y, like = _tail_inputs(kind, B, S, O, with_matrix)
    like_cpu = type(like)(**{**like.model_dump(), "obs_matrix": None if like.obs_matrix is None else like.obs_matrix.cpu()})
    g = torch.Generator().manual_seed(7)
    xd, yd = x.to(DEV), y.to(DEV)
    term = like.kernel_terms(yd)
    assert isinstance(term, tuple) and term[3].dtype == torch.float32 and tuple(term[3].shape) == (3,) and term[3].is_cuda
    # the floor binds on state row (0, 0): every rate there is the floor
    lam00 = _like64(like_cpu).predict(x[0, 0].double())
    assert bool((lam00 == 1e-6).all())
    w = torch.tensor([1.0, 0.5, -2.0, 0.5, 3.0, -1.5])
    worst_v = worst_g = 0.0
    for prior_type, tpos in THETA_VARIANTS:
        prior = Prior(type=PriorType.LOG_NORMAL if prior_type == "log_normal" else PriorType.NORMAL, mean=0.2, std=1.3, dim=P)
        th = torch.rand(B, P, generator=g) * 0.8 + 0.1
        mean, log_std = torch.randn(P, generator=g) * 0.3, torch.randn(P, generator=g) * 0.2 - 0.5
        paths = [torch.randn(B, generator=g) * 3.0 for _ in range(3)]
        args = (xd, yd, like.obs_matrix, term, th.to(DEV), 1 if prior_type == "log_normal" else 0, 0.2, 1.3, mean.to(DEV),
                log_std.to(DEV), tpos)
        out = _hip.elbo_tail_fwd(*args, *[p.to(DEV) for p in paths])
        got = _hip.elbo_tail_bwd(*args, w.to(DEV))
        want_out, want = _tail_reference(x, y, like_cpu, th, prior, mean, log_std, tpos, paths, w)
        for a, b_ in zip(out.double().cpu().tolist(), want_out.tolist()):
            worst_v = max(worst_v, abs(a - b_) / max(1.0, abs(b_)))
        for a, b_ in zip(got[:4], want):
            worst_g = max(worst_g, rel_err(a.double().cpu().numpy(), b_.numpy()))
        assert torch.equal(got[0][0, 0], torch.zeros(S, device=DEV)), got[0][0, 0]      # floored: exactly no gradient
        assert bool((got[0][1:].abs().sum(-1) > 0).all())
        ib = 1.0 / B
        for t, c in zip(got[4:], ((w[0] + w[2]) * ib, (w[3] - w[0]) * ib, w[0] * ib)):
            assert torch.allclose(t, torch.full((B,), float(c), device=DEV), rtol=1e-6, atol=0.0)
    print(f"{kind} B={B} S={S} O={O}: values {worst_v:.2e} (bound 2e-5), gradients {worst_g:.2e} (bound 1e-5)")
    assert worst_v <= 2e-5 and worst_g <= 1e-5


def test_the_training_elbo_takes_the_count_tail(monkeypatch):
    """``compute_evidence_lower_bound`` with a count likelihood: the one-kernel tail (not ``tail_log_terms``), values and gradients
    equal to the torch composition's."""
    from viforsdes_amd import Observations, Prior, PriorType, _hip
    from viforsdes_amd.examples.sdes import LotkaVolterra
    from viforsdes_amd.inference import evidence_lower_bound as em
    from viforsdes_amd.inference.state_space import StateSpace
    from viforsdes_amd.inference.types import DiffusionPathSample
    from viforsdes_amd.models.sde_parameter_posterior import SDEParameterPosterior
    B, T, S, P, dt = 37, 30, 2, 3, 0.1
    g = torch.Generator().manual_seed(11)
    rn = lambda *s: torch.randn(*s, generator=g)
    obs = Observations(times=torch.tensor([0.0, 0.9, 1.0, 2.5, 3.0, 7.0]).to(DEV),
                       values=torch.tensor([[1.0, 2.0], [0.0, 3.0], [2.0, 1.0], [4.0, 0.0], [1.0, 1.0], [3.0, 2.0]]).to(DEV))
    post = SDEParameterPosterior(P, [0, 1, 2]).to(DEV)
    prior = Prior(type=PriorType.LOG_NORMAL, mean=0.2, std=1.3, dim=P)
    base = dict(z=rn(B, T + 1, S).cumsum(1) * 0.1 + 1.0, means=rn(B, T, S) * 0.3,
                chol=torch.tril(rn(B, T, S, S) * 0.2, -1) + torch.diag_embed(torch.rand(B, T, S, generator=g) + 0.5),
                theta=torch.rand(B, P, generator=g) * 0.8 + 0.1)
    calls = []
    real = _hip.elbo_tail_fwd
    monkeypatch.setattr(_hip, "elbo_tail_fwd", lambda *a, **k: (calls.append(a[3]), real(*a, **k))[1])
    for kind in ("poisson", "negbin"):
        like = _like(kind, 1.3)
        results = {}
        for fused in (True, False):
            monkeypatch.setattr(em, "HIP_TAIL", fused)
            leaves = {k: v.clone().to(DEV).requires_grad_(True) for k, v in base.items()}
            sample = DiffusionPathSample(z=leaves["z"], transition_means=leaves["means"], transition_cholesky=leaves["chol"],
                                         state_space=StateSpace(S, [0, 1]))
            res = em.compute_evidence_lower_bound(LotkaVolterra(), obs, like, prior, post, leaves["theta"], sample, dt)
            c = res.components
            vals = [res.evidence_lower_bound, c.observation_log_prob, c.prior_log_prob, c.posterior_log_prob]
            grads = torch.autograd.grad(res.evidence_lower_bound, list(leaves.values()) + [post.mean, post.log_std])
            results[fused] = ([float(v) for v in vals], [t.double().cpu().numpy() for t in grads])
        for a, b_ in zip(results[True][0], results[False][0]):
            assert abs(a - b_) <= 2e-5 * max(1.0, abs(b_))
        for a, b_ in zip(results[True][1], results[False][1]):
            assert rel_err(a, b_) < 1e-5
    assert len(calls) == 2 and all(isinstance(v, tuple) for v in calls)


# ------------------------------------------------------------------------------------------------------------------ 2. log weights
TOL = 1e-5   # tests/test_evidence_gpu.py


def _lw_case(name):
    """(sde, obs, likelihood, prior, theta positive dims, state positive dims, dt, x0): T = 12 steps, kinds 1, 2 and 4."""
    from viforsdes_amd import Observations, Prior, PriorType
    from viforsdes_amd.examples.sdes import LotkaVolterra, OrnsteinUhlenbeck
    if name == "ou":        # kind 1: the state is not positive; the rate is 6 x, floored where a path goes below zero
        obs = Observations(times=torch.tensor([0.0, 0.2, 0.3, 0.6]), values=torch.tensor([[12.0], [9.0], [0.0], [7.0]]))
        return (OrnsteinUhlenbeck(), obs, _like("poisson", 6.0), Prior(type=PriorType.NORMAL, mean=0.0, std=1.0, dim=3), [0, 2], [],
                0.05, torch.tensor([2.0]))
    if name == "lv":        # kind 2, negative binomial through H (prey; prey + predators)
        obs = Observations(times=torch.tensor([0.0, 0.4, 0.4, 1.2]),
                           values=torch.tensor([[71.0, 150.0], [80.0, 160.0], [77.0, 1000.0], [95.0, 0.0]]))
        return (LotkaVolterra(), obs, _like("negbin", 1.0, torch.tensor([[1.0, 0.0], [1.0, 1.0]], device=DEV)),
                Prior(type=PriorType.LOG_NORMAL, mean=0.0, std=1.5, dim=3), [0, 1, 2], [0, 1], 0.1, torch.tensor([71.0, 79.0]))
    if name == "sir":       # kind 4, mass action
        obs = Observations(times=torch.tensor([0.0, 0.4, 0.8, 1.2]), values=torch.tensor([[95.0, 5.0], [93.0, 6.0], [92.0, 0.0], [90.0, 8.0]]))
        return (_sir(), obs, _like("poisson"), Prior(type=PriorType.LOG_NORMAL, mean=-3.0, std=2.0, dim=2), [0, 1], [0, 1], 0.1,
                torch.tensor([95.0, 5.0]))
    assert name == "autoreg"   # kind 4 with a Hill rate law
    obs = Observations(times=torch.tensor([0.0, 0.5, 1.2]), values=torch.tensor([[5.0, 20.0], [8.0, 22.0], [9.0, 25.0]]))
    return (_autoreg(), obs, _like("negbin", 0.8), Prior(type=PriorType.LOG_NORMAL, mean=0.0, std=2.0, dim=4), [0, 1, 2, 3], [0, 1],
            0.1, torch.tensor([5.0, 20.0]))


def _mvn_tril(y, mu, L):
    w = torch.linalg.solve_triangular(L, (y - mu).unsqueeze(-1), upper=False).squeeze(-1)
    return -0.5 * (w * w).sum(-1) - torch.log(torch.diagonal(L, dim1=-2, dim2=-1)).sum(-1) - 0.5 * y.shape[-1] * math.log(2 * math.pi)


@pytest.mark.parametrize("name", ["ou", "lv", "sir", "autoreg"])
def test_per_sample_log_weights_match_float64_composition(name, monkeypatch):
    from viforsdes_amd import _hip
    from viforsdes_amd.core.observations import grid_index
    from viforsdes_amd.inference.evidence import importance_log_weights
    from viforsdes_amd.inference.state_space import StateSpace
    from viforsdes_amd.inference.types import DiffusionPathSample
    from viforsdes_amd.models.sde_parameter_posterior import SDEParameterPosterior
    sde, obs, like, prior, tpos, spos, dt, x0 = _lw_case(name)
    T, B, S, P = 12, 70, sde.state_dim, sde.sde_param_dim
    g = torch.Generator().manual_seed(5)
    post = SDEParameterPosterior(P, tpos)
    with torch.no_grad():
        post.mean.copy_(torch.randn(P, generator=g) * 0.3 + (torch.tensor([-5.5, -1.9]) if name == "sir" else 0.0))
        post.log_std.copy_(torch.randn(P, generator=g) * 0.2 - 1.0)
    theta = post.rsample(B, eps=torch.randn(B, P, generator=g))
    space = StateSpace(S, spos)
    scale = 3.0 if spos else 1.0
    means = torch.randn(B, T, S, generator=g) * scale
    chol = torch.tril(torch.randn(B, T, S, S, generator=g) * 0.3 * scale, -1) + torch.diag_embed(
        torch.exp(torch.randn(B, T, S, generator=g) * 0.3) * scale)
    eps = torch.randn(B, T, S, generator=g)
    z = torch.empty(B, T + 1, S)
    z[:, 0] = space.to_latent(x0.unsqueeze(0)).expand(B, S)
    for t in range(T):
        z[:, t + 1] = z[:, t] + means[:, t] * dt + math.sqrt(dt) * (chol[:, t] @ eps[:, t].unsqueeze(-1)).squeeze(-1)
    to = lambda t: t.to(DEV)
    sample = DiffusionPathSample(z=to(z), transition_means=to(means), transition_cholesky=to(chol), state_space=space)
    obs, post, theta = obs.to(DEV), post.to(DEV), to(theta)
    calls = []
    real = _hip.log_weights
    monkeypatch.setattr(_hip, "log_weights", lambda *a, **k: (calls.append(a[10]), real(*a, **k))[1])
    got = importance_log_weights(sde, obs, like, prior, post, theta, sample, dt)
    assert len(calls) == 1 and isinstance(calls[0], tuple)                    # the kernel route, with the count term
    with torch.no_grad():
        zd = sample.z.double()
        x = zd.clone()
        if spos:
            x[..., spos] = F.softplus(zd[..., spos])
        th = theta.double()
        xf, thf = x[:, :-1].reshape(-1, S), th.unsqueeze(1).expand(B, T, -1).reshape(-1, P)
        f, G = sde.drift(xf, thf).reshape(B, T, S), sde.diffusion(xf, thf).reshape(B, T, S, S)
        sq = math.sqrt(dt)
        comps = dict(sde=_mvn_tril(x[:, 1:], x[:, :-1] + f * dt, G * sq).sum(-1),
                     gen=_mvn_tril(zd[:, 1:], zd[:, :-1] + sample.transition_means.double() * dt,
                                   sample.transition_cholesky.double() * sq).sum(-1),
                     jac=F.logsigmoid(zd[:, 1:, spos]).sum((-1, -2)) if spos else torch.zeros(B, dtype=torch.float64, device=DEV))
        idx = grid_index(obs.times, dt, T)
        comps["obs"] = _like64(like).log_prob(obs.values.double().unsqueeze(0).expand(B, -1, -1), x[:, idx]).sum(-1)
        comps["prior"] = prior.log_prob(th)
        comps["post"] = post.double().log_prob(th)
        post.float()
        want = comps["obs"] + comps["sde"] - comps["gen"] + comps["jac"] + comps["prior"] - comps["post"]
    assert got.shape == (B,) and got.dtype == torch.float32 and bool(torch.isfinite(want).all())
    size = max(float(c.abs().max()) for c in comps.values())
    err = float((got.double() - want).abs().max())
    print(f"{name}: max |log w - ref| = {err:.3e}, largest component {size:.3e}, ratio {err / size:.2e} (bound {TOL:g})")
    assert err <= TOL * size, (err, size)


# ------------------------------------------------------------------------------------------------------- 3. filter, stage by stage
def _pf_case(name, M=64):
    """(sde, observations, likelihood (H on the CPU), theta [M, P], x0 [M, S], dt, positive dims) on the CPU."""
    from viforsdes_amd import Observations
    from viforsdes_amd.examples.sdes import LinearDiagonalSDE, LotkaVolterra, OrnsteinUhlenbeck
    g = torch.Generator().manual_seed(29)
    jitter = lambda base, rel: torch.tensor(base) * (1.0 + rel * (2.0 * torch.rand(M, len(base), generator=g) - 1.0))
    both = torch.tensor([[1.0, 0.0], [1.0, 1.0]])        # the first species; the sum of both
    if name == "ou":           # kind 1: rate 1.5 * 2 x around a mean level of 10 (a 1-dim state has no room for an offset: the OU mean
        # is the offset); x stays far above zero
        obs = Observations(times=torch.tensor([0.0, 0.5, 1.0, 1.0, 2.0]), values=torch.tensor([[31.0], [27.0], [33.0], [30.0], [24.0]]))
        return (OrnsteinUhlenbeck(), obs, _like("poisson", 1.5, torch.tensor([[2.0]])), jitter([0.8, 10.0, 0.5], 0.1),
                torch.full((M, 1), 10.0), 0.05, ())
    if name == "lindiag16":    # kind 3 at S = 16 with a [4, 16] H of positive entries on states that stay positive
        S, O = 16, 4
        H = 0.2 + torch.rand(O, S, generator=g)
        th = torch.cat([0.2 + 0.3 * torch.rand(M, S, generator=g), -2.0 + 0.3 * torch.randn(M, S, generator=g)], 1)
        x0 = 1.0 + torch.rand(M, S, generator=g)
        pos = (0, 3, 9, 15)
        x0[:, pos] = x0[:, pos] * 0.01
        obs = Observations(times=torch.tensor([0.0, 0.5, 1.0, 2.0]),
                           values=torch.tensor([[13.0, 15.0, 9.0, 14.0], [10.0, 8.0, 12.0, 11.0], [9.0, 9.0, 6.0, 10.0], [7.0, 0.0, 5.0, 8.0]]))
        return LinearDiagonalSDE(S), obs, _like("poisson", 1.0, H), th, x0, 0.05, pos
    if name == "sir":          # Poisson on (S, S + I); in every 4th filter hardly anyone is infected and the infection rate is below the
        # removal rate: I dies out and sits at the floor, S stays where it is (every particle misses the data alike)
        obs = Observations(times=torch.tensor(SIR_TIMES), values=torch.tensor(SIR_VALUES) @ both.T)
        x0 = torch.tensor(SIR_VALUES[0]).expand(M, 2).clone()
        th = jitter([0.004, 0.15], 0.1)
        x0[::4, 1], th[::4, 0] = 1e-3, 5e-4
        return _sir(), obs, _like("poisson", 1.0, both), th, x0, 0.1, (0, 1)
    if name == "autoreg":      # negative binomial on (P, P + M); every 4th filter starts with hardly any mRNA: the first Euler step
        # (drift 0.7, noise 0.85) sends a tenth of its particles below zero, and the observation one step in sees them at the floor
        obs = Observations(times=torch.tensor([0.0, 0.1, 5.0, 10.0, 15.0, 20.0]),
                           values=torch.tensor([[20.0, 25.0], [20.0, 26.0], [44.0, 64.0], [65.0, 83.0], [71.0, 85.0], [70.0, 82.0]]))
        x0 = torch.tensor([5.0, 20.0]).expand(M, 2).clone()
        x0[::4, 0] = 0.3
        return (_autoreg(), obs, _like("negbin", 1.0, torch.tensor([[0.0, 1.0], [1.0, 1.0]])), jitter([20.0, 0.5, 0.1, 15.0], 0.1), x0,
                0.1, (0, 1))
    assert name == "lv"        # negative binomial on (prey, prey + predators) at grid rows 0, 1, 3, 3, 8, 20; every 4th filter starts
    # without predators: they sit at the floor
    obs = Observations(times=torch.tensor([0.0, 0.1, 0.3, 0.3, 0.8, 2.0]),
                       values=torch.tensor([[71.0, 150.0], [73.0, 151.0], [78.0, 158.0], [76.0, 153.0], [89.0, 172.0], [128.0, 221.0]]))
    x0 = torch.tensor([71.0, 79.0]).expand(M, 2).clone()
    x0[::4, 1] = 1e-3
    return LotkaVolterra(), obs, _like("negbin", 1.0, both), jitter([0.5, 0.0025, 0.3], 0.03), x0, 0.1, (0, 1)


def _on_device(like):
    return type(like)(**{**like.model_dump(), "obs_matrix": None if like.obs_matrix is None else like.obs_matrix.to(DEV)})


PF_CASES = ["ou", "lindiag16", "sir", "autoreg", "lv"]
PF_SIZES = [64, 1024]
_RUNS = {}


def _cached(name, N):
    if (name, N) not in _RUNS:
        from viforsdes_amd import _hip, particle_filter
        from viforsdes_amd.core.sde import builtin_sde_route
        from viforsdes_amd.inference import particle_filter as pf
        sde, obs, like, th, x0, dt, pos = _pf_case(name)
        assert N <= _hip.particle_filter_max_particles(builtin_sde_route(sde)[0], sde.state_dim)      # 1024: the route's maximum
        calls = []
        real = _hip.particle_filter
        _hip.particle_filter = lambda *a, **k: (calls.append(a[6]), real(*a, **k))[1]
        try:
            key = (0x9E3779B9 ^ N, 0x7F4A7C15 + len(name))
            res = particle_filter(sde, obs.to(DEV), _on_device(like), th.to(DEV), dt, n_particles=N, initial_state=x0.to(DEV),
                                  positive_dims=pos, return_particles=True, key=_key(*key))
        finally:
            _hip.particle_filter = real
        assert len(calls) == 1 and isinstance(calls[0], tuple) and pf.HIP_FILTER          # the kernel route, with the count term
        _RUNS[(name, N)] = (sde, obs, like, th, x0, dt, pos, res, key)
    return _RUNS[(name, N)]


def _log_weights(like, y, parts):
    H = None if like.obs_matrix is None else like.obs_matrix.double().numpy()
    return cref.count_log_weights(y, parts, getattr(like, "dispersion", None), like.scale, H)


@pytest.mark.parametrize("N", PF_SIZES)
@pytest.mark.parametrize("name", PF_CASES)
def test_weights_and_summaries_match_float64_on_the_kernels_particles(name, N):
    sde, obs, like, th, x0, dt, pos, res, key = _cached(name, N)
    M, K = th.shape[0], obs.values.shape[0]
    parts = res.particles.double().cpu().numpy()
    assert np.isfinite(parts).all() and tuple(res.log_weights.shape) == (M, K, N)
    assert torch.equal(res.particles[:, 0].cpu(), x0[:, None, :].expand(M, N, -1))
    got = [t.double().cpu().numpy() for t in (res.increments, res.effective_sample_size, res.filtered_mean, res.filtered_std)]
    e_inc = e_ess = e_mean = e_std = 0.0
    for m in range(M):
        for k in range(K):
            lw = _log_weights(like, obs.values[k].numpy(), parts[m, k])
            inc, ess, mean, std, w = ref.observation_stage(lw, parts[m, k])
            size = (w[:, None] * np.abs(parts[m, k])).sum(axis=0) / w.sum()          # weighted mean of |x|, per dim
            e_inc = max(e_inc, abs(got[0][m, k] - inc) / max(1.0, np.abs(lw[np.isfinite(lw)]).max()))
            e_ess = max(e_ess, abs(got[1][m, k] - ess) / ess)
            e_mean = max(e_mean, float((np.abs(got[2][m, k] - mean) / np.maximum(size, 1e-30)).max()))
            e_std = max(e_std, float((np.abs(got[3][m, k] - std) / (std + 1e-2 * size + 1e-30)).max()))
    print(f"{name} N={N}: increments {e_inc:.2e} (of max(1, |lw|), bound 1e-5), ESS {e_ess:.2e}, mean {e_mean:.2e}, std {e_std:.2e} "
          f"(relative, bound 1e-4)")
    assert e_inc <= 1e-5
    assert e_ess <= 1e-4 and e_mean <= 1e-4 and e_std <= 1e-4
    total = res.increments.double().sum(dim=1)
    assert torch.allclose(res.log_likelihood.double(), total, rtol=1e-6, atol=1e-5 * float(res.increments.abs().max()))
    if pos:
        assert bool((res.particles[..., list(pos)] >= FLOOR).all())
        assert bool((res.particles[:, 1:] == FLOOR).any())                            # the clamp was exercised


@pytest.mark.parametrize("N", PF_SIZES)
@pytest.mark.parametrize("name", PF_CASES)
def test_ancestors_match_float64_systematic_resampling(name, N):
    sde, obs, like, th, x0, dt, pos, res, key = _cached(name, N)
    M, K = th.shape[0], obs.values.shape[0]
    parts = res.particles.double().cpu().numpy()
    anc = res.ancestors.cpu().numpy().astype(np.int64)
    assert anc.min() >= 0 and anc.max() < N
    assert (np.diff(anc, axis=-1) >= 0).all()
    u = ref.resampling_uniforms(M, K, key)
    differ, low = 0, float("inf")
    for m in range(M):
        for k in range(K):
            lw = _log_weights(like, obs.values[k].numpy(), parts[m, k])
            w = np.exp(lw - lw.max())
            low = min(low, w.sum() ** 2 / (w * w).sum())
            d = np.abs(anc[m, k] - ref.systematic_ancestors(w, u[m, k]))
            assert d.max() <= 1, (m, k, int(d.max()))
            differ += int((d != 0).sum())
    print(f"{name} N={N}: {differ} of {anc.size} ancestors differ from float64 ({differ / anc.size:.1e}); smallest float64 ESS {low:.1f}")
    assert low >= N / 20                                                           # there was something to compare
    assert differ <= 1e-3 * anc.size


# ---------------------------------------------------------------------------------------------------------------------- 4. route
def test_route_conditions():
    from viforsdes_amd import Observations, _hip
    from viforsdes_amd.examples.sdes import LinearDiagonalSDE
    from viforsdes_amd.inference import particle_filter as pf
    sde, obs, like, th, x0, dt, pos = _pf_case("sir", 4)
    obs_d, th_d = obs.to(DEV), th.to(DEV)
    for kind in ("poisson", "negbin"):
        lk = _like(kind, 1.0, like.obs_matrix.to(DEV))
        route = pf._kernel_route(sde, obs_d, lk, th_d, 64)
        assert route is not None and route[0] == "reaction_network"
        assert pf._kernel_route(sde, obs_d, lk, th_d, 64, "bridge") is None
        assert pf._kernel_route(sde, obs_d, lk, th_d.double(), 64) is None                                  # fp64
        assert pf._kernel_route(sde, obs_d, lk, th_d, 1088) is None and pf._kernel_route(sde, obs_d, lk, th_d, 2048) is None

        class Sub(type(lk)):
            pass
        sub = Sub(**lk.model_dump())
        assert pf._kernel_route(sde, obs_d, sub, th_d, 64) is None                                          # a subclass
    wide = LinearDiagonalSDE(2)
    obs17 = Observations(times=torch.tensor([0.0, 1.0]), values=torch.ones(2, 17)).to(DEV)
    lk17 = _like("poisson", 1.0, torch.ones(17, 2, device=DEV))
    assert pf._kernel_route(wide, obs17, lk17, torch.zeros(4, 4, device=DEV), 64) is None                   # O > 16
    assert _hip.particle_filter_max_particles("reaction_network", 2) == 1024


def test_above_the_routes_maximum_the_torch_route_runs(monkeypatch):
    from viforsdes_amd import _hip, particle_filter
    sde, obs, like, th, x0, dt, pos = _pf_case("ou", 2)
    calls = []
    real = _hip.particle_filter
    monkeypatch.setattr(_hip, "particle_filter", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    obs2 = type(obs)(times=obs.times[:2], values=obs.values[:2]).to(DEV)
    res = particle_filter(sde, obs2, _on_device(like), th.to(DEV), dt, n_particles=1088, initial_state=x0.to(DEV), key=_key(1, 2))
    assert calls == [] and bool(torch.isfinite(res.log_likelihood).all())
    res = particle_filter(sde, obs2, _on_device(like), th.to(DEV), dt, n_particles=1024, initial_state=x0.to(DEV), key=_key(1, 2))
    assert calls == [1] and bool(torch.isfinite(res.log_likelihood).all())


def test_kernel_route_and_torch_route_agree_on_poisson_sir(monkeypatch):
    from viforsdes_amd import particle_filter
    from viforsdes_amd.inference import particle_filter as pf
    M, N = 4096, 64
    sde, obs, like, th, x0, dt, pos = _pf_case("sir", M)
    th, x0 = th[1:2].expand(M, 2).contiguous(), x0[1:2].expand(M, 2).contiguous()
    lk = _on_device(like)
    run = lambda k: particle_filter(sde, obs.to(DEV), lk, th.to(DEV), dt, n_particles=N, initial_state=x0.to(DEV),
                                    positive_dims=pos, key=_key(*k)).log_likelihood.double().cpu().numpy()
    a = run((31, 32))
    monkeypatch.setattr(pf, "HIP_FILTER", False)
    b = run((33, 34))
    z = abs(a.mean() - b.mean()) / math.sqrt(a.var(ddof=1) / M + b.var(ddof=1) / M)
    print(f"Poisson SIR: mean log p^ kernel {a.mean():.4f}, torch {b.mean():.4f}, two-sample z {z:.2f}")
    assert np.isfinite(a).all() and np.isfinite(b).all() and z < 4.0


def test_bad_count_arguments_are_refused():
    from viforsdes_amd import _hip
    sde, obs, like, th, x0, dt, pos = _pf_case("ou", 4)
    th, x0, values, H = th.to(DEV), x0.to(DEV), obs.values.to(DEV), like.obs_matrix.to(DEV)
    rows = torch.round(obs.times / dt).to(torch.int32).to(DEV)
    const = like.kernel_terms(values)[3]
    call = lambda term, N=64: _hip.particle_filter("ornstein_uhlenbeck", x0, th, rows, values, H, term, _key(1, 2), dt, N, ())
    assert call((1, 1.5, 1.0, const))[0].shape == (4,)
    for term, match in (((3, 1.0, 1.0, const), "count likelihood"), ((1, 0.0, 1.0, const), "scale"), ((2, 1.0, 0.0, const), "dispersion"),
                        ((1, 1.0, 1.0, const[:2]), "row constants")):
        with pytest.raises(ValueError, match=match):
            call(term)
    with pytest.raises(ValueError, match="particles"):
        call((1, 1.5, 1.0, const), N=100)
    with pytest.raises(ValueError, match="Gaussian"):
        _hip.guided_particle_filter("ornstein_uhlenbeck", x0, th, rows, values, H, (1, 1.5, 1.0, const), _key(1, 2), dt, 64, ())
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------------------------------------------- 5. end to end
def test_sir_with_a_poisson_likelihood_end_to_end():
    """The smallest SIR fit of tests/test_reaction_network_gpu.py with a Poisson likelihood on the README's counts: ``infer``,
    ``reweight_parameters``, ``log_evidence`` and ``predict``."""
    from viforsdes_amd import (EncoderConfig, HeadConfig, InferenceConfig, Observations, PretrainConfig, Prior, PriorType,
                               TrainingConfig, infer)
    from viforsdes_amd.console import Console
    sde = _sir()
    horizon, dt = 20.0, 0.1
    obs = Observations(times=torch.tensor(SIR_TIMES), values=torch.tensor(SIR_VALUES))
    like = _like("poisson")
    prior = Prior(type=PriorType.LOG_NORMAL, mean=-3.0, std=2.0, dim=2)
    cfg = InferenceConfig(training=TrainingConfig(time_step=dt, batch_size=32, n_iterations=24),
                          encoder=EncoderConfig(hidden_dim=32, cond_dim=32, num_heads=4, depth=1),
                          head=HeadConfig(hidden_dim=32, num_layers=1), state_positive_dims=[0, 1], sde_param_positive_dims=[0, 1],
                          pretrain=PretrainConfig(n_iterations=30, batch_size=512), console=Console(enabled=False), seed=5)
    post = infer(sde, obs, like, prior, horizon, cfg)
    hist = post.evidence_lower_bound_history
    assert len(hist) == 24 and all(np.isfinite(hist))
    torch.manual_seed(3)
    rw = post.reweight_parameters(sde, like, n_samples=256, n_particles=128, chunk_size=128)
    assert math.isfinite(rw.log_evidence) and rw.sde_parameters.shape == (256, 2) and bool(torch.isfinite(rw.mean).all())
    ev = post.log_evidence(sde, like, n_samples=256, chunk_size=128)
    assert math.isfinite(ev.log_evidence) and ev.n_nonfinite == 0
    pred = post.predict(sde, [horizon, horizon + 2.0], n_samples=128, chunk_size=64, observation_likelihood=like)
    y = pred.observations
    assert y.shape == (128, 2, 2) and bool((y >= 0).all()) and bool((y == y.round()).all())
    nb = _like("negbin")
    assert math.isfinite(post.log_evidence(sde, nb, n_samples=128, chunk_size=128).log_evidence)
