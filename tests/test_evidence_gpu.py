"""GPU: importance log-weights and the log-evidence estimate (inference/evidence.py, csrc/vsde_elbo.hip: log_weight_kernel,
log_weight_accumulate_kernel, VariationalPosterior.log_evidence).

Per-sample parity against a float64 torch composition of the ELBO integrand on the same draws: bound 1e-5 of the largest
per-sample component (fp32 rounding of a T-term sum).  Observed on an MI355X: at most 2.5e-7 of it."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TOL = 1e-5


class LaplaceLikelihood:
    """Not a closed form the fused kernels know: takes the torch fallback."""

    def __init__(self, scale):
        self.scale = scale

    def log_prob(self, observations, state):
        return (-(observations - state).abs() / self.scale - math.log(2.0 * self.scale)).sum(dim=-1)


def _functional_sde():
    from viforsdes_amd import make_sde

    def drift(x, th):
        return th[..., :3] * (1.0 - x)

    def diffusion(x, th):
        d = torch.diag_embed(F.softplus(th[..., 3:6]) + 0.1 + 0.05 * x.abs())
        off = torch.zeros_like(d)
        off[..., 1, 0] = 0.2 * th[..., 0]
        off[..., 2, 1] = -0.1 * x[..., 0]
        return d + off
    return make_sde(drift, diffusion, 3, 6)


def _case(name):
    """(sde, obs, likelihood, prior, theta positive dims, state positive dims, dt, T, B, x0)."""
    from viforsdes_amd import GaussianObservationLikelihood, Observations, Prior, PriorType
    from viforsdes_amd.examples.sdes import LinearDiagonalSDE, LotkaVolterra, OrnsteinUhlenbeck
    g = torch.Generator().manual_seed(11)
    if name in ("ou", "ou_laplace"):
        obs = Observations(times=torch.tensor([0.0, 1.0, 2.5, 5.0]), values=torch.tensor([[2.0], [1.5], [0.8], [1.1]]))
        like = GaussianObservationLikelihood(variance=0.1) if name == "ou" else LaplaceLikelihood(0.3)
        return (OrnsteinUhlenbeck(), obs, like, Prior(type=PriorType.NORMAL, mean=0.0, std=1.0, dim=3), [0, 2], [], 0.05, 100, 300,
                torch.tensor([2.0]))
    if name == "lv":
        obs = Observations(times=torch.tensor([0.0, 10.0, 20.0, 40.0]),
                           values=torch.tensor([[71.0, 79.0], [47.6, 447.2], [80.5, 50.3], [158.1, 66.8]]))
        return (LotkaVolterra(), obs, GaussianObservationLikelihood(variance=1.0),
                Prior(type=PriorType.LOG_NORMAL, mean=0.0, std=1.5, dim=3), [0, 1, 2], [0, 1], 0.1, 400, 257,
                torch.tensor([71.0, 79.0]))
    if name == "lindiag":   # T = 1, obs_matrix [3, 8]
        obs = Observations(times=torch.tensor([0.0, 0.01]), values=torch.randn(2, 3, generator=g))
        H = torch.randn(3, 8, generator=g) * 0.5
        return (LinearDiagonalSDE(8), obs, GaussianObservationLikelihood(variance=0.25, obs_matrix=H),
                Prior(type=PriorType.NORMAL, mean=0.0, std=1.0, dim=16), [], [], 0.01, 1, 100, torch.randn(8, generator=g))
    if name == "functional":   # kind 0: S = 3, obs_matrix [2, 3], a positive state dim, LogNormal prior
        obs = Observations(times=torch.tensor([0.0, 0.5, 1.0, 2.0]), values=torch.rand(4, 2, generator=g) + 0.5)
        H = torch.tensor([[1.0, 0.0, 0.5], [0.0, 1.0, -0.5]])
        return (_functional_sde(), obs, GaussianObservationLikelihood(variance=0.2, obs_matrix=H),
                Prior(type=PriorType.LOG_NORMAL, mean=0.0, std=0.5, dim=6), list(range(6)), [1], 0.02, 100, 513,
                torch.tensor([0.8, 1.2, 0.6]))
    raise KeyError(name)


def _draws(name, clamp_paths=False):
    """Posterior theta from injected eps and paths generated the head's way from injected noise:
    z_{t+1} = z_t + m_t dt + sqrt(dt) L_t eps_t, with random transition means m and lower-triangular factors L."""
    from viforsdes_amd.inference.state_space import StateSpace
    from viforsdes_amd.inference.types import DiffusionPathSample
    from viforsdes_amd.models.sde_parameter_posterior import SDEParameterPosterior
    sde, obs, like, prior, tpos, spos, dt, T, B, x0 = _case(name)
    S, P = sde.state_dim, sde.sde_param_dim
    g = torch.Generator().manual_seed(5)
    post = SDEParameterPosterior(P, tpos)
    with torch.no_grad():
        post.mean.copy_(torch.randn(P, generator=g) * 0.3)
        post.log_std.copy_(torch.randn(P, generator=g) * 0.2 - 1.0)
    theta = post.rsample(B, eps=torch.randn(B, P, generator=g))
    space = StateSpace(S, spos)
    scale = 10.0 if name == "lv" else 1.0
    means = torch.randn(B, T, S, generator=g) * scale
    chol = torch.tril(torch.randn(B, T, S, S, generator=g) * 0.3 * scale, -1) + torch.diag_embed(
        torch.exp(torch.randn(B, T, S, generator=g) * 0.3) * scale)
    eps = torch.randn(B, T, S, generator=g)
    z = torch.empty(B, T + 1, S)
    z[:, 0] = space.to_latent(x0.unsqueeze(0)).expand(B, S)
    if clamp_paths:   # LV: prey near extinction on a third of the paths (softplus(-30) ~ 1e-13): the 1e-6 clamps engage
        z[: B // 3, 0, 0] = -30.0
        means[: B // 3, :, 0] = 0.0
        chol[: B // 3, :, 0, 0] = 1e-3
    for t in range(T):
        z[:, t + 1] = z[:, t] + means[:, t] * dt + math.sqrt(dt) * (chol[:, t] @ eps[:, t].unsqueeze(-1)).squeeze(-1)
    to = lambda t: t.to(DEV)
    sample = DiffusionPathSample(z=to(z), transition_means=to(means), transition_cholesky=to(chol), state_space=space)
    obs_d = obs.to(DEV)
    return sde, obs_d, like, prior, post.to(DEV), to(theta), sample, dt


def _mvn_tril(y, mu, L):
    """log N(y; mu, L L^T), float64, L lower triangular."""
    w = torch.linalg.solve_triangular(L, (y - mu).unsqueeze(-1), upper=False).squeeze(-1)
    S = y.shape[-1]
    return -0.5 * (w * w).sum(-1) - torch.log(torch.diagonal(L, dim1=-2, dim2=-1)).sum(-1) - 0.5 * S * math.log(2 * math.pi)


@torch.no_grad()
def _reference(sde, obs, like, prior, post, theta, sample, dt):
    """Per-sample components of the ELBO integrand in float64 torch: (log w, {component: [B]})."""
    from viforsdes_amd.core.observations import grid_index
    z = sample.z.double()
    B, T1, S = z.shape
    pos = sample.state_space.positive_dims
    x = z.clone()
    if pos:
        x[..., pos] = F.softplus(z[..., pos])
    th = theta.double()
    xf, thf = x[:, :-1].reshape(-1, S), th.unsqueeze(1).expand(B, T1 - 1, -1).reshape(-1, th.shape[-1])
    f = sde.drift(xf, thf).reshape(B, T1 - 1, S)
    G = sde.diffusion(xf, thf).reshape(B, T1 - 1, S, S)
    sq = math.sqrt(dt)
    sde_lp = _mvn_tril(x[:, 1:], x[:, :-1] + f * dt, G * sq).sum(-1)
    gen_lp = _mvn_tril(z[:, 1:], z[:, :-1] + sample.transition_means.double() * dt,
                       sample.transition_cholesky.double() * sq).sum(-1)
    jac = F.logsigmoid(z[:, 1:, pos]).sum((-1, -2)) if pos else torch.zeros(B, dtype=torch.float64, device=z.device)
    idx = grid_index(obs.times, dt, T1 - 1)
    if hasattr(like, "obs_matrix") and like.obs_matrix is not None:
        like = type(like)(variance=like.variance, obs_matrix=like.obs_matrix.double())
    obs_lp = like.log_prob(obs.values.double().unsqueeze(0).expand(B, -1, -1), x[:, idx]).sum(-1)
    prior_lp = prior.log_prob(th)
    post_lp = post.double().log_prob(th)
    post.float()
    comps = dict(obs=obs_lp, sde=sde_lp, gen=gen_lp, jac=jac, prior=prior_lp, post=post_lp)
    return obs_lp + sde_lp - gen_lp + jac + prior_lp - post_lp, comps


@pytest.mark.parametrize("name", ["ou", "lv", "lindiag", "functional", "ou_laplace"])
def test_per_sample_log_weights_match_float64_composition(name):
    from viforsdes_amd.inference.evidence import importance_log_weights
    sde, obs, like, prior, post, theta, sample, dt = _draws(name, clamp_paths=(name == "lv"))
    got = importance_log_weights(sde, obs, like, prior, post, theta, sample, dt)
    ref, comps = _reference(sde, obs, like, prior, post, theta, sample, dt)
    assert got.shape == (theta.shape[0],) and got.dtype == torch.float32
    assert torch.isfinite(ref).all()
    scale = max(float(c.abs().max()) for c in comps.values())
    err = float((got.double() - ref).abs().max())
    print(f"{name}: max |log w - ref| = {err:.3e}, largest component {scale:.3e}, ratio {err / scale:.2e}")
    assert err <= TOL * scale, (err, scale)


@pytest.mark.parametrize("name", ["ou", "lv", "functional"])
def test_mean_log_weight_is_the_elbo(name):
    from viforsdes_amd.inference.evidence import importance_log_weights
    from viforsdes_amd.inference.evidence_lower_bound import compute_evidence_lower_bound
    sde, obs, like, prior, post, theta, sample, dt = _draws(name)
    with torch.no_grad():
        lw = importance_log_weights(sde, obs, like, prior, post, theta, sample, dt)
        elbo = compute_evidence_lower_bound(sde, obs, like, prior, post, theta, sample, dt)
    _, comps = _reference(sde, obs, like, prior, post, theta, sample, dt)
    scale = max(float(c.abs().max()) for c in comps.values())
    assert abs(float(lw.double().mean()) - float(elbo.evidence_lower_bound)) <= TOL * scale


def _run_accumulator(buf, n, chunk):
    from viforsdes_amd import _hip
    state = _hip.log_weight_state(DEV)
    for c in range(0, n, chunk):
        _hip.log_weight_accumulate(buf[c:c + chunk], min(chunk, n - c), state)
    return state


def test_accumulator_against_float64_logsumexp_and_bitwise_repeatable():
    from viforsdes_amd import EvidenceEstimate
    g = torch.Generator().manual_seed(3)
    n, chunk = 10_000, 1024
    lw = torch.randn(n, generator=g, dtype=torch.float64) * 4.0 - 300.0
    lw[torch.randperm(n, generator=g)[:37]] = float("-inf")
    lw32 = lw.float()
    buf = torch.full((10 * chunk,), 50.0)          # the last chunk is partial: what lies beyond n must not count
    buf[:n] = lw32
    buf = buf.to(DEV)
    s1 = _run_accumulator(buf, n, chunk)
    s2 = _run_accumulator(buf, n, chunk)
    assert torch.equal(s1, s2)
    est = EvidenceEstimate.from_state(s1.tolist())
    ref = lw32.double()
    fin = ref[torch.isfinite(ref)]
    le = float(torch.logsumexp(ref, 0)) - math.log(n)
    w = torch.exp(fin - fin.max())
    ess = float(w.sum() ** 2 / (w * w).sum())
    assert est.n_samples == n and est.n_nonfinite == 0
    assert abs(est.log_evidence - le) < 1e-12 * abs(le)
    assert abs(est.effective_sample_size - ess) < 1e-10 * ess
    assert est.evidence_lower_bound == float("-inf")
    # NaN entries: counted, and the estimate is NaN
    buf2 = buf.clone()
    buf2[[3, 4000, 9999]] = float("nan")
    est2 = EvidenceEstimate.from_state(_run_accumulator(buf2, n, chunk).tolist())
    assert est2.n_nonfinite == 3 and est2.n_samples == n and math.isnan(est2.log_evidence)
    # finite weights only: mean log w is the ELBO on the same draws
    buf3 = buf.clone()
    buf3[:n] = torch.where(torch.isfinite(lw32), lw32, torch.tensor(-310.0)).to(DEV)
    est3 = EvidenceEstimate.from_state(_run_accumulator(buf3, n, chunk).tolist())
    assert abs(est3.evidence_lower_bound - float(buf3[:n].double().mean())) < 1e-9 * 300
    assert est3.log_evidence >= est3.evidence_lower_bound


def _fit_ou():
    from viforsdes_amd import (EncoderConfig, GaussianObservationLikelihood, HeadConfig, InferenceConfig, Prior, PriorType,
                               TrainingConfig, infer)
    from viforsdes_amd.console import Console
    from viforsdes_amd.examples.sdes import ou_problem
    sde, obs, _, _, horizon, dt, _, _ = ou_problem()
    # all theta positive: the supports of q and p match.  Observation noise 0.5 and prior width 0.5 keep the posterior one a
    # mean-field q covers (at variance 0.1 / width 1.0 the importance weights are heavy-tailed and the delta-method error is
    # optimistic); 6000 iterations let the EMA weights, which log_evidence uses, catch up with the fit.
    like = GaussianObservationLikelihood(variance=0.5)
    prior = Prior(type=PriorType.LOG_NORMAL, mean=0.0, std=0.5, dim=3)
    cfg = InferenceConfig(training=TrainingConfig(time_step=dt, batch_size=256, n_iterations=6000, learning_rate=2e-3,
                                                  sde_param_lr=2e-2),
                          encoder=EncoderConfig(hidden_dim=32, cond_dim=32, num_heads=4, depth=1),
                          head=HeadConfig(hidden_dim=32, num_layers=1), sde_param_positive_dims=[0, 1, 2],
                          mixed_precision=False, console=Console(enabled=False), seed=1)
    return sde, obs, like, prior, horizon, dt, infer(sde, obs, like, prior, horizon, cfg)


def _prior_predictive(sde, obs, like, prior, horizon, dt, n=2 ** 20, chunk=2 ** 18):
    """log p(y) = log E_{theta ~ prior, x ~ EM(theta) from x0 = y0} p(y | x), the HIP simulator, float64 weights."""
    from viforsdes_amd.core.euler_maruyama import euler_maruyama
    from viforsdes_amd.core.observations import grid_index
    g = torch.Generator(device=DEV).manual_seed(1234)
    values, times = obs.values.to(DEV), obs.times.to(DEV)
    T = round(horizon / dt)
    idx = grid_index(times, dt, T)
    lps = []
    for _ in range(n // chunk):
        theta = torch.exp(prior.mean + prior.std * torch.randn(chunk, 3, device=DEV, generator=g))
        noise = torch.randn(chunk, T, 1, device=DEV, generator=g)
        x = euler_maruyama(sde, values[0].expand(chunk, 1), theta, horizon, dt, (), noise=noise)
        lps.append(like.log_prob(values.double().unsqueeze(0).expand(chunk, -1, -1), x[:, idx].double()).sum(-1))
    lw = torch.nan_to_num(torch.cat(lps), nan=float("-inf"))   # a path that overflowed (large kappa draws) has zero likelihood
    m = lw.max()
    w = torch.exp(lw - m)
    ess = float(w.sum() ** 2 / (w * w).sum())
    return float(m + torch.log(w.sum()) - math.log(n)), math.sqrt(max(1.0 / ess - 1.0 / n, 0.0)), ess


def test_log_evidence_agrees_with_prior_predictive_estimate():
    sde, obs, like, prior, horizon, dt, vp = _fit_ou()
    n = 2 ** 15
    torch.manual_seed(77)
    est = vp.log_evidence(sde, like, n_samples=n, chunk_size=4096, return_log_weights=True)
    assert vp._captured == {} and vp._calls == {}        # sample()'s graph caches are untouched
    pp, pp_se, pp_ess = _prior_predictive(sde, obs, like, prior, horizon, dt)
    z = (est.log_evidence - pp) / math.hypot(est.standard_error, pp_se)
    print(f"log_evidence {est.log_evidence:.4f} +- {est.standard_error:.4f} (ESS {est.effective_sample_size:.0f} / {n}), "
          f"ELBO {est.evidence_lower_bound:.4f}; prior predictive {pp:.4f} +- {pp_se:.4f} (ESS {pp_ess:.0f}); z = {z:.2f}")
    assert est.n_samples == n and est.n_nonfinite == 0 and est.log_weights.shape == (n,)
    assert est.effective_sample_size / n > 0.3, est            # a broken fit cannot pass the comparison by luck
    assert 0.0 < est.effective_sample_size <= n
    assert est.log_evidence >= est.evidence_lower_bound
    assert abs(z) < 4.0, (z, est, pp, pp_se)
    torch.manual_seed(77)
    again = vp.log_evidence(sde, like, n_samples=n, chunk_size=4096)
    assert (again.log_evidence, again.effective_sample_size, again.evidence_lower_bound) == (
        est.log_evidence, est.effective_sample_size, est.evidence_lower_bound)
    # a partial last chunk and the eager-only single-chunk form give finite, consistent estimates too
    small = vp.log_evidence(sde, like, n_samples=1000, chunk_size=384, mixed_precision=True)
    assert small.n_samples == 1000 and abs(small.log_evidence - est.log_evidence) < 6.0 * max(small.standard_error, 0.05)
    one = vp.log_evidence(sde, like, n_samples=200, chunk_size=512)
    assert one.n_samples == 200 and math.isfinite(one.log_evidence)
