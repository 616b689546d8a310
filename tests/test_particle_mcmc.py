"""CPU: the torch route of ``particle_mcmc`` (the specification, float64) and ``VariationalPosterior.refine_parameters``.

* Every iteration of a short run against the float64 numpy step of tests/particle_mcmc_reference.py, given the run's own filter
  outputs: proposals, theta', prior + Jacobian, decisions and carried state within 1e-12 relative.
* Mechanics: keys, thinning, warm-up (nothing adapts after it), every ValueError.
* Exactness: with a synthetic unbiased estimator (exact log-likelihood + sigma eps - sigma^2 / 2, sigma = 1.5) on a correlated 2-D
  Gaussian target, 512 chains reproduce the known means and second moments within |z| <= 4.5 (the two-sided normal tail for about 10
  statistics at a false-alarm rate below 1e-4) -- and the same run with the current estimate refreshed every iteration, the classic
  PMMH bug, does not.
* End to end: the discretised OU model (40 steps, 5 observations) against ``exact_mh``, the same chain with the Kalman likelihood:
  two-sample |z| <= 4.5 per coordinate, split-R^ <= 1.1 for both.
* The reference's own helpers: the vectorised Kalman filter against ``ou_kalman``, and the near-tie share of the step-kernel test
  inputs (tests/test_particle_mcmc_gpu.py) below 0.1 %."""
import itertools
import math

import numpy as np
import pytest
import torch

import particle_filter_reference as pref
import particle_mcmc_reference as ref

F64 = torch.float64


def _key(k0, k1):
    return torch.from_numpy(np.array([k0, k1], dtype=np.uint32).view(np.int32))


def _ou(dtype=F64):
    from viforsdes_amd import GaussianObservationLikelihood, Observations, Prior, PriorType
    from viforsdes_amd.examples.sdes import OrnsteinUhlenbeck
    obs = Observations(times=torch.tensor(ref.OU_TIMES, dtype=dtype), values=torch.tensor(ref.OU_VALUES, dtype=dtype)[:, None])
    prior = Prior(type=PriorType.LOG_NORMAL, mean=ref.OU_PRIOR[1], std=ref.OU_PRIOR[2], dim=3)
    return OrnsteinUhlenbeck(), obs, GaussianObservationLikelihood(variance=ref.OU_VARIANCE), prior


def _close_to(a, b, rel=1e-12):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    fin = np.isfinite(b)
    assert np.array_equal(fin, np.isfinite(a)) and np.array_equal(np.isnan(a), np.isnan(b))
    assert np.array_equal(a[~fin & ~np.isnan(b)], b[~fin & ~np.isnan(b)])
    if fin.any():
        assert np.abs(a[fin] - b[fin]).max() <= rel * max(1.0, np.abs(b[fin]).max())


# ------------------------------------------------------------------------------------------------ 1. every iteration, per element
def _short_run(R, key=(7, 9), n_iterations=6, **kw):
    from viforsdes_amd import Prior, PriorType, particle_mcmc
    sde, obs, like, _ = _ou()
    prior = Prior(type=PriorType.NORMAL, mean=0.3, std=1.2, dim=3)
    g = torch.Generator().manual_seed(3)
    theta0 = torch.stack([0.8 + 0.2 * torch.randn(5, generator=g, dtype=F64), 1.0 + 0.3 * torch.randn(5, generator=g, dtype=F64),
                          torch.exp(-0.5 + 0.3 * torch.randn(5, generator=g, dtype=F64))], dim=1)
    trace = []
    res = particle_mcmc(sde, obs, like, prior, ref.OU_DT, theta0, n_iterations, n_particles=32, filters_per_chain=R,
                        theta_positive_dims=(2,), key=_key(*key), _trace=trace, **kw)
    return theta0, res, trace


@pytest.mark.parametrize("R", [1, 3])
def test_every_iteration_matches_the_numpy_step(R):
    theta0, res, trace = _short_run(R)
    assert len(trace) == 6 and res.samples.shape == (6, 5, 3) and res.samples.dtype == F64
    mask = np.array([False, False, True])
    u0 = np.where(mask, np.log(theta0.numpy()), theta0.numpy())
    cur_u, cur_t, cur_ll = u0.copy(), np.full(5, -np.inf), np.full(5, -np.inf)
    n_acc = np.zeros(5)
    for i, tr in enumerate(trace):
        L, step = tr["scale_tril"].numpy(), tr["step_size"]
        o = ref.open_step(i, (7, 9), cur_u, u0, L, step, mask, 0, 0.3, 1.2, R)
        _close_to(tr["prop_u"].numpy(), o["prop_u"])
        _close_to(tr["theta_prop"].numpy(), o["theta_prop"])
        _close_to(tr["prop_log_prior"].numpy(), o["prop_log_prior"])
        assert np.array_equal(tr["filter_key"].numpy().view(np.uint32), o["filter_key"])
        c = ref.close_step(i, (7, 9), tr["loglik"].numpy(), o["prop_u"], o["prop_log_prior"], cur_u, cur_t, cur_ll)
        assert np.array_equal(tr["accept"].numpy(), c["accept"])
        cur_u, cur_t, cur_ll = c["cur_u"], c["cur_log_target"], c["cur_loglik"]
        n_acc += c["accept"]
        _close_to(tr["cur_u"].numpy(), cur_u)
        _close_to(tr["cur_log_target"].numpy(), cur_t)
        _close_to(tr["cur_loglik"].numpy(), cur_ll)
        _close_to(res.samples[i].numpy(), ref.constrain(cur_u, mask))
        _close_to(res.log_likelihood[i].numpy(), cur_ll)
        _close_to(res.log_target[i].numpy(), cur_t)
    assert trace[0]["accept"].all()                                       # iteration 0 proposes initial_theta and takes it
    _close_to(trace[0]["prop_u"].numpy(), u0)
    _close_to(res.acceptance_rate.numpy(), n_acc / 6)
    _close_to(np.diag(trace[0]["scale_tril"].numpy()), np.maximum(u0.std(axis=0, ddof=1), 1e-3))
    assert trace[0]["step_size"] == 2.38 / math.sqrt(3)


def test_keys():
    _, a, ta = _short_run(1)
    _, b, tb = _short_run(1)
    _, c, tc = _short_run(1, key=(7, 10))
    for f in ("samples", "log_likelihood", "log_target", "acceptance_rate"):
        assert torch.equal(getattr(a, f), getattr(b, f)), f
    assert all(torch.equal(x["prop_u"], y["prop_u"]) for x, y in zip(ta, tb))
    assert all(not torch.equal(x["prop_u"], y["prop_u"]) for x, y in zip(ta[1:], tc[1:]))


def test_thinning_warmup_and_no_adaptation_after_warmup():
    _, res, trace = _short_run(1, n_iterations=30, warmup=12, thin=4, adapt_interval=3)
    kept = list(range(12, 30, 4))
    assert res.samples.shape == (len(kept), 5, 3)
    for k, i in enumerate(kept):
        assert torch.equal(res.log_target[k], trace[i]["cur_log_target"]) and torch.equal(res.log_likelihood[k], trace[i]["cur_loglik"])
        u = torch.where(torch.tensor([False, False, True]), res.samples[k].log(), res.samples[k])
        assert torch.allclose(u, trace[i]["cur_u"], rtol=1e-14, atol=1e-14)
    steps = [t["step_size"] for t in trace]
    assert len(set(steps[:13])) > 2                                       # the step size moved in warm-up (windows of 3) ...
    assert len(set(steps[12:])) == 1 and res.step_size == steps[-1]       # ... and not after it
    assert not torch.equal(trace[5]["scale_tril"], trace[6]["scale_tril"])            # L re-estimated once, at warmup // 2 (C = 5 > P)
    assert all(torch.equal(t["scale_tril"], trace[6]["scale_tril"]) for t in trace[6:])
    assert all(torch.equal(t["scale_tril"], trace[0]["scale_tril"]) for t in trace[:6])
    assert torch.equal(res.proposal_scale_tril, trace[-1]["scale_tril"]) and steps[6] == 2.38 / math.sqrt(3)
    hist = np.concatenate([trace[i]["cur_u"].numpy() for i in range(3, 6)], axis=0)
    _close_to(trace[6]["scale_tril"].numpy(), ref.adapted_scale_tril(hist, None), rel=1e-9)
    acc = sum(t["accept"].sum().item() for t in trace[0:3]) / 15                      # the first window's pooled rate
    assert steps[3] == pytest.approx(steps[0] * math.exp(acc - 0.15), rel=1e-14)
    acc = torch.stack([t["accept"] for t in trace[12:]]).double().mean(dim=0)
    assert torch.allclose(res.acceptance_rate, acc)
    _, frozen, tr2 = _short_run(1, n_iterations=30, warmup=12, adapt=False, adapt_interval=3)
    assert all(torch.equal(t["scale_tril"], tr2[0]["scale_tril"]) for t in tr2)


def test_bad_arguments_are_refused():
    from viforsdes_amd import PoissonObservationLikelihood, particle_mcmc
    sde, obs, like, prior = _ou()
    th = torch.tensor(ref.ou_initial_theta(4))
    ok = dict(n_iterations=4, n_particles=8, theta_positive_dims=(0, 1, 2))
    run = lambda theta=th, **kw: particle_mcmc(sde, obs, like, prior, ref.OU_DT, theta, **{**ok, **kw})
    run()
    tril = torch.eye(3, dtype=F64)
    bad_upper, bad_diag = tril.clone(), tril.clone()
    bad_upper[0, 2], bad_diag[1, 1] = 0.1, 0.0
    for kw in (dict(theta=th[:, :2]), dict(theta=torch.zeros(0, 3, dtype=F64)), dict(n_particles=0), dict(initial_state=torch.zeros(2, dtype=F64)),
               dict(theta=th[:1].expand(2 ** 12, 3), n_particles=2 ** 20), dict(theta=th, filters_per_chain=2 ** 10, n_particles=2 ** 20),
               dict(thin=0), dict(adapt_interval=0), dict(filters_per_chain=0), dict(warmup=-1), dict(warmup=4), dict(n_iterations=0),
               dict(proposal_scale_tril=torch.eye(2, dtype=F64)), dict(proposal_scale_tril=bad_upper), dict(proposal_scale_tril=bad_diag),
               dict(theta=th * torch.tensor([1.0, -1.0, 1.0], dtype=F64)), dict(theta=th * torch.tensor([1.0, 0.0, 1.0], dtype=F64)),
               dict(theta_positive_dims=(3,)), dict(proposal="nope"), dict(step_size=0.0), dict(target_accept=1.0),
               dict(key=torch.tensor([1.0, 2.0])), dict(key=torch.tensor([1, 2, 3]))):
        with pytest.raises(ValueError):
            run(**kw)
    with pytest.raises(ValueError):                                       # proposal's own checks: the bridge needs a Gaussian term
        particle_mcmc(sde, obs, PoissonObservationLikelihood(), prior, ref.OU_DT, th, proposal="bridge", **ok)
    with pytest.raises(ValueError):
        particle_mcmc(sde, obs, like, prior, 0.0, th, **ok)


# -------------------------------------------------------------------------------------- 2. exactness with a synthetic estimator
MU, SIGMA = np.array([0.3, -0.5]), np.array([[0.5, 0.3], [0.3, 0.4]])
KNOWN = np.array([MU[0], MU[1], SIGMA[0, 0] + MU[0] ** 2, SIGMA[0, 1] + MU[0] * MU[1], SIGMA[1, 1] + MU[1] ** 2])


class _FlatInU:
    """log p(theta) that cancels the Jacobian of the positive dim: the target in u is the estimator's Gaussian alone."""

    def log_prob(self, theta):
        return -theta[:, 0].log()


def _gauss_loglik(theta):
    u = torch.stack([theta[:, 0].log(), theta[:, 1]], dim=1) - torch.tensor(MU, dtype=F64)
    return -0.5 * ((u @ torch.tensor(np.linalg.inv(SIGMA), dtype=F64)) * u).sum(dim=1)


def _synthetic_run(n_iterations, warmup, noise=1.5, seed=11):
    from viforsdes_amd import particle_mcmc
    from viforsdes_amd.examples.sdes import LinearDiagonalSDE
    rng = np.random.default_rng(seed)
    eps = lambda n: torch.tensor(rng.standard_normal(n)) * noise - 0.5 * noise * noise
    C = 512
    u0 = rng.multivariate_normal(MU, 2.0 * SIGMA, size=C)
    theta0 = torch.tensor(np.stack([np.exp(u0[:, 0]), u0[:, 1]], axis=1))
    from viforsdes_amd import GaussianObservationLikelihood, Observations
    obs = Observations(times=torch.tensor([0.0, 1.0], dtype=F64), values=torch.zeros(2, 1, dtype=F64))   # unused: the hook replaces the filter
    res = particle_mcmc(LinearDiagonalSDE(1), obs, GaussianObservationLikelihood(variance=1.0), _FlatInU(), 0.5, theta0, n_iterations,
                        warmup=warmup, n_particles=8, theta_positive_dims=(0,), key=_key(21, 22),
                        _estimator=lambda rows, i, fkey: _gauss_loglik(rows) + eps(rows.shape[0]))
    u = torch.stack([res.samples[..., 0].log(), res.samples[..., 1]], dim=-1).numpy()
    stats = np.stack([u[..., 0], u[..., 1], u[..., 0] ** 2, u[..., 0] * u[..., 1], u[..., 1] ** 2], axis=-1).mean(axis=0)   # [C, 5]
    z = (stats.mean(axis=0) - KNOWN) / (stats.std(axis=0, ddof=1) / math.sqrt(C))
    return res, z, eps


def test_chains_are_exact_with_a_noisy_unbiased_estimator_and_not_with_the_estimate_refreshed(monkeypatch):
    import viforsdes_amd.inference.particle_mcmc as mc
    n_iterations, warmup = 400, 150
    res, z, _ = _synthetic_run(n_iterations, warmup)
    print(f"carried estimate: z = {z.round(2).tolist()}, acceptance {float(res.acceptance_rate.mean()):.3f}, R^ {res.r_hat.tolist()}")
    assert np.abs(z).max() <= 4.5
    assert res.n_filters_dead == 0 and res.samples.shape == (n_iterations - warmup, 512, 2)

    # the classic bug: a fresh estimate of the CURRENT point at every iteration
    original, holder = mc._close, {}
    mask, prior = torch.tensor([True, False]), _FlatInU()

    def refreshed_close(iteration, key, loglik, prop_u, prop_lp, cur_u, cur_t, cur_ll):
        if iteration > 0:
            theta = mc.constrain(cur_u, mask)
            cur_ll = _gauss_loglik(theta) + holder["eps"](theta.shape[0])
            cur_t = mc._log_prior_jacobian(prior, theta, cur_u, mask) + cur_ll
        return original(iteration, key, loglik, prop_u, prop_lp, cur_u, cur_t, cur_ll)

    monkeypatch.setattr(mc, "_close", refreshed_close)
    rng = np.random.default_rng(12)
    holder["eps"] = lambda n: torch.tensor(rng.standard_normal(n)) * 1.5 - 0.5 * 1.5 * 1.5
    bad, z_bad, _ = _synthetic_run(n_iterations, warmup)
    print(f"refreshed estimate: z = {z_bad.round(2).tolist()}, acceptance {float(bad.acceptance_rate.mean()):.3f}")
    assert np.abs(z_bad).max() > 4.5


# ------------------------------------------------------------------------------------------ 3. end to end on the discretised OU
OU_RUN = dict(C=128, n_iterations=260, warmup=80)


@pytest.mark.parametrize("R,N", [(1, 64), (2, 32)])
def test_ou_posterior_matches_exact_metropolis_hastings(R, N):
    from viforsdes_amd import particle_mcmc
    import viforsdes_amd.inference.particle_mcmc as mc
    sde, obs, like, prior = _ou()
    C, n, w = OU_RUN["C"], OU_RUN["n_iterations"], OU_RUN["warmup"]
    exact = ref.ou_exact_chains(C, n, w)
    threads = torch.get_num_threads()
    torch.set_num_threads(1)                                              # thousands of tiny ops: threads only cost here
    try:
        res = particle_mcmc(sde, obs, like, prior, ref.OU_DT, torch.tensor(ref.ou_initial_theta(C)), n, warmup=w, n_particles=N,
                            filters_per_chain=R, theta_positive_dims=(0, 1, 2), key=_key(0xABCDEF, 5 + R))
    finally:
        torch.set_num_threads(threads)
    u = res.samples.log().numpy()
    z = ref.two_sample_z(u, exact)
    r_exact, _ = mc.split_r_hat_and_ess(torch.tensor(exact))
    print(f"R = {R}, N = {N}: z = {z.round(2).tolist()}, R^ {res.r_hat.numpy().round(3).tolist()} (exact chain "
          f"{r_exact.numpy().round(3).tolist()}), acceptance {float(res.acceptance_rate.mean()):.3f}, ESS {res.effective_sample_size.tolist()}, "
          f"mean {res.mean.tolist()} +- {res.mean_standard_error.tolist()}, dead {res.n_filters_dead}")
    assert z.max() <= 4.5
    assert float(res.r_hat.max()) <= 1.1 and float(r_exact.max()) <= 1.1
    assert res.samples.shape == (n - w, C, 3) and res.log_likelihood.shape == (n - w, C) and res.acceptance_rate.shape == (C,)
    assert bool(torch.isfinite(res.log_target).all()) and 0.0 < float(res.acceptance_rate.mean()) < 1.0
    flat = res.samples.reshape(-1, 3)
    assert torch.allclose(res.mean, flat.mean(dim=0)) and torch.allclose(res.std, flat.std(dim=0))
    assert torch.allclose(res.quantiles.q50, flat.quantile(0.5, dim=0))
    assert torch.allclose(res.mean_standard_error, res.samples.mean(dim=0).std(dim=0) / math.sqrt(C))


def test_diagnostics_against_direct_formulae():
    import viforsdes_amd.inference.particle_mcmc as mc
    rng = np.random.default_rng(4)
    n, C = 41, 6
    x = np.zeros((n, C, 2))
    for t in range(1, n):                                                 # AR(1) chains: rho = 0.7 and 0 (white noise)
        x[t] = np.array([0.7, 0.0]) * x[t - 1] + rng.standard_normal((C, 2))
    r_hat, ess = mc.split_r_hat_and_ess(torch.tensor(x))
    h = n // 2
    s = np.concatenate([x[:h], x[n - h:]], axis=1)                        # BDA3 11.4: split chains, m = 2 C of length h
    m = s.shape[1]
    W = s.var(axis=0, ddof=1).mean(axis=0)
    var_plus = (h - 1) / h * W + s.mean(axis=0).var(axis=0, ddof=1)
    _close_to(r_hat.numpy(), np.sqrt(var_plus / W), rel=1e-12)
    for p in range(2):
        rho = [1.0 - ((s[t:, :, p] - s[:h - t, :, p]) ** 2).sum() / (m * (h - t)) / (2.0 * var_plus[p]) for t in range(h)]
        T = next((T for T in range(1, h - 2, 2) if rho[T + 1] + rho[T + 2] < 0), None)
        T = T if T is not None else (h - 1 if (h - 1) % 2 == 1 else h - 2)
        _close_to(ess[p].numpy(), m * h / (1.0 + 2.0 * sum(rho[1:T + 1])), rel=1e-9)
    assert ess[1] > ess[0]
    nan_r, nan_e = mc.split_r_hat_and_ess(torch.tensor(x[:3]))
    assert bool(torch.isnan(nan_r).all()) and bool(torch.isnan(nan_e).all())


# ---------------------------------------------------------------------------------------------- 4. the reference's own helpers
def test_vectorised_kalman_matches_ou_kalman():
    thetas = np.array([[0.8, 1.0, 0.5], [1.5, 0.5, 1.0], [0.3, 2.0, 0.3], [2.5, -0.4, 0.05]])
    got = ref.ou_kalman_rows(thetas, ref.OU_DT, ref.OU_VARIANCE, ref.OU_VALUES[0], ref.OU_ROWS, ref.OU_VALUES)
    want = [pref.ou_kalman(t, ref.OU_DT, ref.OU_VARIANCE, np.array([ref.OU_VALUES[0]]), ref.OU_ROWS, np.array(ref.OU_VALUES)[:, None])
            for t in thetas]
    _close_to(got, want, rel=1e-12)


def test_near_ties_of_the_step_kernel_inputs_are_rare():
    g = ref.KERNEL_CASE_GRID
    near = total = 0
    for C, P, R, pt, mask, it in itertools.product(g["C"], g["P"], g["R"], g["prior_type"], g["mask"], (1, 7)):
        case = ref.kernel_case(C, P, R, pt, mask, it)
        out = ref.kernel_case_reference(case)
        tol = ref.tolerance(out["prop_target"], case["cur_log_target"])
        d = out["log_alpha"] - out["log_u"]
        near += int((np.abs(d[np.isfinite(d)]) <= tol).sum())
        total += C
    print(f"near ties: {near} of {total} chains")
    assert near < 1e-3 * total


# --------------------------------------------------------------------------------------------------------- 5. refine_parameters
def _cpu_posterior():
    from viforsdes_amd import EncoderConfig, HeadConfig
    from viforsdes_amd.examples.sdes import ou_problem
    from viforsdes_amd.inference.exponential_moving_average import ExponentialMovingAverage
    from viforsdes_amd.inference.state_space import StateSpace
    from viforsdes_amd.models.variational_sde_posterior import VariationalSDEPosterior
    from viforsdes_amd.posterior.variational_posterior import VariationalPosterior
    torch.manual_seed(0)
    sde, obs, like, prior, horizon, dt, _, theta_pos = ou_problem()
    model = VariationalSDEPosterior(obs.values.shape[1], 1, 3, EncoderConfig(hidden_dim=32, cond_dim=32, num_heads=4, depth=1),
                                    HeadConfig(hidden_dim=32, num_layers=1), theta_pos)
    with torch.no_grad():                                                 # q as a short fit would leave it: off the prior, narrow
        model.sde_parameter_posterior.mean.copy_(torch.tensor([-0.2, 1.0, -0.6]))
        model.sde_parameter_posterior.log_std.copy_(torch.tensor([-1.0, -1.2, -0.9]))
    vp = VariationalPosterior(model=model, exponential_moving_average=ExponentialMovingAverage(model), prior=prior,
                              observations=obs, time_horizon=horizon, time_step=dt, state_space=StateSpace(1, []),
                              evidence_lower_bound_history=[], device=torch.device("cpu"))
    return sde, like, vp


def test_refine_parameters_on_a_cpu_posterior():
    from viforsdes_amd import ParticleMCMCResult
    sde, like, vp = _cpu_posterior()
    torch.manual_seed(8)
    res = vp.refine_parameters(sde, like, n_chains=12, n_iterations=6, warmup=0, n_particles=16, thin=2)
    assert vp._captured == {} and vp._calls == {}
    q = vp.model.sde_parameter_posterior
    torch.manual_seed(8)
    with vp.exponential_moving_average.apply():
        draws = q.rsample(12)
    assert isinstance(res, ParticleMCMCResult) and res.samples.shape == (3, 12, 3) and res.samples.dtype == torch.float32
    assert torch.allclose(res.samples[0], draws, rtol=1e-5)              # iteration 0 takes the start point: the chains start at q draws
    assert torch.equal(res.variational_mean, draws.mean(dim=0)) and torch.equal(res.variational_std, draws.std(dim=0))
    assert torch.allclose(res.proposal_scale_tril, torch.diag(q.log_std.detach().exp()))
    assert res.log_likelihood.shape == (3, 12) and res.acceptance_rate.shape == (12,) and res.r_hat.shape == (3,)
    assert bool((res.samples[..., [0, 2]] > 0).all()) and isinstance(res.n_filters_dead, int)
    with pytest.raises(ValueError):
        vp.refine_parameters(sde, like, n_chains=0)
    with pytest.raises(ValueError):
        vp.refine_parameters(sde, like, proposal="nope")
