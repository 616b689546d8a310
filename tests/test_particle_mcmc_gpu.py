"""GPU: the Metropolis step kernel (csrc/vsde_mcmc.hip) through ``_hip.pmmh_step``, the kernel route of ``particle_mcmc`` and
``VariationalPosterior.refine_parameters`` on the device.

* The step kernel alone, per element against the float64 numpy step of tests/particle_mcmc_reference.py on given inputs (chain
  counts around the 64-thread workgroup, P = 1 / 3 / 16, R = 1 / 3, both priors, every mask, iterations 0 / 1 / 7; NaN and -inf
  estimates, a current target of -inf): proposals, theta', prior + Jacobian and the carried state within 1e-5 max(1, largest
  magnitude of the quantity), the bound the filter tests hold log-weight increments to; the filter key and the R copies of theta'
  bit-exact; decisions equal to float64 wherever ``|log alpha - log_u|`` exceeds that tolerance, at most 1 % of a case's chains
  undecidable; the counter incremented by exactly the accepted chains; rows that are not asked for are not written.
* Argument errors, the kernel route against the torch route under one key (without and with warm-up windows), exactness
  against ``exact_mh`` on the discretised OU model (bootstrap R = 1 / 2 and the bridge), a rate-law network and a
  Poisson-observed network on the kernel route, and ``refine_parameters`` after a short fit."""
import itertools
import math

import numpy as np
import pytest
import torch

import particle_mcmc_reference as ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _key(k0, k1, dev=DEV):
    return torch.from_numpy(np.array([k0, k1], dtype=np.uint32).view(np.int32)).to(dev)


# -------------------------------------------------------------------------------------------------------- 1. the step kernel alone
SENTINEL = -12345.0


def _launch(case, rows="all"):
    """The kernel on a ``kernel_case``: dict of numpy float64 / integer outputs."""
    from viforsdes_amd import _hip
    C, P, R = case["C"], case["P"], case["R"]
    f = lambda a: torch.tensor(np.asarray(a, dtype=np.float32), device=DEV).contiguous()
    t = dict(cur_u=f(case["cur_u"]), cur_log_target=f(case["cur_log_target"]), cur_loglik=f(case["cur_loglik"]), prop_u=f(case["prop_u"]),
             prop_log_prior=f(case["prop_log_prior"]), theta_prop=torch.full((C * R, P), SENTINEL, device=DEV),
             filter_key=torch.zeros(2, dtype=torch.int32, device=DEV), n_accept=torch.full((C,), 5, dtype=torch.int32, device=DEV),
             sample_row=torch.full((C, P), SENTINEL, device=DEV), loglik_row=torch.full((C,), SENTINEL, device=DEV),
             target_row=torch.full((C,), SENTINEL, device=DEV))
    loglik = None if case["loglik_prop"] is None else f(case["loglik_prop"])
    given = {"all": ("sample_row", "loglik_row", "target_row"), "none": (), "sample": ("sample_row",)}[rows]
    _hip.pmmh_step(case["iteration"], torch.tensor(case["L"]), case["step_size"], *case["prior"],
                   [int(i) for i in np.nonzero(case["mask"])[0]], _key(*case["key"]), loglik, t["cur_u"], t["cur_log_target"], t["cur_loglik"],
                   t["prop_u"], t["prop_log_prior"], t["theta_prop"], t["filter_key"], t["n_accept"],
                   **{k: t[k] for k in given})
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in t.items()}


def _err(got, want, rows=None):
    """Largest |got - want| over the finite entries of ``want`` (rows: the chains to compare); non-finite entries must be equal."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if rows is not None:
        got, want = got[rows], want[rows]
    fin = np.isfinite(want)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)])
    return float(np.abs(got[fin] - want[fin]).max()) if fin.any() else 0.0


WORST = {}


@pytest.mark.parametrize("P", ref.KERNEL_CASE_GRID["P"])
@pytest.mark.parametrize("C", ref.KERNEL_CASE_GRID["C"])
def test_step_kernel_matches_float64_per_element(C, P):
    g = ref.KERNEL_CASE_GRID
    worst = dict(prop_u=0.0, theta_prop=0.0, prop_log_prior=0.0, cur_u=0.0, cur_log_target=0.0, cur_loglik=0.0, sample_row=0.0)
    undecidable = 0
    for R, pt, mask, it in itertools.product(g["R"], g["prior_type"], g["mask"], g["iteration"]):
        case = ref.kernel_case(C, P, R, pt, mask, it)
        want, got = ref.kernel_case_reference(case), _launch(case)
        assert np.array_equal(got["filter_key"].view(np.uint32), want["filter_key"])
        copies = got["theta_prop"].reshape(C, R, P)
        assert np.array_equal(copies.view(np.uint32), np.broadcast_to(copies[:, :1], (C, R, P)).view(np.uint32))
        same = np.ones(C, dtype=bool)                                     # chains whose decision is float64's
        if it == 0:
            assert np.array_equal(got["n_accept"], np.full(C, 5))         # nothing closed: state, counter and rows untouched
            for k in ("cur_u", "cur_log_target", "cur_loglik", "prop_u"):
                assert np.array_equal(got[k], np.asarray(case[k], dtype=np.float32), equal_nan=True), k
            assert (got["sample_row"] == SENTINEL).all() and (got["loglik_row"] == SENTINEL).all() and (got["target_row"] == SENTINEL).all()
        else:
            acc = got["n_accept"] - 5
            assert set(np.unique(acc)) <= {0, 1}
            acc = acc.astype(bool)
            tol = ref.tolerance(want["prop_target"], case["cur_log_target"])
            with np.errstate(invalid="ignore"):
                margin = np.abs(want["log_alpha"] - want["log_u"])
            decidable = ~(margin <= tol)                                  # NaN and infinite margins are decided by the rule itself
            assert np.array_equal(acc[decidable], want["accept"][decidable])
            same = acc == want["accept"]
            assert (~decidable).sum() <= 0.01 * C
            undecidable += int((~decidable).sum())
            # the carried state is the proposal's where the kernel accepted, the old one elsewhere: exactly
            moved = np.where(acc[:, None], np.asarray(case["prop_u"], dtype=np.float32), np.asarray(case["cur_u"], dtype=np.float32))
            assert np.array_equal(got["cur_u"], moved)
            for k in ("cur_u", "cur_log_target", "cur_loglik"):
                e = _err(got[k], want[k], same)
                assert e <= ref.tolerance(want[k]), (k, R, pt, mask, it, e)
                worst[k] = max(worst[k], e / ref.tolerance(want[k]))
            assert np.array_equal(got["loglik_row"], got["cur_loglik"], equal_nan=True) and np.array_equal(got["target_row"], got["cur_log_target"], equal_nan=True)
            e = _err(got["sample_row"], want["sample_row"], same)
            assert e <= ref.tolerance(want["sample_row"])
            worst["sample_row"] = max(worst["sample_row"], e / ref.tolerance(want["sample_row"]))
        for k in ("prop_u", "theta_prop", "prop_log_prior"):
            rows = np.repeat(same, R) if k == "theta_prop" else same
            e = _err(got[k], want[k], rows)
            assert e <= ref.tolerance(want[k]), (k, R, pt, mask, it, e)
            worst[k] = max(worst[k], e / ref.tolerance(want[k]))
    WORST[(C, P)] = worst
    print(f"C = {C}, P = {P}: largest error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()) + f"; undecidable chains {undecidable}")


@pytest.mark.parametrize("rows", ["none", "sample"])
def test_rows_not_asked_for_are_not_written(rows):
    case = ref.kernel_case(65, 3, 3, 1, "some", 7)
    full, part = _launch(case), _launch(case, rows)
    for k in ("cur_u", "cur_log_target", "cur_loglik", "prop_u", "prop_log_prior", "theta_prop", "filter_key", "n_accept"):
        assert np.array_equal(full[k], part[k], equal_nan=True), k
    assert (part["loglik_row"] == SENTINEL).all() and (part["target_row"] == SENTINEL).all()
    if rows == "none":
        assert (part["sample_row"] == SENTINEL).all()
    else:
        assert np.array_equal(part["sample_row"], full["sample_row"])


def test_bad_arguments_are_refused():
    from viforsdes_amd import _hip
    f32 = dict(device=DEV, dtype=torch.float32)

    def call(C=5, P=3, R=2, L=None, iteration=1, **kw):
        a = dict(loglik_prop=torch.zeros(C, R, **f32), cur_u=torch.zeros(C, P, **f32), cur_log_target=torch.zeros(C, **f32),
                 cur_loglik=torch.zeros(C, **f32), prop_u=torch.zeros(C, P, **f32), prop_log_prior=torch.zeros(C, **f32),
                 theta_prop=torch.zeros(C * R, P, **f32), filter_key=torch.zeros(2, device=DEV, dtype=torch.int32),
                 n_accept=torch.zeros(C, device=DEV, dtype=torch.int32))
        a.update(kw)
        prior = a.pop("prior", (0, 0.0, 1.0))
        step = a.pop("step_size", 0.5)
        _hip.pmmh_step(iteration, torch.eye(P) if L is None else L, step, *prior, (0,), _key(1, 2), a.pop("loglik_prop"), a.pop("cur_u"),
                       a.pop("cur_log_target"), a.pop("cur_loglik"), a.pop("prop_u"), a.pop("prop_log_prior"), a.pop("theta_prop"),
                       a.pop("filter_key"), a.pop("n_accept"))

    call()
    upper = torch.eye(3)
    upper[0, 1] = 0.25
    for kw in (dict(P=17), dict(C=0), dict(R=0), dict(cur_u=None), dict(cur_log_target=None), dict(n_accept=None), dict(L=upper),
               dict(L=torch.diag(torch.tensor([1.0, 0.0, 1.0]))), dict(L=torch.eye(3) * float("nan")), dict(iteration=-1),
               dict(iteration=0), dict(step_size=0.0), dict(prior=(2, 0.0, 1.0)), dict(prior=(0, 0.0, 0.0))):
        with pytest.raises(ValueError):
            call(**kw)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------- 2. kernel route against torch route
def _ou(dtype=torch.float32):
    from viforsdes_amd import GaussianObservationLikelihood, Observations, Prior, PriorType
    from viforsdes_amd.examples.sdes import OrnsteinUhlenbeck
    obs = Observations(times=torch.tensor(ref.OU_TIMES, dtype=dtype), values=torch.tensor(ref.OU_VALUES, dtype=dtype)[:, None]).to(DEV)
    prior = Prior(type=PriorType.LOG_NORMAL, mean=ref.OU_PRIOR[1], std=ref.OU_PRIOR[2], dim=3)
    return OrnsteinUhlenbeck(), obs, GaussianObservationLikelihood(variance=ref.OU_VARIANCE), prior


def _counted(monkeypatch):
    from viforsdes_amd import _hip
    calls, real = [], _hip.pmmh_step

    def counting(iteration, *a, **kw):
        calls.append(iteration)
        return real(iteration, *a, **kw)

    monkeypatch.setattr(_hip, "pmmh_step", counting)
    return calls


def test_kernel_route_matches_torch_route(monkeypatch):
    from viforsdes_amd import particle_mcmc
    import viforsdes_amd.inference.particle_mcmc as mc
    sde, obs, like, prior = _ou()
    C, key = 65, (0x5EED, 0xFACE)
    theta0 = torch.tensor(ref.ou_initial_theta(C), dtype=torch.float32, device=DEV)
    run = lambda trace: particle_mcmc(sde, obs, like, prior, ref.OU_DT, theta0, 5, n_particles=64, theta_positive_dims=(0, 1, 2),
                                      key=_key(*key), _trace=trace)
    calls, kernel, torch_ = _counted(monkeypatch), [], []
    res_k = run(kernel)
    assert calls == [0, 1, 2, 3, 4, 5]                                    # the route taken is the kernel's: n + 1 launches, no warm-up
    monkeypatch.setattr(mc, "HIP_MCMC", False)
    res_t = run(torch_)
    assert calls == [0, 1, 2, 3, 4, 5] and len(kernel) == len(torch_) == 5
    agree = np.ones(C, dtype=bool)                                        # chains whose decision histories agree so far
    worst = 0.0
    for i, (a, b) in enumerate(zip(kernel, torch_)):
        for k in ("prop_u", "prop_log_prior"):
            x, y = a[k].cpu().numpy().astype(np.float64)[agree], b[k].cpu().numpy().astype(np.float64)[agree]
            e = np.abs(x - y).max()
            assert e <= ref.tolerance(y), (i, k, e)
            worst = max(worst, e / ref.tolerance(y))
        assert torch.equal(a["filter_key"], b["filter_key"])
        da, db = a["accept"].cpu().numpy(), b["accept"].cpu().numpy()
        differ = agree & (da != db)
        if differ.any():                                                  # a decision may differ only at a near tie
            ll = ref.log_mean_exp(b["loglik"].cpu().numpy())
            target = b["prop_log_prior"].cpu().numpy().astype(np.float64) + ll
            before = torch_[i - 1]["cur_log_target"].cpu().numpy().astype(np.float64)
            margin = np.abs(target - before - ref.acceptance_log_uniforms(C, i, key))
            assert (margin[differ] <= ref.tolerance(target, before)).all(), (i, margin[differ])
        agree &= da == db
    print(f"kernel route vs torch route: largest proposal error / bound {worst:.3f}, {int(agree.sum())} of {C} histories agree to the end")
    assert agree.sum() >= 0.9 * C
    assert res_k.samples.shape == res_t.samples.shape == (5, C, 3)


def test_warmup_adapts_alike_on_both_routes(monkeypatch):
    """The kernel route closes iteration i - 1 in the launch that opens iteration i, so an adaptation before iteration i opens it
    again with the new step size / L: step sizes, L and proposals must follow the torch route's through the warm-up windows."""
    from viforsdes_amd import particle_mcmc
    import viforsdes_amd.inference.particle_mcmc as mc
    sde, obs, like, prior = _ou()
    C = 65
    theta0 = torch.tensor(ref.ou_initial_theta(C), dtype=torch.float32, device=DEV)
    run = lambda trace: particle_mcmc(sde, obs, like, prior, ref.OU_DT, theta0, 12, warmup=8, adapt_interval=2, n_particles=64,
                                      theta_positive_dims=(0, 1, 2), key=_key(0xC0FFEE, 77), _trace=trace)
    calls, kernel, torch_ = _counted(monkeypatch), [], []
    res_k = run(kernel)
    assert calls == [0, 1, 2, 2, 3, 4, 4, 5, 6, 6, 7, 8, 8, 9, 10, 11, 12]     # windows end before 2, 4, 6, 8; L changes at 4
    monkeypatch.setattr(mc, "HIP_MCMC", False)
    res_t = run(torch_)
    compared = 0
    for i, (a, b) in enumerate(zip(kernel, torch_)):
        assert a["step_size"] == pytest.approx(b["step_size"], rel=1e-12), i
        la, lb = a["scale_tril"].cpu().double().numpy(), b["scale_tril"].cpu().double().numpy()
        assert np.abs(la - lb).max() <= ref.tolerance(lb), i
        x, y = a["prop_u"].cpu().double().numpy(), b["prop_u"].cpu().double().numpy()
        assert np.abs(x - y).max() <= ref.tolerance(y), i
        compared += 1
        if not torch.equal(a["accept"], b["accept"]):                     # a near tie decided differently: the windows part ways
            break
    print(f"warm-up on both routes: {compared} of 12 iterations compared, step sizes {[round(t['step_size'], 4) for t in kernel]}")
    assert compared >= 5 and not torch.equal(kernel[3]["scale_tril"], kernel[4]["scale_tril"])
    assert kernel[8]["step_size"] == kernel[-1]["step_size"] == res_k.step_size and res_t.samples.shape == res_k.samples.shape == (4, C, 3)


# ------------------------------------------------------------------------------------------------------ 3. exactness on the device
@pytest.mark.parametrize("R,N,proposal", [(1, 64, "bootstrap"), (2, 64, "bootstrap"), (1, 64, "bridge")])
def test_ou_posterior_matches_exact_metropolis_hastings(R, N, proposal, monkeypatch):
    from viforsdes_amd import particle_mcmc
    import viforsdes_amd.inference.particle_mcmc as mc
    sde, obs, like, prior = _ou()
    C, n, w = 256, 400, 150
    exact = ref.ou_exact_chains(C, n, w)
    calls = _counted(monkeypatch)
    theta0 = torch.tensor(ref.ou_initial_theta(C), dtype=torch.float32, device=DEV)
    res = particle_mcmc(sde, obs, like, prior, ref.OU_DT, theta0, n, warmup=w, n_particles=N, filters_per_chain=R,
                        theta_positive_dims=(0, 1, 2), proposal=proposal, key=_key(0xABCDEF, 5 + R))
    assert len(calls) >= n + 1                                            # the kernel route (plus one re-opening per adaptation)
    u = res.samples.log().double().cpu().numpy()
    z = ref.two_sample_z(u, exact)
    r_exact, _ = mc.split_r_hat_and_ess(torch.tensor(exact))
    print(f"{proposal}, R = {R}, N = {N}: z = {z.round(2).tolist()}, R^ {res.r_hat.cpu().numpy().round(3).tolist()} (exact chain "
          f"{r_exact.numpy().round(3).tolist()}), acceptance {float(res.acceptance_rate.mean()):.3f}, ESS "
          f"{res.effective_sample_size.cpu().numpy().round(0).tolist()}, step {res.step_size:.3f}, dead {res.n_filters_dead}")
    assert z.max() <= 4.5
    assert float(res.r_hat.max()) <= 1.1 and float(r_exact.max()) <= 1.1
    assert res.samples.is_cuda and res.samples.shape == (n - w, C, 3) and res.acceptance_rate.shape == (C,)
    assert bool(torch.isfinite(res.log_target).all())


# ------------------------------------------------------------------------------------------- 4. reaction networks, count data
AUTOREG = dict(reactants=[[0, 0], [1, 0], [1, 0], [0, 1]], products=[[1, 0], [1, 1], [0, 0], [0, 0]], species=["M", "P"],
               reactions=["transcription", "translation", "mRNA decay", "protein decay"], rate_constants=["k_tx", "k_tl", 0.1, "d_P"])


def _network_case(name):
    from viforsdes_amd import GaussianObservationLikelihood, Hill, Observations, PoissonObservationLikelihood, Prior, PriorType, ReactionNetworkSDE
    import reaction_networks as nets
    g = torch.Generator().manual_seed(17)
    if name == "autoreg":                                                 # rate laws: the kernel_theta map runs between the launches
        sde = ReactionNetworkSDE(**AUTOREG, rate_laws={"transcription": Hill("P", K="K", n=2, repression=True)})
        obs = Observations(times=torch.tensor([0.0, 0.5, 1.2]), values=torch.tensor([[5.0, 20.0], [8.0, 22.0], [9.0, 25.0]]))
        base, like = torch.tensor([40.0, 1.0, 0.1, 10.0]), GaussianObservationLikelihood(variance=9.0)
        prior = Prior(type=PriorType.LOG_NORMAL, mean=0.0, std=2.0, dim=4)
    else:                                                                 # SIR, Poisson-observed
        sde = ReactionNetworkSDE(**nets.SIR, species=["S", "I"], reactions=["infection", "removal"])
        obs = Observations(times=torch.tensor([0.0, 0.4, 0.8, 1.2]), values=torch.tensor([[95.0, 5.0], [93.0, 6.0], [92.0, 7.0], [90.0, 8.0]]))
        base, like = torch.tensor([0.004, 0.15]), PoissonObservationLikelihood()
        prior = Prior(type=PriorType.LOG_NORMAL, mean=-3.0, std=2.0, dim=2)
    theta0 = base * torch.exp(0.2 * torch.randn(64, base.numel(), generator=g))
    return sde, obs.to(DEV), like, prior, theta0.to(DEV)


@pytest.mark.parametrize("name", ["autoreg", "sir"])
def test_reaction_networks_run_on_the_kernel_route(name, monkeypatch):
    from viforsdes_amd import particle_mcmc
    sde, obs, like, prior, theta0 = _network_case(name)
    P = theta0.shape[1]
    calls, trace = _counted(monkeypatch), []
    res = particle_mcmc(sde, obs, like, prior, 0.1, theta0, 20, n_particles=64, theta_positive_dims=tuple(range(P)), positive_dims=(0, 1),
                        key=_key(3, 4), _trace=trace)
    assert calls == list(range(21))
    rate = float(res.acceptance_rate.mean())
    print(f"{name}: acceptance {rate:.3f}, dead {res.n_filters_dead}, mean {res.mean.tolist()}")
    assert bool(torch.isfinite(res.log_target).all()) and bool(torch.isfinite(res.log_likelihood).all())
    assert 0.0 < rate < 1.0
    assert all(bool((t["theta_prop"] > 0).all()) for t in trace) and bool((res.samples > 0).all())
    assert res.samples.shape == (20, 64, P)


# --------------------------------------------------------------------------------------------------------- 5. refine_parameters
def test_refine_parameters_after_a_short_fit(monkeypatch):
    from viforsdes_amd import (EncoderConfig, GaussianObservationLikelihood, HeadConfig, InferenceConfig, ParticleMCMCResult, Prior,
                               PriorType, TrainingConfig, infer)
    from viforsdes_amd.console import Console
    from viforsdes_amd.examples.sdes import ou_problem
    sde, obs, _, _, horizon, dt, _, _ = ou_problem()
    like = GaussianObservationLikelihood(variance=0.5)                  # the fit of tests/test_particle_filter_gpu.py, 200 iterations
    prior = Prior(type=PriorType.LOG_NORMAL, mean=0.0, std=0.5, dim=3)
    cfg = InferenceConfig(training=TrainingConfig(time_step=dt, batch_size=256, n_iterations=200, learning_rate=2e-3,
                                                  sde_param_lr=2e-2),
                          encoder=EncoderConfig(hidden_dim=32, cond_dim=32, num_heads=4, depth=1),
                          head=HeadConfig(hidden_dim=32, num_layers=1), sde_param_positive_dims=[0, 1, 2],
                          mixed_precision=False, console=Console(enabled=False), seed=1)
    vp = infer(sde, obs, like, prior, horizon, cfg)
    calls = _counted(monkeypatch)
    torch.manual_seed(5)
    res = vp.refine_parameters(sde, like, n_chains=128, n_iterations=120, warmup=60, n_particles=64)
    assert vp._captured == {} and vp._calls == {}
    assert len(calls) >= 121 and isinstance(res, ParticleMCMCResult)
    print(f"refine_parameters: mean {res.mean.tolist()} +- {res.mean_standard_error.tolist()} (q: {res.variational_mean.tolist()}), "
          f"R^ {res.r_hat.tolist()}, acceptance {float(res.acceptance_rate.mean()):.3f}, dead {res.n_filters_dead}")
    assert res.samples.is_cuda and res.samples.shape == (60, 128, 3)
    for t in (res.acceptance_rate, res.r_hat, res.mean, res.variational_mean, res.variational_std, res.mean_standard_error):
        assert bool(torch.isfinite(t).all())
    assert isinstance(res.n_filters_dead, int) and res.n_filters_dead >= 0
