"""CPU: the torch specification of the jump-process particle smoother (viforsdes_amd/inference/jump_smoother.py) and of the
jump-process paths of particle MCMC (``particle_mcmc(..., dynamics="jump", return_paths=True, path_times=...)``):
``jump_segment_states`` against ``jump_segment`` bit for bit and against the independent numpy restatement
(tests/jump_smoother_reference.py) on decidable pairs, the smoother against its own filter, segment 0 against ``jump_process``, the
edge rules and argument checks, the PMMH wiring through ``_trace``, and both against the exact smoothing marginals of
immigration-death observed with Poisson noise (forward-backward on 200 states).  Every call runs with ``max_events <= 4096``."""
import math

import numpy as np
import pytest
import torch

import jump_filter_reference as fref
import jump_process_reference as jref
import jump_smoother_reference as ref
from reaction_networks import BD
from viforsdes_amd import (GaussianObservationLikelihood, Observations, PoissonObservationLikelihood, Prior, PriorType, ReactionNetworkSDE,
                           SmoothedJumpPaths, jump_particle_filter, jump_particle_smoother, jump_process, particle_mcmc)
from viforsdes_amd.core.jump_process import jump_segment, jump_segment_states
from viforsdes_amd.inference import particle_mcmc as mc

KEY = (2024, 78)
CASES = jref.cases()
F64 = torch.float64
TIMES = [0.0, 0.25, 0.25, 1.0]                                    # a zero and a duplicate
PATH_TIMES = [0.0, 0.1, 0.2, 0.25, 0.5, 0.75, 1.0]                # the observation times, two interior times per gap, one at 0
AT_OBS = [0, 3, 3, 6]                                             # q(T_k)


def _obs(times, values, dtype=F64):
    return Observations(times=torch.tensor(times, dtype=F64), values=torch.tensor(values, dtype=dtype))


# -------------------------------------------------------------------------------------------------- 1. jump_segment_states
@pytest.mark.parametrize("dtype", [F64, torch.float32])
@pytest.mark.parametrize("name", ["bd", "sir"])
def test_segment_states_is_jump_segment_and_matches_the_reference(name, dtype):
    spec, x0, theta = CASES[name]
    net = ReactionNetworkSDE(**spec)
    B = 96
    xs, th = jref.per_path_inputs(x0, theta, B, seed=7)
    rates = net.kernel_parameters(torch.from_numpy(th).to(dtype))
    paths = torch.arange(B, dtype=torch.int64) * 5 + 3
    out_times = [0.3, 0.5, 0.5, 0.9, 1.0]
    args = (net, torch.from_numpy(xs), rates, 0.25, 1.0, 2, paths, torch.tensor(KEY), 4096)
    x, ne, st = jump_segment(*args)
    x2, ne2, st2, states = jump_segment_states(*args, out_times)
    assert torch.equal(x, x2) and torch.equal(ne, ne2) and torch.equal(st, st2)
    assert states.dtype == torch.int32 and states.shape == (B, len(out_times), xs.shape[1]) and int(st.sum()) == 0
    assert torch.equal(states[:, -1], x.to(torch.int32))          # the output at t_end is the state the segment ends in
    wx, wf, ws, near, outs = ref.run_segments_states(jref.tables(net), xs, rates.double().numpy(), 0.25, 1.0, 2, paths.numpy(), KEY, 4096, out_times)
    print(f"{name} {dtype}: {int(near.sum())} of {B} pairs undecidable, {int(wf.sum())} events")
    assert near.sum() <= ref.CAP * B
    ok = ~near
    assert np.array_equal(states.numpy()[ok], outs[ok]) and np.array_equal(ne.numpy()[ok], wf[ok]) and np.array_equal(x.numpy()[ok], wx[ok])
    assert wf.sum() > B and (outs[:, 0] != outs[:, -1]).any()     # something happened between the outputs


def test_segment_states_of_a_stopped_path_leaves_minus_one():
    net = ReactionNetworkSDE(**BD)
    x = torch.tensor([[5], [5]])
    rates = net.kernel_parameters(torch.tensor([[200.0, 0.1, 0.0], [4.0, -0.5, 0.0]], dtype=F64))
    _, ne, st, states = jump_segment_states(net, x, rates, 0.0, 10.0, 0, torch.arange(2), torch.tensor(KEY), 3, [0.0, 5.0, 10.0])
    assert st.tolist() == [1, 2] and ne.tolist() == [3, 0]
    assert states[0, 0].tolist() == [5] and states[0, 1:].reshape(-1).tolist() == [-1, -1] and bool((states[1] == -1).all())
    _, _, st, states = jump_segment_states(net, x[:1], rates[:1], 0.0, 10.0, 0, torch.arange(1), torch.tensor(KEY), 3, [])
    assert states.shape == (1, 0, 1) and st.tolist() == [1]


# ------------------------------------------------------------------------------------- 2. the smoother against its own filter
def _bd_problem(M=3):
    spec, x0, theta = CASES["bd"]
    net = ReactionNetworkSDE(**spec)
    xs, th = jref.per_path_inputs(x0, theta, M, seed=2)
    ys = (np.asarray(x0)[None, :] + np.random.default_rng(1).integers(0, 4, size=(len(TIMES), 1))).astype(np.float64)
    return net, _obs(TIMES, ys), PoissonObservationLikelihood(scale=0.9), torch.from_numpy(th), torch.from_numpy(xs)


def test_smoother_is_consistent_with_its_own_filter():
    net, obs, like, th, xs = _bd_problem()
    M, N, D = 3, 64, 5
    kw = dict(n_particles=N, initial_state=xs, key=torch.tensor(KEY), max_events=4096)
    res = jump_particle_smoother(net, obs, like, th, torch.tensor(PATH_TIMES, dtype=F64), n_draws=D, **kw)
    flt = jump_particle_filter(net, obs, like, th, return_particles=True, **kw)
    assert isinstance(res, SmoothedJumpPaths) and res.paths.dtype == torch.int32 and res.paths.shape == (M, D, len(PATH_TIMES), 1)
    assert res.lineage.dtype == torch.int32 and res.lineage.shape == (M, D, len(TIMES)) and res.n_events.dtype == torch.int32
    assert torch.equal(res.path_times, torch.tensor(PATH_TIMES, dtype=F64)) and torch.equal(res.log_likelihood, flt.log_likelihood)
    assert torch.equal(res.increments, flt.increments) and torch.equal(res.stopped, flt.stopped)
    lin = res.lineage.long()
    for k, q in enumerate(AT_OBS):
        assert torch.equal(res.paths[:, :, q], torch.gather(flt.particles[:, k], 1, lin[:, :, k, None].expand(-1, -1, 1))), k
        assert torch.equal(res.n_events[:, :, k], torch.gather(flt.events[:, k], 1, lin[:, :, k])), k
    assert int(res.status.abs().sum()) == 0 and int(res.n_events.sum()) > M * D
    assert bool((res.paths[:, :, 0] == xs[:, None, :]).all())      # the output at 0 is the start state
    for k in range(1, len(TIMES)):
        assert torch.equal(lin[:, :, k - 1], torch.gather(flt.ancestors[:, k - 1].long(), 1, lin[:, :, k]))
    distinct = [[len(np.unique(res.lineage[m, :, k].numpy())) for k in range(len(TIMES))] for m in range(M)]
    assert res.distinct_lineages.tolist() == distinct
    ref.check_replay(net, th, xs.numpy(), TIMES, PATH_TIMES, KEY, flt.particles.numpy().astype(np.int64), res.paths.numpy(), lin.numpy(),
                     res.n_events.numpy(), "bd torch route")
    again = jump_particle_smoother(net, obs, like, th, torch.tensor(PATH_TIMES, dtype=F64), n_draws=D, **kw)
    assert torch.equal(again.paths, res.paths) and torch.equal(again.lineage, res.lineage)


@pytest.mark.parametrize("name,N,like", ref.REPLAY_RUNS, ids=[r[0] for r in ref.REPLAY_RUNS])
def test_the_inputs_of_the_device_checks_stay_under_the_cap(name, N, like):
    """The cases tests/test_jump_smoother_gpu.py replays, through the torch route in float64 with the fp32 values of theta: the
    reference alone flags far fewer (record, segment) pairs than the cap, and the torch route matches it on the others."""
    spec, xs, th, ys, key = ref.replay_case(name, N)
    net = ReactionNetworkSDE(**spec)
    th = torch.from_numpy(th).float().double()
    kw = dict(n_particles=N, initial_state=torch.from_numpy(xs), key=torch.tensor(key), max_events=4096)
    obs = _obs(ref.REPLAY_TIMES, ys)
    res = jump_particle_smoother(net, obs, fref.likelihood(like), th, torch.tensor(ref.REPLAY_PATH_TIMES, dtype=F64), n_draws=7, **kw)
    flt = jump_particle_filter(net, obs, fref.likelihood(like), th, return_particles=True, **kw)
    assert bool(torch.isfinite(res.log_likelihood).all())
    flagged, total = ref.check_replay(net, th.float(), xs, ref.REPLAY_TIMES, ref.REPLAY_PATH_TIMES, key, flt.particles.numpy().astype(np.int64),
                                      res.paths.numpy(), res.lineage.long().numpy(), res.n_events.numpy(), f"{name} N={N} torch route")
    assert flagged <= ref.CAP * total / 4                          # a wide margin


# ------------------------------------------------------------------------------------------------------------ 3. segment 0
def test_segment_zero_is_the_jump_process():
    net, _, like, th, xs = _bd_problem()
    M, N, D = 3, 64, 5
    obs = _obs([0.7, 1.1], [[21.0], [22.0]])
    pt = [0.0, 0.2, 0.7, 0.9]
    res = jump_particle_smoother(net, obs, like, th, torch.tensor(pt, dtype=F64), n_particles=N, n_draws=D, initial_state=xs, key=torch.tensor(KEY),
                                 max_events=4096)
    jp = jump_process(net, xs.repeat_interleave(N, 0), th.repeat_interleave(N, 0), pt[:3], key=KEY, max_events=4096)
    b = torch.arange(M)[:, None] * N + res.lineage[:, :, 0].long()
    assert torch.equal(res.paths[:, :, :3], jp.states[b]) and bool(jp.complete.all())
    assert int((res.paths[:, :, 0] != res.paths[:, :, 2]).sum()) > 0


# ----------------------------------------------------------------------------------------------- 4. edge rules and arguments
def test_a_dead_filter_has_no_sample_and_bad_arguments_are_refused():
    net = ReactionNetworkSDE(**BD)
    theta = torch.tensor([[4.0, 0.5, 0.0]] * 2, dtype=F64)
    like = GaussianObservationLikelihood(variance=4.0)
    dead_obs = _obs([0.5, 1.0, 1.5], [[6.0], [float("nan")], [7.0]])
    pt = torch.tensor([0.0, 0.5, 0.7, 1.5], dtype=F64)
    kw = dict(n_particles=64, n_draws=3, initial_state=torch.tensor([5]), key=torch.tensor(KEY), max_events=4096)
    res = jump_particle_smoother(net, dead_obs, like, theta, pt, **kw)
    assert bool((res.paths == -1).all()) and bool((res.lineage == -1).all()) and res.distinct_lineages.tolist() == [[0] * 3] * 2
    assert int(res.n_events.sum()) == 0 and int(res.status.sum()) == 0 and res.log_likelihood.tolist() == [float("-inf")] * 2
    obs = _obs([0.5, 1.0, 1.5], [[6.0], [6.0], [7.0]])
    ok = jump_particle_smoother(net, obs, like, theta, pt, **kw)
    assert bool((ok.paths >= 0).all()) and bool((ok.lineage >= 0).all()) and int(ok.status.sum()) == 0
    assert jump_particle_smoother(net, obs, like, theta, [1.5], **kw).paths.shape == (2, 3, 1, 1)      # a list is taken as float64
    for bad in (pt.float(), torch.tensor([], dtype=F64), torch.tensor([0.0, float("nan")], dtype=F64), torch.tensor([0.5, 0.2], dtype=F64),
                torch.tensor([-0.1, 0.2], dtype=F64), torch.tensor([0.2, 1.6], dtype=F64), torch.tensor([[0.2, 0.5]], dtype=F64),
                torch.tensor([0.0, float("inf")], dtype=F64)):
        with pytest.raises(ValueError):
            jump_particle_smoother(net, obs, like, theta, bad, **kw)
    with pytest.raises(ValueError):
        jump_particle_smoother(net, obs, like, theta, pt, **{**kw, "n_draws": 0})
    with pytest.raises(ValueError):
        jump_particle_smoother(net, obs, like, theta, pt, **{**kw, "max_events": 0})


# ------------------------------------------------------------------------------------------------------------- 5. PMMH wiring
def _pmmh_problem():
    net = ReactionNetworkSDE(**BD)
    obs = _obs([0.0, 0.25, 0.5], [[30.0], [29.0], [27.0]])              # short segments: the torch route pays per event
    prior = Prior(type=PriorType.LOG_NORMAL, mean=0.0, std=2.0, dim=3)
    g = torch.Generator().manual_seed(3)
    theta = torch.tensor([10.0, 0.5, 0.01], dtype=F64) * (0.8 + 0.4 * torch.rand(8, 3, generator=g, dtype=F64))
    return net, obs, PoissonObservationLikelihood(), prior, theta


def test_pmmh_keeps_jump_paths_without_touching_the_theta_chain():
    net, obs, like, prior, theta = _pmmh_problem()
    kw = dict(n_iterations=30, warmup=10, n_particles=64, theta_positive_dims=(0, 1, 2), key=torch.tensor([11, 12]), dynamics="jump", max_events=4096)
    pt = torch.tensor([0.0, 0.1, 0.25, 0.4, 0.5], dtype=F64)
    a = particle_mcmc(net, obs, like, prior, None, theta, **kw)
    trace = []
    b = particle_mcmc(net, obs, like, prior, None, theta, return_paths=True, path_times=pt, _trace=trace, **kw)
    assert torch.equal(a.samples, b.samples) and torch.equal(a.log_likelihood, b.log_likelihood) and torch.equal(a.acceptance_rate, b.acceptance_rate)
    assert a.paths is None and a.path_times is None and torch.equal(b.path_times, pt)
    assert b.paths.dtype == torch.int32 and b.paths.shape == (20, 8, 5, 1) and b.path_iteration.shape == (20, 8)
    assert b.path_mean.dtype == F64 and b.path_mean.shape == (5, 1) and b.path_mean_standard_error.shape == (5, 1)
    live_seen = 0
    for n in range(20):
        t = trace[10 + n]
        dead = t["cur_noise_path"][:, -1] == mc.DEAD_PATH
        assert torch.equal(b.path_iteration[n] < 0, dead) and torch.equal(b.path_iteration[n][~dead], t["cur_path_iteration"][~dead])
        anchors = t["cur_anchor"]
        assert not anchors.is_floating_point()                         # carried as integers
        assert torch.equal(b.paths[n][~dead][:, [0, 2, 4]], anchors[~dead].to(torch.int32))     # the replay passes through its anchors
        assert bool((b.paths[n][dead] == -1).all())
        live_seen += int((~dead).sum())
    assert live_seen > 100 and bool((b.paths[b.path_iteration >= 0][:, 0] == 30).all())
    live = (b.path_iteration >= 0)[:, :, None, None].expand_as(b.paths)
    assert torch.allclose(b.path_mean, b.paths[live].reshape(-1, 5, 1).double().mean(dim=0))
    with pytest.raises(ValueError, match="path_times"):
        particle_mcmc(net, obs, like, prior, None, theta, return_paths=True, **kw)
    with pytest.raises(ValueError, match="path_times"):
        particle_mcmc(net, obs, like, prior, 0.05, theta, **{**kw, "dynamics": "diffusion"}, return_paths=True, path_times=pt)
    with pytest.raises(ValueError):
        particle_mcmc(net, obs, like, prior, None, theta, return_paths=True, path_times=torch.tensor([0.0, 0.6], dtype=F64), **kw)


def test_the_entry_points_refuse_bad_arguments_before_any_hip_call():
    import ctypes
    from viforsdes_amd import _hip
    lib = _hip.load()
    net = _hip.crn_network(BD["reactants"], [[p - r for p, r in zip(ps, rs)] for ps, rs in zip(BD["products"], BD["reactants"])])
    null, i = ctypes.c_void_p(None), ctypes.c_int

    def filter_replay(M=1, N=64, S=1, P=3, K=2, D=1, Q=1, max_events=16):
        return lib.vsde_crn_jump_filter_replay(ctypes.byref(net), i(M), i(N), i(S), i(P), i(K), i(D), i(Q), null, null, null, null, null, null,
                                               i(max_events), null, null, null, null, null, null, null, null)

    def anchored_replay(B=1, S=1, P=3, K=2, Q=1, max_events=16):
        return lib.vsde_crn_jump_anchored_replay(ctypes.byref(net), i(B), i(S), i(P), i(K), i(Q), null, null, null, null, null, null, null, null,
                                                 i(max_events), null, null, null, null)

    for call, bad, word in ((filter_replay, dict(Q=0), "output times"), (filter_replay, dict(max_events=0), "max_events"),
                            (filter_replay, dict(max_events=2 ** 23 + 1), "max_events"), (filter_replay, dict(D=0), "draws"),
                            (filter_replay, dict(N=0), "particles"), (filter_replay, dict(M=0), "dims"), (filter_replay, dict(K=0), "dims"),
                            (filter_replay, dict(M=2 ** 16, N=2 ** 16), "paths"), (filter_replay, dict(M=2 ** 15, D=2 ** 15, K=2), "segments"),
                            (filter_replay, dict(S=2), ""), (filter_replay, dict(P=2), ""), (filter_replay, {}, "NULL"),
                            (anchored_replay, dict(Q=0), "output times"), (anchored_replay, dict(max_events=0), "max_events"),
                            (anchored_replay, dict(B=0), "dims"), (anchored_replay, dict(B=2 ** 30, K=2), "segments"),
                            (anchored_replay, {}, "NULL")):
        assert call(**bad) < 0, bad
        assert word.encode() in lib.vsde_last_error(), (bad, lib.vsde_last_error())


def test_refine_parameters_passes_path_times_on():
    import inspect
    from viforsdes_amd import VariationalPosterior
    assert "path_times" in inspect.signature(VariationalPosterior.refine_parameters).parameters


# ------------------------------------------------------------------------------------------ exactness against a closed form
ID_TIMES, ID_COUNTS = fref.IMMIGRATION_DEATH_TIMES, fref.IMMIGRATION_DEATH_COUNTS
ID_PATH_TIMES = [0.25, 2.0, 3.0]                                  # two interior times and the last observation


def test_reference_smoothing_marginal_against_direct_enumeration():
    """The forward-backward itself, on a case small enough to check: one observation at t1, the marginal at t < t1 by enumeration."""
    model = ref.ImmigrationDeath(0.7, 5, [1.3], [3.0])
    size, t = 200, 0.5
    first = jref.immigration_death_pmf(5, 2.0, 0.7, t, size)[0]
    lam = np.maximum(np.arange(size), 1e-6)
    lik = np.exp(3 * np.log(lam) - lam - math.lgamma(4.0))
    joint = np.array([first[n] * (jref.immigration_death_pmf(n, 2.0, 0.7, 1.3 - t, size)[0] * lik).sum() for n in range(size)])
    assert abs(model.smoothing_mean(2.0, t) - (joint * np.arange(size)).sum() / joint.sum()) <= 1e-9
    assert abs(model.log_likelihood(2.0) - fref.immigration_death_log_likelihood(2.0, 0.7, 5, [1.3], [3.0])) <= 1e-9
    end = jref.immigration_death_pmf(5, 2.0, 0.7, 1.3, size)[0] * lik
    assert abs(model.smoothing_mean(2.0, 1.3) - (end * np.arange(size)).sum() / end.sum()) <= 1e-9


def test_smoother_matches_the_exact_smoothing_mean_of_immigration_death():
    net = ReactionNetworkSDE(**BD)
    M, N = 512, 128
    model = ref.ImmigrationDeath(0.5, 30, ID_TIMES, ID_COUNTS)
    exact = model.log_likelihood(10.0)
    obs = _obs(ID_TIMES, [[y] for y in ID_COUNTS])
    res = jump_particle_smoother(net, obs, PoissonObservationLikelihood(), torch.tensor([10.0, 0.5, 0.0], dtype=F64).expand(M, 3),
                                 torch.tensor(ID_PATH_TIMES, dtype=F64), n_particles=N, n_draws=1, key=torch.tensor(KEY), max_events=4096)
    est, se, sd = ref.weighted_path_mean(res.log_likelihood.numpy(), exact, res.paths[:, 0, :, 0].numpy())
    want = np.array([model.smoothing_mean(10.0, t) for t in ID_PATH_TIMES])
    print(f"immigration-death smoother: std(r) {sd:.3f}, exact {want}, estimate {est}, z {(est - want) / se}")
    assert int(res.status.sum()) == 0 and sd <= 0.5
    assert (np.abs(est - want) <= 4.5 * se).all()


def test_pmmh_path_mean_matches_the_exact_joint_posterior():
    net = ReactionNetworkSDE(reactants=[[0], [1]], products=[[1], [0]], rate_constants=["birth", 0.5])
    prior = Prior(type=PriorType.LOG_NORMAL, mean=2.0, std=1.0, dim=1)
    times, ys, path_times = ID_TIMES[:3], ID_COUNTS[:3], [0.25, 0.4, 0.5]     # the short problem: the torch route pays per event
    grid = np.linspace(0.01, 160.0, 2000)                          # fewer observations: a wider posterior, a wider grid
    model = ref.ImmigrationDeath(0.5, 30, times, ys)
    p, _ = ref.birth_posterior(model, grid, prior)
    assert p[0] < 1e-6 * p.max() and p[-1] < 1e-6 * p.max()        # the grid holds the posterior
    keep = p > 1e-12 * p.max()
    want = np.array([sum(pg * model.smoothing_mean(g, t) for g, pg in zip(grid[keep], p[keep])) / p[keep].sum() for t in path_times])
    mean = float((p * grid).sum())
    std = math.sqrt(float((p * (grid - mean) ** 2).sum()))
    C, N = 16, 64
    rng = np.random.default_rng(5)
    start = rng.choice(grid, size=C, p=p) + rng.uniform(-0.5, 0.5, size=C) * (grid[1] - grid[0])     # stationary from iteration 0
    obs = _obs(times, [[y] for y in ys])
    res = particle_mcmc(net, obs, PoissonObservationLikelihood(), prior, None, torch.tensor(start, dtype=F64)[:, None], 40, warmup=0,
                        n_particles=N, theta_positive_dims=(0,), proposal_scale_tril=torch.tensor([[std / mean]], dtype=F64), key=torch.tensor([41, 42]),
                        dynamics="jump", max_events=4096, return_paths=True, path_times=torch.tensor(path_times, dtype=F64))
    got, se = res.path_mean[:, 0].numpy(), res.path_mean_standard_error[:, 0].numpy()
    print(f"PMMH paths: exact {want}, chains {got} +- {se}, acceptance {float(res.acceptance_rate.mean()):.3f}")
    assert bool((res.path_iteration >= 0).all())
    assert (np.abs(got - want) <= 4.5 * se).all()
