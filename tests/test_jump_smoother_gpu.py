"""GPU: the jump-segment replay kernel (csrc/vsde_jump_replay.hip) through the public ``jump_particle_smoother`` and
``particle_mcmc(..., dynamics="jump", return_paths=True, path_times=...)``.  The route is asserted with call counters.

* the smoother against the filter kernel's own store, bit for bit: the path at ``T_k`` is the stored particle of its lineage, the
  event counts are the filter's, ``status`` is 0; then the interior outputs against the float64 restatement
  (tests/jump_smoother_reference.py) from the run's own start states, at most 2e-2 of the (record, segment) pairs undecidable
  (asserted first) and every other pair exact; then the kernel's lineage against ``particle_smoother._trace`` of the kernel's
  ancestors.  bd, sir, net4 and chain8 at N = 192, D = 7 and kinetic_chain8 at N = 64, M = 3: S = 1, 2, 4, 8 and the rate-law form,
  three waves in the filter, a draw count that is a multiple of nothing;
* segment 0 against the ``jump_process`` kernel bit for bit; the smallest shapes that can still go wrong; the copy number
  ``2^30 - 1`` through the smoother and through the word view of the PMMH step kernel; the PMMH wiring (same theta chain, launch
  counts, records replay to their anchors); kernel route against torch route in distribution;
* the exact smoothing marginals of immigration-death observed with Poisson noise (forward-backward on 200 states), for the
  smoother (M = 512 filters weighted by ``exp(ll - exact)``) and for the PMMH path mean over the exact posterior of the birth rate.

Every call runs with ``max_events <= 4096``."""
import math

import numpy as np
import pytest
import torch

import jump_filter_reference as fref
import jump_process_reference as jref
import jump_smoother_reference as ref
from reaction_networks import BD, SIR

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F64 = torch.float64
TIMES, PATH_TIMES, RUNS = ref.REPLAY_TIMES, ref.REPLAY_PATH_TIMES, ref.REPLAY_RUNS
AT_OBS = [0, 3, 3, 6]                                             # q(T_k)
CASES = jref.cases()


def _key(k0, k1):
    return fref.key_tensor(k0, k1, DEV)


def _count(monkeypatch, name):
    """A list that receives one entry per call of ``_hip.<name>``."""
    from viforsdes_amd import _hip
    calls, real = [], getattr(_hip, name)
    monkeypatch.setattr(_hip, name, lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    return calls


def _obs(times, values):
    from viforsdes_amd import Observations
    return Observations(times=torch.tensor(times, dtype=F64), values=torch.tensor(values, dtype=torch.float32)).to(DEV)


def _gather(store, lin, k):
    """store [M, K, N, ...] at the slots lin [M, D, K] of observation k."""
    idx = lin[:, :, k]
    return torch.stack([store[m, k][idx[m]] for m in range(store.shape[0])])


def _check_against_filter(res, flt, at_obs):
    lin = res.lineage.long()
    assert res.paths.dtype == torch.int32 and res.lineage.dtype == torch.int32 and res.n_events.dtype == torch.int32
    for k, q in enumerate(at_obs):
        assert torch.equal(res.paths[:, :, q], _gather(flt.particles, lin, k)), k
        assert torch.equal(res.n_events[:, :, k], _gather(flt.events, lin, k)), k
    assert int(res.status.abs().sum()) == 0
    assert torch.equal(res.log_likelihood, flt.log_likelihood) and torch.equal(res.stopped, flt.stopped)


# --------------------------------------------------------------------------------- 6. the smoother against the filter's store
@pytest.mark.parametrize("name,N,like", RUNS, ids=[r[0] for r in RUNS])
def test_smoother_replays_the_filter_kernels_segments(name, N, like, monkeypatch):
    from viforsdes_amd import ReactionNetworkSDE, jump_particle_filter, jump_particle_smoother
    from viforsdes_amd.inference.particle_smoother import _trace
    spec, xs, th, ys, key = ref.replay_case(name, N)              # tests/test_jump_smoother.py holds these inputs to the cap on the CPU
    net = ReactionNetworkSDE(**spec)
    M, D, x0 = 3, 7, xs[0]
    th = torch.from_numpy(th).float()
    obs = _obs(TIMES, ys)
    kw = dict(n_particles=N, initial_state=torch.from_numpy(xs).to(DEV), key=_key(*key), max_events=4096)
    filters, replays = _count(monkeypatch, "jump_particle_filter"), _count(monkeypatch, "jump_filter_replay")
    res = jump_particle_smoother(net, obs, fref.likelihood(like), th.to(DEV), torch.tensor(PATH_TIMES, dtype=F64), n_draws=D, **kw)
    assert filters == [1] and replays == [1]                       # the kernel route, one launch each
    flt = jump_particle_filter(net, obs, fref.likelihood(like), th.to(DEV), return_particles=True, **kw)
    assert res.paths.shape == (M, D, len(PATH_TIMES), len(x0)) and res.paths.is_cuda and bool(torch.isfinite(res.log_likelihood).all())
    _check_against_filter(res, flt, AT_OBS)
    assert bool((res.paths[:, :, 0] == torch.from_numpy(xs).to(DEV)[:, None, :]).all()) and int(res.n_events.sum()) > M * D
    ref.check_replay(net, th, xs, TIMES, PATH_TIMES, key, flt.particles.cpu().numpy().astype(np.int64), res.paths.cpu().numpy(),
                     res.lineage.long().cpu().numpy(), res.n_events.cpu().numpy(), f"{name} N={N}")
    assert torch.equal(res.lineage, _trace(flt.ancestors, res.lineage[:, :, -1]))
    distinct = [[len(np.unique(res.lineage[m, :, k].cpu().numpy())) for k in range(len(TIMES))] for m in range(M)]
    assert res.distinct_lineages.tolist() == distinct


# ------------------------------------------------------------------------------------------------------------ 7. segment 0
@pytest.mark.parametrize("name", ["bd", "autoreg"])
def test_segment_zero_is_the_jump_process_kernel(name, monkeypatch):
    from viforsdes_amd import PoissonObservationLikelihood, ReactionNetworkSDE, jump_particle_smoother, jump_process
    spec, x0, theta = CASES[name]
    net = ReactionNetworkSDE(**spec)
    M, N, D = 3, 64, 5
    xs, th = jref.per_path_inputs(x0, theta, M, seed=4)
    xs, th = torch.from_numpy(xs).to(DEV), torch.from_numpy(th).float().to(DEV)
    pt = [0.0, 0.2, 0.7, 0.9]
    replays = _count(monkeypatch, "jump_filter_replay")
    res = jump_particle_smoother(net, _obs([0.7, 1.1], [x0, x0]), PoissonObservationLikelihood(), th, torch.tensor(pt, dtype=F64), n_particles=N,
                                 n_draws=D, initial_state=xs, key=_key(7, 8), max_events=4096)
    assert replays == [1]
    jp = jump_process(net, xs.repeat_interleave(N, 0), th.repeat_interleave(N, 0), pt[:3], key=_key(7, 8), max_events=4096)
    b = torch.arange(M, device=DEV)[:, None] * N + res.lineage[:, :, 0].long()
    assert torch.equal(res.paths[:, :, :3], jp.states[b]) and bool(jp.complete.all())
    assert int((res.paths[:, :, 0] != res.paths[:, :, 2]).sum()) > 0


# ------------------------------------------------------------------------------------------------------ 8. the smallest shapes
def _bd_pair(theta, times, ys, pt, D, like=None, x0=(5,), N=64, key=(1, 2)):
    """(smoother result, filter result of the same key) on the birth-death network."""
    from viforsdes_amd import PoissonObservationLikelihood, ReactionNetworkSDE, jump_particle_filter, jump_particle_smoother
    net, like = ReactionNetworkSDE(**BD), like or PoissonObservationLikelihood()
    kw = dict(n_particles=N, initial_state=torch.tensor(x0), key=_key(*key), max_events=4096)
    th = torch.tensor(theta, device=DEV)
    res = jump_particle_smoother(net, _obs(times, ys), like, th, torch.tensor(pt, dtype=F64), n_draws=D, **kw)
    return res, jump_particle_filter(net, _obs(times, ys), like, th, return_particles=True, **kw)


def test_smallest_shapes_on_the_device(monkeypatch):
    from viforsdes_amd import PoissonObservationLikelihood, ReactionNetworkSDE, jump_particle_smoother
    replays = _count(monkeypatch, "jump_filter_replay")
    live = [4.0, 0.5, 0.0]
    # three blocks, the last one partly filled: B K = 3 * 50 * 4 = 600 threads; a dead filter (an invalid theta row) among live ones
    res, flt = _bd_pair([live, [4.0, -0.5, 0.0], live], TIMES, [[5.0], [6.0], [5.0], [7.0]], PATH_TIMES, 50)
    assert bool((res.paths[1] == -1).all()) and bool((res.lineage[1] == -1).all()) and res.distinct_lineages[1].tolist() == [0] * 4
    assert int(res.n_events[1].sum()) == 0 and int(res.status.sum()) == 0 and res.log_likelihood[1] == float("-inf")
    lin = res.lineage.long()
    for m in (0, 2):
        for k, q in enumerate(AT_OBS):
            assert torch.equal(res.paths[m, :, q], flt.particles[m, k][lin[m, :, k]]) and torch.equal(res.n_events[m, :, k], flt.events[m, k][lin[m, :, k]])
    assert bool((res.paths[[0, 2]] >= 0).all()) and bool((res.paths[[0, 2], :, 0] == 5).all())
    # Q = 1, inside the last segment: every other segment owns nothing
    res, flt = _bd_pair([live] * 2, TIMES, [[5.0], [6.0], [5.0], [7.0]], [0.6], 3)
    assert res.paths.shape == (2, 3, 1, 1) and bool((res.paths >= 0).all())
    assert torch.equal(res.n_events[:, :, 3], _gather(flt.events, res.lineage.long(), 3))
    # all outputs in the first segment (one at exactly 0, one at exactly T_0), none in the others
    res, flt = _bd_pair([live] * 2, [0.5, 1.0, 1.5], [[5.0], [6.0], [7.0]], [0.0, 0.25, 0.5], 3)
    assert bool((res.paths[:, :, 0] == 5).all()) and torch.equal(res.paths[:, :, 2], _gather(flt.particles, res.lineage.long(), 0))
    _check_against_filter(res, flt, [2])
    # Q = 1 at exactly the last observation
    res, flt = _bd_pair([live] * 2, [0.5, 1.0, 1.5], [[5.0], [6.0], [7.0]], [1.5], 3)
    assert torch.equal(res.paths[:, :, 0], _gather(flt.particles, res.lineage.long(), 2))
    # an absorbed state: SIR with I = 0 never moves
    res = jump_particle_smoother(ReactionNetworkSDE(**SIR), _obs([0.0, 1.0, 2.0], [[40.0, 0.0]] * 3), PoissonObservationLikelihood(),
                                 torch.tensor([[0.01, 0.2]], device=DEV), torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0], dtype=F64), n_particles=64,
                                 n_draws=3, key=_key(1, 2), max_events=4096)
    assert bool((res.paths == torch.tensor([40, 0], dtype=torch.int32, device=DEV)).all()) and int(res.n_events.sum()) == 0
    assert int(res.status.sum()) == 0
    assert replays == [1] * 5


def test_wrappers_refuse_a_bad_ownership_table_and_a_bad_store():
    from viforsdes_amd import ReactionNetworkSDE, _hip
    net = ReactionNetworkSDE(**BD).kernel_descriptor()
    M, N, K, D, Q = 2, 64, 2, 3, 3
    i32 = dict(dtype=torch.int32, device=DEV)
    x0, th = torch.full((M, 1), 5, **i32), torch.tensor([[4.0, 0.5, 0.0]] * M, device=DEV)
    times, pt = torch.tensor([0.5, 1.0], dtype=F64, device=DEV), torch.tensor([0.2, 0.5, 0.8], dtype=F64, device=DEV)
    parts, anc, last = torch.full((M, K, N, 1), 5, **i32), torch.arange(N, **i32).expand(M, K, N).contiguous(), torch.zeros(M, D, **i32)
    good = torch.tensor([0, 2, 3], dtype=torch.int32)
    run = lambda q, **kw: _hip.jump_filter_replay(x0, th, times, pt, q, _key(1, 2), kw.get("max_events", 64), parts, anc, kw.get("last", last),
                                                  network=net)
    assert run(good)[0].shape == (M, D, Q, 1)
    for bad in (torch.tensor([1, 2, 3], dtype=torch.int32), torch.tensor([0, 2, 2], dtype=torch.int32), torch.tensor([0, 3, 2], dtype=torch.int32),
                torch.tensor([0, 2, 4], dtype=torch.int32), torch.tensor([0, 3], dtype=torch.int32), good.long(), good.to(DEV)):
        with pytest.raises(ValueError):
            run(bad)
    with pytest.raises(ValueError):
        run(good, max_events=0)
    with pytest.raises(ValueError):
        run(good, last=last.long())
    obs = torch.tensor([[5.0], [6.0]], device=DEV)
    launch = lambda store: _hip.jump_particle_filter(x0, th, times, obs, None, 4.0, _key(1, 2), 64, N, network=net, store=store)
    out = launch((parts, anc))
    assert out[7] is parts and out[8] is anc and out[9] is None and bool(torch.isfinite(out[0]).all())
    for bad in ((parts.float(), anc), (parts, anc[:, :1]), (parts.cpu(), anc), (parts[..., :0], anc)):
        with pytest.raises(ValueError):
            launch(bad)


# ------------------------------------------------------------------------------------------------------------- 9. 2^30 - 1
def test_a_copy_number_fp32_cannot_hold_survives_the_smoother_and_the_pmmh_path(monkeypatch):
    from viforsdes_amd import GaussianObservationLikelihood, Prior, PriorType, ReactionNetworkSDE, jump_particle_smoother, particle_mcmc
    big = 2 ** 30 - 1
    net, like = ReactionNetworkSDE(**SIR), GaussianObservationLikelihood(variance=1.0)
    obs = _obs([0.5, 1.0], [[float(big), 0.0]] * 2)
    start = torch.tensor([big, 0], dtype=torch.int32, device=DEV)
    pt = torch.tensor([0.0, 0.25, 0.5, 1.0], dtype=F64)
    replays, anchored = _count(monkeypatch, "jump_filter_replay"), _count(monkeypatch, "jump_anchored_replay")
    res = jump_particle_smoother(net, obs, like, torch.tensor([[0.02, 0.5]] * 2, device=DEV), pt, n_particles=64, n_draws=3,
                                 initial_state=torch.tensor([big, 0]), key=_key(1, 2), max_events=4096)
    assert replays == [1] and bool((res.paths == start).all()) and int(res.status.sum()) == 0
    C = 16
    g = torch.Generator().manual_seed(3)
    theta0 = (torch.tensor([0.02, 0.5]) * (0.8 + 0.4 * torch.rand(C, 2, generator=g))).to(DEV)
    out = particle_mcmc(net, obs, like, Prior(type=PriorType.LOG_NORMAL, mean=0.0, std=2.0, dim=2), None, theta0, 12, n_particles=64,
                        theta_positive_dims=(0, 1), initial_state=torch.tensor([big, 0]), key=_key(11, 12), dynamics="jump", max_events=4096,
                        return_paths=True, path_times=pt)
    assert anchored == [1] and out.paths.shape == (12, C, 4, 2) and out.paths.dtype == torch.int32
    live = out.path_iteration >= 0
    assert int(live.sum()) > 0 and bool((out.paths[live] == start).all())          # the word view of the step kernel keeps the integer
    assert bool((out.paths[~live] == -1).all())


# ------------------------------------------------------------------------------------------------------------------ 10. PMMH
def test_pmmh_paths_on_the_device(monkeypatch):
    from viforsdes_amd import PoissonObservationLikelihood, Prior, PriorType, ReactionNetworkSDE, particle_mcmc
    from viforsdes_amd.inference import particle_mcmc as mc
    C, N, n_it = 16, 64, 12
    net = ReactionNetworkSDE(**BD)
    obs = _obs(fref.IMMIGRATION_DEATH_TIMES, [[y] for y in fref.IMMIGRATION_DEATH_COUNTS])
    prior = Prior(type=PriorType.LOG_NORMAL, mean=0.0, std=2.0, dim=3)
    g = torch.Generator().manual_seed(3)
    theta0 = (torch.tensor([10.0, 0.5, 0.01]) * (0.8 + 0.4 * torch.rand(C, 3, generator=g))).to(DEV)
    pt = torch.tensor([0.0, 0.25, 0.5, 1.0, 1.5, 2.0, 3.0], dtype=F64)
    at_obs = [0, 2, 2, 4, 6]
    kw = dict(n_particles=N, theta_positive_dims=(0, 1, 2), key=_key(11, 12), dynamics="jump", max_events=4096)
    a = particle_mcmc(net, obs, PoissonObservationLikelihood(), prior, None, theta0, n_it, **kw)
    filters, anchored, trace = _count(monkeypatch, "jump_particle_filter"), _count(monkeypatch, "jump_anchored_replay"), []
    b = particle_mcmc(net, obs, PoissonObservationLikelihood(), prior, None, theta0, n_it, return_paths=True, path_times=pt, _trace=trace, **kw)
    assert filters == [1] * n_it and anchored == [1]
    assert torch.equal(a.samples, b.samples) and torch.equal(a.log_likelihood, b.log_likelihood) and torch.equal(a.acceptance_rate, b.acceptance_rate)
    assert b.paths.shape == (n_it, C, len(pt), 1) and b.paths.dtype == torch.int32 and b.paths.is_cuda and torch.equal(b.path_times.cpu(), pt)
    assert a.paths is None and a.path_times is None and b.path_mean.dtype == torch.float32
    live_seen = 0
    for n in range(n_it):
        t = trace[n]
        dead = t["cur_noise_path"][:, -1] == mc.DEAD_PATH
        assert torch.equal(b.path_iteration[n] < 0, dead) and torch.equal(b.path_iteration[n][~dead], t["cur_path_iteration"][~dead])
        assert t["cur_anchor"].dtype == torch.int32
        assert torch.equal(b.paths[n][~dead][:, at_obs], t["cur_anchor"][~dead])       # the replay passes through its anchors
        assert bool((b.paths[n][dead] == -1).all())
        live_seen += int((~dead).sum())
    assert live_seen > n_it * C // 2 and bool((b.paths[b.path_iteration >= 0][:, 0] == 30).all())


# ---------------------------------------------------------------------------------------------- 11. kernel route, torch route
def test_kernel_route_and_torch_route_agree_in_distribution(monkeypatch):
    from viforsdes_amd import PoissonObservationLikelihood, ReactionNetworkSDE, jump_particle_smoother
    from viforsdes_amd.inference import jump_filter as jf
    M, N = 256, 128
    net = ReactionNetworkSDE(**SIR)
    obs = _obs(TIMES, [[95.0, 5.0], [93.0, 6.0], [92.0, 7.0], [84.0, 12.0]])
    theta = torch.tensor([0.02, 0.5], device=DEV).expand(M, 2)
    run = lambda k: jump_particle_smoother(net, obs, PoissonObservationLikelihood(), theta, torch.tensor([0.6], dtype=F64), n_particles=N,
                                           n_draws=1, key=_key(*k), max_events=4096).paths[:, 0, 0, 1].double().cpu().numpy()
    replays = _count(monkeypatch, "jump_filter_replay")
    a = run((31, 32))
    monkeypatch.setattr(jf, "HIP_JUMP_FILTER", False)
    b = run((33, 34))
    assert replays == [1]
    z = abs(a.mean() - b.mean()) / math.sqrt(a.var(ddof=1) / M + b.var(ddof=1) / M)
    print(f"SIR: mean I(0.6 | y) kernel {a.mean():.3f}, torch {b.mean():.3f}, two-sample z {z:.2f}")
    assert a.var() > 0 and z <= 4.5


# ------------------------------------------------------------------------------------------ exactness against a closed form
ID_TIMES, ID_COUNTS = fref.IMMIGRATION_DEATH_TIMES, fref.IMMIGRATION_DEATH_COUNTS
ID_PATH_TIMES = [0.25, 2.0, 3.0]                                  # two interior times and the last observation


def test_smoother_matches_the_exact_smoothing_mean_of_immigration_death(monkeypatch):
    from viforsdes_amd import PoissonObservationLikelihood, ReactionNetworkSDE, jump_particle_smoother
    M, N = 512, 128
    model = ref.ImmigrationDeath(0.5, 30, ID_TIMES, ID_COUNTS)
    exact = model.log_likelihood(10.0)
    assert abs(exact - fref.immigration_death_log_likelihood(10.0, 0.5, 30, ID_TIMES, ID_COUNTS)) <= 1e-9
    replays = _count(monkeypatch, "jump_filter_replay")
    res = jump_particle_smoother(ReactionNetworkSDE(**BD), _obs(ID_TIMES, [[y] for y in ID_COUNTS]), PoissonObservationLikelihood(),
                                 torch.tensor([10.0, 0.5, 0.0], device=DEV).expand(M, 3), torch.tensor(ID_PATH_TIMES, dtype=F64), n_particles=N,
                                 n_draws=1, key=_key(21, 22), max_events=4096)
    assert replays == [1] and int(res.status.sum()) == 0 and int(res.stopped.sum()) == 0
    est, se, sd = ref.weighted_path_mean(res.log_likelihood.double().cpu().numpy(), exact, res.paths[:, 0, :, 0].cpu().numpy())
    want = np.array([model.smoothing_mean(10.0, t) for t in ID_PATH_TIMES])
    print(f"immigration-death smoother on the device: std(r) {sd:.3f}, exact {want}, estimate {est}, z {(est - want) / se}")
    assert sd <= 0.5
    assert (np.abs(est - want) <= 4.5 * se).all()


def test_pmmh_path_mean_matches_the_exact_joint_posterior(monkeypatch):
    from viforsdes_amd import PoissonObservationLikelihood, Prior, PriorType, ReactionNetworkSDE, particle_mcmc
    net = ReactionNetworkSDE(reactants=[[0], [1]], products=[[1], [0]], rate_constants=["birth", 0.5])
    prior = Prior(type=PriorType.LOG_NORMAL, mean=2.0, std=1.0, dim=1)
    grid = np.linspace(0.01, 40.0, 1000)
    model = ref.ImmigrationDeath(0.5, 30, ID_TIMES, ID_COUNTS)
    p, _ = ref.birth_posterior(model, grid, prior)
    assert p[0] < 1e-6 * p.max() and p[-1] < 1e-6 * p.max()        # the grid holds the posterior
    keep = p > 1e-12 * p.max()
    want = np.array([sum(pg * model.smoothing_mean(g, t) for g, pg in zip(grid[keep], p[keep])) / p[keep].sum() for t in ID_PATH_TIMES])
    mean = float((p * grid).sum())
    std = math.sqrt(float((p * (grid - mean) ** 2).sum()))
    C, N = 64, 128
    rng = np.random.default_rng(5)
    start = rng.choice(grid, size=C, p=p) + rng.uniform(-0.5, 0.5, size=C) * (grid[1] - grid[0])     # stationary from iteration 0
    filters, anchored = _count(monkeypatch, "jump_particle_filter"), _count(monkeypatch, "jump_anchored_replay")
    res = particle_mcmc(net, _obs(ID_TIMES, [[y] for y in ID_COUNTS]), PoissonObservationLikelihood(), prior, None,
                        torch.tensor(start, dtype=torch.float32, device=DEV)[:, None], 200, warmup=0, n_particles=N, theta_positive_dims=(0,),
                        proposal_scale_tril=torch.tensor([[std / mean]]), key=_key(41, 42), dynamics="jump", max_events=4096, return_paths=True,
                        path_thin=1, path_times=torch.tensor(ID_PATH_TIMES, dtype=F64))
    assert filters == [1] * 200 and anchored == [1]
    got, se = res.path_mean[:, 0].double().cpu().numpy(), res.path_mean_standard_error[:, 0].double().cpu().numpy()
    print(f"PMMH paths on the device: exact {want}, chains {got} +- {se}, acceptance {float(res.acceptance_rate.mean()):.3f}")
    assert bool((res.path_iteration >= 0).all()) and res.paths.shape == (200, C, 3, 1)
    assert (np.abs(got - want) <= 4.5 * se).all()
