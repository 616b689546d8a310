"""GPU: particle MCMC with paths -- the record half of the step kernel (csrc/vsde_mcmc.hip through ``_hip.pmmh_step_paths``), the
replay of carried records (csrc/vsde_anchored.hip: ar_kernel through ``_hip.anchored_replay`` / ``_hip.guided_anchored_replay``), the
kernel route of ``particle_mcmc(return_paths=True)`` and ``VariationalPosterior.refine_parameters(return_paths=True)``.

* The step kernel on synthetic inputs (no filter run), per element against the numpy rule of tests/pmmh_paths_reference.py: chain
  counts around the 64-thread workgroup, P = 1 / 3 / 16, R = 1 / 3, K = 1 / 2 / 5, N = 64 / 128, S = 1 / 3, iterations 1 (closes
  iteration 0, which accepts dead proposals) and 7; ancestors with out-of-range entries, particles holding distinct values, the
  -inf / NaN estimates of ``particle_mcmc_reference.kernel_case``.  Records are integers and copies: exact.  The chosen filter may
  differ from float64 only where the threshold is within ``particle_mcmc_reference.tolerance`` of a boundary, in at most 1 % of a
  case's chains.  The theta half is ``torch.equal`` to ``pmmh_step`` on the same inputs.
* ``anchored_replay`` bit for bit against ``filter_replay`` on the records gathered from a ``particle_smoother`` run, and against
  float64 segments (2e-4 of the largest magnitude, the smoother test's bound) for B = 1 / 257 shuffled records with a key each.
* End to end: the route taken, record identities against a rerun of the kernel filter, the theta chain bit-equal to the run
  without paths, exactness of the path moments on the OU problem against the exact joint posterior (|z| <= 4.5), reaction networks
  and counts, ``refine_parameters``."""
import itertools

import numpy as np
import pytest
import torch

import guided_filter_reference as gref
import particle_mcmc_reference as mref
import particle_smoother_reference as sref
import pmmh_paths_reference as ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SENTINEL, ISENTINEL = -12345.0, -777


def _key(k0, k1, dev=DEV):
    return torch.from_numpy(np.array([k0, k1], dtype=np.uint32).view(np.int32)).to(dev)


def _u32(t):
    return t.cpu().numpy().view(np.uint32).astype(np.int64)


# -------------------------------------------------------------------------------------------------------- 1. the step kernel alone
THETA_HALF = ("cur_u", "cur_log_target", "cur_loglik", "prop_u", "prop_log_prior", "theta_prop", "filter_key", "n_accept", "sample_row",
              "loglik_row", "target_row")


def _launch(case, rows="all", paths=True):
    from viforsdes_amd import _hip
    C, P, R, K, S = case["C"], case["P"], case["R"], case["K"], case["S"]
    f = lambda a: torch.tensor(np.asarray(a, dtype=np.float32), device=DEV).contiguous()
    i32 = lambda a: torch.tensor(np.asarray(a).astype(np.uint32).view(np.int32), device=DEV).contiguous()
    t = dict(cur_u=f(case["cur_u"]), cur_log_target=f(case["cur_log_target"]), cur_loglik=f(case["cur_loglik"]), prop_u=f(case["prop_u"]),
             prop_log_prior=f(case["prop_log_prior"]), theta_prop=torch.full((C * R, P), SENTINEL, device=DEV),
             filter_key=torch.zeros(2, dtype=torch.int32, device=DEV), n_accept=torch.full((C,), 5, dtype=torch.int32, device=DEV),
             sample_row=torch.full((C, P), SENTINEL, device=DEV), loglik_row=torch.full((C,), SENTINEL, device=DEV),
             target_row=torch.full((C,), SENTINEL, device=DEV))
    args = (case["iteration"], torch.tensor(case["L"]), case["step_size"], *case["prior"], [int(i) for i in np.nonzero(case["mask"])[0]],
            _key(*case["key"]), f(case["loglik_prop"]), t["cur_u"], t["cur_log_target"], t["cur_loglik"], t["prop_u"], t["prop_log_prior"],
            t["theta_prop"], t["filter_key"], t["n_accept"])
    state_rows = dict(sample_row=t["sample_row"], loglik_row=t["loglik_row"], target_row=t["target_row"])
    if not paths:
        _hip.pmmh_step(*args, **state_rows)
    else:
        t.update(cur_anchor=f(case["cur_anchor"]), cur_noise_path=i32(case["cur_noise_path"]),
                 cur_path_iteration=torch.tensor(case["cur_path_iteration"], device=DEV),
                 anchor_row=torch.full((C, K, S), SENTINEL, device=DEV), noise_row=torch.full((C, K), ISENTINEL, dtype=torch.int32, device=DEV),
                 iteration_row=torch.full((C,), ISENTINEL, dtype=torch.int32, device=DEV))
        given = {"all": ("anchor_row", "noise_row", "iteration_row"), "none": (), "noise": ("noise_row",)}[rows]
        _hip.pmmh_step_paths(*args, f(case["particles"]), torch.tensor(case["ancestors"], device=DEV), t["cur_anchor"], t["cur_noise_path"],
                             t["cur_path_iteration"], **state_rows, **{k: t[k] for k in given})
    torch.cuda.synchronize()
    return t


def _check_case(case, rows):
    C, R, K, N = case["C"], case["R"], case["K"], case["N"]
    got, plain = _launch(case, rows), _launch(case, paths=False)
    for k in THETA_HALF:                                                   # bit for bit, NaN included
        assert torch.equal(got[k].view(torch.int32), plain[k].view(torch.int32)), k
    it = case["iteration"] - 1
    acc = (got["n_accept"].cpu().numpy() - 5).astype(bool)
    want = ref.draw_records(case["loglik_prop"], case["particles"], case["ancestors"], it, case["key"])
    noise = _u32(got["cur_noise_path"])
    live = acc & (want["r"] >= 0)
    r_kernel = np.where(live, noise[:, -1] // N - np.arange(C) * R, want["r"])
    differ = live & (r_kernel != want["r"])
    if differ.any():                                                       # only where the threshold sits on a boundary of float64 itself
        assert (want["margin"][differ] <= mref.tolerance(np.array([float(R)]))).all(), want["margin"][differ]
        assert differ.sum() <= 0.01 * C
        assert ((r_kernel[differ] >= 0) & (r_kernel[differ] < R)).all()
        want = ref.draw_records(case["loglik_prop"], case["particles"], case["ancestors"], it, case["key"], r_star=r_kernel)
    anchor, path_it = got["cur_anchor"].cpu().numpy(), got["cur_path_iteration"].cpu().numpy()
    old_anchor = np.asarray(case["cur_anchor"], dtype=np.float32)
    assert np.array_equal(noise[acc], want["noise_path"][acc])
    assert np.array_equal(anchor[acc], want["anchors"][acc].astype(np.float32), equal_nan=True)
    assert (path_it[acc] == it).all()
    assert np.array_equal(noise[~acc], case["cur_noise_path"][~acc]) and np.array_equal(anchor[~acc], old_anchor[~acc])
    assert (path_it[~acc] == case["cur_path_iteration"][~acc]).all()
    for name, cur, sentinel in (("anchor_row", "cur_anchor", SENTINEL), ("noise_row", "cur_noise_path", ISENTINEL),
                                ("iteration_row", "cur_path_iteration", ISENTINEL)):
        if rows == "all" or (rows == "noise" and name == "noise_row"):
            assert torch.equal(got[name].view(torch.int32), got[cur].view(torch.int32)), name
        else:
            assert bool((got[name] == sentinel).all()), name
    dead = acc & (want["r"] < 0)
    return int(acc.sum()), int(dead.sum()), int(differ.sum()), bool((np.asarray(case["ancestors"]) >= N).any())


@pytest.mark.parametrize("P", ref.PATH_CASE_GRID["P"])
@pytest.mark.parametrize("C", ref.PATH_CASE_GRID["C"])
def test_step_kernel_records_match_the_numpy_rule(C, P):
    g = ref.PATH_CASE_GRID
    accepted = dead = differing = 0
    clamp_seen = False
    for n, (R, K, N, S, iteration) in enumerate(itertools.product(g["R"], g["K"], g["N"], g["S"], (1, 7))):
        a, d, f, wild = _check_case(ref.path_case(C, P, R, K, N, S, iteration), ("all", "none", "noise")[n % 3])
        accepted, dead, differing, clamp_seen = accepted + a, dead + d, differing + f, clamp_seen or wild
    print(f"C = {C}, P = {P}: {accepted} accepted records, {dead} of them dead, {differing} filter choices on a float64 boundary")
    assert accepted > 0 and clamp_seen
    if C > 4:
        assert dead > 0                                                    # chain 2 (estimates all -inf) is accepted at iteration 0


# ------------------------------------------------------------------------------------------------------ 2. the replay of records
def _smoother_call(name, rows, proposal, N=64, D=3, M=5):
    """One kernel-route ``particle_smoother`` run: (arguments its replay wrapper was given, network, the paths and lineage it
    returned)."""
    from viforsdes_amd import _hip, particle_smoother
    sde, obs, like, th, x0, dt, pos = gref.case(name, M, rows) if proposal == "bridge" else sref.case(name, M, rows)
    entry = "guided_filter_replay" if proposal == "bridge" else "filter_replay"
    calls, real = [], getattr(_hip, entry)

    def recording(*a, **k):
        out = real(*a, **k)
        calls.append((a, k, out))
        return out

    setattr(_hip, entry, recording)
    try:
        particle_smoother(sde, obs.to(DEV), like, th.to(DEV), dt, n_particles=N, n_draws=D, initial_state=x0.to(DEV), positive_dims=pos,
                          key=_key(0x1234 + N, 0x77 + len(name)), proposal=proposal)
    finally:
        setattr(_hip, entry, real)
    assert len(calls) == 1                                                 # the kernel route
    return calls[0]


@pytest.mark.parametrize("rows", [sref.BLOCK_ROWS, sref.LATE_ROWS], ids=["block", "late"])
@pytest.mark.parametrize("name,proposal", [("ou", "bootstrap"), ("lv", "bootstrap"), ("sir", "bootstrap"), ("autoreg", "bootstrap"),
                                           ("ou", "bridge"), ("lv", "bridge")])
def test_anchored_replay_is_filter_replay_bit_for_bit(name, proposal, rows):
    from viforsdes_amd import _hip
    args, kw, (paths, lineage) = _smoother_call(name, rows, proposal)
    if proposal == "bridge":
        kind, x0, th, obs_rows, values, H, variance, key, dt, particles, ancestors, last, pos = args
        model = (values, H, variance)
    else:
        kind, x0, th, obs_rows, key, dt, particles, ancestors, last, pos = args
        model = ()
    M, D, K = lineage.shape
    N, S = particles.shape[2], particles.shape[3]
    lin = lineage.long()
    anchors = torch.gather(particles, 2, lin.permute(0, 2, 1)[..., None].expand(M, K, D, S)).permute(0, 2, 1, 3).reshape(M * D, K, S)
    noise = (torch.arange(M, device=DEV)[:, None, None] * N + lin).to(torch.int32).reshape(M * D, K)
    rep = lambda t: t.repeat_interleave(D, dim=0)
    fn = _hip.guided_anchored_replay if proposal == "bridge" else _hip.anchored_replay
    got = fn(kind, rep(x0), rep(th), obs_rows, *model, anchors.contiguous(), noise, key.reshape(1, 2).repeat(M * D, 1), dt, pos, **kw)
    assert bool(torch.isfinite(paths).all()) and got.shape == (M * D, paths.shape[2], S)
    assert torch.equal(got.view(M, D, -1, S), paths)


@pytest.mark.parametrize("B", [1, 257])
@pytest.mark.parametrize("name,proposal", [("ou", "bootstrap"), ("lv", "bootstrap"), ("sir", "bootstrap"), ("ou", "bridge"), ("lv", "bridge")])
def test_anchored_replay_matches_float64_segments(name, proposal, B):
    """Records that no filter produced: the replay is a function of the record alone, so anchors, noise paths (beyond 2^31 too) and
    keys are drawn at random per record, and records are in no order."""
    from viforsdes_amd import _hip
    from viforsdes_amd.core.sde import builtin_sde_route, kernel_theta
    rows = sref.BLOCK_ROWS
    sde, obs, like, th, x0, dt, pos = gref.case(name, B, rows) if proposal == "bridge" else sref.case(name, B, rows)
    rng = np.random.default_rng(31 * B + len(name))
    K, S, T = len(rows), sde.state_dim, rows[-1]
    perm = rng.permutation(B)
    th, x0 = th[perm], x0[perm]
    anchors = (obs.values[None, :, :S].double().numpy() * (1.0 + 0.1 * rng.uniform(-1, 1, size=(B, K, S)))).astype(np.float32)
    noise = rng.integers(0, 2 ** 32 - 1, size=(B, K), dtype=np.int64)
    keys = rng.integers(0, 2 ** 32, size=(B, 2), dtype=np.int64)
    dead = B // 2 if B > 1 else None
    if dead is not None:
        noise[dead] = ref.DEAD
    kind, network = builtin_sde_route(sde)
    H = like.obs_matrix
    to_i32 = lambda a: torch.tensor(a.astype(np.uint32).view(np.int32), device=DEV)
    common = (torch.tensor(anchors, device=DEV), to_i32(noise), to_i32(keys), dt, pos)
    obs_rows = torch.tensor(rows, dtype=torch.int32, device=DEV)
    theta_dev = kernel_theta(network, th.to(DEV))
    if proposal == "bridge":
        got = _hip.guided_anchored_replay(kind, x0.to(DEV), theta_dev, obs_rows, obs.values.to(DEV), None if H is None else H.to(DEV),
                                          float(like.variance), *common, network=network)
    else:
        got = _hip.anchored_replay(kind, x0.to(DEV), theta_dev, obs_rows, *common, network=network)
    got = got.double().cpu().numpy()
    assert got.shape == (B, T + 1, S)
    live = np.ones(B, dtype=bool)
    if dead is not None:
        live[dead] = False
        assert np.isnan(got[dead]).all()
    assert np.isfinite(got[live]).all() and np.array_equal(got[live, 0], x0.double().numpy()[live])
    theta = th.double().numpy()
    worst = 0.0
    for k in range(K):
        t0, t1 = (rows[k - 1] if k else 0), rows[k]
        if t1 == t0:
            continue
        start = x0.double().numpy() if k == 0 else anchors[:, k - 1].astype(np.float64)
        z = np.concatenate([sref.path_noise([noise[b, k]], T, S, tuple(keys[b]))[:, t0:t1] for b in range(B)], axis=0)
        if proposal == "bridge":
            want = sref.guided_segment_states(sde, start, theta, z, obs.values[k].double().numpy(),
                                              None if H is None else H.double().numpy(), like.variance, dt, pos)
        else:
            want = sref.euler_segment_states(sde, start, theta, z, dt, pos)
        worst = max(worst, float(np.abs(got[live, t0 + 1:t1 + 1] - want[live]).max() / np.abs(want[live]).max()))
    print(f"{name} {proposal} B = {B}: segments {worst:.2e} of the largest magnitude")
    assert worst < 2e-4
    if pos:
        assert (got[live][..., list(pos)] >= sref.FLOOR).all()


# ------------------------------------------------------------------------------------------------------------------ 3. end to end
def _ou():
    from viforsdes_amd import GaussianObservationLikelihood, Observations, Prior, PriorType
    from viforsdes_amd.examples.sdes import OrnsteinUhlenbeck
    obs = Observations(times=torch.tensor(mref.OU_TIMES), values=torch.tensor(mref.OU_VALUES)[:, None]).to(DEV)
    prior = Prior(type=PriorType.LOG_NORMAL, mean=mref.OU_PRIOR[1], std=mref.OU_PRIOR[2], dim=3)
    return OrnsteinUhlenbeck(), obs, GaussianObservationLikelihood(variance=mref.OU_VARIANCE), prior


def _counted(monkeypatch):
    from viforsdes_amd import _hip
    calls = dict(pmmh_step_paths=[], anchored_replay=[], guided_anchored_replay=[])
    for name, log in calls.items():
        def counting(*a, _real=getattr(_hip, name), _log=log, **kw):
            _log.append(a[0])
            return _real(*a, **kw)
        monkeypatch.setattr(_hip, name, counting)
    return calls


def test_kernel_route_records_match_a_rerun_of_the_kernel_filter(monkeypatch):
    from viforsdes_amd import particle_mcmc
    from viforsdes_amd.inference import particle_filter as pf
    sde, obs, like, prior = _ou()
    C, R, N, key = 65, 2, 64, (0x5EED, 0xFACE)
    theta0 = torch.tensor(mref.ou_initial_theta(C), dtype=torch.float32, device=DEV)
    run = lambda **kw: particle_mcmc(sde, obs, like, prior, mref.OU_DT, theta0, 5, n_particles=N, filters_per_chain=R,
                                     theta_positive_dims=(0, 1, 2), key=_key(*key), **kw)
    calls, trace = _counted(monkeypatch), []
    res = run(return_paths=True, _trace=trace)
    assert calls["pmmh_step_paths"] == [0, 1, 2, 3, 4, 5] and len(calls["anchored_replay"]) == 1 and not calls["guided_anchored_replay"]
    plain = run()
    assert len(calls["pmmh_step_paths"]) == 6 and len(calls["anchored_replay"]) == 1      # nothing of the paths without them
    for name in ("samples", "log_likelihood", "log_target", "acceptance_rate"):
        assert torch.equal(getattr(res, name), getattr(plain, name)), name                  # storing particles changes no arithmetic
    assert plain.paths is None and res.paths.is_cuda and res.paths.shape == (5, C, mref.OU_ROWS[-1] + 1, 1)
    rows, K = list(mref.OU_ROWS), len(mref.OU_ROWS)
    x0 = obs.values[0]
    prev_noise, prev_iter, prev_anchor = np.full((C, K), ref.DEAD, dtype=np.int64), np.full(C, -1), np.full((C, K, 1), np.nan, dtype=np.float32)
    boundary = 0
    for i, tr in enumerate(trace):
        out = pf.particle_filter(sde, obs, like, tr["theta_prop"], mref.OU_DT, n_particles=N, initial_state=x0, return_particles=True,
                                 key=tr["filter_key"])
        assert torch.equal(out.log_likelihood.view(C, R), tr["loglik"])                    # the kernel filter is deterministic for a key
        loglik, parts, anc = tr["loglik"].double().cpu().numpy(), out.particles.cpu().numpy(), out.ancestors.cpu().numpy()
        want = ref.draw_records(loglik, parts, anc, i, key)
        acc = tr["accept"].cpu().numpy()
        noise, anchor, it = tr["cur_noise_path"].cpu().numpy(), tr["cur_anchor"].cpu().numpy(), tr["cur_path_iteration"].cpu().numpy()
        r_kernel = np.where(acc, noise[:, -1] // N - np.arange(C) * R, want["r"])
        differ = acc & (r_kernel != want["r"])
        if differ.any():
            assert (want["margin"][differ] <= mref.tolerance(np.array([float(R)]))).all()
            boundary += int(differ.sum())
            want = ref.draw_records(loglik, parts, anc, i, key, r_star=r_kernel)
        assert np.array_equal(noise[acc], want["noise_path"][acc]) and (it[acc] == i).all()
        assert np.array_equal(anchor[acc], want["anchors"][acc].astype(np.float32))        # the gathered particles, exactly
        assert np.array_equal(noise[~acc], prev_noise[~acc]) and np.array_equal(it[~acc], prev_iter[~acc])
        assert np.array_equal(anchor[~acc], prev_anchor[~acc], equal_nan=True)
        prev_noise, prev_iter, prev_anchor = noise, it, anchor
        paths = res.paths[i].cpu().numpy()
        assert np.array_equal(res.path_iteration[i].cpu().numpy(), it) and (it >= 0).all() and np.isfinite(paths).all()
        assert np.array_equal(paths[:, 0], np.broadcast_to(x0.cpu().numpy(), (C, 1)))
        err = float(np.abs(paths[:, rows] - anchor).max() / np.abs(anchor).max())
        assert err < 2e-4, (i, err)
        if i > 0:
            assert np.array_equal(paths[~acc], res.paths[i - 1].cpu().numpy()[~acc])
    assert boundary <= 0.01 * C * len(trace) and sum(int(t["accept"].sum()) for t in trace) > C


@pytest.mark.parametrize("R,proposal", [(1, "bootstrap"), (2, "bootstrap"), (1, "bridge")])
def test_ou_paths_follow_the_exact_joint_posterior(R, proposal, monkeypatch):
    """Per grid row, the per-chain path means against the per-chain means of the exact sampler (``exact_mh`` theta chains, the
    Rauch-Tung-Striebel smoother of every theta) by a two-sample z whose denominator holds both chain spreads, and the same for the
    per-chain mean squared deviation from the exact pooled mean, whose average is the pooled variance (average of the smoothing
    variances plus the variance of the smoothing means).  4.5: the threshold of the theta test of tests/test_particle_mcmc_gpu.py,
    here over 2 x 40 strongly correlated statistics."""
    from viforsdes_amd import particle_mcmc
    sde, obs, like, prior = _ou()
    C, n, w = 256, 400, 150
    m1, m2 = ref.ou_exact_path_moments(C, n, w, stride=1)
    calls = _counted(monkeypatch)
    theta0 = torch.tensor(mref.ou_initial_theta(C), dtype=torch.float32, device=DEV)
    res = particle_mcmc(sde, obs, like, prior, mref.OU_DT, theta0, n, warmup=w, n_particles=64, filters_per_chain=R,
                        theta_positive_dims=(0, 1, 2), proposal=proposal, key=_key(0xABCDEF, 5 + R), return_paths=True, path_thin=5)
    assert len(calls["pmmh_step_paths"]) >= n + 1 and len(calls["anchored_replay"]) + len(calls["guided_anchored_replay"]) == 1
    assert res.paths.shape == (50, C, 41, 1) and bool((res.path_iteration >= 0).all()) and bool(torch.isfinite(res.paths).all())
    z_mean, z_spread = ref.path_moment_z(res.paths[..., 0].double().cpu().numpy(), m1, m2)
    exact_std = np.sqrt(m2.mean(axis=0) - m1.mean(axis=0) ** 2)
    ratio = res.path_std[1:, 0].double().cpu().numpy() / exact_std[1:]
    print(f"{proposal}, R = {R}: largest z of the path means {z_mean.max():.2f}, of the spreads {z_spread.max():.2f}; pooled std / exact "
          f"{ratio.min():.3f} .. {ratio.max():.3f}; acceptance {float(res.acceptance_rate.mean()):.3f}")
    assert z_mean.max() <= 4.5
    assert z_spread.max() <= 4.5


@pytest.mark.parametrize("name", ["autoreg", "sir"])
def test_reaction_networks_and_counts_take_the_kernel_route_with_paths(name, monkeypatch):
    from viforsdes_amd import particle_mcmc
    import test_particle_mcmc_gpu as base
    sde, obs, like, prior, theta0 = base._network_case(name)
    P = theta0.shape[1]
    calls = _counted(monkeypatch)
    run = lambda **kw: particle_mcmc(sde, obs, like, prior, 0.1, theta0, 20, n_particles=64, theta_positive_dims=tuple(range(P)),
                                     positive_dims=(0, 1), key=_key(3, 4), **kw)
    res = run(return_paths=True, path_thin=2)
    assert calls["pmmh_step_paths"] == list(range(21)) and len(calls["anchored_replay"]) == 1
    T = int(round(float(obs.times[-1]) / 0.1))
    assert res.paths.shape == (10, 64, T + 1, 2) and bool((res.path_iteration >= 0).all())
    assert bool(torch.isfinite(res.paths).all()) and bool((res.paths >= sref.FLOOR).all())
    assert torch.equal(res.samples, run().samples)
    print(f"{name}: path mean at the end {res.path_mean[-1].tolist()}, observed {obs.values[-1].tolist()}")


def test_refine_parameters_returns_paths_after_a_short_fit():
    from viforsdes_amd import (EncoderConfig, GaussianObservationLikelihood, HeadConfig, InferenceConfig, Prior, PriorType, TrainingConfig,
                               infer)
    from viforsdes_amd.console import Console
    from viforsdes_amd.examples.sdes import ou_problem
    sde, obs, _, _, horizon, dt, _, _ = ou_problem()
    like = GaussianObservationLikelihood(variance=0.5)                  # the fit of tests/test_particle_mcmc_gpu.py
    prior = Prior(type=PriorType.LOG_NORMAL, mean=0.0, std=0.5, dim=3)
    cfg = InferenceConfig(training=TrainingConfig(time_step=dt, batch_size=256, n_iterations=200, learning_rate=2e-3,
                                                  sde_param_lr=2e-2),
                          encoder=EncoderConfig(hidden_dim=32, cond_dim=32, num_heads=4, depth=1),
                          head=HeadConfig(hidden_dim=32, num_layers=1), sde_param_positive_dims=[0, 1, 2],
                          mixed_precision=False, console=Console(enabled=False), seed=1)
    vp = infer(sde, obs, like, prior, horizon, cfg)
    torch.manual_seed(5)
    res = vp.refine_parameters(sde, like, n_chains=128, n_iterations=120, warmup=60, n_particles=64, return_paths=True, path_thin=4)
    assert vp._captured == {} and vp._calls == {}
    T = int(round(float(obs.times[-1]) / dt))
    assert res.paths.is_cuda and res.paths.shape == (15, 128, T + 1, 1) and res.path_iteration.shape == (15, 128)
    assert res.path_mean.shape == (T + 1, 1) and bool(torch.isfinite(res.path_mean).all()) and bool(torch.isfinite(res.path_mean_standard_error).all())
    assert bool((res.path_quantiles.q05 <= res.path_quantiles.q95).all()) and res.variational_mean is not None
    print(f"refine_parameters with paths: path mean at the observation rows {res.path_mean[::20, 0].tolist()}")
