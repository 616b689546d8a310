"""GPU: the replay kernel (csrc/vsde_filter.hip: rp_kernel) through ``_hip.filter_replay`` / ``_hip.guided_filter_replay`` and the
public ``particle_smoother``, and ``VariationalPosterior.smooth_paths`` on the device.

As in tests/test_particle_filter_gpu.py the kernel is compared against float64 on its own previous stage: what the filter kernel
stored (particles, ancestors) and the final slots the public function handed to the replay wrapper are taken as given.

* lineage: ``lineage[..., K-1]`` is the ``last_slot`` handed in, ``lineage[..., k-1] = ancestors[m, k-1, lineage[..., k]]``, exactly;
* every replayed segment, every step: against a float64 Euler-Maruyama (bridge) segment started from the kernel's stored particle
  and driven by the reference noise of path ``m N + lineage[m, d, k]``: 2e-4 of the largest magnitude, the bound the filter tests
  hold the same step functions to; the segment's endpoint against ``particles[m, k, lineage]`` under the same bound (how many are
  bit-identical is printed: two kernels may contract multiply-adds differently);
* ``paths[..., 0, :] == x0`` exactly, positive dims >= float32(1e-6) with the clamp hit where filters start at the floor, a dead
  filter gives NaN paths and lineage -1;
* routing, agreement of the torch route with the kernel route in distribution (two-sample z < 5), the exact Rauch-Tung-Striebel
  smoother of the discretised OU model (M = 4096, z < 5, variance within 5 sqrt(2 / (M - 1)) relative), ``smooth_paths`` after a
  short fit, and bad arguments."""
import math

import numpy as np
import pytest
import torch

import guided_filter_reference as gref
import particle_smoother_reference as sref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
M = 5


def _key(k0, k1, dev=DEV):
    return torch.from_numpy(np.array([k0, k1], dtype=np.uint32).view(np.int32)).to(dev)


def _counted(fn):
    """(result of fn(), the calls [(args, outputs)] it made to the bootstrap replay wrapper, those to the guided one)."""
    from viforsdes_amd import _hip
    plain, guided = [], []
    real_p, real_g = _hip.filter_replay, _hip.guided_filter_replay

    def record(log, real):
        def wrapped(*a, **k):
            out = real(*a, **k)
            log.append((a, out))
            return out
        return wrapped

    _hip.filter_replay, _hip.guided_filter_replay = record(plain, real_p), record(guided, real_g)
    try:
        out = fn()
    finally:
        _hip.filter_replay, _hip.guided_filter_replay = real_p, real_g
    return out, plain, guided


_RUNS = {}


def _cached(name, rows, N, D, proposal="bootstrap"):
    """One kernel-route run of the case (M = 5), shared by its tests and left unchanged: (case, result, what the replay wrapper was
    given: particles, ancestors, last_slot, key)."""
    tag = (name, None if rows is None else tuple(rows), N, D, proposal)
    if tag not in _RUNS:
        from viforsdes_amd import particle_smoother
        from viforsdes_amd.inference import particle_filter as pf
        case = gref.case(name, M, rows) if proposal == "bridge" else sref.case(name, M, rows)
        sde, obs, like, th, x0, dt, pos = case
        key = (0x9E3779B9 ^ N, 0x7F4A7C15 + len(name) + D)
        res, plain, guided = _counted(lambda: particle_smoother(
            sde, obs.to(DEV), like, th.to(DEV), dt, n_particles=N, n_draws=D, initial_state=x0.to(DEV), positive_dims=pos,
            key=_key(*key), proposal=proposal))
        assert pf.HIP_FILTER and (len(plain), len(guided)) == ((0, 1) if proposal == "bridge" else (1, 0))    # the kernel route, once
        args = (guided or plain)[0][0]
        particles, ancestors, last = args[9:12] if proposal == "bridge" else args[6:9]
        _RUNS[tag] = (case, res, particles.double().cpu().numpy(), ancestors.long().cpu().numpy(), last.long().cpu().numpy(), key)
    return _RUNS[tag]


def _check(name, rows, N, D, proposal):
    (sde, obs, like, th, x0, dt, pos), res, parts, anc, last, key = _cached(name, rows, N, D, proposal)
    rows = np.round(obs.times.numpy() / dt).astype(int)
    K, S, T = len(rows), sde.state_dim, int(rows[-1])
    paths, lin = res.paths.double().cpu().numpy(), res.lineage.long().cpu().numpy()
    assert paths.shape == (M, D, T + 1, S) and lin.shape == (M, D, K) and res.lineage.dtype == torch.int32
    assert parts.shape == (M, K, N, S) and np.isfinite(parts).all() and np.isfinite(paths).all()
    # lineage: exact integer identities
    assert np.array_equal(lin[:, :, -1], last) and last.min() >= 0 and last.max() < N
    for k in range(K - 1, 0, -1):
        assert np.array_equal(lin[:, :, k - 1], np.take_along_axis(anc[:, k - 1], lin[:, :, k], axis=1))
    distinct = res.distinct_lineages.cpu().numpy()
    for m in range(M):
        for k in range(K):
            assert distinct[m, k] == len(set(lin[m, :, k].tolist()))
    # replay
    assert np.array_equal(paths[:, :, 0], np.broadcast_to(x0.double().numpy()[:, None, :], (M, D, S)))
    theta = np.repeat(th.double().numpy(), D, axis=0)
    H = None if like.obs_matrix is None else like.obs_matrix.double().numpy()
    worst = worst_end = 0.0
    same = total = 0
    base = np.arange(M)[:, None] * N
    for k in range(K):
        t0, t1 = (int(rows[k - 1]) if k else 0), int(rows[k])
        stored = np.take_along_axis(parts[:, k], lin[:, :, k, None], axis=1)                       # [M, D, S]
        if t1 > t0:
            assert t1 - t0 <= 400
            start = x0.double().numpy()[:, None, :].repeat(D, axis=1) if k == 0 else \
                np.take_along_axis(parts[:, k - 1], lin[:, :, k - 1, None], axis=1)
            z = sref.path_noise((base + lin[:, :, k]).reshape(M * D), T, S, key)[:, t0:t1]
            if proposal == "bridge":
                want = sref.guided_segment_states(sde, start.reshape(M * D, S), theta, z, obs.values[k].double().numpy(), H,
                                                  like.variance, dt, pos)
            else:
                want = sref.euler_segment_states(sde, start.reshape(M * D, S), theta, z, dt, pos)
            got = paths[:, :, t0 + 1:t1 + 1].reshape(M * D, t1 - t0, S)
            worst = max(worst, float(np.abs(got - want).max() / np.abs(want).max()))
        end = paths[:, :, t1]
        worst_end = max(worst_end, float(np.abs(end - stored).max() / np.abs(stored).max()))
        same, total = same + int((end.astype(np.float32) == stored.astype(np.float32)).all(axis=-1).sum()), total + M * D
    print(f"{name} {proposal} rows {rows.tolist()} N={N} D={D}: segments {worst:.2e}, endpoints vs stored particles {worst_end:.2e} of "
          f"the largest magnitude; {same} of {total} endpoints bit-identical")
    assert worst < 2e-4
    assert worst_end < 2e-4
    if pos:
        assert (paths[..., list(pos)] >= sref.FLOOR).all()
    return paths


SIZES = {"chain6": (64, 512)}
NATURAL = ["lv", "ou", "lindiag16", "sir", "autoreg", "chain6"]


def _params(names, rows):
    return [pytest.param(name, rows, SIZES.get(name, (64, 1024))[big], D, id=f"{name}-{'block' if rows else 'own'}-{'max' if big else '64'}-D{D}")
            for name in names for big in (0, 1) for D in (1, 96)]


# ------------------------------------------------------------------------------------------------------ 1. lineage and replay
@pytest.mark.parametrize("name,rows,N,D", _params(["ou", "lv", "sir"], sref.BLOCK_ROWS) + _params(NATURAL, None))
def test_bootstrap_replay_matches_float64_segments(name, rows, N, D):
    paths = _check(name, rows, N, D, "bootstrap")
    if name in ("lv", "sir") and D == 96:
        assert (paths[:, :, 1:] == sref.FLOOR).any()                # filters 0 and 4 start at the floor: the clamp was exercised


# the rate-law network and the linear-diagonal model (S = 3 through a dense [4, 3] H: the O <= 4 instantiation) at the smallest size:
# with ou / lv / sir every route of the guided replay's dispatch is launched
@pytest.mark.parametrize("name,N,D", [pytest.param(name, N, D, id=f"{name}-{N}-D{D}")
                                      for name in ("ou", "lv", "sir") for N in (64, 1024) for D in (1, 96)]
                         + [pytest.param(name, 64, D, id=f"{name}-64-D{D}") for name in ("autoreg", "lindiag3") for D in (1, 96)])
def test_guided_replay_matches_float64_bridge_segments(name, N, D):
    paths = _check(name, None, N, D, "bridge")
    if name in ("lv", "sir") and D == 96:
        assert (paths[:, :, 1:] == sref.FLOOR).any()


def test_count_likelihood_shares_the_bootstrap_replay():
    from viforsdes_amd import PoissonObservationLikelihood, particle_smoother
    from viforsdes_amd import Observations
    sde, obs, _, th, x0, dt, pos = sref.case("sir", M, sref.BLOCK_ROWS)
    obs = Observations(times=obs.times, values=torch.round(obs.values))              # counts
    res, plain, guided = _counted(lambda: particle_smoother(
        sde, obs.to(DEV), PoissonObservationLikelihood(), th.to(DEV), dt, n_particles=64, n_draws=3, initial_state=x0.to(DEV),
        positive_dims=pos, key=_key(3, 4)))
    assert (len(plain), len(guided)) == (1, 0)
    args, (paths, lineage) = plain[0]
    want = torch.gather(args[6][:, -1], 1, lineage[:, :, -1].long()[..., None].expand(-1, -1, 2))
    err = float((paths[:, :, -1] - want).abs().max() / want.abs().max())
    print(f"Poisson SIR: endpoints vs stored particles {err:.2e}")
    assert err < 2e-4 and bool(torch.isfinite(paths).all())


@pytest.mark.parametrize("proposal", ["bootstrap", "bridge"])
def test_dead_filter_gives_nan_paths(proposal):
    from viforsdes_amd import particle_smoother
    sde, obs, like, th, x0, dt, pos = sref.case("ou", M)
    bad = x0.clone()
    bad[1] = float("nan")
    run = lambda start: _counted(lambda: particle_smoother(sde, obs.to(DEV), like, th.to(DEV), dt, n_particles=64, n_draws=3,
                                                           initial_state=start.to(DEV), key=_key(4, 4), proposal=proposal))
    a, plain, guided = run(bad)
    b, _, _ = run(x0)
    assert len(plain) + len(guided) == 1
    assert float(a.log_likelihood[1]) == float("-inf")
    assert bool(torch.isnan(a.paths[1]).all()) and bool((a.lineage[1] == -1).all()) and bool((a.distinct_lineages[1] == 0).all())
    for m in (0, 2, 3, 4):
        assert torch.equal(a.paths[m], b.paths[m]) and torch.equal(a.lineage[m], b.lineage[m])
        assert bool(torch.isfinite(a.paths[m]).all())


# ------------------------------------------------------------------------------------------------------------------ 2. routing
def _ou_mean_paths(sde, obs, like, dt, key, **kw):
    from viforsdes_amd import particle_smoother
    th = torch.tensor([[0.8, 1.0, 0.5]], device=DEV).expand(512, 3)
    res, plain, guided = _counted(lambda: particle_smoother(sde, obs.to(DEV), like, th, dt, key=_key(*key), **kw))
    return res.paths[:, 0].double().cpu().numpy(), len(plain) + len(guided)


def _two_sample_z(a, b, rows):
    a, b = a[:, rows], b[:, rows]
    se = np.sqrt(a.var(axis=0, ddof=1) / a.shape[0] + b.var(axis=0, ddof=1) / b.shape[0])
    return float((np.abs(a.mean(axis=0) - b.mean(axis=0)) / se).max())


def test_torch_route_cases_agree_with_the_kernel_route(monkeypatch):
    from viforsdes_amd import make_sde
    from viforsdes_amd.examples.sdes import ou_problem
    from viforsdes_amd.inference import particle_filter as pf
    sde, obs, like, _, _, dt, _, _ = ou_problem()
    rows = np.round(obs.times.numpy() / dt).astype(int)[1:]                  # row 0 is x0 in every draw
    kernel, calls = _ou_mean_paths(sde, obs, like, dt, (41, 42), n_particles=256)
    assert calls == 1
    user = make_sde(lambda x, th: th[..., 0:1] * (th[..., 1:2] - x), lambda x, th: th[..., 2:3].reshape(x.shape[0], 1, 1), 1, 3)
    for tag, model, key, kw in [("N = 1088", sde, (43, 44), dict(n_particles=1088)),
                                ("user-defined SDE", user, (45, 46), dict(n_particles=256)),
                                ("HIP_FILTER = False", sde, (47, 48), dict(n_particles=256))]:
        if tag.startswith("HIP"):
            monkeypatch.setattr(pf, "HIP_FILTER", False)
        torch_route, calls = _ou_mean_paths(model, obs, like, dt, key, **kw)
        z = _two_sample_z(kernel, torch_route, rows)
        print(f"OU, {tag}: torch route against kernel route, largest two-sample z of the mean path at the observation rows {z:.2f}")
        assert calls == 0 and z < 5.0


def test_five_state_dims_with_the_bridge_take_the_torch_route_and_agree():
    from viforsdes_amd import GaussianObservationLikelihood, Observations, particle_smoother
    from viforsdes_amd.examples.sdes import LinearDiagonalSDE
    sde, dt, n = LinearDiagonalSDE(5), 0.05, 512
    obs = Observations(times=torch.tensor([0.0, 0.5, 1.0]), values=torch.tensor([[0.5, -0.3, 0.2, 0.1, -0.2], [0.2, 0.1, 0.0, 0.3, -0.1],
                                                                                  [-0.1, 0.3, 0.1, 0.2, 0.0]]))
    like = GaussianObservationLikelihood(variance=0.09)
    th = torch.tensor([[0.7, 0.4, 0.5, 0.6, 0.8, -0.5, -1.0, -0.8, -0.6, -0.7]], device=DEV).expand(n, 10)
    run = lambda key, proposal: _counted(lambda: particle_smoother(sde, obs.to(DEV), like, th, dt, n_particles=256, key=_key(*key),
                                                                   proposal=proposal))
    a, plain, guided = run((51, 52), "bootstrap")
    assert (len(plain), len(guided)) == (1, 0)
    b, plain, guided = run((53, 54), "bridge")
    assert (len(plain), len(guided)) == (0, 0)
    z = max(_two_sample_z(a.paths[:, 0, :, i].double().cpu().numpy(), b.paths[:, 0, :, i].double().cpu().numpy(), [10, 20])
            for i in range(5))
    print(f"linear-diagonal S = 5: bridge (torch route) against bootstrap (kernel route), largest two-sample z {z:.2f}")
    assert z < 5.0


# --------------------------------------------------------------------------------------------------------------- 3. statistics
@pytest.mark.parametrize("proposal", ["bootstrap", "bridge"])
def test_ou_draws_follow_the_exact_smoothing_distribution_on_the_device(proposal):
    from viforsdes_amd import particle_smoother
    from viforsdes_amd.examples.sdes import ou_problem
    sde, obs, like, _, _, dt, _, _ = ou_problem()
    theta, n, N = (0.8, 1.0, 0.5), 4096, 1024
    rows = np.round(obs.times.numpy() / dt).astype(int)
    mean, var = sref.ou_rts(theta, dt, like.variance, obs.values[0].numpy(), rows, obs.values.numpy())
    res, plain, guided = _counted(lambda: particle_smoother(sde, obs.to(DEV), like, torch.tensor([theta], device=DEV).expand(n, 3), dt,
                                                            n_particles=N, n_draws=1, key=_key(17, 23), proposal=proposal))
    assert len(plain) + len(guided) == 1
    x = res.paths[:, 0, :, 0].double().cpu().numpy()
    z = np.abs(x[:, 1:].mean(axis=0) - mean[1:]) / np.sqrt(x[:, 1:].var(axis=0, ddof=1) / n)
    ratio = x[:, 1:].var(axis=0, ddof=1) / var[1:]
    band = 5.0 * math.sqrt(2.0 / (n - 1))
    print(f"OU smoother on the device ({proposal}): max z {z.max():.2f}, variance ratio {ratio.min():.3f} .. {ratio.max():.3f} "
          f"(band +-{band:.3f})")
    assert z.max() < 5.0
    assert np.abs(ratio - 1.0).max() < band


# ---------------------------------------------------------------------------------------------------------------- 4. end to end
def test_smooth_paths_after_a_short_fit():
    from viforsdes_amd import (EncoderConfig, GaussianObservationLikelihood, HeadConfig, InferenceConfig, Prior, PriorType,
                               TrainingConfig, infer)
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
    n = 1024
    torch.manual_seed(5)
    (sp, plain, guided) = _counted(lambda: vp.smooth_paths(sde, like, n_samples=n, n_particles=256, chunk_size=512))
    assert vp._captured == {} and vp._calls == {}
    assert (len(plain), len(guided)) == (2, 0)                          # one replay launch per chunk
    torch.manual_seed(5)
    rw = vp.reweight_parameters(sde, like, n_samples=n, n_particles=256, chunk_size=512)
    assert vp._captured == {} and vp._calls == {}
    print(f"log p(y): smooth_paths {sp.log_evidence:.4f}, reweight_parameters {rw.log_evidence:.4f} (ESS {sp.effective_sample_size:.0f} "
          f"/ {n}); weighted path mean at the observation rows {sp.path_mean[::20, 0].tolist()}")
    assert sp.log_evidence == rw.log_evidence and sp.n_nonfinite == 0
    assert sp.paths.is_cuda and sp.paths.shape == (n, 101, 1) and sp.path_mean.shape == (101, 1) and sp.times.shape == (101,)
    assert bool(torch.isfinite(sp.path_mean).all()) and bool((sp.path_std[1:] > 0).all())
    assert bool((sp.path_quantiles.q05 <= sp.path_quantiles.q50).all()) and bool((sp.path_quantiles.q50 <= sp.path_quantiles.q95).all())


# ----------------------------------------------------------------------------------------------------------------------- 5. ABI
def test_bad_arguments_are_refused():
    from viforsdes_amd import _hip
    sde, obs, like, th, x0, dt, pos = sref.case("ou", 4)
    th, x0 = th.to(DEV), x0.to(DEV)
    rows = torch.round(obs.times / dt).to(torch.int32).to(DEV)
    key, K = _key(1, 2), rows.shape[0]

    def call(kind="ornstein_uhlenbeck", N=64, D=2, S=1, x0=x0, th=th):
        parts = torch.zeros(4, K, N, S, device=DEV)
        anc = torch.arange(N, device=DEV, dtype=torch.int32).expand(4, K, N).contiguous()
        last = torch.zeros(4, D, device=DEV, dtype=torch.int32)
        return _hip.filter_replay(kind, x0, th, rows, key, dt, parts, anc, last)

    paths, lineage = call()
    assert paths.shape == (4, 2, 101, 1) and lineage.shape == (4, 2, K) and bool((lineage == 0).all())
    for N in (32, 100, 1088, 2048):
        with pytest.raises(ValueError, match="particles"):
            call(N=N)
    with pytest.raises(ValueError, match="state_dim"):
        call("linear_diagonal", S=17, x0=torch.zeros(4, 17, device=DEV), th=torch.zeros(4, 34, device=DEV))
    with pytest.raises(ValueError, match="draws"):
        call(D=0)
    parts = torch.zeros(4, K, 64, 1, device=DEV)
    anc = torch.zeros(4, K, 64, device=DEV, dtype=torch.int32)
    last = torch.zeros(4, 2, device=DEV, dtype=torch.int32)
    with pytest.raises(ValueError, match="state_dim"):
        _hip.guided_filter_replay("linear_diagonal", torch.zeros(4, 5, device=DEV), torch.zeros(4, 10, device=DEV), rows,
                                  torch.zeros(K, 5, device=DEV), None, 0.1, key, dt, torch.zeros(4, K, 64, 5, device=DEV), anc, last)
    with pytest.raises(ValueError, match="int32"):
        _hip.filter_replay("ornstein_uhlenbeck", x0, th, rows, key, dt, parts, anc.long(), last)
    with pytest.raises(ValueError, match="expected"):
        _hip.filter_replay("ornstein_uhlenbeck", x0, th, rows, key, dt, parts[:, :-1], anc, last)
    torch.cuda.synchronize()
