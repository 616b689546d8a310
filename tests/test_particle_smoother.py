"""CPU: the torch route of ``particle_smoother`` (the specification) and ``VariationalPosterior.smooth_paths``.

* Stage checks in float64 (OU / Lotka-Volterra / SIR, both proposals, D in {1, 7, N + 5}, grids that start and end inside the
  Philox blocks of four): the final draw is float64 systematic sampling of the final weights with the specified uniform, the lineage
  is the ancestors traced back, the path starts at x0, and the replayed state at every observation row is the filter's stored
  particle (1e-12 relative: in float64 the replay is the filter's own arithmetic).
* Dead filters, keys, validation.
* Statistics: M = 4096 independent draws against the exact Rauch-Tung-Striebel smoother of the discretised OU model: mean z < 5 at
  every grid row, sample variance within 5 sqrt(2 / (M - 1)) relative (5 sigma of a variance estimate from M Gaussian draws).
* smooth_paths returns the numbers of reweight_parameters under the same seed, and float64 numpy weighted moments / quantiles of its
  own draws.
* The six replay entry points refuse bad arguments before any HIP call."""
import math

import numpy as np
import pytest
import torch

import particle_smoother_reference as sref

N = 64


def _key(k0, k1):
    return torch.from_numpy(np.array([k0, k1], dtype=np.uint32).view(np.int32))


def _double(obs):
    from viforsdes_amd import Observations
    return Observations(times=obs.times.double(), values=obs.values.double())


_RUNS = {}


def _run(name, rows, proposal, D, M=3):
    """One float64 smoother run and the filter run of the same key (shared by the stage tests and left unchanged)."""
    tag = (name, tuple(rows), proposal, D)
    if tag not in _RUNS:
        from viforsdes_amd import particle_filter, particle_smoother
        sde, obs, like, th, x0, dt, pos = sref.case(name, M, rows=rows)
        key = (0x51ED270B + D, 0x2545F491 ^ len(name))
        kw = dict(n_particles=N, initial_state=x0.double(), positive_dims=pos, key=_key(*key), proposal=proposal)
        sm = particle_smoother(sde, _double(obs), like, th.double(), dt, n_draws=D, **kw)
        pf = particle_filter(sde, _double(obs), like, th.double(), dt, return_particles=True, **kw)
        _RUNS[tag] = (sm, pf, x0.double(), pos, key)
    return _RUNS[tag]


STAGE = [(name, rows, proposal, D) for name in ("ou", "lv", "sir") for rows in (sref.BLOCK_ROWS, sref.LATE_ROWS)
         for proposal in ("bootstrap", "bridge") for D in (1, 7, N + 5)]


# -------------------------------------------------------------------------------------------------------------- 1. stage checks
@pytest.mark.parametrize("name,rows,proposal,D", STAGE)
def test_stages_match_the_filter_in_float64(name, rows, proposal, D):
    sm, pf, x0, pos, key = _run(name, rows, proposal, D)
    M, K, S = x0.shape[0], len(rows), x0.shape[1]
    assert sm.paths.shape == (M, D, rows[-1] + 1, S) and sm.paths.dtype == torch.float64
    assert sm.lineage.shape == (M, D, K) and sm.lineage.dtype == torch.int32 and sm.distinct_lineages.shape == (M, K)
    for f in ("log_likelihood", "increments", "effective_sample_size", "filtered_mean", "filtered_std"):
        assert torch.equal(getattr(sm, f), getattr(pf, f)), f
    assert bool(torch.isfinite(sm.log_likelihood).all())
    lin = sm.lineage.long()
    # final slots: float64 systematic sampling of the final weights with the specified uniform
    u = sref.smoothing_uniforms(M, key)
    for m in range(M):
        lw = pf.log_weights[m, -1].numpy()
        assert np.array_equal(lin[m, :, -1].numpy(), sref.systematic_draws(np.exp(lw - lw.max()), u[m], D))
    # trace
    for k in range(K - 1, 0, -1):
        assert torch.equal(lin[:, :, k - 1], torch.gather(pf.ancestors[:, k - 1].long(), 1, lin[:, :, k]))
    assert bool((lin >= 0).all()) and bool((lin < N).all())
    for m in range(M):
        for k in range(K):
            assert int(sm.distinct_lineages[m, k]) == len(set(lin[m, :, k].tolist()))
    # replay
    assert torch.equal(sm.paths[:, :, 0], x0[:, None, :].expand(M, D, S))
    assert bool(torch.isfinite(sm.paths).all())
    worst = 0.0
    for k in range(K):
        want = torch.gather(pf.particles[:, k], 1, lin[:, :, k, None].expand(-1, -1, S))
        worst = max(worst, float(((sm.paths[:, :, rows[k]] - want).abs() / want.abs().clamp(min=1e-300)).max()))
    print(f"{name} rows {rows} {proposal} D={D}: replayed state at the observation rows vs stored particle, max relative {worst:.1e}")
    assert worst <= 1e-12
    if pos:
        assert bool((sm.paths[..., list(pos)] >= 1e-6).all())


def test_block_rows_share_a_row_and_late_rows_start_with_steps():
    sm, pf, x0, _, _ = _run("ou", sref.BLOCK_ROWS, "bootstrap", 7)
    assert torch.equal(pf.particles[:, 2], torch.gather(pf.particles[:, 1], 1, pf.ancestors[:, 1].long()[..., None]))
    sm, pf, x0, _, _ = _run("ou", sref.LATE_ROWS, "bootstrap", 7)
    assert not torch.equal(sm.paths[:, :, 1], sm.paths[:, :, 0])          # segment 0 has steps of its own


def test_reference_path_noise_is_forecast_noise_of_those_paths():
    from philox_reference import forecast_noise
    key = (0x1234ABCD, 0xDEADBEEF)
    full = forecast_noise(70, 11, 3, key)
    assert np.array_equal(sref.path_noise([69, 0, 7, 7], 11, 3, key), full[[69, 0, 7, 7]])


# --------------------------------------------------------------------------------------------------------- 2. dead filters, keys
@pytest.mark.parametrize("proposal", ["bootstrap", "bridge"])
def test_dead_filter_gives_nan_paths_and_leaves_the_others_alone(proposal):
    from viforsdes_amd import particle_smoother
    sde, obs, like, th, x0, dt, pos = sref.case("ou", 3)
    bad = x0.clone()
    bad[1] = float("nan")
    kw = dict(n_particles=N, n_draws=5, key=_key(4, 4), proposal=proposal)
    a = particle_smoother(sde, obs, like, th, dt, initial_state=bad, **kw)
    b = particle_smoother(sde, obs, like, th, dt, initial_state=x0, **kw)
    assert float(a.log_likelihood[1]) == float("-inf")
    assert bool(torch.isnan(a.paths[1]).all()) and bool((a.lineage[1] == -1).all()) and bool((a.distinct_lineages[1] == 0).all())
    for m in (0, 2):
        assert torch.equal(a.paths[m], b.paths[m]) and torch.equal(a.lineage[m], b.lineage[m])
        assert bool(torch.isfinite(a.paths[m]).all())


def test_same_key_same_result_and_the_default_key_comes_from_the_torch_generator():
    from viforsdes_amd import particle_smoother
    sde, obs, like, th, x0, dt, pos = sref.case("ou", 2)
    a = particle_smoother(sde, obs, like, th, dt, n_particles=N, n_draws=3, key=_key(1, 2))
    b = particle_smoother(sde, obs, like, th, dt, n_particles=N, n_draws=3, key=_key(1, 2))
    c = particle_smoother(sde, obs, like, th, dt, n_particles=N, n_draws=3, key=_key(1, 3))
    assert torch.equal(a.paths, b.paths) and torch.equal(a.lineage, b.lineage) and not torch.equal(a.paths, c.paths)
    torch.manual_seed(3)
    d = particle_smoother(sde, obs, like, th, dt, n_particles=N)
    torch.manual_seed(3)
    e = particle_smoother(sde, obs, like, th, dt, n_particles=N)
    f = particle_smoother(sde, obs, like, th, dt, n_particles=N)
    assert torch.equal(d.paths, e.paths) and not torch.equal(e.paths, f.paths)
    assert d.paths.shape == (2, 1, 101, 1)
    one = particle_smoother(sde, obs, like, th[0], dt, n_particles=N, key=_key(1, 2))          # theta [P]: M = 1
    assert one.paths.shape == (1, 1, 101, 1)


def test_validation():
    from viforsdes_amd import PoissonObservationLikelihood, particle_smoother
    sde, obs, like, th, x0, dt, pos = sref.case("ou", 1)
    with pytest.raises(ValueError, match="n_draws"):
        particle_smoother(sde, obs, like, th, dt, n_draws=0)
    with pytest.raises(ValueError, match="n_particles"):
        particle_smoother(sde, obs, like, th, dt, n_particles=0)
    with pytest.raises(ValueError, match="time_step"):
        particle_smoother(sde, obs, like, th, 0.0)
    with pytest.raises(ValueError, match="theta"):
        particle_smoother(sde, obs, like, torch.ones(2, 4), dt)
    with pytest.raises(ValueError, match="initial_state"):
        particle_smoother(sde, obs, like, th, dt, initial_state=torch.ones(3, 1))
    with pytest.raises(ValueError, match="key"):
        particle_smoother(sde, obs, like, th, dt, key=torch.zeros(3, dtype=torch.int32))
    with pytest.raises(ValueError, match="proposal"):
        particle_smoother(sde, obs, like, th, dt, proposal="auxiliary")
    with pytest.raises(ValueError, match="bridge"):
        particle_smoother(sde, obs, PoissonObservationLikelihood(), th, dt, proposal="bridge")


# ---------------------------------------------------------------------------------------------------------------- 3. statistics
@pytest.mark.parametrize("proposal", ["bootstrap", "bridge"])
def test_ou_draws_follow_the_exact_smoothing_distribution(proposal):
    from viforsdes_amd import particle_smoother
    from viforsdes_amd.examples.sdes import ou_problem
    sde, obs, like, _, _, dt, _, _ = ou_problem()
    theta, M, n = (0.8, 1.0, 0.5), 4096, 256
    rows = np.round(obs.times.numpy() / dt).astype(int)
    mean, var = sref.ou_rts(theta, dt, like.variance, obs.values[0].numpy(), rows, obs.values.numpy())
    res = particle_smoother(sde, obs, like, torch.tensor([theta]).expand(M, 3), dt, n_particles=n, n_draws=1, key=_key(17, 23),
                            proposal=proposal)
    x = res.paths[:, 0, :, 0].double().numpy()                                   # [M, T+1]: one draw per independent filter
    assert np.array_equal(x[:, 0], np.full(M, 2.0)) and mean[0] == 2.0 and var[0] == 0.0
    z = np.abs(x[:, 1:].mean(axis=0) - mean[1:]) / np.sqrt(x[:, 1:].var(axis=0, ddof=1) / M)
    ratio = x[:, 1:].var(axis=0, ddof=1) / var[1:]
    band = 5.0 * math.sqrt(2.0 / (M - 1))
    print(f"OU smoother ({proposal}): max z {z.max():.2f}, variance ratio {ratio.min():.3f} .. {ratio.max():.3f} (band +-{band:.3f}), "
          f"smallest particle ESS {float(res.effective_sample_size.min()):.0f}")
    assert z.max() < 5.0
    assert np.abs(ratio - 1.0).max() < band


# --------------------------------------------------------------------------------------------------------------- 4. smooth_paths
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
    vp = VariationalPosterior(model=model, exponential_moving_average=ExponentialMovingAverage(model), prior=prior,
                              observations=obs, time_horizon=horizon, time_step=dt, state_space=StateSpace(1, []),
                              evidence_lower_bound_history=[], device=torch.device("cpu"))
    return sde, like, vp


@pytest.mark.parametrize("proposal", ["bootstrap", "bridge"])
def test_smooth_paths_matches_reweight_parameters_and_numpy_moments(proposal):
    from viforsdes_amd import PathReweighting
    from viforsdes_amd.posterior.variational_posterior import QUANTILE_LEVELS
    sde, like, vp = _cpu_posterior()
    n = 300
    torch.manual_seed(21)
    sp = vp.smooth_paths(sde, like, n_samples=n, n_particles=64, chunk_size=128, proposal=proposal)
    assert vp._captured == {} and vp._calls == {}
    torch.manual_seed(21)
    rw = vp.reweight_parameters(sde, like, n_samples=n, n_particles=64, chunk_size=128, proposal=proposal)
    assert isinstance(sp, PathReweighting) and sp.n_samples == n and sp.n_nonfinite == 0
    assert sp.log_evidence == rw.log_evidence and sp.effective_sample_size == rw.effective_sample_size
    assert sp.standard_error == rw.standard_error
    assert torch.equal(sp.filter_effective_sample_size, rw.filter_effective_sample_size)
    assert torch.equal(sp.sde_parameters, rw.sde_parameters) and torch.equal(sp.log_weights, rw.log_weights)
    T1 = 101
    assert sp.paths.shape == (n, T1, 1) and sp.times.shape == (T1,) and abs(float(sp.times[-1]) - 5.0) < 1e-5
    assert sp.path_mean.shape == (T1, 1) and sp.path_std.shape == (T1, 1)
    x = sp.paths.double().numpy().reshape(n, T1)
    lw = sp.log_weights.numpy()
    w = np.exp(lw - lw.max())
    wn = w / w.sum()
    mean = (wn[:, None] * x).sum(axis=0)
    std = np.sqrt((wn[:, None] * (x - mean) ** 2).sum(axis=0))
    assert np.allclose(sp.path_mean.numpy()[:, 0], mean, rtol=1e-5, atol=1e-6)
    assert np.allclose(sp.path_std.numpy()[:, 0], std, rtol=1e-5, atol=1e-6)
    q = sp.path_quantiles
    for level, got in zip(QUANTILE_LEVELS, (q.q05, q.q25, q.q50, q.q75, q.q95)):
        assert got.shape == (T1, 1)
        for t in range(T1):
            order = np.argsort(x[:, t], kind="stable")
            cdf = np.cumsum(wn[order])
            want = x[order, t][min(int((cdf < level).sum()), n - 1)]
            assert abs(float(got[t, 0]) - want) < 1e-6, (level, t)
    assert float(sp.path_mean[0, 0]) == 2.0 and float(sp.path_std[0, 0]) == 0.0         # every path starts at the first observation
    short = vp.smooth_paths(sde, like, n_samples=10, n_particles=64, return_draws=False)
    assert short.paths is None and short.sde_parameters is None and short.log_weights is None
    assert short.path_mean.shape == (T1, 1)


def test_smooth_paths_validation():
    from viforsdes_amd.examples.sdes import LinearDiagonalSDE
    sde, like, vp = _cpu_posterior()
    with pytest.raises(ValueError, match="state_dim"):
        vp.smooth_paths(LinearDiagonalSDE(2), like, n_samples=8)
    with pytest.raises(ValueError, match="n_samples"):
        vp.smooth_paths(sde, like, n_samples=0)
    with pytest.raises(ValueError, match="proposal"):
        vp.smooth_paths(sde, like, n_samples=8, proposal="auxiliary")


# ------------------------------------------------------------------------------------------------------------------------ 5. ABI
def test_replay_entry_points_refuse_bad_arguments_before_any_hip_call():
    """No GPU here: the checks return VSDE_E_BADARG (-1) with every pointer NULL, so nothing was launched or dereferenced."""
    import ctypes
    from viforsdes_amd import _hip
    lib = _hip.load()
    null, dbl = ctypes.c_void_p(None), ctypes.c_double
    ints = lambda *v: [ctypes.c_int(x) for x in v]
    # (x0, theta, obs_rows, key, time_step, mask, particles, ancestors, last_slot, paths, lineage, stream)
    plain_tail = [null] * 4 + [dbl(0.05)] + [null] * 7
    # (x0, theta, obs_rows, obs_values, obs_matrix, variance, key, time_step, mask, particles, ..., stream)
    guided_tail = [null] * 5 + [dbl(0.1), null, dbl(0.05)] + [null] * 7

    def plain(kind, M, n, S, P, K, O, D, T):
        return lib.vsde_filter_replay(*ints(kind, M, n, S, P, K, O, D, T), *plain_tail)

    def guided(kind, M, n, S, P, K, O, D, T):
        return lib.vsde_guided_filter_replay(*ints(kind, M, n, S, P, K, O, D, T), *guided_tail)

    for fn in (plain, guided):
        for args, word in [((1, 4, 100, 1, 3, 6, 1, 2, 100), b"particles"), ((1, 4, 2048, 1, 3, 6, 1, 2, 100), b"particles"),
                           ((1, 4, 64, 1, 3, 6, 1, 0, 100), b"draws"), ((1, 4, 64, 1, 3, 6, 1, -3, 100), b"draws"),
                           ((1, 4, 64, 1, 3, 0, 1, 2, 100), b"K=0"), ((1, 4, 64, 1, 3, 6, 1, 2, -1), b"grid steps"),
                           ((7, 4, 64, 1, 3, 6, 1, 2, 100), b"kind"), ((2, 4, 64, 1, 3, 6, 1, 2, 100), b"Lotka"),
                           ((1, 4, 64, 1, 3, 6, 1, 2, 100), b"NULL")]:
            assert fn(*args) == -1 and word in lib.vsde_last_error(), (fn.__name__, args, lib.vsde_last_error())
    assert plain(3, 4, 64, 17, 34, 6, 17, 2, 100) == -1 and b"state_dim" in lib.vsde_last_error()
    assert plain(3, 4, 64, 2, 4, 6, 17, 2, 100) == -1 and b"obs_dim" in lib.vsde_last_error()
    assert guided(3, 4, 64, 5, 10, 6, 5, 2, 100) == -1 and b"guided particle filter: state_dim" in lib.vsde_last_error()
    assert guided(3, 4, 64, 2, 4, 6, 5, 2, 100) == -1 and b"guided particle filter: obs_dim" in lib.vsde_last_error()
    net = _hip.CrnNetwork()
    net.S, net.R = 2, 17
    kin = _hip.CrnKinetics()
    assert lib.vsde_crn_filter_replay(ctypes.byref(net), *ints(4, 64, 2, 17, 6, 2, 2, 100), *plain_tail) == -1
    assert b"reactions" in lib.vsde_last_error()
    assert lib.vsde_crn_guided_filter_replay(ctypes.byref(net), *ints(4, 64, 2, 17, 6, 2, 2, 100), *guided_tail) == -1
    assert b"reactions" in lib.vsde_last_error()
    net.R = 2
    for entry, tail in ((lib.vsde_crn_filter_replay, plain_tail), (lib.vsde_crn_guided_filter_replay, guided_tail)):
        assert entry(ctypes.byref(net), *ints(4, 64, 2, 2, 6, 2, 0, 100), *tail) == -1 and b"draws" in lib.vsde_last_error()
        assert entry(ctypes.byref(net), *ints(4, 96, 2, 2, 6, 2, 2, 100), *tail) == -1 and b"particles" in lib.vsde_last_error()
        assert entry(ctypes.byref(net), *ints(4, 64, 2, 2, 6, 2, 2, 100), *tail) == -1 and b"NULL" in lib.vsde_last_error()
    kin.law[0] = 9
    for entry, tail in ((lib.vsde_crn_kinetic_filter_replay, plain_tail), (lib.vsde_crn_kinetic_guided_filter_replay, guided_tail)):
        assert entry(ctypes.byref(net), ctypes.byref(kin), *ints(4, 64, 2, 4, 6, 2, 2, 100), *tail) == -1
        assert b"law code" in lib.vsde_last_error()
    kin.law[0] = 0
    for entry, tail in ((lib.vsde_crn_kinetic_filter_replay, plain_tail), (lib.vsde_crn_kinetic_guided_filter_replay, guided_tail)):
        assert entry(ctypes.byref(net), ctypes.byref(kin), *ints(4, 64, 2, 4, 6, 2, 0, 100), *tail) == -1
        assert b"draws" in lib.vsde_last_error()
        assert entry(ctypes.byref(net), ctypes.byref(kin), *ints(4, 64, 2, 4, 6, 2, 2, 100), *tail) == -1
        assert b"NULL" in lib.vsde_last_error()
