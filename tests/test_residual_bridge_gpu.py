"""GPU: the residual-bridge variant of the three kernels that run the filter's step (csrc/vsde_residual.hip: pf_kernel, rp_kernel,
ar_kernel with RES) through the public ``particle_filter`` / ``particle_smoother(..., proposal="residual_bridge")`` and the
``residual=True`` wrappers of ``_hip``.

Stage by stage against float64 on the kernel's own previous stage, as tests/test_guided_filter_gpu.py does and with its bounds:

* propagation and log-ratio: particles and ``log_weights`` at observation k against the float64 reference segment
  (tests/residual_bridge_reference.py, which makes its own passes of the companion path) started from the kernel's particles at
  k - 1 gathered through the kernel's ancestors.  Particles: 2e-4 of the largest magnitude.  ``log_weights``: E32 = the error of
  the SAME reference run in fp32 against float64 on the same starts, measured per segment; the kernel gets 4 E32 + 1e-5 max(1,
  largest finite |lw|);
* increments, ESS, mean, std from the kernel's own log_weights and particles in float64: 1e-5 / 1e-4;
* ancestors against float64 systematic resampling of those weights: at most 1e-3 differ, each by exactly 1, the float64 ESS above
  N / 20 at every observation (rows [0, 1, 3, 3, 8, 20] for every case, the Lotka-Volterra ones included);
* both replays repeat the filter's stored particles at every observation row BIT FOR BIT: what catches a replay whose companion
  path starts from another state than the filter's;
* kernel route against torch route on the SIR network, and the routing of what the kernel does not take."""
import math

import numpy as np
import pytest
import torch

import guided_filter_reference as gref
import particle_filter_reference as ref
import residual_bridge_reference as rref
from philox_reference import forecast_noise

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
PROPOSAL = "residual_bridge"
CASES = ["ou", "lv", "lv_prey", "sir", "chain4", "autoreg", "chain4_full", "lindiag3"]
KIND = {"ou": "ornstein_uhlenbeck", "lv": "lotka_volterra", "lv_prey": "lotka_volterra", "sir": "reaction_network",
        "chain4": "reaction_network", "autoreg": "reaction_network", "chain4_full": "reaction_network", "lindiag3": "linear_diagonal"}
STATE_DIM = {"ou": 1, "chain4": 4, "chain4_full": 4, "lindiag3": 3}


def _key(k0, k1, dev=DEV):
    return torch.from_numpy(np.array([k0, k1], dtype=np.uint32).view(np.int32)).to(dev)


def _max_n(name):
    from viforsdes_amd import _hip
    return _hip.particle_filter_max_particles(KIND[name], STATE_DIM.get(name, 2), proposal=PROPOSAL)


def _counted(fn):
    """(result of fn(), number of residual kernel calls, of bridge kernel calls, of bootstrap kernel calls it made)."""
    from viforsdes_amd import _hip
    calls = {"residual": 0, "bridge": 0, "bootstrap": 0}
    real_g, real_b = _hip.guided_particle_filter, _hip.particle_filter

    def guided(*a, **k):
        calls["residual" if k.get("residual") else "bridge"] += 1
        return real_g(*a, **k)

    def bootstrap(*a, **k):
        calls["bootstrap"] += 1
        return real_b(*a, **k)

    _hip.guided_particle_filter, _hip.particle_filter = guided, bootstrap
    try:
        out = fn()
    finally:
        _hip.guided_particle_filter, _hip.particle_filter = real_g, real_b
    return out, calls["residual"], calls["bridge"], calls["bootstrap"]


_RUNS = {}


def _cached(name, N):
    """One kernel-route run of the case (M = 64), shared by the stage tests and left unchanged."""
    tag = (name, N)
    if tag not in _RUNS:
        from viforsdes_amd import particle_filter
        sde, obs, like, th, x0, dt, pos = gref.case(name, 64, rows=rref.ROWS)
        key = (0x9E3779B9 ^ N, 0x7F4A7C15 + len(name))
        res, residual, bridge, bootstrap = _counted(lambda: particle_filter(
            sde, obs.to(DEV), like, th.to(DEV), dt, n_particles=N, initial_state=x0.to(DEV), positive_dims=pos, return_particles=True,
            key=_key(*key), proposal=PROPOSAL))
        assert (residual, bridge, bootstrap) == (1, 0, 0)            # the public function took the residual kernel, exactly once
        _RUNS[tag] = (sde, obs, like, th, x0, dt, pos, res, key)
    return _RUNS[tag]


def _params():
    return [pytest.param(name, big, id=f"{name}-{'max' if big else '64'}") for name in CASES for big in (False, True)]


def _n(name, big):
    return _max_n(name) if big else 64


def _gauss32(y, x, variance, H):
    x = x.astype(np.float32)
    pred = x if H is None else x @ H.astype(np.float32).T
    r = y.astype(np.float32) - pred
    lw = (np.float32(-0.5) * r * r / np.float32(variance) - np.float32(0.5 * math.log(2.0 * math.pi * variance))).sum(axis=-1)
    return lw.astype(np.float32)


def _segment_references(sde, like, th, dt, pos, start, z, y, N):
    """(x64, lw64, lw32): the reference segment from ``start`` in float64, and its log-weights when run in fp32."""
    H = None if like.obs_matrix is None else like.obs_matrix.double().numpy()
    theta = np.repeat(th.double().numpy(), N, axis=0)
    x64, lr64, _ = rref.residual_segment(gref.sde_coefficients(sde), start, theta, z, y, H, like.variance, dt, pos)
    lw64 = lr64 + ref.gaussian_log_weights(y, x64, like.variance, H)
    x32, lr32, _ = rref.residual_segment(gref.sde_coefficients(sde, np.float32), start, theta, z, y, H, like.variance, dt, pos, np.float32)
    with np.errstate(all="ignore"):
        lw32 = (lr32 + _gauss32(y, x32, like.variance, H)).astype(np.float64)
    return x64, lw64, np.where(np.isnan(lw32), -np.inf, lw32)


def _lw_errors(got, lw64, lw32):
    """(kernel error, fp32 reference error, bound) over the entries finite in float64."""
    ok = np.isfinite(lw64)
    assert ok.any() and np.isfinite(got[ok]).all()
    e_k, e_32 = float(np.abs(got[ok] - lw64[ok]).max()), float(np.abs(lw32[ok] - lw64[ok]).max())
    return e_k, e_32, 4.0 * e_32 + 1e-5 * max(1.0, float(np.abs(lw64[ok]).max()))


# ------------------------------------------------------------------------------------------- 7a. propagation and log-ratio
@pytest.mark.parametrize("name,big", _params())
def test_propagation_and_log_ratio_match_the_float64_segment(name, big):
    N = _n(name, big)
    sde, obs, like, th, x0, dt, pos, res, key = _cached(name, N)
    M, K, S, rows = th.shape[0], obs.values.shape[0], sde.state_dim, rref.ROWS
    parts, anc = res.particles.double().cpu().numpy(), res.ancestors.long().cpu().numpy()
    lw = res.log_weights.double().cpu().numpy()
    assert np.isfinite(parts).all() and lw.shape == (M, K, N)
    assert np.array_equal(parts[:, 0], np.broadcast_to(x0.double().numpy()[:, None, :], (M, N, S)))
    H = None if like.obs_matrix is None else like.obs_matrix.double().numpy()
    noise = forecast_noise(M * N, rows[-1], S, key)
    worst_x = 0.0
    for k in range(K):
        y = obs.values[k].double().numpy()
        if k == 0 or rows[k] == rows[k - 1]:          # no step since the last observation: the plain Gaussian weight
            if k > 0:
                start = np.take_along_axis(parts[:, k - 1], anc[:, k - 1, :, None], axis=1)
                assert np.array_equal(parts[:, k], start)
            want = ref.gaussian_log_weights(y, parts[:, k], like.variance, H)
            ok = np.isfinite(want)
            e = float(np.abs(lw[:, k][ok] - want[ok]).max())
            print(f"{name} N={N} k={k} (no step): log-weight error {e:.2e}")
            assert e <= 1e-5 * max(1.0, float(np.abs(want[ok]).max()))
            continue
        start = np.take_along_axis(parts[:, k - 1], anc[:, k - 1, :, None], axis=1).reshape(M * N, S)
        x64, lw64, lw32 = _segment_references(sde, like, th, dt, pos, start, noise[:, rows[k - 1]:rows[k]], y, N)
        e_x = float(np.abs(parts[:, k].reshape(M * N, S) - x64).max() / np.abs(x64).max())
        e_k, e_32, bound = _lw_errors(lw[:, k].reshape(M * N), lw64, lw32)
        print(f"{name} N={N} k={k} (n = {rows[k] - rows[k - 1]}): particles {e_x:.2e} of the largest magnitude; log-weights: kernel "
              f"{e_k:.2e}, fp32 reference {e_32:.2e}, bound {bound:.2e}")
        worst_x = max(worst_x, e_x)
        assert e_k <= bound
    assert worst_x < 2e-4
    if pos:
        assert (parts[..., list(pos)] >= gref.STATE_FLOOR).all()
        assert (parts[:, 1:][..., list(pos)] == gref.STATE_FLOOR).any()    # the clamp was exercised


# ---------------------------------------------------------------------------------------------- 7b. weights and summaries
@pytest.mark.parametrize("name,big", _params())
def test_summaries_match_float64_on_the_kernels_weights_and_particles(name, big):
    N = _n(name, big)
    sde, obs, like, th, x0, dt, pos, res, key = _cached(name, N)
    M, K = th.shape[0], obs.values.shape[0]
    parts, lws = res.particles.double().cpu().numpy(), res.log_weights.double().cpu().numpy()
    got = [t.double().cpu().numpy() for t in (res.increments, res.effective_sample_size, res.filtered_mean, res.filtered_std)]
    e_inc = e_ess = e_mean = e_std = 0.0
    for m in range(M):
        for k in range(K):
            lw = lws[m, k]
            inc, ess, mean, std, w = ref.observation_stage(lw, parts[m, k])
            size = (w[:, None] * np.abs(parts[m, k])).sum(axis=0) / w.sum()
            e_inc = max(e_inc, abs(got[0][m, k] - inc) / max(1.0, np.abs(lw[np.isfinite(lw)]).max()))
            e_ess = max(e_ess, abs(got[1][m, k] - ess) / ess)
            e_mean = max(e_mean, float((np.abs(got[2][m, k] - mean) / np.maximum(size, 1e-30)).max()))
            e_std = max(e_std, float((np.abs(got[3][m, k] - std) / (std + 1e-2 * size + 1e-30)).max()))
    print(f"{name} N={N}: increments {e_inc:.2e} (of max(1, |lw|)), ESS {e_ess:.2e}, mean {e_mean:.2e}, std {e_std:.2e} (relative)")
    assert e_inc < 1e-5
    assert e_ess < 1e-4 and e_mean < 1e-4 and e_std < 1e-4
    total = res.increments.double().sum(dim=1)
    assert torch.allclose(res.log_likelihood.double(), total, rtol=1e-6, atol=1e-5 * float(res.increments.abs().max()))


# --------------------------------------------------------------------------------------------------------- 7c. ancestors
@pytest.mark.parametrize("name,big", _params())
def test_ancestors_match_float64_systematic_resampling(name, big):
    N = _n(name, big)
    sde, obs, like, th, x0, dt, pos, res, key = _cached(name, N)
    M, K = th.shape[0], obs.values.shape[0]
    lws = res.log_weights.double().cpu().numpy()
    anc = res.ancestors.cpu().numpy().astype(np.int64)
    assert anc.min() >= 0 and anc.max() < N
    assert (np.diff(anc, axis=-1) >= 0).all()
    u = ref.resampling_uniforms(M, K, key)
    differ, low = 0, float("inf")
    for m in range(M):
        for k in range(K):
            w = np.exp(lws[m, k] - lws[m, k].max())
            low = min(low, w.sum() ** 2 / (w * w).sum())
            d = np.abs(anc[m, k] - ref.systematic_ancestors(w, u[m, k]))
            assert d.max() <= 1, (m, k, int(d.max()))
            differ += int((d != 0).sum())
    print(f"{name} N={N}: {differ} of {anc.size} ancestors differ from float64 ({differ / anc.size:.1e}); smallest float64 ESS {low:.1f}")
    assert low > N / 20
    assert differ <= 1e-3 * anc.size


# ------------------------------------------------------------------------------------------------------ 8. both replays
REPLAY_CASES = ["ou", "lv", "lv_prey", "sir", "autoreg", "chain4", "chain4_full", "lindiag3"]


def _smoother_call(name, N, D=3, M=5):
    """One kernel-route ``particle_smoother`` run with the residual bridge: (arguments its replay wrapper was given, its keyword
    arguments, the paths and lineage it returned, the filter's result for the same key)."""
    from viforsdes_amd import _hip, particle_filter, particle_smoother
    sde, obs, like, th, x0, dt, pos = gref.case(name, M, rows=rref.ROWS)
    calls, real = [], _hip.guided_filter_replay

    def recording(*a, **k):
        out = real(*a, **k)
        calls.append((a, k, out))
        return out

    kw = dict(n_particles=N, initial_state=x0.to(DEV), positive_dims=pos, key=_key(0x1234 + N, 0x77 + len(name)), proposal=PROPOSAL)
    _hip.guided_filter_replay = recording
    try:
        sm = particle_smoother(sde, obs.to(DEV), like, th.to(DEV), dt, n_draws=D, **kw)
    finally:
        _hip.guided_filter_replay = real
    assert len(calls) == 1 and calls[0][1].get("residual") is True         # the kernel route, the residual replay
    pf = particle_filter(sde, obs.to(DEV), like, th.to(DEV), dt, return_particles=True, **kw)
    assert torch.equal(pf.log_likelihood, sm.log_likelihood)
    return calls[0], sm, pf


@pytest.mark.parametrize("name", REPLAY_CASES)
def test_both_replays_repeat_the_filters_stored_particles_bit_for_bit(name):
    from viforsdes_amd import _hip
    N = 64
    (args, kw, (paths, lineage)), sm, pf = _smoother_call(name, N)
    kind, x0, th, obs_rows, values, H, variance, key, dt, particles, ancestors, last, pos = args
    rows = rref.ROWS
    M, D, K = lineage.shape
    S = particles.shape[3]
    assert torch.equal(particles, pf.particles) and torch.equal(sm.paths, paths) and bool(torch.isfinite(paths).all())
    lin = lineage.long()
    # the genealogy replay: the path of a draw passes through the stored particle of its lineage at every observation row
    stored = torch.gather(pf.particles, 2, lin.permute(0, 2, 1)[..., None].expand(M, K, D, S)).permute(0, 2, 1, 3)     # [M, D, K, S]
    for k in range(K):
        assert torch.equal(paths[:, :, rows[k]].view(torch.int32), stored[:, :, k].view(torch.int32)), k
    # the anchored replay of the same records: the same paths, so the same stored particles
    anchors = stored.reshape(M * D, K, S).contiguous()
    noise = (torch.arange(M, device=DEV)[:, None, None] * N + lin).to(torch.int32).reshape(M * D, K)
    rep = lambda t: t.repeat_interleave(D, dim=0)
    got = _hip.guided_anchored_replay(kind, rep(x0), rep(th), obs_rows, values, H, variance, anchors, noise,
                                      key.reshape(1, 2).repeat(M * D, 1), dt, pos, **kw)
    assert got.shape == (M * D, rows[-1] + 1, S)
    assert torch.equal(got.view(M, D, -1, S).view(torch.int32), paths.view(torch.int32))
    for k in range(K):
        assert torch.equal(got[:, rows[k]].view(torch.int32), anchors[:, k].view(torch.int32)), k
    # and the bridge's replay of these records is another path: the flag reaches the kernel
    other = _hip.guided_anchored_replay(kind, rep(x0), rep(th), obs_rows, values, H, variance, anchors, noise,
                                        key.reshape(1, 2).repeat(M * D, 1), dt, pos, **{**kw, "residual": False})
    if name != "ou":                                  # the OU drift is linear: there the two proposals agree to rounding
        assert not torch.equal(other, got)


def test_pmmh_path_records_replay_through_their_anchors_bit_for_bit(monkeypatch):
    """``particle_mcmc(return_paths=True, proposal="residual_bridge")`` on the kernel route: every kept path passes through the
    anchors of its record (the filter's stored particles) at the observation rows, bit for bit."""
    import particle_mcmc_reference as mref
    from viforsdes_amd import GaussianObservationLikelihood, Observations, Prior, PriorType, _hip, particle_mcmc
    from viforsdes_amd.examples.sdes import OrnsteinUhlenbeck
    obs = Observations(times=torch.tensor(mref.OU_TIMES), values=torch.tensor(mref.OU_VALUES)[:, None]).to(DEV)
    prior = Prior(type=PriorType.LOG_NORMAL, mean=mref.OU_PRIOR[1], std=mref.OU_PRIOR[2], dim=3)
    like = GaussianObservationLikelihood(variance=mref.OU_VARIANCE)
    calls, real = [], _hip.guided_anchored_replay

    def recording(*a, **k):
        out = real(*a, **k)
        calls.append((a, k, out))
        return out

    monkeypatch.setattr(_hip, "guided_anchored_replay", recording)
    res = particle_mcmc(OrnsteinUhlenbeck(), obs, like, prior, mref.OU_DT, torch.tensor(mref.ou_initial_theta(5), device=DEV,
                                                                                       dtype=torch.float32), 6,
                        n_particles=64, filters_per_chain=2, theta_positive_dims=(0, 1, 2), key=_key(11, 13), proposal=PROPOSAL,
                        return_paths=True)
    assert len(calls) == 1 and calls[0][1].get("residual") is True
    a, _, paths = calls[0]
    anchors = a[7]
    assert bool(torch.isfinite(res.paths).all()) and bool((res.path_iteration >= 0).all())
    for k, row in enumerate(mref.OU_ROWS):
        assert torch.equal(paths[:, row].view(torch.int32), anchors[:, k].view(torch.int32)), k


# --------------------------------------------------------------------------------------- 9. kernel route against torch route
def test_kernel_route_and_torch_route_agree_on_the_sir_network(monkeypatch):
    from viforsdes_amd import particle_filter
    from viforsdes_amd.inference import particle_filter as pf
    M, N = 512, 128
    sde, obs, like, th, x0, dt, pos = gref.case("sir", M, rows=rref.ROWS)
    th, x0 = th[1:2].expand(M, 2).contiguous(), x0[1:2].expand(M, 2).contiguous()
    run = lambda k: particle_filter(sde, obs.to(DEV), like, th.to(DEV), dt, n_particles=N, initial_state=x0.to(DEV),
                                    positive_dims=pos, key=_key(*k), proposal=PROPOSAL).log_likelihood.double().cpu().numpy()
    a, residual, _, _ = _counted(lambda: run((31, 32)))
    monkeypatch.setattr(pf, "HIP_FILTER", False)
    b, residual_off, _, _ = _counted(lambda: run((33, 34)))
    assert (residual, residual_off) == (1, 0)
    z = abs(a.mean() - b.mean()) / math.sqrt(a.var(ddof=1) / M + b.var(ddof=1) / M)
    print(f"SIR, residual bridge: mean log p^ kernel {a.mean():.4f}, torch {b.mean():.4f}, two-sample z {z:.2f}")
    assert z < 5.0


# ------------------------------------------------------------------------------------------------------------- 10. routing
def test_too_many_particles_take_the_torch_route():
    from viforsdes_amd import _hip, particle_filter
    assert _hip.particle_filter_max_particles("reaction_network", 4, proposal=PROPOSAL) == 512
    sde, obs, like, th, x0, dt, pos = gref.case("chain4", 2, rows=rref.ROWS)
    run = lambda n: _counted(lambda: particle_filter(sde, obs.to(DEV), like, th.to(DEV), dt, n_particles=n, initial_state=x0.to(DEV),
                                                     positive_dims=pos, key=_key(1, 2), proposal=PROPOSAL))
    res, residual, bridge, bootstrap = run(1024)
    assert (residual, bridge, bootstrap) == (0, 0, 0) and bool(torch.isfinite(res.log_likelihood).all())
    res, residual, bridge, bootstrap = run(512)
    assert (residual, bridge, bootstrap) == (1, 0, 0) and bool(torch.isfinite(res.log_likelihood).all())


def test_residual_entry_point_refuses_what_it_cannot_take():
    from viforsdes_amd import _hip
    key, rows = _key(1, 2), torch.tensor([0, 2], dtype=torch.int32, device=DEV)
    z = lambda *s: torch.zeros(*s, device=DEV)
    run = lambda S, O, N, H=None: _hip.guided_particle_filter("linear_diagonal", z(4, S), z(4, 2 * S), rows, z(2, O), H, 0.1, key, 0.05, N, (),
                                                              residual=True)
    out = run(4, 4, 64)
    assert len(out) == 8 and out[0].shape == (4,) and out[7] is None and bool(torch.isfinite(out[0]).all())
    with pytest.raises(ValueError, match="state_dim"):
        run(5, 5, 64)
    with pytest.raises(ValueError, match="obs_dim"):
        run(2, 5, 64, z(5, 2))
    for N in (0, 32, 100, 2048):
        with pytest.raises(ValueError, match="particles"):
            run(2, 2, N)
    assert run(4, 4, 512)[0].shape == (4,)
    with pytest.raises(ValueError, match="particles"):                      # S = 4: 512 at most
        run(4, 4, 1024)
    assert run(3, 3, 1024)[0].shape == (4,)
    torch.cuda.synchronize()
