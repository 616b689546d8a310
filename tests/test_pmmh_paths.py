"""CPU: particle MCMC with paths on the torch route (the specification, float64) -- ``particle_mcmc(return_paths=True)``.

* The theta chain is the chain without paths, bit for bit, and ``path_thin`` only thins.
* Record identities on a traced 6-iteration run (C = 5, R = 2, N = 64, the OU problem of tests/particle_mcmc_reference.py): for every
  chain accepted at iteration i the record is the numpy rule of tests/pmmh_paths_reference.py applied to a rerun of the iteration's
  filter (filter, slot, lineage exactly; anchors ``torch.equal`` to the gathered particles); a rejecting chain keeps its record; kept
  paths repeat where nothing was accepted; ``paths[.., 0] == x0``; ``paths[.., rows[k]]`` against ``anchors[k]`` within 2e-4 of the
  largest magnitude, the bound tests/test_particle_smoother_gpu.py holds replayed endpoints to.
* The draw rule on the numpy reference alone: over 20 000 (chain, iteration) pairs the ancestor of a uniformly chosen offspring slot,
  averaged over the resampling uniform, follows the weights, and the chosen filter follows the estimates, each frequency within 4.5
  binomial standard errors.
* Dead records, every new ValueError, and the reference's vectorised smoother against ``ou_rts``.
* The new entry points refuse bad arguments with VSDE_E_BADARG before any HIP call: called through ctypes with pointers that are
  never read, no device needed."""
import ctypes

import numpy as np
import pytest
import torch

import particle_mcmc_reference as mref
import particle_smoother_reference as sref
import pmmh_paths_reference as ref

F64 = torch.float64
KEY = (11, 13)


def _key(k0, k1):
    return torch.from_numpy(np.array([k0, k1], dtype=np.uint32).view(np.int32))


def _ou(variance=mref.OU_VARIANCE):
    from viforsdes_amd import GaussianObservationLikelihood, Observations, Prior, PriorType
    from viforsdes_amd.examples.sdes import OrnsteinUhlenbeck
    obs = Observations(times=torch.tensor(mref.OU_TIMES, dtype=F64), values=torch.tensor(mref.OU_VALUES, dtype=F64)[:, None])
    prior = Prior(type=PriorType.LOG_NORMAL, mean=mref.OU_PRIOR[1], std=mref.OU_PRIOR[2], dim=3)
    return OrnsteinUhlenbeck(), obs, GaussianObservationLikelihood(variance=variance), prior


def _run(n_iterations=6, C=5, R=2, variance=mref.OU_VARIANCE, **kw):
    from viforsdes_amd import particle_mcmc
    sde, obs, like, prior = _ou(variance)
    theta0 = torch.tensor(mref.ou_initial_theta(C), dtype=F64)
    return particle_mcmc(sde, obs, like, prior, mref.OU_DT, theta0, n_iterations, n_particles=64, filters_per_chain=R,
                         theta_positive_dims=(0, 1, 2), key=_key(*KEY), **kw)


def test_theta_chain_is_unchanged_and_path_thin_only_thins():
    plain, paths = _run(), _run(return_paths=True)
    for name in ("samples", "log_likelihood", "log_target", "acceptance_rate"):
        assert torch.equal(getattr(plain, name), getattr(paths, name)), name
    for name in ("paths", "path_iteration", "path_mean", "path_std", "path_quantiles", "path_mean_standard_error"):
        assert getattr(plain, name) is None, name
    T = mref.OU_ROWS[-1]
    assert paths.paths.shape == (6, 5, T + 1, 1) and paths.paths.dtype == F64
    assert paths.path_iteration.shape == (6, 5) and paths.path_iteration.dtype == torch.int32
    for t in (paths.path_mean, paths.path_std, paths.path_mean_standard_error, *vars(paths.path_quantiles).values()):
        assert t.shape == (T + 1, 1) and bool(torch.isfinite(t).all())
    assert torch.allclose(paths.path_mean, paths.paths.reshape(30, T + 1, 1).mean(dim=0))
    thinned = _run(return_paths=True, path_thin=4)
    assert torch.equal(thinned.samples, plain.samples)
    assert thinned.paths.shape == (2, 5, T + 1, 1) and torch.equal(thinned.paths, paths.paths[::4])
    assert torch.equal(thinned.path_iteration, paths.path_iteration[::4])


def test_record_identities_against_a_rerun_of_every_filter():
    from viforsdes_amd.inference import particle_filter as pf
    from viforsdes_amd.inference.particle_mcmc import filter_key
    C, R, N = 5, 2, 64
    trace = []
    res = _run(return_paths=True, _trace=trace)
    sde, obs, like, _ = _ou()
    rows = list(mref.OU_ROWS)
    K = len(rows)
    x0 = obs.values[0]
    assert len(trace) == 6
    prev_anchor, prev_noise = np.full((C, K, 1), np.nan), np.full((C, K), ref.DEAD, dtype=np.int64)
    prev_iter = np.full(C, -1)
    accepted_any = 0
    for i, tr in enumerate(trace):
        fkey = filter_key(i, _key(*KEY))
        assert torch.equal(fkey, tr["filter_key"])
        out = pf.particle_filter(sde, obs, like, tr["theta_prop"], mref.OU_DT, n_particles=N, initial_state=x0, return_particles=True,
                                 key=fkey)
        assert torch.equal(out.log_likelihood.reshape(C, R), tr["loglik"])             # the rerun is the iteration's filter
        want = ref.draw_records(tr["loglik"].numpy(), out.particles.numpy(), out.ancestors.numpy(), i, KEY)
        assert (want["margin"] > 1e-9).all()                                            # no filter choice sits on a boundary
        acc = tr["accept"].numpy()
        noise, anchor, it = tr["cur_noise_path"].numpy(), tr["cur_anchor"], tr["cur_path_iteration"].numpy()
        for c in range(C):
            if acc[c]:
                accepted_any += 1
                m, lin = c * R + want["r"][c], want["lineage"][c]
                assert 0 <= want["J"][c] < N and lin[K - 1] == int(out.ancestors[m, K - 1, want["J"][c]])
                assert np.array_equal(noise[c], m * N + lin) and it[c] == i
                gathered = out.particles[m][torch.arange(K), torch.as_tensor(lin)]
                assert torch.equal(anchor[c], gathered)
            else:
                assert np.array_equal(noise[c], prev_noise[c]) and it[c] == prev_iter[c]
                assert np.array_equal(anchor[c].numpy(), prev_anchor[c], equal_nan=True)
        prev_anchor, prev_noise, prev_iter = anchor.numpy().copy(), noise.copy(), it.copy()
        # the kept row of iteration i (no warm-up, thin = path_thin = 1) is the carried record, replayed
        assert np.array_equal(res.path_iteration[i].numpy(), it)
        live = it >= 0
        assert live.all()                                                               # iteration 0 accepts every finite start
        paths = res.paths[i].numpy()
        assert np.array_equal(paths[:, 0], np.broadcast_to(x0.numpy(), (C, 1)))
        ends = paths[:, rows]                                                           # [C, K, 1]
        assert np.abs(ends - anchor.numpy()).max() <= 2e-4 * np.abs(anchor.numpy()).max()
        if i > 0:
            same = ~acc
            assert np.array_equal(res.paths[i].numpy()[same], res.paths[i - 1].numpy()[same])
            assert (np.abs(res.paths[i].numpy()[acc] - res.paths[i - 1].numpy()[acc]).max(axis=(1, 2)) > 0).all()
    assert accepted_any > C                                                             # chains moved after iteration 0
    assert np.isfinite(res.paths.numpy()).all()


def test_draw_rule_follows_the_weights_and_the_estimates():
    n_chains, n_iter, N, R = 200, 100, 8, 3
    w = np.array([0.02, 0.30, 0.05, 0.18, 0.0, 0.25, 0.12, 0.08])
    loglik = np.log(np.array([0.5, 0.2, 0.3])) - 17.0
    rng = np.random.default_rng(5)
    slots, filters = np.zeros(N), np.zeros(R)
    for i in range(n_iter):
        v0, v1 = ref.path_uniforms(n_chains, i, KEY)
        J = ref.final_slot(v1, N)
        u = rng.random(n_chains)
        for c in range(n_chains):
            anc = sref.systematic_draws(w, u[c], N)                                     # the filter's systematic resampling
            slots[ref.trace_lineage(anc[None, :], J[c])[0]] += 1
        r, _ = ref.choose_filter(np.broadcast_to(loglik, (n_chains, R)), v0)
        filters += np.bincount(r, minlength=R)
    n = n_chains * n_iter
    assert n == 20000 and slots.sum() == n and filters.sum() == n
    for got, p in ((slots, w / w.sum()), (filters, np.exp(loglik) / np.exp(loglik).sum())):
        se = np.sqrt(p * (1.0 - p) / n)
        z = np.abs(got / n - p) / np.where(se > 0, se, 1.0)
        print(f"frequencies {np.round(got / n, 4).tolist()} against {np.round(p, 4).tolist()}: largest z {z.max():.2f}")
        assert (got[p == 0] == 0).all() and z.max() <= 4.5


def test_dead_records_have_no_path():
    res = _run(n_iterations=3, variance=1e-320, return_paths=True)                      # every filter dies at the second observation
    assert res.n_filters_dead == 3 * 5
    assert bool((res.path_iteration == -1).all()) and bool(torch.isnan(res.paths).all())
    assert bool(torch.isnan(res.path_mean).all()) and bool(torch.isneginf(res.log_target).all())


def test_bad_arguments_are_refused():
    for kw in (dict(path_thin=0), dict(return_paths=True, path_thin=-1),
               dict(return_paths=True, _estimator=lambda rows, i, key: torch.zeros(rows.shape[0], dtype=F64))):
        with pytest.raises(ValueError):
            _run(**kw)


def test_vectorised_smoother_is_ou_rts():
    theta = np.exp(np.random.default_rng(2).normal(0.0, 0.5, size=(3, 3)))
    mean, var = ref.ou_rts_rows(theta, mref.OU_DT, mref.OU_VARIANCE, mref.OU_VALUES[0], mref.OU_ROWS, mref.OU_VALUES)
    for m, v, th in zip(mean, var, theta):
        wm, wv = sref.ou_rts(th, mref.OU_DT, mref.OU_VARIANCE, [mref.OU_VALUES[0]], mref.OU_ROWS, np.array(mref.OU_VALUES)[:, None])
        assert np.abs(m - wm).max() <= 1e-12 and np.abs(v - wv).max() <= 1e-12


# ------------------------------------------------------------------------------------- the entry points' checks, without a device
BADARG = -1        # include/vsde_hip.h: VSDE_E_BADARG
PTR = ctypes.c_void_p(0x1000)      # "some device pointer": a refused call reads none of them
NULL = ctypes.c_void_p(None)


def _step_paths(lib, **kw):
    a = dict(C=5, P=3, R=2, iteration=1, N=64, K=3, S=2, particles=PTR, ancestors=PTR, cur_anchor=PTR, cur_noise_path=PTR,
             cur_path_iteration=PTR, cur_u=PTR)
    a.update(kw)
    L = (ctypes.c_float * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    mask = (ctypes.c_uint8 * 3)(1, 0, 0)
    i, d = ctypes.c_int, ctypes.c_double
    return lib.vsde_pmmh_step_paths(i(a["C"]), i(a["P"]), i(a["R"]), i(a["iteration"]), L, d(0.5), i(0), d(0.0), d(1.0), mask, PTR, PTR, a["cur_u"],
                                    PTR, PTR, PTR, PTR, PTR, PTR, NULL, NULL, NULL, PTR, i(a["N"]), i(a["K"]), i(a["S"]), a["particles"],
                                    a["ancestors"], a["cur_anchor"], a["cur_noise_path"], a["cur_path_iteration"], NULL, NULL, NULL, NULL)


def _replay(lib, guided=False, **kw):
    a = dict(kind=3, B=4, S=2, P=4, K=3, O=2, T=10, x0=PTR, theta=PTR, obs_rows=PTR, anchors=PTR, noise_path=PTR, keys=PTR, paths=PTR,
             obs_values=PTR, time_step=0.1)
    a.update(kw)
    i, d = ctypes.c_int, ctypes.c_double
    mask = (ctypes.c_uint8 * 32)()
    model = (a["obs_values"], NULL, d(0.5)) if guided else ()
    fn = lib.vsde_guided_anchored_replay if guided else lib.vsde_anchored_replay
    return fn(i(a["kind"]), i(a["B"]), i(a["S"]), i(a["P"]), i(a["K"]), i(a["O"]), i(a["T"]), a["x0"], a["theta"], a["obs_rows"], *model,
              a["anchors"], a["noise_path"], a["keys"], d(a["time_step"]), mask, a["paths"], NULL)


def test_entry_points_refuse_bad_arguments_before_any_hip_call():
    from viforsdes_amd import _hip
    lib = _hip.load()
    for kw in (dict(K=0), dict(N=0), dict(S=0), dict(particles=NULL), dict(ancestors=NULL), dict(cur_anchor=NULL), dict(cur_noise_path=NULL),
               dict(cur_path_iteration=NULL), dict(cur_u=NULL), dict(P=17), dict(C=0), dict(C=2 ** 22, N=1024)):
        assert _step_paths(lib, **kw) == BADARG, kw
        assert lib.vsde_last_error()
    for kw in (dict(K=0), dict(B=0), dict(S=17, P=34, O=17), dict(S=0, P=0), dict(T=-1), dict(B=2 ** 30, K=2), dict(time_step=0.0),
               dict(x0=NULL), dict(theta=NULL), dict(obs_rows=NULL), dict(anchors=NULL), dict(noise_path=NULL), dict(keys=NULL),
               dict(paths=NULL), dict(kind=7)):
        assert _replay(lib, **kw) == BADARG, kw
    for kw in (dict(S=5, P=10, O=5), dict(S=2, O=5), dict(K=0), dict(obs_values=NULL), dict(anchors=NULL), dict(T=-1)):
        assert _replay(lib, guided=True, **kw) == BADARG, kw
    # the descriptor forms forward to the same body: a NULL network is refused as well
    assert lib.vsde_crn_anchored_replay(NULL, *[ctypes.c_int(v) for v in (4, 2, 2, 3, 2, 10)], *[PTR] * 6, ctypes.c_double(0.1),
                                        (ctypes.c_uint8 * 32)(), PTR, NULL) == BADARG
