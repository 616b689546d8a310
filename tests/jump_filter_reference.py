"""numpy float64 restatement of the jump-process particle filter (viforsdes_amd/inference/jump_filter.py), written independently
of the package: one particle and one event at a time on the uniforms of the specified Philox stream (counter {e >> 1, segment, b,
7}; tests/philox_reference.py), with the propensities and the selection rule of tests/jump_process_reference.py and the observation
stage of tests/particle_filter_reference.py.

A network is the plain tables of ``jump_process_reference.tables``; ``rates [M, 2R]`` are the effective constants.  A likelihood
is a tuple: ``("gaussian", variance, H)``, ``("poisson", scale, H)`` or ``("nb", dispersion, scale, H)`` with ``H`` an ``[O, S]``
array or None."""
import math

import numpy as np

import count_likelihood_reference as cref
import jump_process_reference as jref
import particle_filter_reference as pref
from philox_reference import _uniform, philox4x32_10


def segment_uniforms(path, pair, segment, key):
    """The four fp32 uniforms (widened to float64) of events ``2 pair`` (the first two: u1, u2) and ``2 pair + 1`` (the last two)
    of path ``path`` in segment ``segment``."""
    k0, k1 = (int(v) & 0xFFFFFFFF for v in key)
    w = philox4x32_10(np.asarray([pair]), segment, np.asarray([path]), 7, k0, k1)
    return [float(_uniform(v)[0]) for v in w]


def run_segment(tab, x, rates, t_start, t_end, segment, path, key, max_events):
    """One particle over one segment: (state [S], events fired, status, undecidable).  ``undecidable``: an fp32 implementation of
    the same rule may legitimately differ: some event has ``u2 a0`` within ``1e-5 a0`` of a boundary ``c_j`` (``choose``'s rule),
    or some tested instant has ``|t_next - t_end| <= 1e-5 (t_next - t_start)``."""
    x, t, fired, near, u = np.asarray(x, dtype=np.int64).copy(), float(t_start), 0, False, None
    while True:
        if fired == max_events:
            return x, fired, 1, near
        a = jref.propensities(tab, x[None], rates[None])[0]
        if not np.all(np.isfinite(a) & (a >= 0)) or not np.isfinite(a.sum()):
            return x, fired, 2, near
        a0 = np.cumsum(a)[-1]
        if a0 == 0:
            return x, fired, 0, near
        if fired % 2 == 0:
            u = segment_uniforms(path, fired // 2, segment, key)
        u1, u2 = u[2 * (fired % 2)], u[2 * (fired % 2) + 1]
        t_next = t + -math.log(u1) / a0
        near = near or abs(t_next - t_end) <= 1e-5 * (t_next - t_start)
        if t_end < t_next:
            return x, fired, 0, near
        j, close = jref.choose(a[None], np.asarray([u2]))
        near = near or bool(close[0])
        x = x + tab["change"][int(j[0])]
        t = t_next
        fired += 1


def run_segments(tab, x, rates, t_start, t_end, segment, paths, key, max_events):
    """``run_segment`` for n particles at once: x [n, S], rates [2R] or [n, 2R], paths [n] -> (states [n, S], events fired [n],
    status [n], undecidable [n]).  The same rule on the same uniforms, one event index at a time over the particles still
    running; tests/test_jump_sweep.py holds it to ``run_segment`` particle by particle."""
    x = np.asarray(x, dtype=np.int64).copy()
    n = x.shape[0]
    rates = np.broadcast_to(np.asarray(rates, dtype=np.float64), (n, np.shape(rates)[-1]))
    paths = np.asarray(paths, dtype=np.int64)
    k0, k1 = (int(v) & 0xFFFFFFFF for v in key)
    t, fired, status = np.full(n, float(t_start)), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    near, live = np.zeros(n, dtype=bool), np.ones(n, dtype=bool)
    while live.any():
        idx = np.nonzero(live)[0]
        capped = fired[idx] == max_events
        status[idx[capped]], live[idx[capped]] = 1, False
        idx = idx[~capped]
        a = jref.propensities(tab, x[idx], rates[idx])
        bad = ~(np.all(np.isfinite(a) & (a >= 0), axis=1) & np.isfinite(a.sum(axis=1)))
        status[idx[bad]], live[idx[bad]] = 2, False
        idx, a = idx[~bad], a[~bad]
        a0 = np.cumsum(a, axis=1)[:, -1] if len(idx) else np.zeros(0)
        live[idx[a0 == 0]] = False
        idx, a, a0 = idx[a0 != 0], a[a0 != 0], a0[a0 != 0]
        if not len(idx):
            continue
        e = fired[idx]
        w = philox4x32_10(e >> 1, segment, paths[idx], 7, k0, k1)
        odd = (e & 1) == 1
        u1 = _uniform(np.where(odd, w[2], w[0])).astype(np.float64)
        u2 = _uniform(np.where(odd, w[3], w[1])).astype(np.float64)
        t_next = t[idx] + -np.log(u1) / a0
        near[idx] |= np.abs(t_next - t_end) <= 1e-5 * (t_next - t_start)
        past = t_end < t_next
        live[idx[past]] = False
        idx, a, u2, t_next = idx[~past], a[~past], u2[~past], t_next[~past]
        if not len(idx):
            continue
        j, close = jref.choose(a, u2)
        near[idx] |= close
        x[idx] += tab["change"][j]
        t[idx] = t_next
        fired[idx] += 1
    return x, fired, status, near


def log_weights(like, y, x):
    """lw [N] of the states x [N, S] (integers) for the observation y [O]; NaN counts as -inf."""
    x = np.asarray(x, dtype=np.float64)
    if like[0] == "gaussian":
        return pref.gaussian_log_weights(y, x, like[1], like[2])
    if like[0] == "poisson":
        return cref.count_log_weights(y, x, None, like[1], like[2])
    return cref.count_log_weights(y, x, like[1], like[2], like[3])


def stage(lw, x, u):
    """(increment, ess, mean [S], std [S], ancestors [N]) of one filter at one observation from lw [N] and x [N, S], with the
    dead-filter rule."""
    N = len(lw)
    if not np.isfinite(lw.max()):
        nan = np.full(x.shape[1], np.nan)
        return -np.inf, 0.0, nan, nan, np.arange(N)
    inc, ess, mean, std, w = pref.observation_stage(lw, np.asarray(x, dtype=np.float64))
    return inc, ess, mean, std, pref.systematic_ancestors(w, u)


def run_filter(tab, x0, rates, times, ys, like, N, key, max_events, vectorized=False):
    """The whole filter: a dict of ``log_likelihood [M]``, ``increments``, ``ess [M, K]``, ``mean``, ``std [M, K, S]``, ``stopped
    [M, K]``, ``mean_events [M, K]``, ``particles [M, K, N, S]``, ``ancestors``, ``log_weights``, ``events [M, K, N]``, and
    ``undecidable [M, K, N]`` (``run_segment``'s flag).  ``vectorized``: the segments through ``run_segments``."""
    x0, rates = np.asarray(x0, dtype=np.int64), np.asarray(rates, dtype=np.float64)
    times, ys = np.asarray(times, dtype=np.float64), np.asarray(ys, dtype=np.float64)
    M, S = x0.shape
    K = len(times)
    u = pref.resampling_uniforms(M, K, key)
    out = dict(increments=np.zeros((M, K)), ess=np.zeros((M, K)), mean=np.zeros((M, K, S)), std=np.zeros((M, K, S)),
               stopped=np.zeros((M, K), dtype=np.int64), mean_events=np.zeros((M, K)), particles=np.zeros((M, K, N, S), dtype=np.int64),
               ancestors=np.zeros((M, K, N), dtype=np.int64), log_weights=np.zeros((M, K, N)), events=np.zeros((M, K, N), dtype=np.int64),
               undecidable=np.zeros((M, K, N), dtype=bool))
    for m in range(M):
        x = np.repeat(x0[m][None], N, axis=0)
        for k in range(K):
            status = np.zeros(N, dtype=np.int64)
            if vectorized:
                x, out["events"][m, k], status, out["undecidable"][m, k] = run_segments(
                    tab, x, rates[m], times[k - 1] if k else 0.0, times[k], k, m * N + np.arange(N), key, max_events)
            else:
                for j in range(N):
                    x[j], out["events"][m, k, j], status[j], out["undecidable"][m, k, j] = run_segment(
                        tab, x[j], rates[m], times[k - 1] if k else 0.0, times[k], k, m * N + j, key, max_events)
            lw = np.where(status != 0, -np.inf, log_weights(like, ys[k], x))
            inc, ess, mean, std, anc = stage(lw, x, u[m, k])
            out["increments"][m, k], out["ess"][m, k], out["mean"][m, k], out["std"][m, k] = inc, ess, mean, std
            out["stopped"][m, k], out["mean_events"][m, k] = int((status != 0).sum()), out["events"][m, k].mean()
            out["particles"][m, k], out["ancestors"][m, k], out["log_weights"][m, k] = x, anc, lw
            x = x[anc]
    out["log_likelihood"] = out["increments"].sum(axis=1)
    return out


# --- what the GPU files need to make a kernel-route run (tests/test_jump_filter_gpu.py, tests/test_jump_sweep_gpu.py)
def key_tensor(k0, k1, dev):
    import torch
    return torch.from_numpy(np.array([k0, k1], dtype=np.uint32).view(np.int32)).to(dev)


def likelihood(spec):
    """The package's likelihood of a tuple of this module (see the module docstring)."""
    import torch
    from viforsdes_amd import GaussianObservationLikelihood, NegativeBinomialObservationLikelihood, PoissonObservationLikelihood
    H = None if spec[-1] is None else torch.tensor(spec[-1], dtype=torch.float32)
    if spec[0] == "gaussian":
        return GaussianObservationLikelihood(variance=spec[1], obs_matrix=H)
    if spec[0] == "poisson":
        return PoissonObservationLikelihood(scale=spec[1], obs_matrix=H)
    return NegativeBinomialObservationLikelihood(dispersion=spec[1], scale=spec[2], obs_matrix=H)


def counted(monkeypatch=None):
    """A list that receives one entry per launch of the kernel through ``_hip.jump_particle_filter``."""
    from viforsdes_amd import _hip
    calls, real = [], _hip.jump_particle_filter
    wrapped = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    if monkeypatch is not None:
        monkeypatch.setattr(_hip, "jump_particle_filter", wrapped)
    return calls, real, wrapped


# --- the three stage checks of one kernel-route run ``res`` (JumpParticleFilterResult with particles) on its own previous stage
# (tests/test_jump_filter_gpu.py, tests/test_jump_sweep_gpu.py)
def check_propagation(net, th, xs, times, res, key, label="", vectorized=False):
    """Segment k again in float64 from the kernel's particles at k - 1 gathered through the kernel's ancestors: at most 2e-2 of
    the (particle, segment) pairs are flagged undecidable (asserted first), every other pair matches the kernel exactly, state and
    event count.  th: theta fp32 [M, P] (torch), xs: start states [M, S].  Returns (flagged, pairs)."""
    tab = jref.tables(net)
    rates = net.kernel_parameters(th.double()).numpy()
    parts, anc, events = res.particles.cpu().numpy().astype(np.int64), res.ancestors.cpu().numpy().astype(np.int64), res.events.cpu().numpy()
    M, K, N = parts.shape[:3]
    assert int(res.stopped.sum()) == 0
    flagged, checked = 0, []
    for m in range(M):
        for k in range(K):
            start = np.repeat(xs[m][None], N, axis=0) if k == 0 else parts[m, k - 1][anc[m, k - 1]]
            if vectorized:
                x, fired, status, near = run_segments(tab, start, rates[m], times[k - 1] if k else 0.0, times[k], k, m * N + np.arange(N),
                                                      key, 4096)
                assert (status == 0).all()
                flagged += int(near.sum())
                checked += list(((x == parts[m, k]).all(axis=1) & (fired == events[m, k]))[~near])
                continue
            for j in range(N):
                x, fired, status, near = run_segment(tab, start[j], rates[m], times[k - 1] if k else 0.0, times[k], k, m * N + j, key, 4096)
                assert status == 0
                flagged += bool(near)
                if not near:
                    checked.append(bool(np.array_equal(x, parts[m, k, j])) and fired == events[m, k, j])
    total = M * K * N
    print(f"{label}: the reference flags {flagged} of {total} (particle, segment) pairs ({flagged / total:.1e}); "
          f"{len(checked) - sum(checked)} of the other {len(checked)} differ; mean events {float(res.mean_events.mean()):.1f}")
    assert flagged <= 2e-2 * total                                  # the reference's own share first: a cap, not a tolerance
    assert all(checked)
    assert events.sum() > total                                     # something happened
    mean_events = events.reshape(M, K, N).mean(axis=2)
    np.testing.assert_allclose(res.mean_events.cpu().numpy(), mean_events, rtol=1e-5, atol=1e-6)
    return flagged, total


def check_weights_and_summaries(like, ys, res, label=""):
    """Weights and summaries from the kernel's particles in float64: log-weights and increments within 1e-5 max(1, largest finite
    |lw|); ESS, mean, std to 1e-4 relative (the mean relative to the weighted mean of |x|, the std with a floor of 1e-2 of that
    size).  Returns the five worst errors."""
    import torch
    parts = res.particles.double().cpu().numpy()
    M, K = parts.shape[:2]
    got = [t.double().cpu().numpy() for t in (res.increments, res.effective_sample_size, res.filtered_mean, res.filtered_std, res.log_weights)]
    e_lw = e_inc = e_ess = e_mean = e_std = 0.0
    for m in range(M):
        for k in range(K):
            lw = log_weights(like, ys[k], parts[m, k])
            inc, ess, mean, std, w = pref.observation_stage(lw, parts[m, k])
            size = (w[:, None] * np.abs(parts[m, k])).sum(axis=0) / w.sum()          # weighted mean of |x|, per dim
            scale = max(1.0, np.abs(lw[np.isfinite(lw)]).max())
            e_lw = max(e_lw, float(np.abs(got[4][m, k] - lw).max()) / scale)
            e_inc = max(e_inc, abs(got[0][m, k] - inc) / scale)
            e_ess = max(e_ess, abs(got[1][m, k] - ess) / ess)
            e_mean = max(e_mean, float((np.abs(got[2][m, k] - mean) / np.maximum(size, 1e-30)).max()))
            e_std = max(e_std, float((np.abs(got[3][m, k] - std) / (std + 1e-2 * size + 1e-30)).max()))
    print(f"{label}: log-weights {e_lw:.2e}, increments {e_inc:.2e} (of max(1, |lw|), bound 1e-5), ESS {e_ess:.2e}, "
          f"mean {e_mean:.2e}, std {e_std:.2e} (relative, bound 1e-4)")
    assert e_lw <= 1e-5 and e_inc <= 1e-5
    assert e_ess <= 1e-4 and e_mean <= 1e-4 and e_std <= 1e-4
    total = res.increments.double().sum(dim=1)
    assert torch.allclose(res.log_likelihood.double(), total, rtol=1e-6, atol=1e-5 * float(res.increments.abs().max()))
    return e_lw, e_inc, e_ess, e_mean, e_std


def check_ancestors(like, ys, res, key, label=""):
    """Ancestors against float64 systematic resampling of the float64 weights of the kernel's particles with the specified
    uniform: the float64 particle ESS above N / 20 first; then at most 1e-3 of the entries differ, each by exactly 1, and they
    never decrease in j.  Returns (differing entries, entries)."""
    parts = res.particles.double().cpu().numpy()
    anc = res.ancestors.cpu().numpy().astype(np.int64)
    M, K, N = anc.shape
    u = pref.resampling_uniforms(M, K, key)
    differ, low, worst = 0, float("inf"), 0
    for m in range(M):
        for k in range(K):
            lw = log_weights(like, ys[k], parts[m, k])
            w = np.exp(lw - lw.max())
            low = min(low, w.sum() ** 2 / (w * w).sum())
            d = np.abs(anc[m, k] - pref.systematic_ancestors(w, u[m, k]))
            worst, differ = max(worst, int(d.max())), differ + int((d != 0).sum())
    print(f"{label}: {differ} of {anc.size} ancestors differ from float64 ({differ / anc.size:.1e}), largest difference "
          f"{worst}; smallest float64 ESS {low:.1f}")
    assert low > N / 20                                            # there was something to compare
    assert anc.min() >= 0 and anc.max() < N and (np.diff(anc, axis=-1) >= 0).all()      # never decrease in j
    assert worst <= 1 and differ <= 1e-3 * anc.size
    return differ, anc.size


# --- the exact likelihood of immigration-death (0 -> X at rate birth, X -> 0 at rate death x) observed with Poisson noise: the
# forward algorithm on the states 0 .. size - 1 with the transition rows of jump_process_reference.immigration_death_pmf
def immigration_death_log_likelihood(birth, death, x0, times, ys, scale=1.0, size=200):
    states = np.arange(size, dtype=np.float64)
    lam = np.maximum(scale * states, cref.RATE_FLOOR)
    alpha = np.zeros(size)
    alpha[int(x0)] = 1.0
    ll, t_prev = 0.0, 0.0
    for t, y in zip(times, ys):
        dt = float(t) - t_prev
        if dt > 0:
            rows = np.stack([jref.immigration_death_pmf(n, birth, death, dt, size)[0] for n in range(size)])
            alpha = alpha @ rows
        t_prev = float(t)
        alpha = alpha * np.exp(y * np.log(lam) - lam - math.lgamma(y + 1.0))
        total = alpha.sum()
        ll += math.log(total)
        alpha = alpha / total
    return ll


IMMIGRATION_DEATH_TIMES = [0.0, 0.5, 0.5, 1.5, 3.0]
IMMIGRATION_DEATH_COUNTS = [30.0, 27.0, 24.0, 22.0, 19.0]
