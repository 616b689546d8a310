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


def run_filter(tab, x0, rates, times, ys, like, N, key, max_events):
    """The whole filter: a dict of ``log_likelihood [M]``, ``increments``, ``ess [M, K]``, ``mean``, ``std [M, K, S]``, ``stopped
    [M, K]``, ``mean_events [M, K]``, ``particles [M, K, N, S]``, ``ancestors``, ``log_weights``, ``events [M, K, N]``."""
    x0, rates = np.asarray(x0, dtype=np.int64), np.asarray(rates, dtype=np.float64)
    times, ys = np.asarray(times, dtype=np.float64), np.asarray(ys, dtype=np.float64)
    M, S = x0.shape
    K = len(times)
    u = pref.resampling_uniforms(M, K, key)
    out = dict(increments=np.zeros((M, K)), ess=np.zeros((M, K)), mean=np.zeros((M, K, S)), std=np.zeros((M, K, S)),
               stopped=np.zeros((M, K), dtype=np.int64), mean_events=np.zeros((M, K)), particles=np.zeros((M, K, N, S), dtype=np.int64),
               ancestors=np.zeros((M, K, N), dtype=np.int64), log_weights=np.zeros((M, K, N)), events=np.zeros((M, K, N), dtype=np.int64))
    for m in range(M):
        x = np.repeat(x0[m][None], N, axis=0)
        for k in range(K):
            status = np.zeros(N, dtype=np.int64)
            for j in range(N):
                x[j], out["events"][m, k, j], status[j], _ = run_segment(tab, x[j], rates[m], times[k - 1] if k else 0.0, times[k], k,
                                                                        m * N + j, key, max_events)
            lw = np.where(status != 0, -np.inf, log_weights(like, ys[k], x))
            inc, ess, mean, std, anc = stage(lw, x, u[m, k])
            out["increments"][m, k], out["ess"][m, k], out["mean"][m, k], out["std"][m, k] = inc, ess, mean, std
            out["stopped"][m, k], out["mean_events"][m, k] = int((status != 0).sum()), out["events"][m, k].mean()
            out["particles"][m, k], out["ancestors"][m, k], out["log_weights"][m, k] = x, anc, lw
            x = x[anc]
    out["log_likelihood"] = out["increments"].sum(axis=1)
    return out


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
