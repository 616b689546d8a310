"""numpy float64 restatement of the replay of the jump-process smoother (viforsdes_amd/inference/jump_smoother.py), written
independently of the package on tests/philox_reference.py and tests/jump_process_reference.py: ``jump_filter_reference.run_segments``
extended with output times, and the exact smoothing marginals of immigration-death observed with Poisson noise (forward-backward
on 200 states) that the smoother and the PMMH paths are held to.  ``replay_records`` / ``score_records`` are the general form (records
that bring their own start state, theta row, path slots and key, any event cap, stopped segments) the replay sweep scores with.

A (record, segment) pair is *undecidable* (an fp32 implementation of the same rule may legitimately differ) if ``run_segment``'s two
conditions hold (an event with ``u2 a0`` within ``1e-5 a0`` of a boundary ``c_j``, or a tested instant within ``1e-5 (t_next -
t_start)`` of ``t_end``), or some tested instant has ``|t_next - t_q| <= 1e-5 (t_next - t_start)`` for an owned output time ``t_q``."""
import math

import numpy as np

import count_likelihood_reference as cref
import jump_process_reference as jref
from philox_reference import _uniform, philox4x32_10

CAP = 2e-2                      # the share of undecidable (record, segment) pairs a check accepts: asserted first, a cap, not a tolerance


def ownership(path_times, obs_times):
    """q_begin [K + 1]: segment k owns the outputs q_begin[k] .. q_begin[k+1] - 1, the t_q with T_{k-1} < t_q <= T_k (segment 0:
    0 <= t_q <= T_0)."""
    path_times, obs_times = np.asarray(path_times, dtype=np.float64), np.asarray(obs_times, dtype=np.float64)
    return np.concatenate([[0], [(path_times <= t).sum() for t in obs_times]]).astype(np.int64)


def run_segments_states(tab, x, rates, t_start, t_end, segment, paths, key, max_events, out_times, _counter=None, _late=False):
    """``jump_filter_reference.run_segments`` that also reads the path at ``out_times`` [Q] (non-decreasing, owned by the segment):
    (states [n, S], events fired [n], status [n], undecidable [n], outputs [n, Q, S]).  An output takes the state after every event
    with time <= t_q; a stopped path (status 1 or 2) leaves -1 in the outputs it did not reach.

    ``_counter`` and ``_late`` are not part of the rule: tests/test_jump_replay_sweep.py injects two defects through them to show
    that the scorer rejects them (the first Philox counter word of event e, ``e >> 1`` by the rule; outputs that take the state after
    the event at ``t_next`` instead of before it)."""
    x = np.asarray(x, dtype=np.int64).copy()
    n, S = x.shape
    out_times = np.asarray(out_times, dtype=np.float64).reshape(-1)
    Q = len(out_times)
    rates = np.broadcast_to(np.asarray(rates, dtype=np.float64), (n, np.shape(rates)[-1]))
    paths = np.asarray(paths, dtype=np.int64)
    k0, k1 = (int(v) & 0xFFFFFFFF for v in key)
    t, fired, status = np.full(n, float(t_start)), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    near, live = np.zeros(n, dtype=bool), np.ones(n, dtype=bool)
    outs, q = np.full((n, Q, S), -1, dtype=np.int64), np.zeros(n, dtype=np.int64)
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
        live[idx[a0 == 0]] = False                                  # absorbed: the remaining outputs are filled below
        idx, a, a0 = idx[a0 != 0], a[a0 != 0], a0[a0 != 0]
        if not len(idx):
            continue
        e = fired[idx]
        w = philox4x32_10(e >> 1 if _counter is None else _counter(e), segment, paths[idx], 7, k0, k1)
        odd = (e & 1) == 1
        u1 = _uniform(np.where(odd, w[2], w[0])).astype(np.float64)
        u2 = _uniform(np.where(odd, w[3], w[1])).astype(np.float64)
        t_next = t[idx] + -np.log(u1) / a0
        width = 1e-5 * (t_next - t_start)
        near[idx] |= np.abs(t_next - t_end) <= width
        past = t_end < t_next
        if Q:
            near[idx] |= (np.abs(t_next[:, None] - out_times[None, :]) <= width[:, None]).any(axis=1)
            upto = np.searchsorted(out_times, t_next, side="left")  # the number of t_q < t_next
            due = (np.arange(Q)[None, :] >= q[idx][:, None]) & (np.arange(Q)[None, :] < upto[:, None])
            rows, cols = np.nonzero(due)
            now = x[idx]
            if _late and (~past).any():                             # the injected defect: the state after the event at t_next
                now[~past] += tab["change"][jref.choose(a[~past], u2[~past])[0]]
            outs[idx[rows], cols] = now[rows]
            q[idx] = np.maximum(q[idx], upto)
        live[idx[past]] = False
        idx, a, u2, t_next = idx[~past], a[~past], u2[~past], t_next[~past]
        if not len(idx):
            continue
        j, close = jref.choose(a, u2)
        near[idx] |= close
        x[idx] += tab["change"][j]
        t[idx] = t_next
        fired[idx] += 1
    rest = (np.arange(Q)[None, :] >= q[:, None]) & (status == 0)[:, None]
    rows, cols = np.nonzero(rest)
    outs[rows, cols] = x[rows]
    return x, fired, status, near, outs


def check_replay(net, th, xs, times, path_times, key, particles, paths, lineage, n_events, label=""):
    """The replay of one smoother run against float64, segment by segment from the run's own start states: ``particles [M, K, N,
    S]`` (the filter's store), ``paths [M, D, Q, S]``, ``lineage`` / ``n_events [M, D, K]`` (numpy), th: theta fp32 [M, P] (torch),
    xs [M, S].  At most ``CAP`` of the (record, segment) pairs are undecidable (asserted first); every other pair matches exactly:
    the owned outputs, the event count and the particle the segment ends in.  Returns (flagged, pairs)."""
    tab = jref.tables(net)
    rates = net.kernel_parameters(th.double()).numpy()
    M, D, K = lineage.shape
    N = particles.shape[2]
    begin = ownership(path_times, times)
    flagged, wrong = 0, 0
    for m in range(M):
        for k in range(K):
            lin = lineage[m, :, k]
            start = np.repeat(xs[m][None], D, axis=0) if k == 0 else particles[m, k - 1][lineage[m, :, k - 1]]
            x, fired, status, near, outs = run_segments_states(tab, start, rates[m], times[k - 1] if k else 0.0, times[k], k, m * N + lin, key,
                                                               4096, path_times[begin[k]:begin[k + 1]])
            assert (status == 0).all()
            same = (outs == paths[m, :, begin[k]:begin[k + 1]]).all(axis=(1, 2)) & (fired == n_events[m, :, k]) \
                & (x == particles[m, k][lin]).all(axis=1)
            flagged += int(near.sum())
            wrong += int((~same & ~near).sum())
    total = M * D * K
    print(f"{label}: the reference flags {flagged} of {total} (record, segment) pairs ({flagged / total:.1e}); {wrong} of the others differ")
    assert flagged <= CAP * total
    assert wrong == 0
    return flagged, total


# --- the general form: records that bring their own start state, theta row, path slots and key; any event cap; stopped segments
DEAD_PATH = 0xFFFFFFFF          # noise_path[K - 1] of a record without a path


def trace(ancestors, last):
    """lineage [M, D, K] (int64) from ancestors [M, K, N] and the final slots last [M, D]; a slot outside 0 .. N - 1 is a dead draw:
    -1 at every observation."""
    ancestors, last = np.asarray(ancestors, dtype=np.int64), np.asarray(last, dtype=np.int64)
    M, K, N = ancestors.shape
    dead = (last < 0) | (last >= N)
    cols = [np.where(dead, 0, last)]
    for k in range(K - 1, 0, -1):
        cols.append(np.take_along_axis(ancestors[:, k - 1], cols[-1], axis=1))
    return np.where(dead[:, :, None], -1, np.stack(cols[::-1], axis=2))


def records_of_lineage(particles, lineage, xs, rates, key):
    """The B = M D records of the draws of M filters, record r = m D + d, in numpy: (x0 [B, S], rates [B, .], anchors [B, K, S] =
    particles[m, k, lineage[m, d, k]], noise_path [B, K] = m N + lineage[m, d, k] (DEAD_PATH in the last column of a dead draw, whose
    other entries are 0), keys [B, 2])."""
    particles, lineage = np.asarray(particles, dtype=np.int64), np.asarray(lineage, dtype=np.int64)
    M, D, K = lineage.shape
    N = particles.shape[2]
    dead = lineage[:, :, -1] < 0
    slot = np.where(dead[:, :, None], 0, lineage)
    anchors = np.stack([particles[m, np.arange(K)[None, :], slot[m]] for m in range(M)]).reshape(M * D, K, -1)
    noise = np.where(dead[:, :, None], 0, np.arange(M)[:, None, None] * N + slot)
    noise[:, :, -1] = np.where(dead, DEAD_PATH, noise[:, :, -1])
    keys = np.repeat(np.asarray([[int(v) & 0xFFFFFFFF for v in key]], dtype=np.int64), M * D, axis=0)
    return np.repeat(np.asarray(xs, dtype=np.int64), D, axis=0), np.repeat(np.asarray(rates, dtype=np.float64), D, axis=0), anchors, \
        noise.reshape(M * D, K), keys


def anchored_inputs(particles, lineage, x0, theta, key):
    """``records_of_lineage`` in torch on the tensors' device, as ``_hip.jump_anchored_replay`` takes them: particles int32 [M, K, N,
    S], lineage int32 [M, D, K] (-1: dead), x0 int32 [M, S], theta [M, P], key: two int32 words -> (x0 [B, S], theta [B, P], anchors int32
    [B, K, S], noise_path int32 [B, K] (uint32 bits), keys int32 [B, 2])."""
    import torch
    M, D, K = lineage.shape
    N, S = particles.shape[2], particles.shape[3]
    lin = lineage.long()
    dead = lin[:, :, -1] < 0
    slot = torch.where(dead[:, :, None], torch.zeros_like(lin), lin)
    anchors = torch.gather(particles, 2, slot.permute(0, 2, 1)[..., None].expand(M, K, D, S)).permute(0, 2, 1, 3).reshape(M * D, K, S)
    noise = torch.arange(M, device=lin.device)[:, None, None] * N + slot
    noise = torch.where(dead[:, :, None], torch.zeros_like(noise), noise)
    noise[:, :, -1] = torch.where(dead, torch.full_like(noise[:, :, -1], DEAD_PATH), noise[:, :, -1])
    noise = torch.where(noise >= 2 ** 31, noise - 2 ** 32, noise).to(torch.int32).reshape(M * D, K)
    return x0.repeat_interleave(D, 0).contiguous(), theta.repeat_interleave(D, 0).contiguous(), anchors.contiguous(), noise.contiguous(), \
        key.reshape(1, 2).to(torch.int32).repeat(M * D, 1).contiguous()


def replay_records(tab, x0, rates, anchors, noise_path, keys, times, path_times, max_events, begin=None, **defect):
    """The float64 replay of B records: segment k of record r runs from ``anchors[r, k - 1]`` (``x0[r]`` for k = 0) on the uniforms of
    path ``noise_path[r, k]`` under ``keys[r]`` with ``rates[r]``, for at most ``max_events`` events, and writes the outputs it owns
    (``ownership``; ``begin``: another table, for an injected defect).  A record with ``noise_path[r, K - 1] = DEAD_PATH`` is dead:
    paths -1, events and status 0.  One ``run_segments_states`` call per segment and distinct key, over all live records.  Returns a
    dict: ``paths [B, Q, S]`` (-1 where nothing was written), ``n_events``, ``status``, ``undecidable [B, K]``, ``ends [B, K, S]``."""
    x0, anchors, noise_path = np.asarray(x0, dtype=np.int64), np.asarray(anchors, dtype=np.int64), np.asarray(noise_path, dtype=np.int64)
    keys, rates = np.asarray(keys, dtype=np.int64) & 0xFFFFFFFF, np.asarray(rates, dtype=np.float64)
    B, K, S = anchors.shape
    begin = ownership(path_times, times) if begin is None else begin
    out = dict(paths=np.full((B, len(path_times), S), -1, dtype=np.int64), n_events=np.zeros((B, K), dtype=np.int64),
               status=np.zeros((B, K), dtype=np.int64), undecidable=np.zeros((B, K), dtype=bool), ends=np.full((B, K, S), -1, dtype=np.int64))
    live = noise_path[:, -1] != DEAD_PATH
    for key in np.unique(keys[live], axis=0):
        idx = np.nonzero(live & (keys == key[None, :]).all(axis=1))[0]
        for k in range(K):
            x, fired, status, near, outs = run_segments_states(tab, x0[idx] if k == 0 else anchors[idx, k - 1], rates[idx], times[k - 1] if k else 0.0,
                                                               times[k], k, noise_path[idx, k], tuple(int(v) for v in key), max_events,
                                                               path_times[begin[k]:begin[k + 1]], **defect)
            out["paths"][idx, begin[k]:begin[k + 1]] = outs
            out["n_events"][idx, k], out["status"][idx, k], out["undecidable"][idx, k], out["ends"][idx, k] = fired, status, near, x
    return out


def score_records(want, paths, n_events, status, ends, times, path_times, label="", quiet=False):
    """A replay launch of B records against ``want``, the ``replay_records`` of the same inputs at the same cap: ``paths [B, Q, S]``,
    ``n_events`` / ``status [B, K]`` as the launch returned them, ``ends [B, K, S]`` the states its segments are to end in (the
    anchors, or the stored particles along the lineage).  At most ``CAP`` of the B K (record, segment) pairs of the launch are
    undecidable (asserted first); every other pair matches exactly: the owned outputs with their -1, the event count, the status,
    and for status 0 the end state.  A dead record is never undecidable.  Returns (flagged, differing, pairs); raises AssertionError."""
    paths, n_events, status, ends = (np.asarray(v, dtype=np.int64) for v in (paths, n_events, status, ends))
    B, K = want["status"].shape
    assert paths.shape == want["paths"].shape and n_events.shape == (B, K) and status.shape == (B, K) and ends.shape == want["ends"].shape
    begin = ownership(path_times, times)
    same = (n_events == want["n_events"]) & (status == want["status"])
    same &= (want["status"] != 0) | (want["ends"] == ends).all(axis=2) | (want["ends"] == -1).all(axis=2)      # ends -1: a dead record
    for k in range(K):
        same[:, k] &= (paths[:, begin[k]:begin[k + 1]] == want["paths"][:, begin[k]:begin[k + 1]]).all(axis=(1, 2))
    flagged, wrong, total = int(want["undecidable"].sum()), int((~same & ~want["undecidable"]).sum()), B * K
    if not quiet:
        print(f"{label}: the reference flags {flagged} of {total} (record, segment) pairs ({flagged / total:.1e}); {wrong} of the others differ; "
              f"{int(want['n_events'].sum())} events, segments by status {np.bincount(want['status'].reshape(-1), minlength=3).tolist()}")
    assert flagged <= CAP * total
    assert wrong == 0
    return flagged, int((~same).sum()), total


# --- the inputs of the replay checks the CPU and GPU tests share: (network arguments, likelihood tuple of jump_filter_reference,
# start states [3, S], theta float64 [3, P], observations [K, S], key).  tests/test_jump_smoother.py runs them through the torch route
# in float64 and asserts the cap with the reference alone, before tests/test_jump_smoother_gpu.py relies on them
REPLAY_TIMES = [0.0, 0.25, 0.25, 1.0]                              # a zero and a duplicate
REPLAY_PATH_TIMES = [0.0, 0.1, 0.2, 0.25, 0.5, 0.75, 1.0]          # the observation times, two interior times per gap, one at 0
REPLAY_RUNS = [("bd", 192, ("poisson", 0.9, None)), ("sir", 192, ("poisson", 0.9, None)), ("net4", 192, ("gaussian", 25.0, None)),
               ("chain8", 192, ("gaussian", 25.0, None)), ("kinetic_chain8", 64, ("gaussian", 2500.0, None))]


def replay_case(name, N):
    spec, x0, theta = jref.cases()[name]
    xs, th = jref.per_path_inputs(x0, theta, 3, seed=len(name))
    ys = np.round(np.asarray(x0, dtype=np.float64)[None, :] + np.random.default_rng(N).integers(0, 3, size=(len(REPLAY_TIMES), len(x0))))
    return spec, xs, th, ys, (0x9E3779B9 ^ N, 0x7F4A7C15 + len(name))


# --- the exact smoothing marginals of immigration-death (0 -> X at rate birth, X -> 0 at rate death x) observed with Poisson noise
class ImmigrationDeath:
    """Forward-backward on the states 0 .. size - 1.  The transition over a gap dt is binomial thinning (a molecule survives with
    e^{-death dt}; its matrix does not depend on the birth rate and is formed once per gap) followed by a convolution with a
    Poisson(birth / death (1 - e^{-death dt})) vector: the transition of ``_birth_posterior`` in tests/test_jump_filter_gpu.py."""

    def __init__(self, death, x0, times, ys, size=200):
        self.death, self.x0, self.times, self.ys, self.size = float(death), int(x0), [float(t) for t in times], [float(y) for y in ys], size
        self.states = np.arange(size, dtype=np.float64)
        self.lgam = np.array([math.lgamma(k + 1.0) for k in range(size)])
        lam = np.maximum(self.states, cref.RATE_FLOOR)
        self.lik = [np.exp(y * np.log(lam) - lam - math.lgamma(y + 1.0)) for y in self.ys]
        self._thin = {}

    def _parts(self, birth, dt):
        dt = round(dt, 12)
        if dt not in self._thin:
            q = math.exp(-self.death * dt)
            self._thin[dt] = np.array([[math.comb(n, k) * q ** k * (1 - q) ** (n - k) if k <= n else 0.0 for k in range(self.size)]
                                       for n in range(self.size)])
        mu = birth / self.death * (1.0 - math.exp(-self.death * dt))
        return self._thin[dt], np.exp(self.states * math.log(mu) - mu - self.lgam)

    def _forward(self, alpha, birth, dt):
        """alpha T: the law after the gap dt of a state with law alpha."""
        thin, pois = self._parts(birth, dt)
        return np.convolve(alpha @ thin, pois)[:self.size]

    def _backward(self, beta, birth, dt):
        """T beta with T[n, m] = sum_k thin[n, k] pois[m - k]."""
        thin, pois = self._parts(birth, dt)
        return thin @ np.convolve(beta[::-1], pois)[:self.size][::-1]

    def log_likelihood(self, birth):
        alpha = np.zeros(self.size)
        alpha[self.x0] = 1.0
        t_prev, ll = 0.0, 0.0
        for t, lik in zip(self.times, self.lik):
            if t > t_prev:
                alpha = self._forward(alpha, birth, t - t_prev)
            t_prev = t
            alpha = alpha * lik
            ll += math.log(alpha.sum())
            alpha = alpha / alpha.sum()
        return ll

    def smoothing_mean(self, birth, t):
        """E[x_t | y] for 0 <= t <= the last observation time: observations at times <= t enter the forward half."""
        alpha = np.zeros(self.size)
        alpha[self.x0] = 1.0
        t_prev = 0.0
        first_after = len(self.times)
        for k, (tk, lik) in enumerate(zip(self.times, self.lik)):
            if tk > t:
                first_after = k
                break
            if tk > t_prev:
                alpha = self._forward(alpha, birth, tk - t_prev)
            t_prev = tk
            alpha = alpha * lik
            alpha = alpha / alpha.sum()
        if t > t_prev:
            alpha = self._forward(alpha, birth, t - t_prev)
        beta = np.ones(self.size)
        for k in range(len(self.times) - 1, first_after - 1, -1):
            beta = beta * self.lik[k]
            before = self.times[k - 1] if k > first_after else t
            if self.times[k] > before:
                beta = self._backward(beta, birth, self.times[k] - before)
            beta = beta / beta.max()
        post = alpha * beta
        return float((post * self.states).sum() / post.sum())


def birth_posterior(model, grid, prior):
    """(p [G], log p [G]) of the birth rate on the uniform ``grid`` under ``prior`` (the package's Prior, one dim)."""
    import torch
    logp = np.array([model.log_likelihood(b) for b in grid])
    logp = logp + prior.log_prob(torch.tensor(grid, dtype=torch.float64)[:, None]).reshape(-1).numpy()
    p = np.exp(logp - logp.max())
    return p / p.sum(), logp


def weighted_path_mean(loglik, exact, x):
    """The self-normalised estimate ``sum r_m x_m / sum r_m`` with ``r_m = exp(ll_m - exact)`` over M independent filters (``E[p^
    f(x_draw)] = p(y) E[f(x) | y]``: no O(1 / N) bias) and its delta-method standard error; x [M, ...]: (estimate, se, std(r))."""
    r = np.exp(np.asarray(loglik, dtype=np.float64) - exact)
    x = np.asarray(x, dtype=np.float64)
    M = len(r)
    rb = r.reshape((M,) + (1,) * (x.ndim - 1))
    est = (rb * x).sum(axis=0) / r.sum()
    se = np.sqrt(((rb * (x - est)) ** 2).sum(axis=0)) / r.sum()
    return est, se, float(r.std(ddof=1))
