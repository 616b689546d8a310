"""numpy float64 restatement of tau-leaping (viforsdes_amd/core/tau_leap.py, viforsdes_amd/inference/tau_leap_filter.py), written
independently of the package on the specified Philox stream (counter {t, j | ((q >> 1) << 16), b, 8}; tests/philox_reference.py),
with the propensities of tests/jump_process_reference.py and the observation stage of tests/jump_filter_reference.py.

A network is the plain tables of ``jump_process_reference.tables``; ``rates [B, 2R]`` are the effective constants; ``tau`` is the
step as the route under test holds it (``float(np.float32(time_step))`` for the fp32 kernels)."""
import math

import numpy as np

import jump_filter_reference as jfref
import jump_process_reference as jref
import particle_filter_reference as pref
from philox_reference import _uniform, philox4x32_10

MAX_RATE = float(2 ** 30)
MAX_COPY = 2 ** 30
FLAG_EPS = 2.0 ** -20        # 16 fp32 roundings; the longest propensity chain of the specification (Hill n = 4, gate, tau) has 11
_lgamma = np.vectorize(math.lgamma, otypes=[np.float64])


def attempt_uniforms(step, reaction, path, attempt, key):
    """(u1, u2) float64 arrays: the fp32 uniforms of attempt q of reaction j at step t of path b, widened."""
    step, reaction, path, attempt = np.broadcast_arrays(*(np.asarray(v, dtype=np.int64) for v in (step, reaction, path, attempt)))
    k0, k1 = (int(v) & 0xFFFFFFFF for v in key)
    w = philox4x32_10(step, reaction | ((attempt >> 1) << 16), path, 8, k0, k1)
    odd = (attempt & 1) == 1
    return (_uniform(np.where(odd, w[2], w[0])).astype(np.float64), _uniform(np.where(odd, w[3], w[1])).astype(np.float64))


def poisson_draws(lam, step, reaction, path, key):
    """(n, attempts, ok) int64 / int64 / bool arrays of the draws for the rates ``lam`` (float64, finite, >= 0) on the words of
    (step, reaction, path), all broadcast together and flattened: ``attempts`` is 0 for lam == 0, 1 for the inversion, the PTRS
    attempts otherwise; ``ok`` False where the 32nd attempt was rejected."""
    lam, step, reaction, path = np.broadcast_arrays(np.asarray(lam, dtype=np.float64), *(np.asarray(v, dtype=np.int64)
                                                                                        for v in (step, reaction, path)))
    lam, step, reaction, path = lam.ravel(), step.ravel(), reaction.ravel(), path.ravel()
    n, attempts, ok = np.zeros(lam.shape, dtype=np.int64), np.zeros(lam.shape, dtype=np.int64), np.ones(lam.shape, dtype=bool)
    small = np.nonzero((lam > 0) & (lam < 10.0))[0]
    if len(small):
        l = lam[small]
        u1 = attempt_uniforms(step[small], reaction[small], path[small], 0, key)[0]
        p = np.exp(-l)
        F, m = p.copy(), np.zeros(len(small), dtype=np.int64)
        go = np.ones(len(small), dtype=bool)
        while True:
            go = go & (u1 > F) & (m < 63)
            if not go.any():
                break
            m[go] += 1
            p[go] = p[go] * (l[go] / m[go])
            F[go] = F[go] + p[go]
        n[small], attempts[small] = m, 1
    idx = np.nonzero(lam >= 10.0)[0]
    for q in range(32):
        if not len(idx):
            break
        l = lam[idx]
        b = 0.931 + 2.53 * np.sqrt(l)
        a = -0.059 + 0.02483 * b
        inv_alpha = 1.1239 + 1.1328 / (b - 3.4)
        v_r = 0.9277 - 3.6224 / (b - 2.0)
        u1, V = attempt_uniforms(step[idx], reaction[idx], path[idx], q, key)
        Uc = u1 - 0.5
        us = 0.5 - np.abs(Uc)
        accept = np.zeros(len(idx), dtype=bool)
        m = np.zeros(len(idx))
        alive = ~((us < 0.013) & (V > us))                     # us can be 0: this test comes before n is formed
        w = np.nonzero(alive)[0]
        m[w] = np.floor(((2.0 * a[w]) / us[w] + b[w]) * Uc[w] + l[w] + 0.43)
        squeeze = alive & (us >= 0.07) & (V <= v_r)
        accept |= squeeze
        w = np.nonzero(alive & ~squeeze & (m >= 0))[0]
        lhs = (np.log(V[w]) + np.log(inv_alpha[w])) - np.log(a[w] / (us[w] * us[w]) + b[w])
        rhs = (-l[w] + m[w] * np.log(l[w])) - _lgamma(m[w] + 1.0)
        accept[w] = lhs <= rhs
        attempts[idx] = q + 1
        n[idx[accept]] = m[accept].astype(np.int64)
        idx = idx[~accept]
    ok[idx] = False
    return n, attempts, ok


def flagged_draws(lam, step, reaction, path, key):
    """(n, flagged): the draws at ``lam`` and whether an implementation that forms ``lam`` with fp32 roundings may legitimately
    differ: the result or the attempt count differs between ``lam (1 - 2^-20)`` and ``lam (1 + 2^-20)``, or the two straddle 10."""
    lam, step, reaction, path = (v.ravel() for v in np.broadcast_arrays(np.asarray(lam, dtype=np.float64), step, reaction, path))
    n = poisson_draws(lam, step, reaction, path, key)[0]
    lo, hi = lam * (1.0 - FLAG_EPS), lam * (1.0 + FLAG_EPS)
    n_lo, q_lo, _ = poisson_draws(lo, step, reaction, path, key)
    n_hi, q_hi, _ = poisson_draws(hi, step, reaction, path, key)
    return n, (n_lo != n_hi) | (q_lo != q_hi) | ((lo < 10.0) != (hi < 10.0))


def apply_draws(tab, x, raw):
    """The reactions in order with the cap on the running state: (x_new [B, S], reduced [B]) from x [B, S] and the raw draws [B, R],
    in integers."""
    x = np.asarray(x, dtype=np.int64).copy()
    reduced = np.zeros(x.shape[0], dtype=np.int64)
    for j in range(tab["reactants"].shape[0]):
        n = np.asarray(raw[:, j], dtype=np.int64).copy()
        for i, r in enumerate(tab["reactants"][j]):
            if r > 0:
                n = np.minimum(n, x[:, i] // int(r))
        reduced += n < raw[:, j]
        x += n[:, None] * tab["change"][j][None, :]
    return x, reduced


def step_rates(tab, x, rates, tau):
    """(lam [B, R] float64, invalid [B]): the rates of a step and whether a propensity or a rate stops the path."""
    with np.errstate(invalid="ignore", over="ignore"):
        a = jref.propensities(tab, x, rates)
        lam = a * float(tau)
        invalid = ~np.all(np.isfinite(a) & (a >= 0), axis=1) | np.any(lam > MAX_RATE, axis=1)
    return lam, invalid


def leap(tab, x, rates, tau, step_begin, step_end, paths, key, draws=None):
    """Steps step_begin .. step_end - 1 of the paths: (x [B, S], status [B], capped [B]); ``draws [B, E, R]`` takes the raw draws of the
    steps t < E the paths complete."""
    x = np.asarray(x, dtype=np.int64).copy()
    B, R = x.shape[0], tab["reactants"].shape[0]
    rates = np.broadcast_to(np.asarray(rates, dtype=np.float64), (B, np.shape(rates)[-1]))
    paths = np.asarray(paths, dtype=np.int64)
    status, capped = np.zeros(B, dtype=np.int64), np.zeros(B, dtype=np.int64)
    live = np.ones(B, dtype=bool)
    for t in range(int(step_begin), int(step_end)):
        idx = np.nonzero(live)[0]
        if not len(idx):
            break
        lam, bad = step_rates(tab, x[idx], rates[idx], tau)
        status[idx[bad]], live[idx[bad]] = 2, False
        idx, lam = idx[~bad], lam[~bad]
        if not len(idx):
            continue
        n, _, ok = poisson_draws(lam, t, np.arange(R)[None, :], paths[idx][:, None], key)
        raw, ok = n.reshape(len(idx), R), ok.reshape(len(idx), R).all(axis=1)
        xn, reduced = apply_draws(tab, x[idx], raw)
        ok = ok & ~np.any(xn > MAX_COPY, axis=1)
        status[idx[~ok]], live[idx[~ok]] = 2, False
        done = idx[ok]
        x[done], capped[done] = xn[ok], capped[done] + reduced[ok]
        if draws is not None and t < draws.shape[1]:
            draws[done, t] = raw[ok]
    return x, status, capped


def simulate(tab, x0, rates, rows, tau, key, E):
    """(states [B, K, S], status [B], capped [B], draws [B, E, R]) as ``tau_leap_process`` defines them."""
    x = np.asarray(x0, dtype=np.int64).copy()
    B, S = x.shape
    R = tab["reactants"].shape[0]
    states = np.full((B, len(rows), S), -1, dtype=np.int64)
    status, capped = np.zeros(B, dtype=np.int64), np.zeros(B, dtype=np.int64)
    draws = np.full((B, E, R), -1, dtype=np.int64)
    t = 0
    for k, row in enumerate(rows):
        live = np.nonzero(status == 0)[0]
        log = np.full((len(live), E, R), -1, dtype=np.int64)
        x[live], st, cap = leap(tab, x[live], np.asarray(rates)[live], tau, t, row, live, key, log)
        done = log[:, :, 0] >= 0
        draws[live] = np.where(done[:, :, None], log, draws[live])
        status[live], capped[live] = st, capped[live] + cap
        t = int(row)
        ok = status == 0
        states[ok, k] = x[ok]
    return states, status, capped, draws


def run_filter(tab, x0, rates, rows, tau, ys, like, N, key):
    """The whole filter: a dict of ``log_likelihood [M]``, ``increments``, ``ess [M, K]``, ``mean``, ``std [M, K, S]``, ``stopped``,
    ``capped [M, K]``, ``particles [M, K, N, S]``, ``ancestors``, ``log_weights [M, K, N]``."""
    x0, rates, ys = np.asarray(x0, dtype=np.int64), np.asarray(rates, dtype=np.float64), np.asarray(ys, dtype=np.float64)
    M, S = x0.shape
    K = len(rows)
    u = pref.resampling_uniforms(M, K, key)
    out = dict(increments=np.zeros((M, K)), ess=np.zeros((M, K)), mean=np.zeros((M, K, S)), std=np.zeros((M, K, S)),
               stopped=np.zeros((M, K), dtype=np.int64), capped=np.zeros((M, K), dtype=np.int64),
               particles=np.zeros((M, K, N, S), dtype=np.int64), ancestors=np.zeros((M, K, N), dtype=np.int64),
               log_weights=np.zeros((M, K, N)))
    for m in range(M):
        x = np.repeat(x0[m][None], N, axis=0)
        for k in range(K):
            x, status, capped = leap(tab, x, rates[m], tau, rows[k - 1] if k else 0, rows[k], m * N + np.arange(N), key)
            with np.errstate(invalid="ignore", divide="ignore"):
                lw = jfref.log_weights(like, ys[k], x)
            lw = np.where((status != 0) | np.isnan(lw), -np.inf, lw)
            inc, ess, mean, std, anc = jfref.stage(lw, x, u[m, k])
            out["increments"][m, k], out["ess"][m, k], out["mean"][m, k], out["std"][m, k] = inc, ess, mean, std
            out["stopped"][m, k], out["capped"][m, k] = int((status != 0).sum()), int(capped.sum())
            out["particles"][m, k], out["ancestors"][m, k], out["log_weights"][m, k] = x, anc, lw
            x = x[anc]
    out["log_likelihood"] = out["increments"].sum(axis=1)
    return out


# --- the checks of one kernel call on its own log (tests/test_tau_leap_gpu.py): no whole trajectory is compared
def check_process(net, xs, th32, rows, time_step, res, key, label=""):
    """The simulator kernel against float64 on the state before every step, rebuilt from x0 and the kernel's own logged draws (the
    log must hold every step: E >= rows[-1]).  The reference's flagged share of the draws is asserted first (at most 1e-2: a cap,
    not a tolerance); every unflagged draw equals the kernel's; ``states``, ``capped`` and ``status`` follow exactly, in integers,
    from the kernel's draws.  Returns a dict of the counts the case conditions are about."""
    import torch
    tab = jref.tables(net)
    xs = np.asarray(xs, dtype=np.int64)
    rates = net.kernel_parameters(torch.as_tensor(th32, dtype=torch.float32)).double().numpy()
    tau = float(np.float32(time_step))
    draws = res.draws.cpu().numpy().astype(np.int64)
    B, E, R = draws.shape
    T = int(rows[-1])
    assert E >= T and res.draws.dtype == torch.int32
    taken = draws[:, :, 0] >= 0
    assert np.array_equal(taken[:, :, None] & np.ones(R, dtype=bool), draws >= 0)              # a row is whole or -1
    n_steps = taken.sum(axis=1)
    assert np.array_equal(taken, np.arange(E)[None, :] < n_steps[:, None]) and n_steps.max() <= T   # a prefix of each path
    x, capped = xs.copy(), np.zeros(B, dtype=np.int64)
    states = np.full((B, len(rows), xs.shape[1]), -1, dtype=np.int64)
    lam_all, n_all, where = [], [], []
    stop_legit = np.ones(B, dtype=bool)
    for t in range(T + 1):
        for k, row in enumerate(rows):
            if row == t:
                reached = n_steps >= t
                states[reached, k] = x[reached]
        if t == T:
            break
        idx = np.nonzero(taken[:, t])[0]
        lam, bad = step_rates(tab, x[idx], rates[idx], tau)
        assert not bad.any()                                       # a step the kernel took has valid float64 rates
        lam_all.append(lam)
        n_all.append(draws[idx, t])
        where.append(np.stack(np.broadcast_arrays(np.full((len(idx), R), t), np.arange(R)[None, :], idx[:, None]), axis=-1))
        # a path that stopped at this step: float64 on the same state stops too, or sits within the fp32 margin of a bound
        stopped = np.nonzero(n_steps == t)[0]
        if len(stopped):
            lam_s, bad_s = step_rates(tab, x[stopped], rates[stopped], tau)
            near = np.any(lam_s > MAX_RATE * (1.0 - FLAG_EPS), axis=1)
            n_s, _, ok_s = poisson_draws(np.where(bad_s[:, None], 0.0, lam_s), t, np.arange(R)[None, :], stopped[:, None], key)
            xn_s, _ = apply_draws(tab, x[stopped], n_s.reshape(len(stopped), R))
            stop_legit[stopped] = bad_s | near | ~ok_s.reshape(len(stopped), R).all(axis=1) | np.any(xn_s > MAX_COPY, axis=1)
        xn, reduced = apply_draws(tab, x[idx], draws[idx, t])
        assert xn.min() >= 0 and xn.max() <= MAX_COPY
        x[idx], capped[idx] = xn, capped[idx] + reduced
    lam_all, n_all, where = np.concatenate(lam_all).ravel(), np.concatenate(n_all).ravel(), np.concatenate(where).reshape(-1, 3)
    n_ref, flagged = flagged_draws(lam_all, where[:, 0], where[:, 1], where[:, 2], key)
    differ = n_ref != n_all
    total = len(n_all)
    print(f"{label}: {total} draws, lam up to {lam_all.max():.1f}: the reference flags {int(flagged.sum())} ({flagged.mean():.1e}); "
          f"{int((differ & ~flagged).sum())} of the others differ ({int(differ.sum())} in all); capped {int(capped.sum())}, "
          f"stopped paths {int((n_steps < T).sum())}")
    assert flagged.sum() <= 1e-2 * total                           # the reference's own share first: a cap, not a tolerance
    assert not np.any(differ & ~flagged)
    assert np.array_equal(res.states.cpu().numpy(), states) and res.states.dtype == torch.int32
    assert np.array_equal(res.capped.cpu().numpy(), capped)
    assert np.array_equal(res.status.cpu().numpy(), np.where(n_steps < T, 2, 0))
    assert stop_legit.all()
    return dict(draws=total, zero=int((lam_all == 0).sum()), inversion=int(((lam_all > 0) & (lam_all < 10.0)).sum()),
                ptrs=int((lam_all >= 10.0).sum()), capped=int(capped.sum()), flagged=int(flagged.sum()), max_rate=float(lam_all.max()),
                stopped=int((n_steps < T).sum()))


def flagged_leap(tab, x, rates, tau, step_begin, step_end, paths, key):
    """``leap`` that also says which paths are flagged: some draw of the path is flagged (``flagged_draws``) or some rate sits
    within the fp32 margin of 2^30: (x, status, capped, flagged [B])."""
    x = np.asarray(x, dtype=np.int64).copy()
    B, R = x.shape[0], tab["reactants"].shape[0]
    rates = np.broadcast_to(np.asarray(rates, dtype=np.float64), (B, np.shape(rates)[-1]))
    paths = np.asarray(paths, dtype=np.int64)
    status, capped, flagged = np.zeros(B, dtype=np.int64), np.zeros(B, dtype=np.int64), np.zeros(B, dtype=bool)
    for t in range(int(step_begin), int(step_end)):
        idx = np.nonzero(status == 0)[0]
        if not len(idx):
            break
        lam, bad = step_rates(tab, x[idx], rates[idx], tau)
        flagged[idx] |= np.any(np.abs(lam - MAX_RATE) <= MAX_RATE * FLAG_EPS, axis=1)
        status[idx[bad]] = 2
        idx, lam = idx[~bad], lam[~bad]
        if not len(idx):
            continue
        _, f = flagged_draws(lam, t, np.arange(R)[None, :], paths[idx][:, None], key)
        flagged[idx] |= f.reshape(len(idx), R).any(axis=1)
        x[idx], st, cap = leap(tab, x[idx], rates[idx], tau, t, t + 1, paths[idx], key)
        status[idx], capped[idx] = st, capped[idx] + cap
    return x, status, capped, flagged


def check_filter_propagation(net, th, xs, rows, time_step, res, key, label=""):
    """Segment k again in float64 from the kernel's particles at k - 1 gathered through the kernel's ancestors: at most 2e-2 of the
    (particle, segment) pairs are flagged (asserted first), every other pair equals the kernel exactly: the state, and per segment
    the stopped and capped counts when no pair of it is flagged.  th: theta fp32 [M, P] (torch), xs: start states [M, S]."""
    tab = jref.tables(net)
    rates = net.kernel_parameters(th.double()).numpy()
    tau = float(np.float32(time_step))
    parts, anc = res.particles.cpu().numpy().astype(np.int64), res.ancestors.cpu().numpy().astype(np.int64)
    stopped, capped = res.stopped.cpu().numpy(), res.capped.cpu().numpy()
    M, K, N = parts.shape[:3]
    flagged, wrong, steps = 0, 0, 0
    for m in range(M):
        for k in range(K):
            start = np.repeat(np.asarray(xs[m], dtype=np.int64)[None], N, axis=0) if k == 0 else parts[m, k - 1][anc[m, k - 1]]
            x, status, cap, flag = flagged_leap(tab, start, rates[m], tau, rows[k - 1] if k else 0, rows[k], m * N + np.arange(N), key)
            flagged += int(flag.sum())
            wrong += int(((x != parts[m, k]).any(axis=1) & ~flag).sum())
            steps += int(rows[k] - (rows[k - 1] if k else 0))
            if not flag.any():
                wrong += int(stopped[m, k] != (status != 0).sum()) + int(capped[m, k] != cap.sum())
    total = M * K * N
    print(f"{label}: the reference flags {flagged} of {total} (particle, segment) pairs ({flagged / total:.1e}); {wrong} of the others "
          f"differ; {steps // M} steps a filter")
    assert flagged <= 2e-2 * total                                  # the reference's own share first: a cap, not a tolerance
    assert wrong == 0
    return flagged, total


def counted(name, monkeypatch=None):
    """A list that receives one entry per launch through ``_hip.<name>``; (calls, real, wrapped)."""
    from viforsdes_amd import _hip
    calls, real = [], getattr(_hip, name)
    wrapped = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    if monkeypatch is not None:
        monkeypatch.setattr(_hip, name, wrapped)
    return calls, real, wrapped


# --- the exact likelihood of the tau-leap of pure death (X -> 0 at rate d x) observed with Poisson noise: the forward recursion
# over the states 0 .. x0 with the capped-Poisson transition n ~ min(Poisson(d x tau), x)
def pure_death_log_likelihood(death, tau, x0, rows, ys, scale=1.0):
    import count_likelihood_reference as cref
    size = int(x0) + 1
    step = np.zeros((size, size))
    for x in range(size):
        lam = death * x * tau
        pmf = np.array([math.exp(n * math.log(lam) - lam - math.lgamma(n + 1.0)) if lam > 0 else float(n == 0) for n in range(x)])
        step[x, x - np.arange(x)] = pmf                            # n < x firings
        step[x, 0] += 1.0 - pmf.sum()                              # the cap: everything at or above x
    rate = np.maximum(scale * np.arange(size, dtype=np.float64), cref.RATE_FLOOR)
    alpha = np.zeros(size)
    alpha[int(x0)] = 1.0
    ll, t = 0.0, 0
    for row, y in zip(rows, ys):
        for _ in range(int(row) - t):
            alpha = alpha @ step
        t = int(row)
        alpha = alpha * np.exp(y * np.log(rate) - rate - math.lgamma(y + 1.0))
        total = alpha.sum()
        ll += math.log(total)
        alpha = alpha / total
    return ll


# --- the cases of the kernel tests (tests/test_tau_leap_gpu.py); tests/test_tau_leap.py asserts on the CPU the conditions on them
# that concern the float64 reference alone.  (network, start state, theta in parameter_names order, time step)
SIM_B, SIM_STEPS, SIM_ROWS = 256, 16, [0, 5, 5, 16]


def sim_cases():
    import reaction_networks as rn
    return {
        "sir": (rn.SIR, [12000, 120], [1.6e-4, 0.5], 0.25),                  # rates 50 .. 1800: PTRS where the accept test cancels most
        "immigration_death": (dict(reactants=[[0], [1]], products=[[1], [0]]), [0], [0.4, 0.8], 0.5),   # lam = 0 and the inversion
        "repress3": (rn.REPRESS3, [5, 0, 10], [60.0, 40.0, 0.4, 5.0], 0.5),   # Hill n = 2, 3, 4: the longest propensity chain
        "kinetic_chain8": (rn.KINETIC_CHAIN8, [3, 2, 2, 1, 1, 1, 0, 0], [3.0, 4.0, 0.2, 2.0, 3.0], 0.5),   # 8 species, 16 reactions
    }


def sim_case(name):
    """(net, xs int64 [B, S], th32 [B, P], time step, key) of a simulator case: per-path start states and constants
    (jump_process_reference.per_path_inputs); path 5 of "sir" has a negative constant and stops at step 0."""
    from viforsdes_amd import ReactionNetworkSDE
    names = sorted(sim_cases())
    spec, x0, theta, tau = sim_cases()[name]
    xs, th = jref.per_path_inputs(x0, theta, SIM_B, seed=40 + names.index(name))
    th = th.astype(np.float32)
    if name == "sir":
        th[5, 0] = -th[5, 0]
    return ReactionNetworkSDE(**spec), xs, th, tau, (0x51ED270B, 77 + names.index(name))


FILTER_M, FILTER_ROWS = 4, [3, 3, 7]           # segments of 3, 0 and 4 steps
H1, H2 = [[1.0, 0.5]], [[1.0, 1.0], [0.0, 1.0]]
FILTER_RUNS = [(name, N) for name in ("sir_poisson", "sir_nb_h", "autoreg_gauss_h") for N in (64, 256)]


def filter_case(name, N):
    """(net, theta fp32 [M, P] (torch), xs [M, S], ys [K, O], likelihood spec of jump_filter_reference, time step, key) of a filter
    case; rates of at most 200, the observations at the rounded mean of 32 float64 paths, so that the filters stay alive."""
    import torch
    import reaction_networks as rn
    from viforsdes_amd import ReactionNetworkSDE
    spec, x0, theta, tau, like = {
        "sir_poisson": (rn.SIR, [400, 5], [0.004, 0.5], 0.25, ("poisson", 0.9, None)),
        "sir_nb_h": (rn.SIR, [400, 5], [0.004, 0.5], 0.25, ("nb", 5.0, 1.0, np.array(H2))),
        "autoreg_gauss_h": (rn.AUTOREG, [2, 10], [50.0, 2.0, 0.3, 8.0], 0.2, ("gaussian", 25.0, np.array(H1))),
    }[name]
    net = ReactionNetworkSDE(**spec)
    xs, th = jref.per_path_inputs(x0, theta, FILTER_M, seed=len(name))
    th32 = torch.from_numpy(th).float()
    rates = net.kernel_parameters(th32.double()).numpy()
    mean = simulate(jref.tables(net), np.repeat(xs[:1], 32, axis=0), np.repeat(rates[:1], 32, axis=0), FILTER_ROWS, float(np.float32(tau)),
                    (1, 2), 0)[0].mean(axis=0)
    scale = like[1] if like[0] == "poisson" else like[2] if like[0] == "nb" else 1.0
    ys = np.round(scale * (mean if like[-1] is None else mean @ like[-1].T))
    return net, th32, xs, ys, like, tau, (0x9E3779B9 ^ N, 0x7F4A7C15 + len(name))
