"""float64 / exact-integer numpy helpers for the tests of particle MCMC with paths: the draw of a proposal's path record (the rule
of viforsdes_amd/inference/particle_mcmc.py, steps 5-7, and include/vsde_hip.h: vsde_pmmh_step_paths) from the numpy Philox of
tests/philox_reference.py, one launch of vsde_pmmh_step_paths on given inputs, the inputs of the step-kernel test, and the exact
joint-posterior path moments of the discretised Ornstein-Uhlenbeck problem of tests/particle_mcmc_reference.py."""
import numpy as np

import particle_mcmc_reference as mref
from philox_reference import _uniform, philox4x32_10

DEAD = 0xFFFFFFFF


def path_uniforms(C, iteration, key):
    """(v0, v1), float32 [C] each: ((w >> 8) + 0.5) 2^-24 of the first and second word of philox4x32_10({iteration, 0, c, 6}, key)."""
    k0, k1 = mref._key(key)
    w = philox4x32_10(iteration, 0, np.arange(C), 6, k0, k1)
    return _uniform(w[0]), _uniform(w[1])


def choose_filter(loglik, v0):
    """(r* [C], margin [C]) in float64 for estimates loglik [C, R] without NaN and not all -inf per row: r* = min(#{r : C_r <= v0
    C_{R-1}}, R - 1) over the inclusive sums C of exp(loglik - max); margin = min_r |v0 C_{R-1} - C_r|, the distance of the threshold
    from the nearest boundary."""
    loglik = np.asarray(loglik, dtype=np.float64)
    w = np.exp(loglik - loglik.max(axis=1, keepdims=True))
    cum = np.maximum.accumulate(np.cumsum(w, axis=1), axis=1)
    tau = np.asarray(v0, dtype=np.float64)[:, None] * cum[:, -1:]
    return np.minimum((cum <= tau).sum(axis=1), loglik.shape[1] - 1), np.abs(tau - cum).min(axis=1)


def final_slot(v1, N):
    """J = min(floor(v1 N), N - 1) with the product formed in float32, as the kernel and the torch route form it."""
    return np.minimum(np.floor(np.asarray(v1, dtype=np.float32) * np.float32(N)).astype(np.int64), N - 1)


def trace_lineage(ancestors, J):
    """lineage [K] of one filter: lineage[K-1] = a[K-1, J], lineage[k-1] = a[k-1, lineage[k]], every entry clamped into [0, N - 1]
    (ancestors [K, N] integers)."""
    K, N = ancestors.shape
    lin = np.empty(K, dtype=np.int64)
    lin[K - 1] = min(max(int(ancestors[K - 1, J]), 0), N - 1)
    for k in range(K - 1, 0, -1):
        lin[k - 1] = min(max(int(ancestors[k - 1, lin[k]]), 0), N - 1)
    return lin


def draw_records(loglik, particles, ancestors, iteration, key, r_star=None):
    """The proposals' records of one iteration: dict(r [C], J [C], lineage [C, K], anchors [C, K, S], noise_path [C, K] (int64 holding
    uint32), margin [C]) from loglik [C, R], particles [C R, K, N, S], ancestors [C R, K, N].  A chain whose estimates are all -inf
    or hold a NaN is dead: r = J = lineage = -1, noise_path all ones, anchors NaN, margin inf.  ``r_star``: use these filter choices
    instead of the float64 ones (a kernel's, where the threshold sits on a boundary)."""
    loglik = np.asarray(loglik, dtype=np.float64)
    C, R = loglik.shape
    _, K, N, S = particles.shape
    v0, v1 = path_uniforms(C, iteration, key)
    with np.errstate(invalid="ignore"):
        mx = loglik.max(axis=1)
    live = mx > -np.inf                                                   # False for NaN too
    out = dict(r=np.full(C, -1), J=np.full(C, -1), lineage=np.full((C, K), -1), anchors=np.full((C, K, S), np.nan),
               noise_path=np.full((C, K), DEAD, dtype=np.int64), margin=np.full(C, np.inf))
    if live.any():
        r, margin = choose_filter(loglik[live], v0[live])
        out["r"][live], out["margin"][live] = r, margin
    if r_star is not None:
        out["r"][live] = np.asarray(r_star)[live]
    J = final_slot(v1, N)
    for c in np.nonzero(live)[0]:
        m = c * R + out["r"][c]
        lin = trace_lineage(np.asarray(ancestors[m]), J[c])
        out["J"][c], out["lineage"][c] = J[c], lin
        out["anchors"][c] = np.asarray(particles[m])[np.arange(K), lin]
        out["noise_path"][c] = m * N + lin
    return out


# ------------------------------------------------------------------------------------------ inputs of the step-kernel test (paths)
PATH_CASE_GRID = dict(C=(1, 63, 65, 300), P=(1, 3, 16), R=(1, 3), K=(1, 2, 5), N=(64, 128), S=(1, 3))


def path_case(C, P, R, K, N, S, iteration=7):
    """A ``particle_mcmc_reference.kernel_case`` (LogNormal prior, mixed mask; ``iteration`` 1 closes iteration 0, which accepts a
    proposal whose estimates are all -inf: a dead record) with the store of its filters: particles
    [C R, K, N, S] holding distinct fp32 values (the flat index), ancestors [C R, K, N] random with one entry in 16 out of range
    (below 0 or at least N), and the chains' previous records (distinct from anything a draw can give)."""
    case = mref.kernel_case(C, P, R, 1, "some", iteration)
    rng = np.random.default_rng(77 * C + 13 * P + 5 * R + 3 * K + N + S + iteration)
    M = C * R
    case["particles"] = np.arange(M * K * N * S, dtype=np.float32).reshape(M, K, N, S)        # < 2^24: exact in fp32
    assert case["particles"].size < 2 ** 24
    anc = rng.integers(0, N, size=(M, K, N))
    wild = rng.random(size=anc.shape) < 1.0 / 16.0
    anc[wild] = rng.choice([-1, -7, N, N + 3, 2 ** 30], size=int(wild.sum()))
    case["ancestors"] = anc.astype(np.int32)
    case["cur_anchor"] = -1.0 - rng.random(size=(C, K, S)).astype(np.float32)
    case["cur_noise_path"] = (2 ** 31 + rng.integers(0, 1000, size=(C, K))).astype(np.int64)
    case["cur_path_iteration"] = np.full(C, 3, dtype=np.int32)
    case.update(K=K, N=N, S=S)
    return case


# ---------------------------------------------------------------------- the joint posterior of the OU problem: exact path moments
_OU_PATH_CACHE = {}


def ou_rts_rows(theta, dt, variance, x0, rows, ys):
    """``particle_smoother_reference.ou_rts`` vectorised over theta [M, 3] = (kappa, mu, sigma): smoothing mean and variance
    [M, T+1] of the scalar model (the same Kalman and Rauch-Tung-Striebel recursions on scalars; tests/test_pmmh_paths.py holds it
    to ``ou_rts``)."""
    theta = np.asarray(theta, dtype=np.float64)
    a, c, q = 1.0 - theta[:, 0] * dt, theta[:, 0] * theta[:, 1] * dt, theta[:, 2] ** 2 * dt
    M, T = theta.shape[0], int(rows[-1])
    mp, Pp, mf, Pf = (np.zeros((T + 1, M)) for _ in range(4))
    m, P = np.full(M, float(x0)), np.zeros(M)
    for t in range(T + 1):
        if t > 0:
            m, P = a * m + c, a * a * P + q
        mp[t], Pp[t] = m, P
        for k in [k for k, row in enumerate(rows) if row == t]:
            g = P / (P + variance)
            m, P = m + g * (float(ys[k]) - m), P - g * P
        mf[t], Pf[t] = m, P
    ms, Ps = mf.copy(), Pf.copy()
    for t in range(T - 1, -1, -1):
        G = Pf[t] * a / Pp[t + 1]
        ms[t] = mf[t] + G * (ms[t + 1] - mp[t + 1])
        Ps[t] = Pf[t] + G * G * (Ps[t + 1] - Pp[t + 1])
    return ms.T, Ps.T


def ou_exact_path_moments(C, n_iterations, warmup, stride=5):
    """Per chain of ``particle_mcmc_reference.ou_exact_chains`` (every ``stride``-th kept state): (mean [C, T+1], second moment
    [C, T+1]) of x_{0:T} under the chain's mixture of exact smoothing distributions: the average over its theta of the
    Rauch-Tung-Striebel mean, and of variance + mean^2 (so second moment - mean^2 is the average of the variances plus the
    variance of the means).  Computed once per argument tuple and left unchanged."""
    args = (C, n_iterations, warmup, stride)
    if args not in _OU_PATH_CACHE:
        u = mref.ou_exact_chains(C, n_iterations, warmup)[::stride]
        n = u.shape[0]
        mean, var = ou_rts_rows(np.exp(u.reshape(n * C, 3)), mref.OU_DT, mref.OU_VARIANCE, mref.OU_VALUES[0], mref.OU_ROWS, mref.OU_VALUES)
        m1 = mean.reshape(n, C, -1).mean(axis=0)
        m2 = (var + mean * mean).reshape(n, C, -1).mean(axis=0)
        m1.setflags(write=False)
        m2.setflags(write=False)
        _OU_PATH_CACHE[args] = (m1, m2)
    return _OU_PATH_CACHE[args]


def path_moment_z(paths, exact_m1, exact_m2):
    """(z of the means [T], z of the spreads [T]) over grid rows 1 .. T between PMMH paths [n, C, T+1] (one state dim) and the exact
    per-chain moments [C, T+1]: two-sample z of the per-chain means, and of the per-chain mean squared deviations from the pooled
    exact mean (their expectation is the pooled variance whatever the autocorrelation of a chain, which a per-chain sample variance
    is not); each denominator is the root of the summed squared standard errors from the spread over the chains of either side."""
    x = np.asarray(paths, dtype=np.float64)[:, :, 1:]
    e1, e2 = exact_m1[:, 1:], exact_m2[:, 1:]
    C = x.shape[1]
    mu = e1.mean(axis=0)
    a, b = x.mean(axis=0), e1
    z_mean = np.abs(a.mean(axis=0) - b.mean(axis=0)) / np.sqrt(a.var(axis=0, ddof=1) / C + b.var(axis=0, ddof=1) / C)
    sa, sb = ((x - mu) ** 2).mean(axis=0), e2 - 2.0 * mu * e1 + mu * mu
    z_spread = np.abs(sa.mean(axis=0) - sb.mean(axis=0)) / np.sqrt(sa.var(axis=0, ddof=1) / C + sb.var(axis=0, ddof=1) / C)
    return z_mean, z_spread
