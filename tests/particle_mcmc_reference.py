"""float64 numpy helpers for the particle-MCMC tests: one Metropolis step (close + open, the rule of
viforsdes_amd/inference/particle_mcmc.py and include/vsde_hip.h: vsde_pmmh_step) from the numpy Philox of tests/philox_reference.py,
the exact log-likelihood of the discretised scalar Ornstein-Uhlenbeck model vectorised over theta rows, and ``exact_mh``: the same
chain rule (proposals, acceptance, warm-up) with an exact likelihood in place of the particle filter's estimate."""
import math

import numpy as np

from philox_reference import _uniform, box_muller, philox4x32_10

_MASK = 0xFFFFFFFF
_HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)


def _key(key):
    return tuple(int(v) & _MASK for v in key)


def proposal_normals(C, P, iteration, key):
    """z [C, P]: normal j of chain c is the Box-Muller normal j & 3 of philox4x32_10({iteration, j >> 2, c, 3}, key)."""
    k0, k1 = _key(key)
    c, blk = np.meshgrid(np.arange(C), np.arange((P + 3) // 4), indexing="ij")
    w = philox4x32_10(iteration, blk, c, 3, k0, k1)
    z0, z1 = box_muller(w[0], w[1])
    z2, z3 = box_muller(w[2], w[3])
    return np.stack([z0, z1, z2, z3], axis=-1).reshape(C, -1)[:, :P]


def acceptance_log_uniforms(C, iteration, key):
    k0, k1 = _key(key)
    return np.log(_uniform(philox4x32_10(iteration, 0, np.arange(C), 4, k0, k1)[0]).astype(np.float64))


def filter_key(iteration, key):
    k0, k1 = _key(key)
    w = philox4x32_10(iteration, 0, 0, 5, k0, k1)
    return np.array([int(w[0]), int(w[1])], dtype=np.uint32)


def constrain(u, mask):
    with np.errstate(over="ignore"):
        return np.where(mask, np.exp(u), u)


def log_prior_jacobian(theta, u, mask, prior_type, prior_mean, prior_std):
    """log p(theta) (prior_type 0: iid Normal, 1: iid LogNormal) + sum over the positive dims of u."""
    with np.errstate(invalid="ignore", divide="ignore"):
        if prior_type == 1:
            lg = np.where(mask, u, np.log(theta))
            zed = (lg - prior_mean) / prior_std
            lp = -0.5 * zed * zed - math.log(prior_std) - _HALF_LOG_2PI - lg
        else:
            zed = (theta - prior_mean) / prior_std
            lp = -0.5 * zed * zed - math.log(prior_std) - _HALF_LOG_2PI
    return lp.sum(axis=-1) + np.where(mask, u, 0.0).sum(axis=-1)


def log_mean_exp(loglik):
    """[C] from [C, R]: NaN if a row holds a NaN (or +inf), -inf if all of it is -inf."""
    loglik = np.asarray(loglik, dtype=np.float64)
    mx = loglik.max(axis=1, keepdims=True)
    safe = np.where(np.isneginf(mx), 0.0, mx)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (safe + np.log(np.exp(loglik - safe).sum(axis=1, keepdims=True)) - math.log(loglik.shape[1]))[:, 0]


def close_step(iteration, key, loglik, prop_u, prop_log_prior, cur_u, cur_target, cur_loglik):
    """The end of iteration ``iteration``: dict(cur_u, cur_log_target, cur_loglik, accept, log_alpha, log_u, prop_target)."""
    ll = log_mean_exp(loglik)
    target = prop_log_prior + ll
    log_u = acceptance_log_uniforms(cur_u.shape[0], iteration, key)
    with np.errstate(invalid="ignore"):
        log_alpha = target - cur_target
        ok = ~np.isnan(target)
        acc = ok if iteration == 0 else ok & ~np.isneginf(target) & (log_u < log_alpha)
    return dict(cur_u=np.where(acc[:, None], prop_u, cur_u), cur_log_target=np.where(acc, target, cur_target),
                cur_loglik=np.where(acc, ll, cur_loglik), accept=acc, log_alpha=log_alpha, log_u=log_u, prop_target=target)


def open_step(iteration, key, cur_u, prop_u, L, step_size, mask, prior_type, prior_mean, prior_std, R):
    """The start of iteration ``iteration``: dict(prop_u, theta_prop [C R, P], prop_log_prior, filter_key).  Iteration 0 proposes
    ``prop_u`` as given."""
    C, P = cur_u.shape
    if iteration > 0:
        prop_u = cur_u + step_size * (proposal_normals(C, P, iteration, key) @ np.asarray(L, dtype=np.float64).T)
    theta = constrain(prop_u, mask)
    return dict(prop_u=prop_u, theta_prop=np.repeat(theta, R, axis=0), filter_key=filter_key(iteration, key),
                prop_log_prior=log_prior_jacobian(theta, prop_u, mask, prior_type, prior_mean, prior_std))


def step(iteration, key, L, step_size, mask, prior_type, prior_mean, prior_std, R, loglik_prop, cur_u, cur_target, cur_loglik, prop_u,
         prop_log_prior):
    """One launch of vsde_pmmh_step in float64: closes iteration ``iteration - 1`` (unless loglik_prop is None) and opens
    ``iteration``.  Returns the dict of close_step (when closed) merged with that of open_step and ``sample_row``."""
    f64 = lambda v: np.asarray(v, dtype=np.float64)
    out = dict(cur_u=f64(cur_u), cur_log_target=f64(cur_target), cur_loglik=f64(cur_loglik))
    if loglik_prop is not None:
        out = close_step(iteration - 1, key, f64(loglik_prop), f64(prop_u), f64(prop_log_prior), f64(cur_u), f64(cur_target), f64(cur_loglik))
    out["sample_row"] = constrain(out["cur_u"], mask)
    out.update(open_step(iteration, key, out["cur_u"], f64(prop_u), L, step_size, mask, prior_type, prior_mean, prior_std, R))
    return out


def ou_kalman_rows(theta, dt, variance, x0, rows, ys):
    """Exact log-likelihood [M] of the Euler-Maruyama-discretised scalar Ornstein-Uhlenbeck model for theta [M, 3] = (kappa, mu,
    sigma): the scalar Kalman filter of particle_filter_reference.ou_kalman, vectorised over the rows."""
    theta = np.asarray(theta, dtype=np.float64)
    kappa, mu, sigma = theta[:, 0], theta[:, 1], theta[:, 2]
    a, c, q = 1.0 - kappa * dt, kappa * mu * dt, sigma * sigma * dt
    m, p = np.full(theta.shape[0], float(x0)), np.zeros(theta.shape[0])
    t, ll = 0, np.zeros(theta.shape[0])
    with np.errstate(all="ignore"):
        for row, y in zip(rows, np.asarray(ys, dtype=np.float64).reshape(-1)):
            while t < row:
                m, p = a * m + c, a * a * p + q
                t += 1
            r, s = y - m, p + variance
            ll += -0.5 * (r * r / s + np.log(2.0 * np.pi * s))
            g = p / s
            m, p = m + g * r, p - g * p
    return ll


def adapted_scale_tril(history, current):
    """Lower Cholesky factor of cov(history [n, P]) + 1e-8 I, or ``current`` if that is not positive definite."""
    P = history.shape[1]
    cov = np.cov(history.T).reshape(P, P) + 1e-8 * np.eye(P)
    if not np.isfinite(cov).all():
        return current
    try:
        return np.linalg.cholesky(cov)
    except np.linalg.LinAlgError:
        return current


def exact_mh(log_likelihood, u0, mask, prior, n_iterations, warmup, key, scale_tril=None, step_size=None, thin=1, adapt=True,
             target_accept=0.15, adapt_interval=25):
    """The chain rule of ``particle_mcmc`` with ``log_likelihood(theta [C, P]) -> [C]`` (exact, float64) in place of the filter:
    the same proposals, acceptance rule, defaults and warm-up.  ``prior = (prior_type, mean, std)``.  Returns (u [n_keep, C, P],
    acceptance rate [C] after warm-up)."""
    u0 = np.asarray(u0, dtype=np.float64)
    C, P = u0.shape
    mask = np.asarray(mask, dtype=bool)
    L = np.asarray(scale_tril, dtype=np.float64) if scale_tril is not None else \
        (np.diag(np.maximum(u0.std(axis=0, ddof=1), 1e-3)) if C > 1 else np.eye(P))
    step_size = 2.38 / math.sqrt(P) if step_size is None else float(step_size)
    adapt = adapt and C > P
    cur_u, cur_t, cur_ll = u0.copy(), np.full(C, -np.inf), np.full(C, -np.inf)
    w4, w2 = warmup // 4, warmup // 2
    history, kept, window, kept_acc = [], [], 0, np.zeros(C)
    for i in range(n_iterations):
        if 0 < i <= warmup and i % adapt_interval == 0:
            step_size *= math.exp(window / (C * adapt_interval) - target_accept)
            window = 0
        if adapt and i == w2 and w4 < w2:
            L = adapted_scale_tril(np.concatenate(history, axis=0), L)
            step_size = 2.38 / math.sqrt(P)
        o = open_step(i, key, cur_u, u0, L, step_size, mask, *prior, 1)
        c = close_step(i, key, log_likelihood(o["theta_prop"])[:, None], o["prop_u"], o["prop_log_prior"], cur_u, cur_t, cur_ll)
        cur_u, cur_t, cur_ll = c["cur_u"], c["cur_log_target"], c["cur_loglik"]
        window += int(c["accept"].sum())
        if i >= warmup:
            kept_acc += c["accept"]
            if (i - warmup) % thin == 0:
                kept.append(cur_u)
        elif w4 <= i < w2:
            history.append(cur_u)
    return np.stack(kept), kept_acc / (n_iterations - warmup)


# ------------------------------------------------------------------------------------------------ inputs of the step-kernel tests
KERNEL_CASE_KEY = (0x0BADCAFE, 0x13572468)
KERNEL_CASE_GRID = dict(C=(1, 63, 65, 300), P=(1, 3, 16), R=(1, 3), prior_type=(0, 1), mask=("none", "some", "all"),
                        iteration=(0, 1, 7))


def kernel_case(C, P, R, prior_type, mask, iteration):
    """Given inputs of one vsde_pmmh_step launch, every array holding fp32 values: ordinary chains plus (C > 4: chains 1..4; C = 1:
    one of them, by the case) a NaN estimate, estimates all -inf, a current target of -inf, and one -inf among R estimates.
    ``loglik_prop`` is None at iteration 0 (nothing to close)."""
    rng = np.random.default_rng(1000003 * C + 10007 * P + 101 * R + 11 * prior_type + 3 * iteration + len(mask))
    f32 = lambda v: np.asarray(v, dtype=np.float32)
    pos = np.zeros(P, dtype=bool)
    if mask == "all":
        pos[:] = True
    elif mask == "some":
        pos[::2] = True
    # LogNormal prior: log(theta') of a dim that is not log-transformed amplifies the fp32 rounding of u' by 1 / theta', which is a
    # property of the inputs and not of the kernel, so those cases keep theta' away from zero (u around 2..3.5, a small L); one chain
    # sits at -1 on such a dim, where the prior is NaN on both sides
    scale = 0.1 if prior_type == 1 else 1.0
    L = f32(np.tril(rng.normal(size=(P, P)) * 0.3 * scale))
    L[np.arange(P), np.arange(P)] = f32((0.2 + np.abs(rng.normal(size=P)) * 0.5) * scale)
    prior = (prior_type, 0.2, 1.3)
    cur_u = np.abs(rng.normal(size=(C, P))) * 0.5 + 2.0 if prior_type == 1 else rng.normal(size=(C, P)) * 0.5
    if prior_type == 1 and C > 5 and not pos.all():
        cur_u[5, np.nonzero(~pos)[0][0]] = -1.0
    cur_u = f32(cur_u).astype(np.float64)
    prop_u = f32(cur_u + rng.normal(size=(C, P)) * 0.3 * scale).astype(np.float64)
    cur_ll = f32(rng.normal(size=C) * 2.0 - 20.0).astype(np.float64)
    cur_t = f32(log_prior_jacobian(constrain(cur_u, pos), cur_u, pos, *prior) + cur_ll).astype(np.float64)
    prop_lp = f32(log_prior_jacobian(constrain(prop_u, pos), prop_u, pos, *prior)).astype(np.float64)
    loglik = f32(rng.normal(size=(C, R)) * 2.0 - 20.0).astype(np.float64)
    special = {c: c for c in range(1, 5)} if C > 4 else {0: (P + R + iteration) % 5}
    for c, what in special.items():
        if what == 1:
            loglik[c, R // 2] = np.nan
        elif what == 2:
            loglik[c] = -np.inf
        elif what == 3:
            cur_t[c] = cur_ll[c] = -np.inf
        elif what == 4:
            loglik[c, 0] = -np.inf          # R = 1: all of them
    case = dict(C=C, P=P, R=R, iteration=iteration, key=KERNEL_CASE_KEY, L=L, step_size=0.7, mask=pos, prior=prior,
                loglik_prop=None if iteration == 0 else loglik, cur_u=cur_u, cur_log_target=cur_t, cur_loglik=cur_ll, prop_u=prop_u,
                prop_log_prior=prop_lp)
    if iteration > 0 and C < 100:
        # the tests allow 1 % of a case's chains to be undecidable (a near tie of float64 itself): below 100 chains that is none,
        # so a chain of such a case that draws a near tie (about 1 in 10^4 does) has its estimates moved by 0.01
        out = kernel_case_reference(case)
        with np.errstate(invalid="ignore"):
            near = np.abs(out["log_alpha"] - out["log_u"]) <= tolerance(out["prop_target"], cur_t)
        loglik[near] = f32(loglik[near] + 0.01).astype(np.float64)
    return case


def kernel_case_reference(case):
    """``step`` on a ``kernel_case``."""
    return step(case["iteration"], case["key"], case["L"], case["step_size"], case["mask"], *case["prior"], case["R"],
                case["loglik_prop"], case["cur_u"], case["cur_log_target"], case["cur_loglik"], case["prop_u"], case["prop_log_prior"])


def tolerance(*arrays):
    """1e-5 max(1, largest finite magnitude in the arrays): the bound of the filter tests' log-weight increments."""
    big = [np.abs(a[np.isfinite(a)]).max() for a in (np.asarray(a, dtype=np.float64) for a in arrays) if np.isfinite(a).any()]
    return 1e-5 * max([1.0] + big)


# -------------------------------------------------------------------------------- the end-to-end problem: discretised OU, 40 steps
OU_TIMES, OU_VALUES, OU_DT, OU_VARIANCE = (0.0, 0.5, 1.0, 1.5, 2.0), (2.0, 1.5, 0.8, 1.2, 0.9), 0.05, 0.1
OU_ROWS = (0, 10, 20, 30, 40)
OU_PRIOR = (1, 0.0, 0.5)                 # iid LogNormal(0, 0.5) on (kappa, mu, sigma): all three walk in log space
OU_MASK = (True, True, True)
_OU_CACHE = {}


def ou_initial_theta(C):
    """Start points [C, 3]: draws of the prior."""
    return np.exp(np.random.default_rng(20240607).normal(OU_PRIOR[1], OU_PRIOR[2], size=(C, 3)))


def ou_exact_chains(C, n_iterations, warmup):
    """u [n_keep, C, 3] of ``exact_mh`` on the OU problem with its own key, computed once per (C, n_iterations, warmup)."""
    args = (C, n_iterations, warmup)
    if args not in _OU_CACHE:
        ll = lambda th: ou_kalman_rows(th, OU_DT, OU_VARIANCE, OU_VALUES[0], OU_ROWS, OU_VALUES)
        u, _ = exact_mh(ll, np.log(ou_initial_theta(C)), OU_MASK, OU_PRIOR, n_iterations, warmup, (0x600DF00D, 0x0EC5AC7))
        u.setflags(write=False)
        _OU_CACHE[args] = u
    return _OU_CACHE[args]


def two_sample_z(u_a, u_b):
    """|z| [P] between the posterior means of two sets of independent chains u [n, C, P]: the difference of the means of the
    per-chain means over the root of the summed squared standard errors, each from the spread over its chains."""
    a, b = np.asarray(u_a, dtype=np.float64).mean(axis=0), np.asarray(u_b, dtype=np.float64).mean(axis=0)
    se = np.sqrt(a.var(axis=0, ddof=1) / a.shape[0] + b.var(axis=0, ddof=1) / b.shape[0])
    return np.abs(a.mean(axis=0) - b.mean(axis=0)) / se
