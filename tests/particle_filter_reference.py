"""float64 numpy helpers for the particle-filter tests: the exact likelihood of a linear-Gaussian model (Kalman filter), the
filter's observation stage (weights, summaries, systematic resampling) and its resampling uniforms from the numpy Philox of
tests/philox_reference.py."""
import numpy as np

from philox_reference import _uniform, philox4x32_10

_MASK = 0xFFFFFFFF


def kalman_log_likelihood(A, c, Q, H, R, x0, rows, ys):
    """log p(y_0 .. y_{K-1} | x at row 0 = x0) of  x_{t+1} = A x_t + c + N(0, Q),  y_k = H x_{rows[k]} + N(0, R)  (all float64;
    several observations may share a row; an observation at row 0 contributes log N(y; H x0, R))."""
    A, c, Q, H, R = (np.asarray(v, dtype=np.float64) for v in (A, c, Q, H, R))
    m, P = np.asarray(x0, dtype=np.float64).copy(), np.zeros_like(Q)
    t, ll = 0, 0.0
    for row, y in zip(rows, np.asarray(ys, dtype=np.float64)):
        while t < row:
            m, P = A @ m + c, A @ P @ A.T + Q
            t += 1
        r, Sy = y - H @ m, H @ P @ H.T + R
        ll += -0.5 * (r @ np.linalg.solve(Sy, r) + np.linalg.slogdet(2.0 * np.pi * Sy)[1])
        G = P @ H.T @ np.linalg.inv(Sy)
        m, P = m + G @ r, P - G @ H @ P
    return float(ll)


def ou_kalman(theta, dt, variance, x0, rows, ys):
    """Exact log-likelihood of the Euler-Maruyama-discretised Ornstein-Uhlenbeck model, theta = (kappa, mu, sigma)."""
    kappa, mu, sigma = (float(v) for v in theta)
    return kalman_log_likelihood([[1.0 - kappa * dt]], [kappa * mu * dt], [[sigma * sigma * dt]], [[1.0]], [[variance]], x0, rows, ys)


def linear_diagonal_kalman(theta, dt, variance, H, x0, rows, ys):
    """Exact log-likelihood of the discretised LinearDiagonalSDE(S): theta = (a [S], b [S]), G = diag(softplus(b) + 1e-3)."""
    theta = np.asarray(theta, dtype=np.float64)
    S = theta.size // 2
    g = np.log1p(np.exp(theta[S:])) + 1e-3
    O = np.asarray(H).shape[0]
    return kalman_log_likelihood(np.diag(1.0 - theta[:S] * dt), np.zeros(S), np.diag(g * g * dt), H, variance * np.eye(O), x0, rows, ys)


def gaussian_log_weights(y, x, variance, H=None):
    """lw [..., N] of particles x [..., N, S] for one observation y [O] (float64); NaN counts as -inf."""
    x = np.asarray(x, dtype=np.float64)
    pred = x if H is None else x @ np.asarray(H, dtype=np.float64).T
    r = np.asarray(y, dtype=np.float64) - pred
    lw = (-0.5 * r * r / variance - 0.5 * np.log(2.0 * np.pi * variance)).sum(axis=-1)
    return np.where(np.isnan(lw), -np.inf, lw)


def observation_stage(lw, x):
    """(increment, ess, mean [S], std [S], w [N]) of one filter at one observation from lw [N], x [N, S] (float64, max finite)."""
    mx = lw.max()
    w = np.exp(lw - mx)
    s1 = w.sum()
    xs = np.where(w[:, None] > 0, x, 0.0)
    mean = (w[:, None] * xs).sum(axis=0) / s1
    std = np.sqrt((w[:, None] * np.where(w[:, None] > 0, x - mean, 0.0) ** 2).sum(axis=0) / s1)
    return mx + np.log(s1) - np.log(len(lw)), s1 * s1 / (w * w).sum(), mean, std, w


def systematic_ancestors(w, u):
    """ancestor_j = min(#{i : C_i <= (j + u) / N C_{N-1}}, N - 1) in float64, w [N] >= 0."""
    w = np.asarray(w, dtype=np.float64)
    N = w.size
    C = np.cumsum(w)
    tau = (np.arange(N) + float(u)) / N * C[-1]
    return np.minimum(np.searchsorted(C, tau, side="right"), N - 1)


def resampling_uniforms(M, K, key):
    """u [M, K]: ((w0 >> 8) + 0.5) 2^-24 (fp32) with w0 the first word of philox4x32_10({k, 0, m, 1}, key)."""
    k0, k1 = (int(v) & _MASK for v in key)
    m, k = np.meshgrid(np.arange(M), np.arange(K), indexing="ij")
    return _uniform(philox4x32_10(k, 0, m, 1, k0, k1)[0])
