"""numpy helpers for the residual-bridge particle-filter tests: an independent restatement of one residual segment
(``proposal="residual_bridge"`` of viforsdes_amd/inference/particle_filter.py).  It makes its own passes of the deterministic
companion path eta (the whole path is tabulated first, so eta_end is its last row and f(eta) is read from the table), takes
psi^-1 from a general solver, not from the specification's triangular solves, and runs in float64 (the reference) or float32 (what
fp32 arithmetic alone costs on the same inputs).  Cases, rows and the shared pieces are those of tests/guided_filter_reference.py."""
import numpy as np

from guided_filter_reference import PIVOT_FLOOR, STATE_FLOOR, floored_cholesky

# Where tests/guided_filter_reference.py shortens the Lotka-Volterra cases (LV_ROWS: the last row 14 instead of 20, because the
# bridge filter's float64 ESS falls below N / 20 over 12 steps) the residual bridge keeps the full 12-step segment: measured on the
# CPU in float64 with M = 64 filters and the GPU test's keys, the smallest ESS over filters and observations is 28.7 of 64 and 572
# of 1024 (lv), 29.7 and 616 (lv_prey); tests/test_residual_bridge.py lists every case
ROWS = [0, 1, 3, 3, 8, 20]   # n = 1, a shared row, a segment inside one Philox block of four, segments that cross blocks


def rows_of(name):
    return ROWS


def _clamp(x, positive_dims, dtype):
    for i in positive_dims:
        x[:, i] = np.where(x[:, i] < dtype(STATE_FLOOR), dtype(STATE_FLOOR), x[:, i])
    return x


def companion_path(coef, start, theta, n, dt, positive_dims=(), dtype=np.float64):
    """The noise-free Euler path from ``start`` [B, S]: (eta [n + 1, B, S], f(eta) [n, B, S], bound [n]) with ``bound[s]`` whether
    the clamp changed any entry in step s."""
    eta = np.empty((n + 1,) + start.shape, dtype=dtype)
    drift = np.empty((n,) + start.shape, dtype=dtype)
    bound = np.zeros(n, dtype=bool)
    eta[0] = np.asarray(start, dtype=dtype)
    theta = np.asarray(theta, dtype=dtype)
    for s in range(n):
        drift[s] = coef(eta[s], theta)[0]
        raw = (eta[s] + dtype(dt) * drift[s]).astype(dtype)
        eta[s + 1] = _clamp(raw.copy(), positive_dims, dtype)
        bound[s] = bool((eta[s + 1] != raw).any())
    return eta, drift, bound


def residual_segment(coef, start, theta, z, y, H, variance, dt, positive_dims=(), dtype=np.float64):
    """The states and log-ratios after the ``n = z.shape[1]`` residual-bridge steps towards the observation ``y [O]`` that lies n
    grid steps ahead: start [B, S], theta [B, P], z [B, n, S] (the steps' normals) -> (x [B, S], lr [B], eta_bound [n]), all
    arithmetic in ``dtype``."""
    x = np.asarray(start, dtype=dtype).copy()
    theta, z, y = np.asarray(theta, dtype=dtype), np.asarray(z, dtype=dtype), np.asarray(y, dtype=dtype)
    B, S = x.shape
    n = z.shape[1]
    Hm = np.eye(S, dtype=dtype) if H is None else np.asarray(H, dtype=dtype)
    O = Hm.shape[0]
    dt, var, eye_o, eye_s = dtype(dt), dtype(variance), np.eye(O, dtype=dtype), np.eye(S, dtype=dtype)
    lr = np.zeros(B, dtype=dtype)
    with np.errstate(all="ignore"):
        eta, f_eta, bound = companion_path(coef, x, theta, n, dt, positive_dims, dtype)
        for step in range(n):
            left = dtype(n - step)
            f, L = coef(x, theta)
            A = np.sqrt(dt) * np.einsum("ok,bki->boi", Hm, L)
            psi = left * np.einsum("boi,bqi->boq", A, A) + var * eye_o
            ahead = eta[n] + (x - eta[step]) + left * dt * (f - f_eta[step])
            e = y[None, :] - ahead @ Hm.T
            sol = np.linalg.solve(psi, np.concatenate([A, e[..., None]], axis=-1)).astype(dtype)   # psi^-1 [A | e]
            m = np.einsum("boi,bo->bi", A, sol[..., -1])
            C = eye_s[None] - np.einsum("boi,bok->bik", A, sol[..., :-1])
            Mf = floored_cholesky(C, PIVOT_FLOOR, dtype)
            zs = z[:, step]
            eps = m + np.einsum("bik,bk->bi", Mf, zs)
            lr = lr - dtype(0.5) * (eps * eps).sum(axis=-1) + dtype(0.5) * (zs * zs).sum(axis=-1) \
                + np.log(np.diagonal(Mf, axis1=1, axis2=2)).sum(axis=-1)
            x = _clamp(x + f * dt + np.sqrt(dt) * np.einsum("bik,bk->bi", L, eps), positive_dims, dtype)
            x, lr = x.astype(dtype), lr.astype(dtype)
    return x, lr, bound
