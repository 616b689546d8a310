"""float64 numpy helpers for the particle-smoother tests: the exact smoothing distribution of a linear-Gaussian model (Kalman filter
plus Rauch-Tung-Striebel smoother, start state known), the final draw of the smoother (systematic sampling with D thresholds, its
uniform from the numpy Philox of tests/philox_reference.py), reference segments that keep every step, and the cases both test files
share (those of tests/test_particle_filter_gpu.py and a 6-species network)."""
import numpy as np
import torch

import guided_filter_reference as gref
from philox_reference import _uniform, box_muller, philox4x32_10

_MASK = 0xFFFFFFFF
FLOOR = float(np.float32(1e-6))
BLOCK_ROWS = [0, 3, 3, 10, 17]      # a segment inside one Philox block of four, a shared row, segments that start and end inside blocks
LATE_ROWS = [2, 7, 7, 13]           # the first observation lies after the start: segment 0 has steps of its own


def rts_smoother(A, c, Q, H, R, x0, rows, ys):
    """(mean [T+1, S], cov [T+1, S, S]) of x_t | y_0 .. y_{K-1}, t = 0 .. T = rows[-1], for x_{t+1} = A x_t + c + N(0, Q),
    y_k = H x_{rows[k]} + N(0, R), x at row 0 = x0 (all float64; several observations may share a row)."""
    A, c, Q, H, R = (np.asarray(v, dtype=np.float64) for v in (A, c, Q, H, R))
    ys, T, S = np.asarray(ys, dtype=np.float64), int(rows[-1]), A.shape[0]
    mp, Pp = np.zeros((T + 1, S)), np.zeros((T + 1, S, S))          # predicted (before the row's observations)
    mf, Pf = np.zeros((T + 1, S)), np.zeros((T + 1, S, S))          # filtered (after them)
    m, P = np.asarray(x0, dtype=np.float64).copy(), np.zeros((S, S))
    for t in range(T + 1):
        if t > 0:
            m, P = A @ m + c, A @ P @ A.T + Q
        mp[t], Pp[t] = m, P
        for k in [k for k, row in enumerate(rows) if row == t]:
            r, Sy = ys[k] - H @ m, H @ P @ H.T + R
            G = P @ H.T @ np.linalg.inv(Sy)
            m, P = m + G @ r, P - G @ H @ P
        mf[t], Pf[t] = m, P
    ms, Ps = mf.copy(), Pf.copy()
    for t in range(T - 1, -1, -1):
        G = Pf[t] @ A.T @ np.linalg.inv(Pp[t + 1])
        ms[t] = mf[t] + G @ (ms[t + 1] - mp[t + 1])
        Ps[t] = Pf[t] + G @ (Ps[t + 1] - Pp[t + 1]) @ G.T
    return ms, Ps


def ou_rts(theta, dt, variance, x0, rows, ys):
    """Smoothing mean and variance [T+1] of the Euler-Maruyama-discretised Ornstein-Uhlenbeck model, theta = (kappa, mu, sigma)."""
    kappa, mu, sigma = (float(v) for v in theta)
    m, P = rts_smoother([[1.0 - kappa * dt]], [kappa * mu * dt], [[sigma * sigma * dt]], [[1.0]], [[variance]], x0, rows, ys)
    return m[:, 0], P[:, 0, 0]


def linear_diagonal_rts(theta, dt, variance, H, x0, rows, ys):
    """Smoothing mean [T+1, S] and covariance [T+1, S, S] of the discretised LinearDiagonalSDE(S): theta = (a [S], b [S])."""
    theta = np.asarray(theta, dtype=np.float64)
    S = theta.size // 2
    g = np.log1p(np.exp(theta[S:])) + 1e-3
    O = np.asarray(H).shape[0]
    return rts_smoother(np.diag(1.0 - theta[:S] * dt), np.zeros(S), np.diag(g * g * dt), H, variance * np.eye(O), x0, rows, ys)


def systematic_draws(w, u, D):
    """slot_d = min(#{i : C_i <= (d + u) / D C_{N-1}}, N - 1) for d = 0 .. D - 1 in float64, w [N] >= 0."""
    w = np.asarray(w, dtype=np.float64)
    C = np.maximum.accumulate(np.cumsum(w))
    tau = (np.arange(D) + float(u)) / D * C[-1]
    return np.minimum(np.searchsorted(C, tau, side="right"), w.size - 1)


def smoothing_uniforms(M, key):
    """u [M]: ((w0 >> 8) + 0.5) 2^-24 (fp32) with w0 the first word of philox4x32_10({0, 0, m, 2}, key)."""
    k0, k1 = (int(v) & _MASK for v in key)
    return _uniform(philox4x32_10(0, 0, np.arange(M), 2, k0, k1)[0])


def path_noise(paths, T, S, key):
    """``forecast_noise`` of tests/philox_reference.py for the given path indices only: float64 [len(paths), T, S]."""
    k0, k1 = (int(v) & _MASK for v in key)
    nblk = (T + 3) // 4
    blk, i, b = np.meshgrid(np.arange(nblk), np.arange(S), np.asarray(paths, dtype=np.int64), indexing="ij")
    w = philox4x32_10(blk, i, b, 0, k0, k1)
    z = np.stack([*box_muller(w[0], w[1]), *box_muller(w[2], w[3])], axis=1)          # [nblk, 4, S, B]
    return np.ascontiguousarray(z.reshape(nblk * 4, S, -1)[:T].transpose(2, 0, 1))


def euler_segment_states(sde, start, theta, z, dt, positive_dims=()):
    """Every state [B, n, S] of the n = z.shape[1] float64 Euler-Maruyama steps from start [B, S] with the normals z [B, n, S]."""
    from viforsdes_amd.core.euler_maruyama import euler_maruyama
    z = torch.as_tensor(z, dtype=torch.float64)
    out = euler_maruyama(sde, torch.as_tensor(start, dtype=torch.float64), torch.as_tensor(theta, dtype=torch.float64),
                         z.shape[1] * dt, dt, tuple(positive_dims), noise=z)
    return out[:, 1:].numpy()


def guided_segment_states(sde, start, theta, z, y, H, variance, dt, positive_dims=()):
    """Every state [B, n, S] of the n guided steps towards y that lies n steps ahead (tests/guided_filter_reference.py:
    guided_segment keeps the end only: a segment of j steps towards an observation n steps ahead is not one of its calls, so the
    steps are its own rule, restated with the states kept)."""
    coef = gref.sde_coefficients(sde)
    x = np.asarray(start, dtype=np.float64).copy()
    theta, z, y = (np.asarray(v, dtype=np.float64) for v in (theta, z, y))
    S, n = x.shape[1], z.shape[1]
    Hm = np.eye(S) if H is None else np.asarray(H, dtype=np.float64)
    out = np.empty((x.shape[0], n, S))
    with np.errstate(all="ignore"):
        for step in range(n):
            left = float(n - step)
            f, L = coef(x, theta)
            A = np.sqrt(dt) * np.einsum("ok,bki->boi", Hm, L)
            psi = left * np.einsum("boi,bqi->boq", A, A) + variance * np.eye(Hm.shape[0])
            e = y[None, :] - (x + left * dt * f) @ Hm.T
            sol = np.linalg.solve(psi, np.concatenate([A, e[..., None]], axis=-1))
            m = np.einsum("boi,bo->bi", A, sol[..., -1])
            C = np.eye(S)[None] - np.einsum("boi,bok->bik", A, sol[..., :-1])
            Mf = gref.floored_cholesky(C, gref.PIVOT_FLOOR)
            eps = m + np.einsum("bik,bk->bi", Mf, z[:, step])
            x = x + f * dt + np.sqrt(dt) * np.einsum("bik,bk->bi", L, eps)
            for i in positive_dims:
                x[:, i] = np.where(x[:, i] < FLOOR, FLOOR, x[:, i])
            out[:, step] = x
    return out


SIR = dict(reactants=[[1, 1], [0, 1]], products=[[0, 2], [0, 0]])
AUTOREG_KW = dict(reactants=[[0, 0], [1, 0], [1, 0], [0, 1]], products=[[1, 0], [1, 1], [0, 0], [0, 0]], species=["M", "P"],
                  reactions=["transcription", "translation", "mRNA decay", "protein decay"],
                  rate_constants=["k_tx", "k_tl", 0.1, "d_P"])
# a conversion chain 0 -> A -> B -> C -> D -> E -> F -> 0 of six species
CHAIN6 = dict(reactants=[[0] * 6] + [[1 if i == j else 0 for i in range(6)] for j in range(6)],
              products=[[1, 0, 0, 0, 0, 0]] + [[1 if i == j + 1 else 0 for i in range(6)] for j in range(6)])


def case(name, M, rows=None):
    """(sde, observations, likelihood, theta [M, P], x0 [M, S], dt, positive dims) on the CPU, fp32: the cases of
    tests/test_particle_filter_gpu.py (every 4th filter of the positive-state cases starts at or near the 1e-6 floor) and "chain6".
    ``rows``: observe at these grid rows instead of the case's own times (the first len(rows) values, repeated if need be)."""
    from viforsdes_amd import GaussianObservationLikelihood, Hill, Observations, ReactionNetworkSDE
    from viforsdes_amd.examples.sdes import LinearDiagonalSDE, LotkaVolterra, ou_problem
    g = torch.Generator().manual_seed(29)
    jitter = lambda base, rel: torch.tensor(base) * (1.0 + rel * (2.0 * torch.rand(M, len(base), generator=g) - 1.0))
    if name == "ou":
        sde, obs, like, _, _, dt, _, _ = ou_problem()
        out = sde, obs, like, jitter([0.8, 1.0, 0.5], 0.2), obs.values[0].expand(M, 1).clone(), dt, ()
    elif name == "lv":
        obs = Observations(times=torch.tensor([0.0, 10.0, 20.0, 20.0, 40.0]),
                           values=torch.tensor([[71.0, 79.0], [50.0, 390.0], [115.0, 63.0], [110.0, 66.0], [140.0, 95.0]]))
        x0 = obs.values[0].expand(M, 2).clone()
        x0[::4] = torch.rand(len(x0[::4]), 2, generator=g) * 1e-3
        out = LotkaVolterra(), obs, GaussianObservationLikelihood(variance=3600.0), jitter([0.5, 0.0025, 0.3], 0.03), x0, 0.1, (0, 1)
    elif name == "lindiag16":
        S, O = 16, 5
        H = torch.randn(O, S, generator=g) / 4.0
        obs = Observations(times=torch.tensor([0.0, 0.5, 1.0, 2.0]), values=torch.randn(4, O, generator=g) * 0.3)
        th = torch.cat([0.2 + torch.rand(M, S, generator=g), -1.0 + 0.5 * torch.randn(M, S, generator=g)], 1)
        x0 = 0.5 * torch.randn(M, S, generator=g)
        pos = (0, 3, 9, 15)
        x0[:, pos] = x0[:, pos].abs() * 0.02
        out = LinearDiagonalSDE(S), obs, GaussianObservationLikelihood(variance=0.5, obs_matrix=H), th, x0, 0.05, pos
    elif name == "sir":
        sde = ReactionNetworkSDE(**SIR, species=["S", "I"], reactions=["infection", "removal"])
        obs = Observations(times=torch.tensor([0.0, 1.0, 2.0, 3.0, 5.0]),
                           values=torch.tensor([[95.0, 5.0], [93.0, 6.0], [90.5, 6.5], [88.0, 7.5], [83.0, 8.5]]))
        x0 = obs.values[0].expand(M, 2).clone()
        x0[::4, 1] = 1e-3
        out = sde, obs, GaussianObservationLikelihood(variance=64.0), jitter([0.004, 0.25], 0.1), x0, 0.05, (0, 1)
    elif name == "autoreg":
        sde = ReactionNetworkSDE(**AUTOREG_KW, rate_laws={"transcription": Hill("P", K="K", n=2, repression=True)})
        obs = Observations(times=torch.tensor([0.0, 5.0, 10.0, 15.0, 20.0]),
                           values=torch.tensor([[5.0, 20.0], [20.0, 44.0], [18.0, 65.0], [14.5, 71.0], [12.5, 70.0]]))
        out = sde, obs, GaussianObservationLikelihood(variance=100.0), jitter([20.0, 0.5, 0.1, 15.0], 0.1), \
            obs.values[0].expand(M, 2).clone(), 0.1, (0, 1)
    else:
        assert name == "chain6"
        sde = ReactionNetworkSDE(**CHAIN6, species=list("ABCDEF"), reactions=["in", "ab", "bc", "cd", "de", "ef", "out"])
        start = torch.tensor([40.0, 35.0, 30.0, 25.0, 20.0, 15.0])
        obs = Observations(times=torch.tensor([0.0, 0.5, 1.0, 2.0]),
                           values=torch.stack([start, start * 0.97, start * 0.95, start * 0.92]))
        x0 = start.expand(M, 6).clone()
        x0[::4, 5] = 1e-3
        out = sde, obs, GaussianObservationLikelihood(variance=25.0), jitter([20.0, 0.5, 0.6, 0.7, 0.8, 0.9, 1.0], 0.1), x0, 0.05, \
            tuple(range(6))
    if rows is None:
        return out
    sde, obs, like, th, x0, dt, pos = out
    idx = [min(i, obs.values.shape[0] - 1) for i in range(len(rows))]
    obs = Observations(times=torch.tensor(rows, dtype=torch.float64).mul(dt).float(), values=obs.values[idx].clone())
    return sde, obs, like, th, x0, dt, pos
