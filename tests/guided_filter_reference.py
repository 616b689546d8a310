"""numpy helpers for the guided (bridge) particle-filter tests: an independent restatement of one guided segment (the modified
diffusion bridge of viforsdes_amd/inference/particle_filter.py, written with psi^-1 from a general solver, not with the
specification's triangular solves), a Kalman filter, and the test cases both test files share.  Every function takes a ``dtype``:
float64 is the reference, float32 measures what fp32 arithmetic alone costs on the same inputs."""
import numpy as np
import torch

PIVOT_FLOOR = 1e-6
STATE_FLOOR = float(np.float32(1e-6))
ROWS = [0, 1, 3, 3, 8, 20]   # n = 1, a shared row, a segment inside one Philox block of four, segments that cross blocks
# Lotka-Volterra at its own observation variance 1.0: over the 12 steps 8 -> 20 the float64 bridge filter's ESS falls to 2.8 of 64 and
# 19 of 1024 particles in some of the 64 filters (below the N / 20 the ancestor test needs); over 6 steps it stays above 27 and 600
# (weights over a long guided segment of a nonlinear model are heavy-tailed).  Every other case keeps the 12-step segment; the chain
# network (bimolecular step) needs an observation variance of 4.0 for that: at 1.0 one filter of 64 falls to 27 of 512 now and then
LV_ROWS = [0, 1, 3, 3, 8, 14]


def rows_of(name):
    return LV_ROWS if name in ("lv", "lv_prey") else ROWS


SIR = dict(reactants=[[1, 1], [0, 1]], products=[[0, 2], [0, 0]])
AUTOREG_KW = dict(reactants=[[0, 0], [1, 0], [1, 0], [0, 1]], products=[[1, 0], [1, 1], [0, 0], [0, 0]], species=["M", "P"],
                  reactions=["transcription", "translation", "mRNA decay", "protein decay"],
                  rate_constants=["k_tx", "k_tl", 0.1, "d_P"])
# a chain 0 -> A -> B -> C -> D -> 0 with a dimerisation-like step B + C -> D
CHAIN4 = dict(reactants=[[0, 0, 0, 0], [1, 0, 0, 0], [0, 1, 0, 0], [0, 1, 1, 0], [0, 0, 0, 1]],
              products=[[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1], [0, 0, 0, 0]])


def sde_coefficients(sde, dtype=np.float64):
    """``coef(x [B, S], theta [B, P]) -> (f [B, S], L [B, S, S])`` of an SDE's own torch drift / diffusion, evaluated in ``dtype``."""
    tdt = torch.float64 if dtype == np.float64 else torch.float32

    def coef(x, theta):
        xt, tt = torch.from_numpy(np.ascontiguousarray(x)).to(tdt), torch.from_numpy(np.ascontiguousarray(theta)).to(tdt)
        return sde.drift(xt, tt).numpy().astype(dtype), sde.diffusion(xt, tt).numpy().astype(dtype)
    return coef


def floored_cholesky(c, floor, dtype=np.float64):
    """Lower Cholesky factor of c [B, n, n], every pivot floored at ``floor`` (None: not floored) before its square root."""
    B, n, _ = c.shape
    out = np.zeros((B, n, n), dtype=dtype)
    for j in range(n):
        s = c[:, j, j] - (out[:, j, :j] ** 2).sum(axis=-1)
        if floor is not None:
            s = np.where(s < dtype(floor), dtype(floor), s)
        out[:, j, j] = np.sqrt(s)
        for i in range(j + 1, n):
            out[:, i, j] = (c[:, i, j] - (out[:, i, :j] * out[:, j, :j]).sum(axis=-1)) / out[:, j, j]
    return out


def guided_segment(coef, start, theta, z, y, H, variance, dt, positive_dims=(), dtype=np.float64):
    """The states and log-ratios after the ``n = z.shape[1]`` guided Euler steps towards the observation ``y [O]`` that lies n grid
    steps ahead: start [B, S], theta [B, P], z [B, n, S] (the steps' normals) -> (x [B, S], lr [B]), all arithmetic in ``dtype``."""
    x = np.asarray(start, dtype=dtype).copy()
    theta, z, y = np.asarray(theta, dtype=dtype), np.asarray(z, dtype=dtype), np.asarray(y, dtype=dtype)
    B, S = x.shape
    Hm = np.eye(S, dtype=dtype) if H is None else np.asarray(H, dtype=dtype)
    O = Hm.shape[0]
    dt, var, eye_o, eye_s = dtype(dt), dtype(variance), np.eye(O, dtype=dtype), np.eye(S, dtype=dtype)
    lr = np.zeros(B, dtype=dtype)
    n = z.shape[1]
    with np.errstate(all="ignore"):
        for step in range(n):
            left = dtype(n - step)
            f, L = coef(x, theta)
            A = np.sqrt(dt) * np.einsum("ok,bki->boi", Hm, L)
            psi = left * np.einsum("boi,bqi->boq", A, A) + var * eye_o
            e = y[None, :] - (x + left * dt * f) @ Hm.T
            sol = np.linalg.solve(psi, np.concatenate([A, e[..., None]], axis=-1)).astype(dtype)   # psi^-1 [A | e]
            m = np.einsum("boi,bo->bi", A, sol[..., -1])
            C = eye_s[None] - np.einsum("boi,bok->bik", A, sol[..., :-1])
            Mf = floored_cholesky(C, PIVOT_FLOOR, dtype)
            zs = z[:, step]
            eps = m + np.einsum("bik,bk->bi", Mf, zs)
            lr = lr - dtype(0.5) * (eps * eps).sum(axis=-1) + dtype(0.5) * (zs * zs).sum(axis=-1) \
                + np.log(np.diagonal(Mf, axis1=1, axis2=2)).sum(axis=-1)
            x = x + f * dt + np.sqrt(dt) * np.einsum("bik,bk->bi", L, eps)
            for i in positive_dims:
                x[:, i] = np.where(x[:, i] < dtype(STATE_FLOOR), dtype(STATE_FLOOR), x[:, i])
            x, lr = x.astype(dtype), lr.astype(dtype)
    return x, lr


def gaussian_log_density(y, mean, cov):
    """log N(y; mean [B, O], cov [B, O, O]) in float64."""
    r = np.asarray(y, dtype=np.float64)[None, :] - mean
    sol = np.linalg.solve(cov, r[..., None])[..., 0]
    return -0.5 * ((r * sol).sum(axis=-1) + np.linalg.slogdet(2.0 * np.pi * cov)[1])


def kalman_log_likelihood(A, c, Q, H, R, x0, rows, ys, dtype=np.float64):
    """log p(y_0 .. y_{K-1} | x at row 0 = x0) of x_{t+1} = A x_t + c + N(0, Q), y_k = H x_{rows[k]} + N(0, R) in ``dtype``."""
    A, c, Q, H, R = (np.asarray(v, dtype=dtype) for v in (A, c, Q, H, R))
    m, P = np.asarray(x0, dtype=dtype).copy(), np.zeros_like(Q)
    t, ll = 0, dtype(0.0)
    for row, y in zip(rows, np.asarray(ys, dtype=dtype)):
        while t < row:
            m, P = A @ m + c, A @ P @ A.T + Q
            t += 1
        r, Sy = y - H @ m, H @ P @ H.T + R
        ll += dtype(-0.5) * (r @ np.linalg.solve(Sy, r) + np.linalg.slogdet(dtype(2.0 * np.pi) * Sy)[1])
        G = P @ H.T @ np.linalg.inv(Sy)
        m, P = m + G @ r, P - G @ H @ P
    return float(ll)


def ou_kalman(theta, dt, variance, x0, rows, ys, dtype=np.float64):
    """Exact log-likelihood of the Euler-Maruyama-discretised Ornstein-Uhlenbeck model, theta = (kappa, mu, sigma)."""
    kappa, mu, sigma = (float(v) for v in theta)
    return kalman_log_likelihood([[1.0 - kappa * dt]], [kappa * mu * dt], [[sigma * sigma * dt]], [[1.0]], [[variance]], x0, rows, ys,
                                 dtype)


def autoreg():
    from viforsdes_amd import Hill, ReactionNetworkSDE
    return ReactionNetworkSDE(**AUTOREG_KW, rate_laws={"transcription": Hill("P", K="K", n=2, repression=True)})


def _observations(sde, theta, x0, dt, pos, H, variance, rows, seed):
    """Observations at ``rows`` of one float64 Euler-Maruyama path of the model from x0 (torch generator ``seed``), with noise."""
    from viforsdes_amd import Observations
    g = torch.Generator().manual_seed(seed)
    x, th = x0.double()[None, :].clone(), theta.double()[None, :]
    values, t = [], 0
    for row in rows:
        while t < row:
            z = torch.randn(1, x.shape[1], generator=g, dtype=torch.float64)
            x = x + sde.drift(x, th) * dt + torch.einsum("bij,bj->bi", sde.diffusion(x, th), z) * dt ** 0.5
            for i in pos:
                x[:, i] = x[:, i].clamp(min=1e-6)
            t += 1
        pred = x[0] if H is None else H.double() @ x[0]
        values.append(pred + variance ** 0.5 * torch.randn(pred.shape, generator=g, dtype=torch.float64))
    return Observations(times=torch.tensor(rows, dtype=torch.float64).mul(dt).float(), values=torch.stack(values).float())


INTERIOR = {"lv": [71.0, 79.0], "lv_prey": [71.0, 79.0], "chain4": [30.0, 40.0, 35.0, 25.0], "chain4_full": [30.0, 40.0, 35.0, 25.0],
            "lindiag3": [2.0, 0.5, -0.4]}


def case(name, M=64, rows=None, interior=False):
    """(sde, observations, likelihood, theta [M, P], x0 [M, S], dt, positive dims) on the CPU, fp32.  Every 4th filter of the
    positive-state cases starts with one species (the chains: two) AT the 1e-6 floor.  The observations are shared by the filters of
    a case and sharp (Lotka-Volterra: variance 1.0 on a prey population of 70-160), so a start that is many standard deviations away
    from them starves any filter, guided or not: the species that start at the floor are ones the data path itself keeps near it (the
    Lotka-Volterra predators start at 0.5 and die out), which is also what makes the clamp bind in every filter.
    ``interior``: every filter starts well inside the positive orthant instead (``INTERIOR``), so that no clamp binds."""
    from viforsdes_amd import GaussianObservationLikelihood, ReactionNetworkSDE
    from viforsdes_amd.examples.sdes import LinearDiagonalSDE, LotkaVolterra, OrnsteinUhlenbeck
    rows = rows_of(name) if rows is None else rows
    g = torch.Generator().manual_seed(31)
    jitter = lambda base, rel: torch.tensor(base) * (1.0 + rel * (2.0 * torch.rand(M, len(base), generator=g) - 1.0))
    H, pos, low = None, (0, 1), None
    if name == "ou":
        sde, base, rel, start, dt, var, pos = OrnsteinUhlenbeck(), [0.8, 1.0, 0.5], 0.2, [2.0], 0.05, 0.01, ()
    elif name == "lv":
        sde, base, rel, start, dt, var = LotkaVolterra(), [0.5, 0.0025, 0.3], 0.03, [71.0, 0.5], 0.1, 1.0
        low = lambda n: torch.tensor([[71.0, 1e-6]]).expand(n, 2)
    elif name == "lv_prey":
        sde, base, rel, start, dt, var = LotkaVolterra(), [0.5, 0.0025, 0.3], 0.03, [71.0, 0.5], 0.1, 1.0
        H = torch.tensor([[1.0, 0.0]])
        low = lambda n: torch.tensor([[71.0, 1e-6]]).expand(n, 2)
    elif name == "sir":
        sde = ReactionNetworkSDE(**SIR, species=["S", "I"], reactions=["infection", "removal"])
        base, rel, start, dt, var = [0.004, 0.25], 0.1, [95.0, 5.0], 0.05, 1.0
        low = lambda n: torch.tensor([[95.0, 1e-6]]).expand(n, 2)
    elif name in ("chain4", "chain4_full"):      # observed through a [2, 4] H, or every species observed (H absent, O = 4)
        sde = ReactionNetworkSDE(**CHAIN4, species=["A", "B", "C", "D"], reactions=["in", "ab", "bc", "bcd", "out"])
        base, rel, start, dt, var, pos = [30.0, 0.8, 0.5, 0.01, 0.4], 0.03, [30.0, 40.0, 0.5, 0.3], 0.05, 4.0, (0, 1, 2, 3)
        H = torch.tensor([[1.0, 0.0, 1.0, 0.0], [0.0, 1.0, 0.0, 2.0]]) if name == "chain4" else None
        low = lambda n: torch.tensor([[30.0, 40.0, 1e-6, 1e-6]]).expand(n, 4)
    elif name == "lindiag3":                     # three independent linear SDEs coupled by a dense [4, 3] H (O = 4 > S)
        sde, start, dt, var, pos = LinearDiagonalSDE(3), [0.1, 0.5, -0.4], 0.05, 0.04, (0,)
        H = torch.tensor([[1.0, 0.5, -0.3], [-0.4, 1.2, 0.6], [0.7, -0.8, 1.0], [0.3, 0.9, 0.5]])
        base, rel = [0.7, 0.4, 1.1, -2.5, -0.5, -1.5], 0.2
        low = lambda n: torch.tensor([[1e-6, 0.5, -0.4]]).expand(n, 3)
    else:
        assert name == "autoreg"
        sde, base, rel, start, dt, var = autoreg(), [20.0, 0.5, 0.1, 15.0], 0.1, [0.5, 20.0], 0.1, 2.0
        low = lambda n: torch.tensor([[1e-6, 20.0]]).expand(n, 2)
    if interior:
        start, low = INTERIOR.get(name, start), None
    theta, start = jitter(base, rel), torch.tensor(start)
    obs = _observations(sde, torch.tensor(base), start, dt, pos, H, var, rows, seed=7)
    x0 = start.expand(M, len(start)).clone()
    if low is not None:
        x0[::4] = low(len(x0[::4]))
    return sde, obs, GaussianObservationLikelihood(variance=var, obs_matrix=H), theta, x0, dt, pos
