"""The particle-filter sweep: a pure-Python mirror of the host dispatch of the three filter kernels
(csrc/vsde_filter_kernels.h: pf_kernel, rp_kernel, ar_kernel), the enumerated set of their instantiations, one generated and
seeded case per instantiation, and the float64 scoring both test files share (tests/test_filter_sweep_bounds.py on the CPU,
tests/test_filter_sweep_gpu.py on the device).  Nothing here needs a GPU.

An instantiation is ``(KIND, NS, NR, KIN, NO, CNT, RES)``; ``ALL[op]`` for ``op`` in "filter", "replay", "anchored" lists them
(252, 186, 186: the replay kernels have no count form, their CNT is always False)."""
import math

import numpy as np
import torch

import count_likelihood_reference as cref
import guided_filter_reference as gref
import particle_filter_reference as ref
import reaction_networks as rn
import residual_bridge_reference as rref
from philox_reference import box_muller

_MASK = 0xFFFFFFFF
FLOOR = float(np.float32(1e-6))
OPS = ("filter", "replay", "anchored")
KIND_NAMES = {1: "ornstein_uhlenbeck", 2: "lotka_volterra", 3: "linear_diagonal", 4: "reaction_network"}
PROPOSALS = ("bootstrap", "bridge", "residual_bridge")
PF_MAX_N, PF_MAX_S, PF_MAX_O, GUIDED_MAX_S, GUIDED_MAX_O, CRN_MAX_S, CRN_MAX_R, WAVE = 1024, 16, 16, 4, 4, 8, 16, 64
RESIDUAL_FULL_S = 3

# the call shape of every cell
M, N, D = 3, 64, 2
ROWS = [0, 3, 3, 10, 17]        # an observation at row 0, a shared row, segments that start and end inside a Philox block of four
BIG_M, BIG_ROWS = 2, [0, 3, 10]
PROPAGATION_BOUND = 2e-4        # of the largest magnitude of the segment (tests/test_particle_filter_gpu.py)
ANCESTOR_MARGIN = 1e-5          # of C_{N-1}: the fp32 scalar bound of the scan and the threshold (fewer than 30 roundings)
KEY_MARGIN = 3.0                # a case's key leaves no float64 threshold within KEY_MARGIN * ANCESTOR_MARGIN of a cumulative sum


# ------------------------------------------------------------------------------------------------------------ dispatch mirror
def pf_max_n(kind, S, guided=False, residual=False):
    """csrc/vsde_filter_step.h: pf_max_n."""
    return PF_MAX_N // 2 if (kind == 4 and S > 4) or (guided and S > 3) or (residual and S > RESIDUAL_FULL_S) else PF_MAX_N


def instantiation(op, kind, S, R, kinetic, proposal, O, count):
    """``(KIND, NS, NR, KIN, NO, CNT, RES, max_n)`` of a call of ``op`` ("filter", "replay", "anchored") on a model of built-in
    ``kind`` 1..4 with S state dims (kind 4: R reactions, ``kinetic``: with rate laws), ``proposal`` and O observed dims, ``count``:
    with a count observation term -- or a string, the reason the host refuses the call.  Written from route_check, pf_check /
    anchored_replay's checks, route_dispatch, crn_dispatch and the three host bodies; ``max_n`` is the filter's particle limit."""
    if op not in OPS or proposal not in PROPOSALS:
        return "unknown operation or proposal"
    guided, residual = proposal != "bootstrap", proposal == "residual_bridge"
    if kind == 4:                                                   # route_check: crn_net
        if not 1 <= S <= CRN_MAX_S:
            return f"reaction network: {S} species"
        if not 1 <= R <= CRN_MAX_R:
            return f"reaction network: {R} reactions"
    elif kind not in (1, 2, 3):
        return f"unknown built-in SDE kind {kind}"
    elif (kind == 1 and S != 1) or (kind == 2 and S != 2):          # kind_check
        return "state_dim does not belong to the kind"
    if kinetic and kind != 4:
        return "rate laws belong to a reaction network"
    if guided and not 1 <= S <= GUIDED_MAX_S:                       # pf_check
        return f"guided: state_dim {S}"
    if guided and not 1 <= O <= GUIDED_MAX_O:
        return f"guided: obs_dim {O}"
    if not 1 <= S <= PF_MAX_S:
        return f"state_dim {S}"
    if not 1 <= O <= PF_MAX_O:
        return f"obs_dim {O}"
    if count and (guided or op != "filter"):
        return "the count term belongs to the bootstrap filter"
    NR = {1: 3, 2: 3, 3: 2}.get(kind) or (4 if R <= 4 else 8 if R <= 8 else CRN_MAX_R)      # EmDims<KIND>::P / crn_dispatch
    NO = 0 if not guided else 2 if O <= 2 else 4
    return (kind, S, NR, bool(kinetic), NO, bool(count), residual, pf_max_n(kind, S, guided, residual))


def _routes(diag_max, crn_max):
    """route_dispatch<diag_max, crn_max>: (KIND, NS, NR, KIN)."""
    return ([(1, 1, 3, False), (2, 2, 3, False)] + [(3, s, 2, False) for s in range(1, diag_max + 1)]
            + [(4, s, nr, kin) for s in range(1, crn_max + 1) for nr in (4, 8, 16) for kin in (False, True)])


def _enumerate(with_count):
    boot = [r + (0, cnt, False) for r in _routes(PF_MAX_S, CRN_MAX_S) for cnt in ((False, True) if with_count else (False,))]
    return boot + [r + (no, False, res) for r in _routes(GUIDED_MAX_S, GUIDED_MAX_S) for no in (2, 4) for res in (False, True)]


ALL = {"filter": _enumerate(True), "replay": _enumerate(False), "anchored": _enumerate(False)}


def refusal_classes():
    """Every distinct (kind, S, proposal) of the filter's dispatch, with a (R, kinetic) of the class: the cells of the N-limit test."""
    out = []
    for proposal in PROPOSALS:
        for kind, S, _, _ in _routes(*((PF_MAX_S, CRN_MAX_S) if proposal == "bootstrap" else (GUIDED_MAX_S, GUIDED_MAX_S))):
            if (kind, S, proposal) not in out:
                out.append((kind, S, proposal))
    return out


# ------------------------------------------------------------------------------------------------------------ model generator
class Case:
    """One generated call: the model (``sde``, ``kind``, ``theta [M, P]``, ``x0 [M, S]``, ``dt``, ``pos``), the observations
    (``rows``, ``values [K, O]``, ``H`` or None, ``like``; ``variance`` for a Gaussian term), ``proposal``, ``key`` (two words),
    ``N`` and ``elem``, the instantiation it is generated for.  All tensors fp32 on the CPU."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def name(self):
        k, s, nr, kin, no, cnt, res = self.elem
        tag = f"k{k}-S{s}" + (f"-R{nr}" + ("k" if kin else "") if k == 4 else "")
        tag += "-count" if cnt else f"-{'res' if res else 'bridge'}{no}" if no else ""
        return tag + ("" if self.N == N else f"-N{self.N}")

    def call(self, op):
        """The arguments of ``instantiation`` for this case's call of ``op``."""
        return (op, self.elem[0], self.sde.state_dim, getattr(self.sde, "num_reactions", 0), self.elem[3], self.proposal,
                self.values.shape[1], self.count is not None and op == "filter")


NAMED = {(3, 8, False): (rn.NET3, [0.02, 0.3, 2.0, 2.0, 0.2], [8.0, 8.0, 6.0]),
         (4, 8, False): (rn.NET4, [5.0, 0.05, 0.01, 0.5, 0.3, 0.02], [12.0, 8.0, 6.0, 3.0]),
         (8, 16, False): (rn.CHAIN8, [4.0, 1.0, 0.8, 1.2, 1.0, 0.9, 1.1, 1.0, 0.7], [5.0, 4.0, 3.0, 3.0, 3.0, 3.0, 3.0, 3.0]),
         (3, 8, True): (rn.REPRESS3, [6.0, 4.0, 0.4, 5.0], [5.0, 3.0, 10.0]),
         (8, 16, True): (rn.KINETIC_CHAIN8, [3.0, 4.0, 0.2, 2.0, 3.0], [3.0, 3.0, 3.0, 3.0, 3.0, 3.0, 3.0, 3.0])}


def _model(elem, g):
    """(sde, base theta [P], start [S], dt, positive dims) of an instantiation; the named networks of tests/reaction_networks.py
    serve the Gaussian bootstrap instantiation of their cell."""
    from viforsdes_amd import ReactionNetworkSDE
    from viforsdes_amd.examples.sdes import LinearDiagonalSDE, LotkaVolterra, OrnsteinUhlenbeck
    kind, S, NR, kin, NO, cnt, res = elem
    if kind == 1:
        return OrnsteinUhlenbeck(), [0.8, 1.0, 0.5], [2.0], 0.05, ()
    if kind == 2:
        return LotkaVolterra(), [0.5, 0.0025, 0.3], [71.0, 79.0], 0.1, (0, 1)
    if kind == 3:
        theta = torch.cat([0.2 + torch.rand(S, generator=g), -1.0 + 0.5 * torch.randn(S, generator=g)])
        pos = tuple(range(0, S, 3))
        if cnt:        # rates must stay positive: every dim starts at 2..3
            return LinearDiagonalSDE(S), theta.tolist(), (2.0 + torch.rand(S, generator=g)).tolist(), 0.05, pos
        start = 0.5 * torch.randn(S, generator=g)
        start[list(pos)] = 0.5 + start[list(pos)].abs()
        return LinearDiagonalSDE(S), theta.tolist(), start.tolist(), 0.05, pos
    named = NAMED.get((S, NR, kin)) if NO == 0 and not cnt else None
    kw, theta, start = named if named is not None else rn.sweep_network(S, NR, kin)
    return ReactionNetworkSDE(**kw), theta, start, 0.05, tuple(range(S))


def _key_words(index, salt, big):
    return ((0x9E3779B9 ^ (index * 2654435761)) & _MASK, (0x7F4A7C15 + 7919 * salt + (1 << 20) * int(big)) & _MASK)


def _build(elem, index, salt=0, big=False):
    from viforsdes_amd import (GaussianObservationLikelihood, NegativeBinomialObservationLikelihood, Observations,
                               PoissonObservationLikelihood)
    kind, S, NR, kin, NO, cnt, res = elem
    g = torch.Generator().manual_seed(1000 + index)
    sde, base, start, dt, pos = _model(elem, g)
    base, start = torch.tensor(base), torch.tensor(start)
    m, rows = (BIG_M, BIG_ROWS) if big else (M, ROWS)
    proposal = "residual_bridge" if res else "bridge" if NO else "bootstrap"
    # the observed dims: guided NO = 2: O = 2 (O = 1 for half of the S = 1 cells), NO = 4: O = 4; bootstrap: 1..4 through a dense H,
    # or every dim; the count cells alternate with and without an obs_matrix
    alt = index % 2 == 1
    if NO:
        O = 4 if NO == 4 else 1 if (S == 1 and alt) else 2
        dense = O != S or alt
    elif cnt:
        O, dense = (S, False) if (index // 4) % 2 == 0 else (1 + S % 4, True)
    else:
        O, dense = (S, False) if kind != 3 and alt else (1 + (S + index) % 4, True)
    H = None
    if dense:
        H = 0.2 + 0.8 * torch.rand(O, S, generator=g) if kind != 3 or cnt else torch.randn(O, S, generator=g) / 2.0
    if kind == 3:
        theta = base[None, :] + torch.cat([0.1 * torch.rand(m, S, generator=g), 0.2 * torch.randn(m, S, generator=g)], 1)
    else:
        theta = base[None, :] * (1.0 + 0.1 * (2.0 * torch.rand(m, len(base), generator=g) - 1.0))
    # the spread of the particles over the longest gap of the rows, and from it the observation noise: O times the largest predicted
    # variance, so that the weights of O dims together keep about e^-1 of the particles
    gap = max(b - a for a, b in zip(rows[:-1], rows[1:]))
    L = sde.diffusion(start.double()[None], base.double()[None])[0]
    spread = gap * dt * (L @ L.T).diagonal()
    Hd = torch.eye(S, dtype=torch.float64) if H is None else H.double()
    pred_var = (Hd * Hd) @ spread
    variance = float(O * pred_var.max())
    if kind == 4 and S == 1 and NO:
        variance *= 20.0      # one observed species: a sharper bridge pulls every particle off the floor before the observation's row
    x0 = start.expand(m, S).clone()
    if pos:
        x0[-1, list(pos)] = 1e-3 * start[list(pos)]          # the last filter: every positive dim near the 1e-6 floor
    count = None
    clean = gref._observations(sde, base, start, dt, pos, H, 0.0 if cnt else variance, rows, seed=7 + index)
    values = clean.values
    if cnt:
        count = "negative_binomial" if (index // 2) % 2 else "poisson"
        scale = float(((Hd @ start.double()).mean() / (O * pred_var.mean())).clamp(min=0.05))
        values = torch.round((scale * values).clamp(min=0.0))
        like = PoissonObservationLikelihood(scale=scale, obs_matrix=H) if count == "poisson" else \
            NegativeBinomialObservationLikelihood(scale=scale, obs_matrix=H, dispersion=10.0)
        variance = None
    else:
        like = GaussianObservationLikelihood(variance=variance, obs_matrix=H)
    return Case(elem=elem, index=index, sde=sde, kind=KIND_NAMES[kind], theta=theta.float(), x0=x0.float(), dt=dt, pos=pos, rows=rows,
                values=values.float(), H=H, like=like, variance=variance, count=count, proposal=proposal, N=N if not big else
                pf_max_n(kind, S, NO > 0, res), M=m, key=_key_words(index, salt, big),
                obs=Observations(times=torch.tensor(rows, dtype=torch.float64).mul(dt).float(), values=values.float()))


# per case (in the order of ALL["filter"]) the key salt ``find_salts`` found: the first for which the float64 filter of the case
# meets the reference conditions of tests/test_filter_sweep_bounds.py (ESS, floor, and no resampling threshold within KEY_MARGIN
# ANCESTOR_MARGIN C_{N-1} of a cumulative sum).  Conditions on the float64 reference alone: no kernel output enters
SALTS = (0, 5, 4, 1, 65, 1, 20, 14, 0, 7, 68, 0, 14, 48, 14, 16, 3, 6, 74, 3, 3, 0, 45, 0, 12, 1, 20, 27, 6, 0, 59, 0, 23, 9, 26,
         2, 12, 0, 6, 1, 4, 0, 7, 9, 40, 11, 9, 11, 3, 11, 19, 26, 6, 2, 8, 9, 94, 11, 4, 24, 13, 4, 17, 2, 25, 4, 34, 3, 40, 10,
         13, 5, 0, 3, 0, 10, 12, 0, 3, 3, 17, 4, 0, 22, 4, 11, 22, 0, 3, 6, 9, 2, 4, 8, 8, 15, 6, 11, 18, 2, 0, 0, 0, 0, 11, 13,
         42, 3, 1, 3, 1, 1, 4, 4, 7, 5, 2, 0, 0, 1, 7, 22, 8, 8, 1, 3, 0, 11, 7, 18, 16, 3, 3, 19, 18, 8, 2, 5, 3, 12, 27, 10, 14,
         20, 6, 1, 33, 38, 26, 55, 2, 1, 11, 1, 6, 33, 9, 11, 0, 6, 6, 35, 1, 7, 5, 11, 8, 2, 6, 0, 7, 8, 6, 4, 1, 0, 10, 5, 1,
         11, 11, 33, 9, 22, 28, 5, 19, 1, 7, 20, 47, 31, 22, 0, 19, 2, 9, 15, 10, 7, 10, 10, 4, 2, 8, 2, 27, 13, 7, 11, 1, 23, 0,
         10, 14, 6, 0, 3, 5, 0, 0, 1, 7, 2, 26, 58, 4, 6, 0, 1, 9, 13, 2, 6, 22, 14, 23, 20, 5, 7, 11, 6, 32, 0, 12, 18, 4, 3, 10,
         10, 1, 17)


def cases():
    """The 252 cases, one per element of ALL["filter"], in its order."""
    return [_build(elem, i, SALTS[i] if i < len(SALTS) else 0) for i, elem in enumerate(ALL["filter"])]


def large_cells():
    """The instantiations run at N = max_n as well (M = 2, K = 3): kind 3 bootstrap at S = 14, 15, 16, Gaussian and count (N = 1024:
    the six functions whose dynamic LDS passes 64 KiB); kind 4 bootstrap at NR = 16, both KIN forms, S = 4 (1024) and 5..8 (512);
    guided and residual at S = 3 (1024) and S = 4 (512), kind 3 and kind 4 at NR = 16 in its kinetic form (NO = 4)."""
    cells = [(3, s, 2, False, 0, cnt, False) for s in (14, 15, 16) for cnt in (False, True)]
    cells += [(4, s, 16, kin, 0, False, False) for s in (4, 5, 6, 7, 8) for kin in (False, True)]
    cells += [(k, s, nr, kin, 4, False, res) for s in (3, 4) for res in (False, True) for k, nr, kin in ((3, 2, False), (4, 16, True))]
    return cells


def large_cases():
    return [_build(elem, ALL["filter"].index(elem), 0, big=True) for elem in large_cells()]


# ---------------------------------------------------------------------------------------------------------- float64 torch route
def key_tensor(key):
    return torch.from_numpy(np.array(key, dtype=np.uint32).view(np.int32).copy())


def torch_filter(case, dtype=torch.float64):
    """The case through the torch route (the specification) on the CPU in ``dtype``, particles kept."""
    from viforsdes_amd import particle_filter
    return particle_filter(case.sde, case.obs, case.like, case.theta.to(dtype), case.dt, n_particles=case.N,
                           initial_state=case.x0.to(dtype), positive_dims=case.pos, return_particles=True, key=key_tensor(case.key),
                           proposal=case.proposal)


def undecidable(w, u):
    """Which entries j of one resampling (weights w [N] >= 0 in float64, uniform u) float64 cannot decide for fp32: the threshold
    (j + u) / N C_{N-1} lies within ``margin`` C_{N-1} of a cumulative sum.  Returns the distance of every threshold to its nearest
    cumulative sum, as a fraction of C_{N-1}."""
    w = np.asarray(w, dtype=np.float64)
    n = w.size
    C = np.cumsum(w)
    tau = (np.arange(n) + float(u)) / n * C[-1]
    i = np.clip(np.searchsorted(C, tau), 1, n - 1)
    return np.minimum(np.abs(C[i] - tau), np.abs(C[i - 1] - tau)) / C[-1]


def log_weights64(case, k, x, lr=None):
    """float64 lw [..., N] of particles x [..., N, S] at observation k (plus the guided log-ratio ``lr``)."""
    y = case.values[k].double().numpy()
    H = None if case.H is None else case.H.double().numpy()
    if case.count is None:
        lw = ref.gaussian_log_weights(y, x, case.variance, H)
    else:
        lw = cref.count_log_weights(y, x, None if case.count == "poisson" else case.like.dispersion, case.like.scale, H)
    return lw if lr is None else np.where(np.isnan(lw + lr), -np.inf, lw + lr)


# ------------------------------------------------------------------------------------------------------- float64 numpy segments
def path_noise(paths, keys, T, S):
    """The stream's normals [B, T, S] (float64) of path indices ``paths [B]`` under ``keys``: one (k0, k1) or [B, 2] words."""
    keys = np.asarray(keys, dtype=np.uint64) & np.uint64(_MASK)
    nblk = (T + 3) // 4
    blk, i, b = np.meshgrid(np.arange(nblk), np.arange(S), np.asarray(paths, dtype=np.int64), indexing="ij")
    k0, k1 = (keys[0], keys[1]) if keys.ndim == 1 else (keys[:, 0][None, None, :], keys[:, 1][None, None, :])
    w = _philox(blk, i, b, k0, k1)
    z = np.stack([*box_muller(w[0], w[1]), *box_muller(w[2], w[3])], axis=1)
    return np.ascontiguousarray(z.reshape(nblk * 4, S, -1)[:T].transpose(2, 0, 1))


def _philox(c0, c1, c2, k0, k1):
    """philox4x32_10({c0, c1, c2, 0}, key) with a key per element (tests/philox_reference.py takes one key per call)."""
    m0, m1, w0, w1, mask = (np.uint64(v) for v in (0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, _MASK))
    c = [np.asarray(v, dtype=np.uint64) & mask for v in np.broadcast_arrays(c0, c1, c2, np.zeros_like(c0))]
    k0, k1 = np.asarray(k0, dtype=np.uint64), np.asarray(k1, dtype=np.uint64)
    for _ in range(10):
        p0, p1 = m0 * c[0], m1 * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & mask, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & mask]
        k0, k1 = (k0 + w0) & mask, (k1 + w1) & mask
    return [v.astype(np.uint32) for v in c]


def segment(case, start, theta, z, k, dtype=np.float64):
    """Every state [B, n, S] and the summed log-ratio [B] (zeros for the bootstrap step) of the n = z.shape[1] steps of the case's
    proposal from ``start [B, S]`` towards observation k: the bootstrap steps are ``euler_maruyama`` itself; the guided ones
    restate tests/guided_filter_reference.py: guided_segment / tests/residual_bridge_reference.py: residual_segment with the
    states kept (``test_filter_sweep_bounds.py`` holds the restatement to those two, end state and log-ratio)."""
    B, n, S = z.shape
    if case.proposal == "bootstrap":
        from viforsdes_amd.core.euler_maruyama import euler_maruyama
        tdt = torch.float64 if dtype == np.float64 else torch.float32
        out = euler_maruyama(case.sde, torch.as_tensor(start).to(tdt), torch.as_tensor(theta).to(tdt), n * case.dt, case.dt, case.pos,
                             noise=torch.as_tensor(z).to(tdt))
        return out[:, 1:].numpy().astype(dtype), np.zeros(B, dtype=dtype)
    coef = gref.sde_coefficients(case.sde, dtype)
    x = np.asarray(start, dtype=dtype).copy()
    theta, z, y = np.asarray(theta, dtype=dtype), np.asarray(z, dtype=dtype), case.values[k].numpy().astype(dtype)
    Hm = np.eye(S, dtype=dtype) if case.H is None else case.H.numpy().astype(dtype)
    dt, var, eye_o, eye_s = dtype(case.dt), dtype(case.variance), np.eye(Hm.shape[0], dtype=dtype), np.eye(S, dtype=dtype)
    lr, out = np.zeros(B, dtype=dtype), np.empty((B, n, S), dtype=dtype)
    residual = case.proposal == "residual_bridge"
    with np.errstate(all="ignore"):
        if residual:
            eta, f_eta, _ = rref.companion_path(coef, x, theta, n, dt, case.pos, dtype)
        for step in range(n):
            left = dtype(n - step)
            f, Lm = coef(x, theta)
            A = np.sqrt(dt) * np.einsum("ok,bki->boi", Hm, Lm)
            psi = left * np.einsum("boi,bqi->boq", A, A) + var * eye_o
            ahead = eta[n] + (x - eta[step]) + left * dt * (f - f_eta[step]) if residual else x + left * dt * f
            e = y[None, :] - ahead @ Hm.T
            sol = np.linalg.solve(psi, np.concatenate([A, e[..., None]], axis=-1)).astype(dtype)
            mvec = np.einsum("boi,bo->bi", A, sol[..., -1])
            C = eye_s[None] - np.einsum("boi,bok->bik", A, sol[..., :-1])
            Mf = gref.floored_cholesky(C, gref.PIVOT_FLOOR, dtype)
            eps = mvec + np.einsum("bik,bk->bi", Mf, z[:, step])
            lr = lr - dtype(0.5) * (eps * eps).sum(axis=-1) + dtype(0.5) * (z[:, step] ** 2).sum(axis=-1) \
                + np.log(np.diagonal(Mf, axis1=1, axis2=2)).sum(axis=-1)
            x = x + f * dt + np.sqrt(dt) * np.einsum("bik,bk->bi", Lm, eps)
            for i in case.pos:
                x[:, i] = np.where(x[:, i] < dtype(FLOOR), dtype(FLOOR), x[:, i])
            x, lr = x.astype(dtype), lr.astype(dtype)
            out[:, step] = x
    return out, lr


def gauss32(y, x, variance, H):
    """The Gaussian observation term in fp32 arithmetic (the E32 run of the guided log-weights)."""
    x = x.astype(np.float32)
    pred = x if H is None else x @ H.astype(np.float32).T
    r = y.astype(np.float32) - pred
    return (np.float32(-0.5) * r * r / np.float32(variance) - np.float32(0.5 * math.log(2.0 * math.pi * variance))).sum(axis=-1)


def last_slots(case, salt=0):
    """last_slot [M, D] int32 drawn on the host (seeded): any slot is a valid final draw for the replay kernels."""
    g = np.random.default_rng(50000 + case.index + salt)
    return g.integers(0, case.N, size=(case.M, D)).astype(np.int32)


def find_salts(indices=None, tries=400):
    """The SALTS table: per case the first key salt whose float64 filter meets the reference conditions (see SALTS)."""
    out = []
    for i, elem in enumerate(ALL["filter"]):
        if indices is not None and i not in indices:
            continue
        for salt in range(tries):
            if reference_conditions(_build(elem, i, salt))["ok"]:
                break
        else:
            salt = -1
        out.append(salt)
    return out


def reference_conditions(case, res=None):
    """The conditions on the float64 reference alone, measured: smallest particle ESS of the first M - 1 filters, whether the last
    filter hit the floor, the undecidable entries at ANCESTOR_MARGIN, and the smallest threshold distance; ``ok``: ESS > N / 20,
    floor hit where there are positive dims, and no threshold within KEY_MARGIN ANCESTOR_MARGIN."""
    res = torch_filter(case) if res is None else res
    parts = res.particles.numpy()
    lw = res.log_weights.numpy()
    u = ref.resampling_uniforms(case.M, len(case.rows), case.key)
    ess, near, n_und = float("inf"), float("inf"), 0
    for m in range(case.M):
        for k in range(len(case.rows)):
            w = np.exp(lw[m, k] - lw[m, k].max())
            if m < case.M - 1:
                ess = min(ess, float(w.sum() ** 2 / (w * w).sum()))
            d = undecidable(w, u[m, k])
            near, n_und = min(near, float(d.min())), n_und + int((d <= ANCESTOR_MARGIN).sum())
    floor_hit = bool(case.pos) and bool((parts[-1, 1:][..., list(case.pos)] == 1e-6).any())
    ok = ess > case.N / 20 and (floor_hit or not case.pos) and near > KEY_MARGIN * ANCESTOR_MARGIN and bool(np.isfinite(parts).all())
    return dict(ok=ok, ess=ess, floor_hit=floor_hit, undecidable=n_und, near=near, entries=lw.size)
