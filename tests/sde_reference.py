"""float64 references, per-element magnitudes, bounds and test inputs of the SDE-side kernels: the ELBO path terms and tail
(csrc/vsde_elbo.hip) and the Euler-Maruyama simulator of the built-in kinds 1..4 (csrc/vsde_sde.hip).  Plain functions on numpy
arrays: tests/test_sde_ops_gpu.py compares the kernels with them, tests/test_sde_bounds.py checks on the CPU that the bounds hold
for a correct float32 evaluation and reject an emulation of the kernels' arithmetic with a defect injected.

Values.  Independent of the C oracle: ``path_reference`` is torch.distributions.MultivariateNormal(scale_tril=...) + logsigmoid
in float64 with autograd for the six gradients; ``tail_reference`` is torch.distributions Normal / LogNormal (Poisson /
NegativeBinomial for the count entry points, their values pinned to tests/count_likelihood_reference.py) in float64 with
autograd; the simulator is scored teacher-forced (``em_forward_check``: x_{t+1} from the kernel's OWN x_t, per (b, t), no
accumulated drift) and its gradient by the float64 reverse recursion on the kernel's own trajectory (``em_adjoint``); kind 4
steps with ReactionNetworkSDE.drift / .diffusion in float64 torch.

Magnitudes.  Every written-out formula (``path_formulas``, ``tail_formulas``, ``em_step``, ``em_adjoint``) is evaluated on ``VM``
pairs (value, magnitude): the magnitude of a leaf is its absolute value, of a + b and a - b the SUM of the magnitudes, of a b
the product, of a / b magnitude(a) magnitude(b) / b^2, of log / exp / sigmoid the absolute value of the result, of sqrt(a)
the larger of sqrt(magnitude) and magnitude / (2 sqrt(a)).  So the magnitude of the residual is |y| + |m0| + |d| dt, the
substitutions run with |A|, a path term is sum_t (quad / 2 + |log d_ii| + S log(2 pi) / 2), g_z[tau] carries |v_tau| + |v_tau-1| + |jac term|, and a batch
mean or g_post_* the sum over b of the terms' magnitudes.  tests/test_sde_bounds.py pins the values of these formulas to the
autograd references to 1e-12 of the magnitude.

Bounds.  |got - ref| <= c 2^-24 magnitude per element, never relative to a tensor's maximum; where the magnitude is zero (the
strict upper triangle of g_chol / g_diffusion) the kernel's value must be exactly zero.  One c per family, 4 x the worst ratio
|f32 - f64| / (2^-24 magnitude) of a correct float32 evaluation (the C oracle's f32 instantiation for the path terms, the
observation / prior / posterior sums and the simulator; float32 torch for the tail's gradients, the count likelihoods and
kind 4, which the oracle does not have), measured on the CPU over every case of tests/test_sde_ops_gpu.py; the factor 4 covers
__logf / __expf / fast_rcp and the kernels' summation trees:

    family                       worst CPU ratio   c       worst ratio on an MI355X
    path forward                 66.71             270     5.61
    path backward                 9.48             39      9.47
    tail (Gaussian and count)     2.83             12      2.88
    EM step (kinds 1..4)          2.53             10.5    2.62
    EM adjoint (kinds 1..3)       4.88             20      4.88
    EM adjoint (kind 4)          28.80             120     53.48
    the kind-4 sweep (every <4, S, NR, KIN>, tests/sde_sweep_reference.py, on the cases of tests/test_sde_sweep_gpu.py):
    EM step, S != 2               2.57             10.5    4.48
    EM step, S = 2                3.77             15.5    3.01     (C_EM_STEP_S2 of the sweep's module)
    EM adjoint                   18.48             120     3.90

The path-forward ratio is the oracle's own: it adds the S T same-sign log-sigmoid terms of a path one after the other (9,600 at
S 16, T 600), while the kernel sums 256 partial sums in a tree.  Kind 4 has a sixth constant because the magnitudes of its
adjoint are |a| |J| with the step's Jacobians J taken from autograd, which does not see the cancellation inside J (the Cholesky
factor of the diffusion); the magnitudes of its step are written out like the others (``crn_step_formula``).

tests/test_sde_bounds.py asserts that the CPU ratios stay within c / 4.

The simulator's inputs (``em_case``) keep the noise small (0.01 N(0, 1)) except at the clamp sites -- the last step of the first
chunk, the first step of the next, and step T -- where the noise of every third path and of the last path is -100 on one
dimension, and at the step after a site, where it is +100: a clamped state leaves the floor decisively, so that every one-step
value is below half the floor or above twice it (asserted on the reference, no element is excused).

A cell of the kind-4 sweep (``sw-S<S>-NR<NR>[-k][-R<R>]``, tests/sde_sweep_reference.py) is a name ``crn_sde``, ``EM_KINDS`` and
``em_case`` take like a named network; its inputs, the species it clamps, its kick and the magnitude of its diffusion factor are
read off the float64 reference (``sweep_theta`` .. ``sweep_big``, ``_first_order_factor``), and a rate-law cell takes the kind-4
reverse step on the effective constants [B, 2R].
"""
import functools

import numpy as np
import torch

F64 = np.float64
C24 = 2.0 ** -24
LOG_2PI = float(np.log(2.0 * np.pi))
EM_FLOOR = 1e-6

# c per family: 4 x the measured CPU ratio, rounded up (see the table above)
C_PATH_FWD = 270.0
C_PATH_BWD = 39.0
C_TAIL = 12.0
C_EM_STEP = 10.5
C_EM_ADJ = 20.0
C_EM_ADJ_CRN = 120.0     # kind 4: the magnitudes of its adjoint are |a| |J| with J from autograd, blind to the cancellation inside J


def is_sweep(name):
    """Whether ``name`` is a cell of the kind-4 sweep (tests/sde_sweep_reference.py), e.g. ``sw-S5-NR4-k``."""
    import reaction_networks as N
    return N.is_sweep_name(name)


def is_crn(name):
    """Whether ``name`` is a reaction network of ``crn_sde``."""
    return name in CRN or name in CRN_KINETIC or name == "sir" or is_sweep(name)


def em_crn(name):
    """Whether the simulator case ``name`` runs kind 4: the networks of ``CRN`` and every cell of the sweep, rate laws included."""
    return name in CRN or is_sweep(name)


def em_adj_c(name):
    return C_EM_ADJ_CRN if em_crn(name) else C_EM_ADJ


# ------------------------------------------------------------------------------------------------------ (value, magnitude)
def _mag(x):
    return float(abs(x)) if isinstance(x, (int, float)) else np.abs(x)


class VM:
    """A value and the magnitude of the formula that made it (module docstring)."""
    __slots__ = ("v", "m")

    def __init__(self, v, m=None):
        self.v = v
        self.m = _mag(v) if m is None else m

    @staticmethod
    def of(o):
        return o if isinstance(o, VM) else VM(o)

    def __add__(self, o):
        o = VM.of(o)
        return VM(self.v + o.v, self.m + o.m)

    __radd__ = __add__

    def __sub__(self, o):
        o = VM.of(o)
        return VM(self.v - o.v, self.m + o.m)

    def __rsub__(self, o):
        return VM.of(o) - self

    def __neg__(self):
        return VM(-self.v, self.m)

    def __mul__(self, o):
        o = VM.of(o)
        return VM(self.v * o.v, self.m * o.m)

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = VM.of(o)
        return VM(self.v / o.v, self.m * o.m / (o.v * o.v))

    def __getitem__(self, idx):
        return VM(self.v[idx], self.m[idx])

    def sum(self, axis):
        return VM(self.v.sum(axis, dtype=self.v.dtype), self.m.sum(axis, dtype=self.m.dtype))

    def where(self, cond, other):
        other = VM.of(other)
        return VM(np.where(cond, self.v, other.v).astype(self.v.dtype), np.where(cond, self.m, other.m).astype(self.v.dtype))


def vm_stack(items, axis=-1):
    return VM(np.stack([i.v for i in items], axis), np.stack([i.m for i in items], axis))


def vm_sqrt(a):
    """sqrt: the square root of the magnitude, or the first-order m / (2 sqrt(v)) where the radicand cancels."""
    r = np.sqrt(a.v)
    return VM(r, np.maximum(np.sqrt(a.m), a.m / (2 * r)).astype(r.dtype))


def vm_max(a, floor):
    """max(a, floor): the floor is exact."""
    hit = a.v < floor
    return VM(np.where(hit, floor, a.v).astype(a.v.dtype), np.where(hit, floor, a.m).astype(a.v.dtype))


def _log(x):
    return VM(np.log(x))


def _sigmoid(x):
    """1 / (1 + exp(-x)), overflow-free."""
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1 / (1 + e), e / (1 + e)).astype(x.dtype)


def _log_sigmoid(x):
    return (np.minimum(x, 0) - np.log1p(np.exp(-np.abs(x)))).astype(x.dtype)


def _softplus(x):
    return (np.maximum(x, 0) + np.log1p(np.exp(-np.abs(x)))).astype(x.dtype)


# ------------------------------------------------------------------------------------------------------------ the check
def ratio(got, ref, mag):
    """Worst |got - ref| / (2^-24 magnitude) over the elements with a magnitude; inf where a zero-magnitude element is not exactly
    the reference, or where ``got`` is not finite."""
    got, ref, mag = (np.asarray(a, F64) for a in (got, ref, mag))
    assert got.shape == ref.shape == mag.shape, (got.shape, ref.shape, mag.shape)
    assert np.isfinite(ref).all() and np.isfinite(mag).all() and (mag >= 0).all(), "reference or magnitude not finite"
    if got.size == 0:
        return 0.0
    err = np.abs(got - ref)
    if not np.isfinite(err).all() or (err[mag == 0] != 0).any():
        return float("inf")
    nz = mag > 0
    return float((err[nz] / (C24 * mag[nz])).max()) if nz.any() else 0.0


def conditioning(ref, mag):
    """Worst magnitude / |ref| over the elements with a non-zero reference: finite by construction of the inputs."""
    ref, mag = np.asarray(ref, F64), np.asarray(mag, F64)
    nz = ref != 0
    return float((mag[nz] / np.abs(ref[nz])).max()) if nz.any() else 0.0


# ============================================================================================================ path terms
PATH_NAMES = ("sde", "gen", "jac")
PATH_GRADS = ("g_z", "g_x", "g_means", "g_chol", "g_drift", "g_diffusion")
PATH_MASKS = ("none", "all", "alt", "last")
SATURATED = (-100.0, -20.0, 0.0, 20.0, 100.0)


def positive_dims(mask, S):
    return {"none": [], "all": list(range(S)), "alt": list(range(0, S, 2)), "last": [S - 1]}[mask]


@functools.lru_cache(maxsize=4)
def path_case(S, B, T, mask, seed=0):
    """float32 inputs of the path-term kernels: z a cumulative sum (the residual cancels as in training) with the saturated
    values on rows 1..5 of path 0 at a positive dimension, factors with diagonal in [0.5, 1.5], strict-lower entries
    0.2 randn / sqrt(S) and NaN above the diagonal."""
    rng = np.random.default_rng(1000 * S + 10 * T + B + seed)
    pos = positive_dims(mask, S)
    z = np.cumsum(0.3 * rng.standard_normal((B, T + 1, S)), axis=1)
    sat_dim = pos[-1] if pos else S - 1
    n = min(len(SATURATED), T)
    z[0, 1:1 + n, sat_dim] = SATURATED[:n]
    z = z.astype(np.float32)
    x = z.astype(F64)
    x[..., pos] = _softplus(x[..., pos])

    def factor():
        a = np.tril(0.2 * rng.standard_normal((B, T, S, S)) / np.sqrt(S), -1)
        a[..., np.arange(S), np.arange(S)] = rng.uniform(0.5, 1.5, (B, T, S))
        a[..., np.triu_indices(S, 1)[0], np.triu_indices(S, 1)[1]] = np.nan
        return a.astype(np.float32)

    c = dict(S=S, B=B, T=T, mask=mask, pos=pos, dt=0.1, z=z, x=x.astype(np.float32),
             means=(0.5 * rng.standard_normal((B, T, S))).astype(np.float32), chol=factor(),
             drift=(0.5 * rng.standard_normal((B, T, S))).astype(np.float32), diffusion=factor())
    for k in ("g_sde", "g_gen", "g_jac"):
        c[k] = (rng.standard_normal(B) + np.where(rng.random(B) < 0.5, -1.5, 1.5)).astype(np.float32)
    return c


def _tri(y, m0, d, A, dt, s, S, raw_diag_dim=None):
    """w = (A s)^-1 (y - (m0 + d dt)), v = (A s)^-T w and log N(y; m0 + d dt, (A s)(A s)^T), all VM."""
    w, v = [None] * S, [None] * S
    quad, logdet, dii = 0.0, 0.0, []
    for i in range(S):
        acc = y[..., i] - (m0[..., i] + d[..., i] * dt)
        for j in range(i):
            acc = acc - (A[..., i, j] * s) * w[j]
        dii.append(A[..., i, i] if i == raw_diag_dim else A[..., i, i] * s)
        w[i] = acc / dii[i]
        quad = w[i] * w[i] + quad
        logdet = _log(dii[i].v) + logdet
    for i in range(S - 1, -1, -1):
        acc = w[i]
        for j in range(i + 1, S):
            acc = acc - (A[..., j, i] * s) * v[j]
        v[i] = acc / dii[i]
    lp = -(0.5 * (S * LOG_2PI + quad)) - logdet
    return w, v, lp


PATH_DEFECTS = ("drop_last_step", "drop_step_256", "mask_last_ignored", "diag_without_sqrt_dt", "gz_minus_v_missing_at_256",
                "diag_term_missing_last", "sigmoid_of_plus_z")


def path_formulas(c, dtype=F64, defect=None):
    """The kernels' formulas written out on VM pairs in ``dtype``: {name: VM} for the three terms and the six gradients."""
    S, B, T = c["S"], c["B"], c["T"]
    f = lambda a: VM(np.asarray(a, dtype))
    z, x, means, chol, drift, diff = (f(c[k]) for k in ("z", "x", "means", "chol", "drift", "diffusion"))
    gs, gg, gj = (f(c[k])[:, None] for k in ("g_sde", "g_gen", "g_jac"))
    dt, s = float(dtype(c["dt"])), float(dtype(np.sqrt(c["dt"])))
    pos = [i for i in c["pos"] if not (defect == "mask_last_ignored" and i == S - 1)]
    ws, vs, lps = _tri(x[:, 1:], x[:, :-1], drift, diff, dt, s, S)
    wg, vg, lpg = _tri(z[:, 1:], z[:, :-1], means, chol, dt, s, S, S - 1 if defect == "diag_without_sqrt_dt" else None)
    jac_t = VM(np.zeros((B, T), dtype))
    for i in pos:
        jac_t = jac_t + VM(_log_sigmoid(z.v[:, 1:, i]))
    keep = np.ones(T, bool)
    if defect == "drop_last_step":
        keep[T - 1] = False
    if defect == "drop_step_256" and T > 256:
        keep[256] = False
    out = {"sde": lps[:, keep].sum(1), "gen": lpg[:, keep].sum(1), "jac": jac_t[:, keep].sum(1)}

    zero = VM(np.zeros((B, 1), dtype))

    def ends(g, v, i, skip_prev_at=None):
        cur = VM(np.concatenate([(g * v[i]).v, zero.v], 1), np.concatenate([(g * v[i]).m, zero.m], 1))      # tau < T
        prv = VM(np.concatenate([zero.v, (g * v[i]).v], 1), np.concatenate([zero.m, (g * v[i]).m], 1))      # tau > 0
        if skip_prev_at is not None and skip_prev_at <= T:
            prv.v[:, skip_prev_at] = 0
        return cur - prv

    gz, gx = [], []
    for i in range(S):
        gx.append(ends(gs, vs, i))
        t = ends(gg, vg, i, 256 if defect == "gz_minus_v_missing_at_256" else None)
        if i in pos:
            zi = z.v[:, 1:, i]
            sg = gj * VM(_sigmoid(zi if defect == "sigmoid_of_plus_z" else -zi))
            t = t + VM(np.concatenate([zero.v, sg.v], 1), np.concatenate([zero.m, sg.m], 1))
        gz.append(t)
    out["g_z"], out["g_x"] = vm_stack(gz), vm_stack(gx)
    out["g_means"] = vm_stack([gg * vg[i] * dt for i in range(S)])
    out["g_drift"] = vm_stack([gs * vs[i] * dt for i in range(S)])

    def g_factor(g, A, w, v, no_diag_at=None):
        zero_bt = VM(np.zeros((B, T), dtype))
        rows = []
        for i in range(S):
            row = []
            for j in range(S):
                if j > i:
                    row.append(zero_bt)
                    continue
                val = g * s * v[i] * w[j]
                if i == j and i != no_diag_at:
                    val = val - g / A[..., i, i]
                row.append(val)
            rows.append(vm_stack(row))
        return vm_stack(rows, -2)

    out["g_chol"] = g_factor(gg, chol, wg, vg, S - 1 if defect == "diag_term_missing_last" else None)
    out["g_diffusion"] = g_factor(gs, diff, ws, vs)
    for k, a in out.items():
        assert a.v.dtype == dtype and a.m.dtype == dtype, (k, a.v.dtype, a.m.dtype)
    return out


def _t64(a, grad=False):
    return torch.tensor(np.asarray(a, F64), dtype=torch.float64, requires_grad=grad)


@functools.lru_cache(maxsize=4)
def _path_reference(S, B, T, mask, seed):
    c = path_case(S, B, T, mask, seed)
    MVN = torch.distributions.MultivariateNormal
    z, x, means, drift = (_t64(c[k], True) for k in ("z", "x", "means", "drift"))
    chol, diff = (_t64(np.nan_to_num(c[k], nan=0.0), True) for k in ("chol", "diffusion"))
    dt, s = c["dt"], np.sqrt(c["dt"])
    sde = MVN(x[:, :-1] + drift * dt, scale_tril=torch.tril(diff) * s, validate_args=False).log_prob(x[:, 1:]).sum(1)
    gen = MVN(z[:, :-1] + means * dt, scale_tril=torch.tril(chol) * s, validate_args=False).log_prob(z[:, 1:]).sum(1)
    jac = torch.nn.functional.logsigmoid(z[:, 1:, c["pos"]]).sum((1, 2))
    loss = (_t64(c["g_sde"]) * sde + _t64(c["g_gen"]) * gen + _t64(c["g_jac"]) * jac).sum()
    grads = torch.autograd.grad(loss, [z, x, means, chol, drift, diff], allow_unused=True)
    out = {"sde": sde, "gen": gen, "jac": jac}
    out.update(zip(PATH_GRADS, grads))
    return {k: v.detach().numpy() for k, v in out.items()}


def path_reference(c):
    """float64 values of the three terms and the six gradients from MultivariateNormal / logsigmoid and autograd."""
    return _path_reference(c["S"], c["B"], c["T"], c["mask"], 0)


@functools.lru_cache(maxsize=4)
def _path_magnitudes(S, B, T, mask, seed):
    return {k: a.m for k, a in path_formulas(path_case(S, B, T, mask, seed)).items()}


def path_magnitudes(c):
    return _path_magnitudes(c["S"], c["B"], c["T"], c["mask"], 0)


def path_ratios(c, got):
    """(forward, backward) worst ratios of ``got`` {name: array} against the float64 reference of case ``c``; asserts first that
    magnitude / |ref| of the reference is finite."""
    ref, mag = path_reference(c), path_magnitudes(c)
    assert all(np.isfinite(conditioning(ref[k], mag[k])) for k in ref)
    worst = lambda names: max([ratio(got[k], ref[k], mag[k]) for k in names if k in got], default=0.0)
    return worst(PATH_NAMES), worst(PATH_GRADS)


def path_shapes():
    """(S, B, T, mask) of every path-term case of the GPU file."""
    out = [(S, 3, 257, m) for S in range(1, 17) for m in PATH_MASKS]
    out += [(S, B, T, m) for S in (1, 2, 3, 8, 16) for T in (1, 2, 255, 256, 600) for B in (1, 3) for m in PATH_MASKS]
    return out


# ================================================================================================================== tail
TAIL_DIMS = ((2, 2, 3, False), (3, 16, 16, True), (16, 1, 5, True), (16, 16, 16, False))
TAIL_BS = (1, 2, 255, 256, 257, 700)
TAIL_KS = (0, 1, 5)
TAIL_MASKS = ("none", "all", "last")
TAIL_OUT = ("out", "g_x_obs", "g_theta", "g_post_mean", "g_post_log_std", "g_sde", "g_gen", "g_jac")
G_OUT = (1.0, -0.7, 0.45, 1.6, -2.2, 0.3)          # the six upstream weights: non-zero, distinct, no pair cancels


COUNT_SCALE, COUNT_DISPERSION, RATE_FLOOR = 1.3, 4.0, 1e-6
COUNT_SHAPES = ((257, 0, 5, 1, "all", "poisson"), (257, 1, 5, 0, "last", "negbin"))


@functools.lru_cache(maxsize=None)
def tail_case(B, dims, K, lognormal, mask, count=None, seed=0):
    """float32 inputs of the tail kernels; ``count`` ("poisson" / "negbin"): integer observations 0..6 for the count entry points
    (scale 1.3, dispersion 4), where a negative prediction binds the rate floor."""
    S, O, P, with_matrix = TAIL_DIMS[dims]
    rng = np.random.default_rng(7919 * B + 101 * dims + 11 * K + seed)
    f = lambda a: np.asarray(a, np.float32)
    c = _tail_case(rng, f, B, dims, K, lognormal, mask, S, O, P, with_matrix)
    c["count"] = count
    if count:
        c["obs_values"] = f(rng.integers(0, 7, (K, O)))
    return c


def _tail_case(rng, f, B, dims, K, lognormal, mask, S, O, P, with_matrix):
    return dict(B=B, K=K, S=S, O=O, P=P, dims=dims, mask=mask, pos=positive_dims(mask, P), lognormal=int(lognormal),
                x_obs=f(rng.random((B, K, S)) + 0.5), obs_values=f(rng.standard_normal((K, O)) + 1.0),
                obs_matrix=f(0.5 * rng.standard_normal((O, S))) if with_matrix else None, variance=0.3,
                theta=f(0.8 * rng.random((B, P)) + 0.1), prior_mean=0.2, prior_std=1.3,
                post_mean=f(0.3 * rng.standard_normal(P)), post_log_std=f(0.2 * rng.standard_normal(P) - 0.5),
                sde_lp=f(50 * rng.standard_normal(B)), gen_lp=f(50 * rng.standard_normal(B)), jac=f(10 * rng.standard_normal(B)),
                g_out=f(G_OUT))


TAIL_DEFECTS = ("paths_from_256_dropped", "divide_by_256", "log_std_minus_one_missing", "obs_matrix_transposed",
                "theta_bit_15_ignored")


def _count_terms(kind, y, pred, dtype):
    """(log-density, d / d pred) per (b, k, o) of the count likelihoods in their raw form: Poisson y log lam - lam - lgamma(y + 1),
    negative binomial lgamma(y + r) - lgamma(r) - lgamma(y + 1) + r log(r / (r + lam)) + y log(lam / (r + lam)), with
    lam = max(scale pred, 1e-6); a log carries |log| plus the relative magnitude of its argument."""
    import math
    lg = lambda a: VM(np.vectorize(math.lgamma, otypes=[np.float64])(np.asarray(a, F64)).astype(dtype))
    vlog = lambda a: VM(np.log(a.v), np.abs(np.log(a.v)) + a.m / np.abs(a.v))
    sp = COUNT_SCALE * pred
    assert ((sp.v < 0.5 * RATE_FLOOR) | (sp.v > 2 * RATE_FLOOR)).all(), "a rate lies within a factor 2 of the floor: change the input"
    free = sp.v >= RATE_FLOOR
    lam = vm_max(sp, RATE_FLOOR)
    yb = y[None]
    zero = VM(np.zeros_like(lam.v))
    if kind == "poisson":
        term = (yb * vlog(lam)).where(yb.v > 0, zero) - lam - lg(yb.v + 1.0)
        d = (COUNT_SCALE * (yb - lam) / lam).where(free, zero)
    else:
        r = COUNT_DISPERSION
        term = (lg(yb.v + r) - float(math.lgamma(r)) - lg(yb.v + 1.0) + r * (float(np.log(r)) - vlog(r + lam))
                + (yb * (vlog(lam) - vlog(r + lam))).where(yb.v > 0, zero))
        d = (COUNT_SCALE * r * (yb - lam) / (lam * (r + lam))).where(free, zero)
    return term, d


def tail_formulas(c, dtype=F64, defect=None):
    """The tail kernels' formulas written out on VM pairs: {name: VM} for out [6] and the seven gradients."""
    B, K, S, O, P = (c[k] for k in ("B", "K", "S", "O", "P"))
    f = lambda a: VM(np.asarray(a, dtype))
    x, y, th, qm, ls = (f(c[k]) for k in ("x_obs", "obs_values", "theta", "post_mean", "post_log_std"))
    inv_var = float(dtype(1.0 / c["variance"]))
    log_norm = float(dtype(-0.5 * np.log(2.0 * np.pi * c["variance"])))
    pm, pis = float(dtype(c["prior_mean"])), float(dtype(1.0 / c["prior_std"]))
    pconst = float(dtype(-np.log(c["prior_std"]) - 0.5 * LOG_2PI))
    H = None
    if c["obs_matrix"] is not None:
        Hm = np.asarray(c["obs_matrix"], dtype)
        H = f(Hm.reshape(S, O).T if defect == "obs_matrix_transposed" else Hm)
    pos = np.zeros(P, bool)
    pos[[i for i in c["pos"] if not (defect == "theta_bit_15_ignored" and i == 15)]] = True
    ln = bool(c["lognormal"])
    Bdiv = float(256 if defect == "divide_by_256" else B)
    nb = min(B, 256) if defect == "paths_from_256_dropped" else B

    if H is None:
        pred = x
    else:
        pred = VM(np.zeros((B, K, O), dtype))
        for i in range(S):
            pred = pred + H[None, None, :, i] * x[:, :, i:i + 1]
    r = y[None] - pred
    if c.get("count"):
        obs_t, dterm = _count_terms(c["count"], y, pred, dtype)
        obs = obs_t.sum(2).sum(1)
    else:
        obs = (-(0.5 * r * r * inv_var) + log_norm).sum(2).sum(1)
    lg = VM(np.log(np.asarray(c["theta"], dtype)))
    up = lg if ln else th
    zp = (up - pm) * pis
    prior_t = -(0.5 * zp * zp) + pconst
    if ln:
        prior_t = prior_t - lg
    prior = prior_t.sum(1)
    e = VM(np.exp(-ls.v))
    uq = lg.where(pos[None], th)
    zq = (uq - qm[None]) * e[None]
    post_t = -(0.5 * zq * zq) - ls[None] - 0.5 * LOG_2PI
    post = (post_t - lg).where(pos[None], post_t).sum(1)
    sl, gl, jc = (f(c[k]) for k in ("sde_lp", "gen_lp", "jac"))
    terms = [obs + sl - gl + jc + prior - post, obs, sl, gl, prior, post]
    out = {"out": vm_stack([t[:nb].sum(0) / Bdiv for t in terms])}
    out["sample_terms"] = vm_stack([obs, prior, post], 0)              # per path [3, B]: what the log-weight kernel adds to its path sum

    g = [VM(float(v)) for v in np.asarray(c["g_out"], dtype)]
    ib = 1.0 / Bdiv
    w_obs, w_sde, w_gen, w_jac = (g[0] + g[1]) * ib, (g[0] + g[2]) * ib, (g[3] - g[0]) * ib, g[0] * ib
    w_prior, w_post = (g[0] + g[4]) * ib, (g[5] - g[0]) * ib
    gr = w_obs * dterm if c.get("count") else w_obs * r * inv_var     # d / d pred, [B, K, O]
    if H is None:
        out["g_x_obs"] = gr
    else:
        cols = []
        for i in range(S):
            acc = VM(np.zeros((B, K), dtype))
            for o in range(O):
                acc = acc + gr[:, :, o] * H[o, i]
            cols.append(acc)
        out["g_x_obs"] = vm_stack(cols)
    gt_prior = (-(zp * pis) - 1.0) / th if ln else -(zp * pis)
    gt_post = ((-(zq * e[None]) - 1.0) / th).where(pos[None], -(zq * e[None]))
    out["g_theta"] = w_prior * gt_prior + w_post * gt_post
    out["g_post_mean"] = (w_post * zq * e[None])[:nb].sum(0)
    out["g_post_log_std"] = (w_post * (zq * zq if defect == "log_std_minus_one_missing" else zq * zq - 1.0))[:nb].sum(0)
    full = lambda w: VM(np.full(B, w.v, dtype), np.full(B, w.m, dtype))
    out["g_sde"], out["g_gen"], out["g_jac"] = full(w_sde), full(w_gen), full(w_jac)
    for k, a in out.items():
        assert a.v.dtype == dtype and a.m.dtype == dtype, (k, a.v.dtype, a.m.dtype)
    return out


def tail_reference(c, dtype=torch.float64):
    """Values and gradients of the tail from torch.distributions Normal / LogNormal and autograd, in ``dtype``."""
    D = torch.distributions
    t = lambda a, grad=False: torch.tensor(np.asarray(a), dtype=dtype, requires_grad=grad)
    x, th, qm, ls = (t(c[k], True) for k in ("x_obs", "theta", "post_mean", "post_log_std"))
    sl, gl, jc = (t(c[k], True) for k in ("sde_lp", "gen_lp", "jac"))
    y = t(c["obs_values"])
    pred = x if c["obs_matrix"] is None else x @ t(c["obs_matrix"]).t()
    if c.get("count"):
        lam = (COUNT_SCALE * pred).clamp(min=RATE_FLOOR)
        if c["count"] == "poisson":
            obs = D.Poisson(lam, validate_args=False).log_prob(y).sum((1, 2))
        else:       # torch's NegativeBinomial(total_count r, probs p): mean r p / (1 - p) = lam
            obs = D.NegativeBinomial(t(COUNT_DISPERSION), probs=lam / (lam + COUNT_DISPERSION), validate_args=False).log_prob(y).sum((1, 2))
    else:
        obs = D.Normal(pred, t(c["variance"] ** 0.5), validate_args=False).log_prob(y).sum((1, 2))
    fam = D.LogNormal if c["lognormal"] else D.Normal
    prior = fam(t(c["prior_mean"]), t(c["prior_std"]), validate_args=False).log_prob(th).sum(1)
    pos = torch.zeros(c["P"], dtype=torch.bool)
    pos[c["pos"]] = True
    sd = torch.exp(ls)
    post = torch.where(pos, D.LogNormal(qm, sd, validate_args=False).log_prob(th),
                       D.Normal(qm, sd, validate_args=False).log_prob(th)).sum(1)
    terms = [obs + sl - gl + jc + prior - post, obs, sl, gl, prior, post]
    out = torch.stack([v.mean() for v in terms])
    grads = torch.autograd.grad((out * t(c["g_out"])).sum(), [x, th, qm, ls, sl, gl, jc], allow_unused=True)
    if c.get("count") and dtype == torch.float64:     # the observation term's value from tests/count_likelihood_reference.py
        import count_likelihood_reference as cr
        x64, H = np.asarray(c["x_obs"], F64), c["obs_matrix"]
        y64 = np.asarray(c["obs_values"], F64)[None]
        lp = (cr.poisson_log_prob(y64, x64, COUNT_SCALE, H) if c["count"] == "poisson"
              else cr.negative_binomial_log_prob(y64, x64, COUNT_DISPERSION, COUNT_SCALE, H)).sum(1)
        assert np.abs(lp - obs.detach().numpy()).max() <= 1e-10 * np.abs(lp).max()
        out = out.detach().clone()
        out[0] += float(lp.mean()) - float(out[1])
        out[1] = float(lp.mean())
    res = {"out": out}
    res.update(zip(TAIL_OUT[1:], [torch.zeros_like(v) if g is None else g for g, v in zip(grads, [x, th, qm, ls, sl, gl, jc])]))
    return {k: v.detach().numpy() for k, v in res.items()}


def tail_ratio(c, got, ref=None, mag=None):
    """Worst ratio of ``got`` {name: array} against the float64 reference of case ``c``: per element for the per-path gradients,
    against the sum over b of the terms' magnitudes for out [6] and g_post_*."""
    ref = tail_reference(c) if ref is None else ref
    mag = {k: a.m for k, a in tail_formulas(c).items()} if mag is None else mag
    assert all(np.isfinite(conditioning(ref[k], mag[k])) for k in ref)
    return max([ratio(got[k], ref[k], mag[k]) for k in TAIL_OUT if k in got], default=0.0)


def tail_shapes():
    """(B, dims index, K, lognormal, mask) of every Gaussian tail case of the GPU file (the count cases: COUNT_SHAPES)."""
    return [(B, d, K, ln, m) for B in TAIL_BS for d in range(len(TAIL_DIMS)) for K in TAIL_KS for ln in (0, 1) for m in TAIL_MASKS]


# ============================================================================================================= simulator
def em_chunk(S):
    """csrc/vsde_sde.hip: em_chunk, the steps the simulator stages in LDS at a time."""
    return 32 if S <= 2 else 16 if S <= 4 else 8


class _EmKinds(dict):
    """name -> (kernel kind, S, CH = em_chunk(S)); a cell of the kind-4 sweep is looked up by its name and is not listed."""

    def __missing__(self, name):
        import reaction_networks as N
        if not N.is_sweep_name(name):
            raise KeyError(name)
        S = N.sweep_cell(name)[0]
        return ("reaction_network", S, em_chunk(S))


EM_KINDS = _EmKinds({"ou": ("ornstein_uhlenbeck", 1, 32), "lv": ("lotka_volterra", 2, 32), "diag5": ("linear_diagonal", 5, 8),
                     "diag8": ("linear_diagonal", 8, 8)})
EM_KINDS.update({"net3": ("reaction_network", 3, 16), "chain8": ("reaction_network", 8, 8)})
CRN = ("net3", "chain8")
ORACLE_KIND = {"ou": "ou", "lv": "lv", "diag5": "linear_diagonal", "diag8": "linear_diagonal"}
EM_BS = (1, 63, 64, 65, 130)
EM_PATHS = 64
EM_BIG = 100.0


def em_ts(name):
    ch = EM_KINDS[name][2]
    return (1, ch - 1, ch, ch + 1, 2 * ch + 3)


def em_sites(name, T):
    """1-based steps whose result is clamped on purpose: the last step of the first chunk, the first of the next, step T."""
    ch = EM_KINDS[name][2]
    return sorted({t for t in (ch, ch + 1, T) if t <= T})


CRN_KINETIC = {"autoreg": "AUTOREG", "repress3": "REPRESS3", "chain8k": "KINETIC_CHAIN8", "clamp2": "CLAMP2"}


class _HillFactor(torch.autograd.Function):
    """g = a / (c + a) (activation) or c / (c + a) (repression), a = u^n, c = K^n, u = clamp(x, min=0), as
    viforsdes_amd.core.reaction_network.propensities forms it, with the derivatives written out: dg/du = +-n u^(n-1) c / (c + a)^2
    (passed to x where x >= 0, torch.clamp's rule), dg/dK = -+n K^(n-1) a / (c + a)^2.  Autograd through the quotient gives the same
    numbers up to rounding, but rounding noise where they are exactly zero (dg/dK at u = 0, dg/du of n > 1 at u = 0), and a
    per-element bound has to hold the kernels to the exact zero there.  tests/test_sde_aux_bounds.py pins these derivatives to the
    package's autograd."""

    @staticmethod
    def forward(ctx, x, K, n, activation):
        u = x.clamp(min=0)
        a, c = u, K
        for _ in range(n - 1):
            a, c = a * u, c * K
        ctx.save_for_backward(x, u, K, a, c)
        ctx.n, ctx.activation = n, activation
        return (a if activation else c) / (c + a)

    @staticmethod
    def backward(ctx, g):
        x, u, K, a, c = ctx.saved_tensors
        n, sign = ctx.n, (1.0 if ctx.activation else -1.0)
        den2 = (c + a) * (c + a)
        gu = torch.where(x >= 0, n * u ** (n - 1) * c / den2, torch.zeros_like(x))
        gk = n * K ** (n - 1) * a / den2
        return g * sign * gu, -(g * sign * gk), None, None


def _kinetic_propensities(sde, x, rates):
    """h [.., R] of a rate-law network on its effective constants [.., 2R]: ``propensities`` of the package with the Hill factor's
    derivatives written out (``_HillFactor``)."""
    Rn = sde.num_reactions
    cols = []
    for j, row in enumerate(sde.reactants):
        if sde.laws[j] is not None:
            code, s, n = sde.laws[j][:3]
            cols.append(rates[..., j] * _HillFactor.apply(x[..., s], rates[..., Rn + j], n, code == 1))
            continue
        m = rates[..., j]
        for i, r in enumerate(row):
            for _ in range(r):
                m = m * x[..., i]
        cols.append(m)
    return torch.stack(cols, dim=-1)


@functools.lru_cache(maxsize=None)
def crn_sde(name):
    """The reaction network of a kind-4 case: A + B <-> C with in / outflow (S 3, R 5) and the 8-species conversion chain (R 9);
    for tests/sde_aux_reference.py also SIR (S 2, R 2) and the rate-law networks of tests/reaction_networks.py.  A rate-law
    network comes back as a copy whose parameters ARE the effective constants [.., 2R] the kinetic entry points take (its map
    theta -> constants replaced by the identity), so that values and gradients refer to those constants."""
    import copy

    import reaction_networks as N
    from viforsdes_amd import ReactionNetworkSDE
    if is_sweep(name):
        # a cell of the sweep: reaction_networks.sweep_network; base_theta [P] and start [S] are its constants and start state
        S, NR, kinetic, Rn = N.sweep_cell(name)
        kw, base, start = N.sweep_network(S, NR, kinetic, Rn)
        spec = ReactionNetworkSDE(**kw)
        if not kinetic:
            spec.rate_dim = spec.num_reactions
            spec.base_theta, spec.start = np.asarray(base, F64), np.asarray(start, F64)
            return spec
    if name in CRN_KINETIC or is_sweep(name):
        if name in CRN_KINETIC:
            spec = ReactionNetworkSDE(**getattr(N, CRN_KINETIC[name]))
        sde = copy.copy(spec)
        if is_sweep(name):
            sde.base_theta, sde.start = np.asarray(base, F64), np.asarray(start, F64)
        sde.rates_of = spec.kernel_parameters                   # theta [.., P] -> effective constants [.., 2R]
        sde.kernel_parameters = lambda rates: rates
        sde.autograd_propensities = sde._propensities           # the package's own, for the pin of _HillFactor
        sde._propensities = functools.partial(_kinetic_propensities, sde)
        sde.rate_dim = 2 * sde.num_reactions
        return sde
    sde = ReactionNetworkSDE(**{"net3": N.NET3, "chain8": N.CHAIN8, "sir": N.SIR}[name])
    sde.rate_dim = sde.num_reactions
    return sde


@functools.lru_cache(maxsize=None)
def em_case(name, B, T, seed=0):
    """float32 inputs of the simulator (module docstring).  Parameters under which the adjoint does not grow over 2 CH + 3 steps:
    reaction networks rate constants in [0.3, 0.8], x0 in [1.6, 2.4], dt = 0.05 (dissipative mass-action drifts);
    OU kappa in [0.5, 1] (kappa dt <= 0.1), mu = 1, sigma in [0.3, 0.6]; LV theta = (0.8, 0.0025, 0.3) (1 + 0.1 U) from
    (u, v) = (120, 200) (0.9 + 0.2 U), next to its equilibrium (t3 / t2, t1 / t2); linear-diagonal a in [0.2, 0.5], b = 0.5 N(0, 1).
    dt = 0.1 for kinds 1..3, every state dimension positive."""
    kind, S, ch = EM_KINDS[name]
    rng = np.random.default_rng(31 * B + 7 * T + len(name) + seed)
    if name == "ou":
        theta = np.stack([rng.uniform(0.5, 1.0, B), np.ones(B), rng.uniform(0.3, 0.6, B)], 1)
        x0 = rng.uniform(0.8, 1.2, (B, 1))
    elif name == "lv":
        theta = np.array([0.8, 0.0025, 0.3]) * (1 + 0.1 * rng.random((B, 3)))
        x0 = np.array([120.0, 200.0]) * (0.9 + 0.2 * rng.random((B, 2)))
    elif is_sweep(name):
        theta, x0 = sweep_theta(name, rng, B), sweep_states(name, rng, (B,))
    elif name in CRN:
        theta = rng.uniform(0.3, 0.8, (B, crn_sde(name).sde_param_dim))
        x0 = rng.uniform(1.6, 2.4, (B, S))
    else:
        theta = np.concatenate([rng.uniform(0.2, 0.5, (B, S)), 0.5 * rng.standard_normal((B, S))], 1)
        x0 = rng.uniform(0.8, 1.2, (B, S))
    noise = 0.01 * rng.standard_normal((B, T, S))
    sites = em_sites(name, T)
    # (path, dimension) pairs that are clamped at the sites; kind 4: the last species, whose noise enters no other row of G
    # (a cell of the sweep: the last species whose pivot is not floored -- a floored pivot is 1e-3 and moves nothing)
    last = sweep_hit_dim(name) if is_sweep(name) else S - 1
    hit = [(b, last if em_crn(name) else b % S) for b in range(B) if b % 3 == 0 or b == B - 1]
    big = sweep_big(name) if is_sweep(name) else EM_BIG
    if is_sweep(name):
        noise[..., sweep_zeroed(name)] = 0.0
    for b, d in hit:
        for t in sites:
            noise[b, t - 1, d] = -big
            # (a cell of the sweep leaves the floor on its drift alone, see sde_sweep_reference: every species has an inflow)
            if t + 1 <= T and t + 1 not in sites and not is_sweep(name):
                noise[b, t, d] = big
    f = lambda a: np.asarray(a, np.float32)
    return dict(name=name, kind=kind, S=S, B=B, T=T, ch=ch, dt=0.05 if em_crn(name) else 0.1, pos=list(range(S)), x0=f(x0), theta=f(theta), noise=f(noise),
                g_traj=f(rng.standard_normal((B, T + 1, S))), sites=sites, hit=hit)


def _crn_torch(name, x, th, e, dtype, grad=False):
    td = torch.float64 if dtype == F64 else torch.float32
    x = torch.tensor(np.asarray(x), dtype=td)
    th = torch.tensor(np.asarray(th), dtype=td).expand(*x.shape[:-1], -1).contiguous()
    e = torch.tensor(np.asarray(e), dtype=td)
    return x.requires_grad_(grad), th.requires_grad_(grad), e


def _crn_step_torch(sde, x, th, e, dt):
    return x + sde.drift(x, th) * dt + torch.einsum("...ik,...k->...i", sde.diffusion(x, th), e) * dt ** 0.5


def crn_coef_formula(name, x, th, dtype=F64):
    """Kind 4 written out on VM pairs: (f [S], L [S][S] lower triangle, gates): propensities (mass action, or for a rate-law
    reaction k_j g_j with the Hill factor g_j a quotient of positive terms, whose magnitude is its value), drift nu^T h,
    Sigma = sum_j h_j nu_j nu_j^T and its Cholesky factor with the 1e-6 floors of ReactionNetworkSDE.diffusion; ``gates`` are
    the quantities the floors test (VM)."""
    sde = crn_sde(name)
    S, Rn = sde.state_dim, sde.num_reactions
    x, th = (VM(np.asarray(a, dtype)) for a in (x, th))
    h = []
    for j, row in enumerate(sde.reactants):
        m = th[..., j] + 0.0 * x[..., 0]                                    # broadcast theta against the states
        m = VM(m.v, np.abs(m.v))
        if sde.laws[j] is not None:
            code, sp, n = sde.laws[j][:3]
            u = np.maximum(x.v[..., sp], 0) + 0 * m.v
            K = th.v[..., Rn + j] + 0 * m.v
            a, c = u, K
            for _ in range(n - 1):
                a, c = a * u, c * K
            h.append(m * VM((a if code == 1 else c) / (c + a)))
            continue
        for i, r in enumerate(row):
            for _ in range(r):
                m = m * x[..., i]
        h.append(m)
    nu = sde.change
    zero = VM(np.zeros_like(h[0].v))
    f = [sum((float(nu[j][i]) * h[j] for j in range(Rn) if nu[j][i]), zero) for i in range(S)]
    sig = [[sum((float(nu[j][i] * nu[j][k]) * h[j] for j in range(Rn) if nu[j][i] * nu[j][k]), zero) for k in range(S)] for i in range(S)]
    L = [[None] * S for _ in range(S)]
    gates = []
    for j in range(S):
        acc = sig[j][j]
        for k in range(j):
            acc = acc - L[j][k] * L[j][k]
        L[j][j] = vm_sqrt(vm_max(acc, EM_FLOOR))
        gates += [acc, L[j][j]]
        c = vm_max(L[j][j], EM_FLOOR)
        for i in range(j + 1, S):
            a = sig[i][j]
            for k in range(j):
                a = a - L[i][k] * L[j][k]
            L[i][j] = a / c
    if is_sweep(name):
        L = _first_order_factor(sig, L, S, dtype)
    return f, L, gates


def _first_order_factor(sig, L, S, dtype):
    """The factor's entries with the smaller of two magnitudes, for the cells of the sweep.  The recursion's own magnitude multiplies
    the inflation of every Cholesky level into the next: harmless in the named networks (a chain does not cancel), but 1e30 to
    1e120 times the value in the last rows of a generated network of 7 or 8 species, where a bound made from it holds a kernel to
    nothing.  The other is the first-order perturbation of a Cholesky factor, dL = L Phi(L^-1 dSigma L^-T) with Phi the strict lower
    triangle plus half the diagonal, taken with absolute values: |L| + |L| Phi(|L^-1| (m(Sigma) + |L| |L|^T) |L^-T|), where m(Sigma) is
    the magnitude of the covariance's own sum and |L| |L|^T the backward error of the factorisation, both in units of the rounding.
    A floored pivot enters as the 1e-3 it is.  Either is a magnitude of a correct evaluation's error, so their minimum is one."""
    shape = np.broadcast(*[sig[i][k].v for i in range(S) for k in range(i + 1)]).shape
    Lv, mS = np.zeros(shape + (S, S)), np.zeros(shape + (S, S))
    for i in range(S):
        for k in range(i + 1):
            Lv[..., i, k] = L[i][k].v
            mS[..., i, k] = mS[..., k, i] = sig[i][k].m
    absL = np.abs(Lv)
    finite = np.isfinite(Lv).all((-1, -2), keepdims=True)              # a path started at NaN stays NaN: no inverse to take
    inv = np.abs(np.linalg.inv(np.where(finite, Lv, np.eye(S))))
    M = inv @ (mS + absL @ np.swapaxes(absL, -1, -2)) @ np.swapaxes(inv, -1, -2)
    phi = np.tril(M, -1)
    idx = np.arange(S)
    phi[..., idx, idx] = 0.5 * M[..., idx, idx]
    m1 = absL + absL @ phi
    out = [[None] * S for _ in range(S)]
    for i in range(S):
        for k in range(i + 1):
            out[i][k] = VM(L[i][k].v, np.minimum(L[i][k].m, m1[..., i, k]).astype(dtype))
    return out


# --- the cells of the kind-4 sweep (tests/sde_sweep_reference.py): inputs around the network's own constants and start state
SWEEP_JITTER = 0.2


def sweep_theta(name, rng, B):
    """[B, rate_dim] constants of a cell: its base theta jittered by +-20 %; of a rate-law cell the effective constants [B, 2R]
    of that theta, formed in float32 as the package forms them."""
    sde = crn_sde(name)
    th = sde.base_theta * (1 + SWEEP_JITTER * rng.uniform(-1, 1, (B, len(sde.base_theta))))
    return th if sde.plain else sde.rates_of(torch.tensor(th, dtype=torch.float32)).numpy()


def sweep_states(name, rng, shape):
    """[*shape, S] states of a cell: its start state (populations of 6..10) jittered by +-20 %."""
    sde = crn_sde(name)
    return sde.start * (1 + SWEEP_JITTER * rng.uniform(-1, 1, tuple(shape) + (sde.state_dim,)))


@functools.lru_cache(maxsize=None)
def sweep_floored(name):
    """The floored pivots of a cell: the columns j whose Cholesky radicand (``gates[2j]`` of ``crn_coef_formula``) is under the
    floor in float64 at the cell's start state and base constants.  Structural: the covariance has the rank of the
    stoichiometric vectors, so the same columns floor at every state of the case (tests/test_sde_sweep_bounds.py asserts it)."""
    sde = crn_sde(name)
    th = sde.base_theta if sde.plain else sde.rates_of(torch.tensor(sde.base_theta, dtype=torch.float64)).numpy()
    gates = crn_coef_formula(name, sde.start[None], th[None])[2]
    return tuple(j for j in range(sde.state_dim) if float(gates[2 * j].v[0]) < EM_FLOOR)


def sweep_zeroed(name):
    """The noise / g_diffusion columns set to exactly zero: the floored pivots of a cell with two or more of them, none otherwise.
    The adjoint divides by the floored c = 1e-3 once per floored pivot on the way, which with two of them turns the forward's
    rounding noise into the gradient: no float64 comparison can score that.  With one floored pivot the path stays scored."""
    fl = sweep_floored(name)
    return list(fl) if len(fl) >= 2 else []


def sweep_hit_dim(name):
    """The species clamped at the sites: the last one, whose noise enters no other row of G, as in the named networks.  A cell with
    floored pivots: species 2, the product of the second-order reaction and reactant of none there.  A floored pivot is 1e-3 and
    moves nothing, and the last pivot above the floored ones is what one reaction leaves after all the others are eliminated: it
    cancels a few hundred times, and a kick through it into the rows below turns that into the gradient (float32 torch: 400 to
    1200 times the magnitude's rounding); the pivot of species 2 cancels some ten times."""
    fl = sweep_floored(name)
    assert not fl or 2 not in fl
    return 2 if fl else crn_sde(name).state_dim - 1


@functools.lru_cache(maxsize=None)
def sweep_big(name):
    """The noise at a clamp site of a cell: EM_BIG times the smallest integer that makes the kick L_dd big sqrt(dt) of the hit
    species at the start state at least EM_BIG sqrt(dt) = 22, against populations of at most 12."""
    sde, d = crn_sde(name), sweep_hit_dim(name)
    th = sde.base_theta if sde.plain else sde.rates_of(torch.tensor(sde.base_theta, dtype=torch.float64)).numpy()
    L = crn_coef_formula(name, sde.start[None], th[None])[1]
    return EM_BIG * max(1.0, float(np.ceil(1.0 / float(L[d][d].v[0]))))


def crn_step_formula(name, x, th, e, dt, dtype=F64):
    """The kind-4 step on VM pairs, from the coefficients of ``crn_coef_formula``."""
    f, L, _ = crn_coef_formula(name, x, th, dtype)
    S = len(f)
    x, e = (VM(np.asarray(a, dtype)) for a in (x, e))
    dt, s = float(dtype(dt)), float(dtype(np.sqrt(dt)))
    zero = VM(np.zeros_like(f[0].v))
    return vm_stack([x[..., i] + f[i] * dt + sum((L[i][k] * e[..., k] for k in range(i + 1)), zero) * s for i in range(S)])


def _crn_step(name, x, th, e, dt, dtype):
    """Kind 4: the value from the float64 (``dtype``) torch statement of the network's drift and Cholesky diffusion factor
    (ReactionNetworkSDE.drift / .diffusion), the magnitude from ``crn_step_formula``."""
    sde = crn_sde(name)
    xt, tt, et = _crn_torch(name, x, th, e, dtype)
    return VM(_crn_step_torch(sde, xt, tt, et, dt).numpy(), crn_step_formula(name, x, th, e, dt, dtype).m)


def _crn_step_bwd(name, x, th, e, a, dt, dtype):
    """Kind 4: ax = a J_x, gth = a J_theta from the step's Jacobians (autograd, one row per species); magnitudes with |J|."""
    sde, S = crn_sde(name), EM_KINDS[name][1]
    x, th, e = _crn_torch(name, x, th, e, dtype, grad=True)
    y = _crn_step_torch(sde, x, th, e, dt)
    # (a rate-law cell: th are the effective constants [.., 2R]; the K of a mass-action reaction enters nothing: a zero column)
    rows = [torch.autograd.grad(y[..., i].sum(), [x, th], retain_graph=True, allow_unused=True) for i in range(S)]
    rows = [[torch.zeros_like(v) if g is None else g for g, v in zip(r, (x, th))] for r in rows]
    Jx, Jt = (np.stack([r[k].numpy() for r in rows], -2) for k in (0, 1))          # [.., S (output), S or P]
    vjp = lambda J: VM(np.einsum("...i,...ij->...j", a.v, J), np.einsum("...i,...ij->...j", a.m, np.abs(J)))
    return vjp(Jx), vjp(Jt)


def em_step(name, x, th, e, dt, dtype=F64):
    """One unclamped step y = x + f dt + (G e) sqrt(dt) as a VM [..., S]; x, e [..., S], th [..., P] broadcast against them."""
    if is_crn(name):
        return _crn_step(name, x, th, e, dt, dtype)
    S = np.shape(x)[-1]
    x, th, e = (VM(np.asarray(a, dtype)) for a in (x, th, e))
    dt, s = float(dtype(dt)), float(dtype(np.sqrt(dt)))
    if name == "ou":
        return x + th[..., 0:1] * (th[..., 1:2] - x) * dt + th[..., 2:3] * e * s
    if name == "lv":
        u, v, t1, t2, t3 = x[..., 0], x[..., 1], th[..., 0], th[..., 1], th[..., 2]
        uv = t2 * u * v
        l00 = vm_sqrt(vm_max(t1 * u + uv, EM_FLOOR))
        l10 = -uv / vm_max(l00, EM_FLOOR)
        l11 = vm_sqrt(vm_max(t3 * v + uv - l10 * l10, EM_FLOOR))
        return vm_stack([u + (t1 * u - uv) * dt + (l00 * e[..., 0]) * s,
                         v + (uv - t3 * v) * dt + (l10 * e[..., 0] + l11 * e[..., 1]) * s])
    g = VM(_softplus(th.v[..., S:])) + 1e-3
    return x + (-th[..., :S] * x) * dt + (g * e) * s


def em_step_bwd(name, x, th, e, a, dt, dtype=F64):
    """(ax, gth): the vector-Jacobian product of ``em_step`` for a = dL/dy (a VM), as VM."""
    if em_crn(name):
        return _crn_step_bwd(name, x, th, e, a, dt, dtype)
    S = EM_KINDS[name][1]
    x, th, e = (VM(np.asarray(t, dtype)) for t in (x, th, e))
    dt, s = float(dtype(dt)), float(dtype(np.sqrt(dt)))
    if name == "ou":
        a0, x0 = a[..., 0], x[..., 0]
        gth = vm_stack([a0 * (th[..., 1] - x0) * dt, a0 * th[..., 0] * dt, a0 * e[..., 0] * s])
        return vm_stack([a0 * (1.0 - th[..., 0] * dt)]), gth
    if name == "lv":
        u, v, t1, t2, t3 = x[..., 0], x[..., 1], th[..., 0], th[..., 1], th[..., 2]
        a0, a1, e0, e1 = a[..., 0], a[..., 1], e[..., 0], e[..., 1]
        zero = VM(np.zeros_like(u.v))
        uv = t2 * u * v
        q00r = t1 * u + uv
        l00 = vm_sqrt(vm_max(q00r, EM_FLOOR))
        c = vm_max(l00, EM_FLOOR)
        l10 = -uv / c
        q11r = t3 * v + uv - l10 * l10
        l11 = vm_sqrt(vm_max(q11r, EM_FLOOR))
        d_f0, d_f1, d_l11 = a0 * dt, a1 * dt, a1 * e1 * s
        d_l00, d_l10 = a0 * e0 * s, a1 * e0 * s
        d_q11 = (d_l11 / (2.0 * l11)).where(q11r.v >= EM_FLOOR, zero)
        d_t3, d_v, d_uv = d_q11 * v, a1 + d_q11 * t3, d_q11
        d_l10 = d_l10 + (-2.0 * l10) * d_q11
        d_uv = d_uv + (-d_l10) / c
        d_l00 = (d_l00 + d_l10 * uv / (c * c)).where(l00.v >= EM_FLOOR, d_l00)
        d_q00 = (d_l00 / (2.0 * l00)).where(q00r.v >= EM_FLOOR, zero)
        d_t1, d_u, d_uv = d_q00 * u, a0 + d_q00 * t1, d_uv + d_q00
        d_t1, d_u, d_uv = d_t1 + d_f0 * u, d_u + d_f0 * t1, d_uv - d_f0
        d_uv, d_t3, d_v = d_uv + d_f1, d_t3 - d_f1 * v, d_v - d_f1 * t3
        return vm_stack([d_u + d_uv * t2 * v, d_v + d_uv * t2 * u]), vm_stack([d_t1, d_uv * u * v, d_t3])
    sg = VM(_sigmoid(th.v[..., S:]))
    ga, gb = a * (-x) * dt, a * sg * e * s
    return a * (1.0 - th[..., :S] * dt), VM(np.concatenate([ga.v, gb.v], -1), np.concatenate([ga.m, gb.m], -1))


def em_forward_check(c, traj):
    """Teacher-forced float64 one-step values from the GIVEN trajectory: (ref [B, T, S] after the clamp, magnitude, below) with
    ``below`` the elements whose unclamped value is under the floor; asserts that none lies between half and twice the floor."""
    traj = np.asarray(traj, F64)
    y = em_step(c["name"], traj[:, :-1], np.asarray(c["theta"], F64)[:, None, :], c["noise"], c["dt"])
    below = y.v < 0.5 * EM_FLOOR
    assert (below | (y.v > 2 * EM_FLOOR)).all(), "an unclamped one-step value lies within a factor 2 of the floor: change the input"
    return np.where(below, np.float32(EM_FLOOR).astype(F64), y.v), y.m, below


EM_DEFECTS_FWD = ("noise_row_of_previous_chunk", "partial_group_last_path_reads_path_0")
EM_DEFECTS_BWD = ("clamp_test_on_x_t", "g_x0_without_g_traj_0")


def em_simulate(c, dtype=np.float32, defect=None):
    """Free-running trajectory [B, T + 1, S] in ``dtype`` (the forward kernels' arithmetic, vectorised over the paths)."""
    B, T, S, ch = c["B"], c["T"], c["S"], c["ch"]
    noise = np.asarray(c["noise"], dtype).copy()
    if defect == "partial_group_last_path_reads_path_0" and B % EM_PATHS:
        noise[B - 1] = noise[(B - 1) // EM_PATHS * EM_PATHS]
    traj = np.empty((B, T + 1, S), dtype)
    traj[:, 0] = c["x0"]
    floor = dtype(EM_FLOOR)
    for t in range(T):
        row = t - 1 if (defect == "noise_row_of_previous_chunk" and t > 0 and t % ch == 0) else t
        y = em_step(c["name"], traj[:, t], c["theta"], noise[:, row], c["dt"], dtype).v
        traj[:, t + 1] = np.where(y < floor, floor, y)
    return traj


def em_adjoint(c, traj, dtype=F64, defect=None):
    """Reverse recursion on the GIVEN trajectory (a clamped entry == float32(1e-6) passes no gradient): (g_x0, g_theta) as VM."""
    B, T, S = c["B"], c["T"], c["S"]
    traj = np.asarray(traj, dtype)
    g_traj = np.asarray(c["g_traj"], dtype)
    floor = dtype(np.float32(EM_FLOOR))
    a = VM(np.zeros((B, S), dtype))
    gth = VM(np.zeros((B, c["theta"].shape[1]), dtype))
    for t in range(T - 1, -1, -1):
        a = a + VM(g_traj[:, t + 1])
        clamped = traj[:, t if defect == "clamp_test_on_x_t" else t + 1] == floor
        a = VM(np.where(clamped, 0, a.v).astype(dtype), np.where(clamped, 0, a.m).astype(dtype))
        a, g = em_step_bwd(c["name"], traj[:, t], c["theta"], c["noise"][:, t], a, c["dt"], dtype)
        gth = gth + g
    if defect != "g_x0_without_g_traj_0":
        a = a + VM(g_traj[:, 0])
    return a, gth


def em_ratios(c, traj, g_x0, g_theta):
    """(step, adjoint) worst ratios of a trajectory and its gradients against the teacher-forced float64 step and the float64
    reverse recursion on that trajectory; the clamped elements must equal float32(1e-6) exactly."""
    ref, mag, below = em_forward_check(c, traj)
    traj = np.asarray(traj)
    if not (traj[:, 0] == c["x0"]).all() or not (traj[:, 1:][below] == np.float32(EM_FLOOR)).all():
        return float("inf"), float("inf")
    step = ratio(np.where(below, ref, traj[:, 1:]), ref, mag)
    a, gth = em_adjoint(c, traj)
    return step, max(ratio(g_x0, a.v, a.m), ratio(g_theta, gth.v, gth.m))


def em_clamped_at_sites(c, traj):
    """Whether every (path, dimension) pair of ``c["hit"]`` sits on the floor at every clamp site."""
    return all(traj[b, t, d] == np.float32(EM_FLOOR) for b, d in c["hit"] for t in c["sites"])


def em_shapes():
    return [(name, B, T) for name in EM_KINDS for B in EM_BS for T in em_ts(name)]
