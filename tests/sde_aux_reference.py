"""float64 references, per-element magnitudes, bounds and test inputs of the kernels of csrc/vsde_elbo.hip and csrc/vsde_sde.hip
that tests/sde_reference.py does not cover: the importance log-weight kernel (log_weight_kernel), the coefficient kernels
(coef_fwd_kernel, coef_bwd_kernel, coef_diag_fwd_kernel, coef_diag_bwd_kernel) and the forecast kernel, plus the inputs of the
log-weight accumulator's cases.  Same style and the same machinery as tests/sde_reference.py (``VM`` pairs, ``ratio``, ``_tri``,
``tail_formulas``, ``em_step``, ``crn_coef_formula``): tests/test_sde_aux_ops_gpu.py compares the kernels with these functions,
tests/test_sde_aux_bounds.py checks on the CPU that the bounds hold for a correct float32 evaluation and reject an emulation of
the kernels' arithmetic with a defect injected.

Values.  Log weights: MultivariateNormal(scale_tril=...) and logsigmoid in float64 torch on x = softplus(z), the model's own drift /
diffusion callables, and per path the tail of ``sde_reference.tail_reference`` (Normal / LogNormal, the count likelihoods pinned
to tests/count_likelihood_reference.py).  Coefficients and their vector-Jacobian product: the package's SDE classes
(OrnsteinUhlenbeck, LotkaVolterra, LinearDiagonalSDE, ReactionNetworkSDE(rate_laws=...)) in float64 torch with autograd.  A
rate-law network is differentiated with respect to the effective constants rates [B, 2R] the kinetic entry points take, not with
respect to theta through the map, and the derivatives of its Hill factor are written out (``sde_reference._HillFactor``, pinned to
the package's autograd): autograd through the quotient leaves rounding noise where they are exactly zero (modifier at 0), and the
bound holds the kernels to the exact zero there.  Forecast: teacher-forced like the simulator; with every step requested the
kernel returns its whole trajectory, and the reference of row t + 1 is ``em_step(x_t of the kernel, theta, z_ref[t])`` in float64
with z_ref the numpy Philox / Box-Muller stream (tests/philox_reference.py), followed by the floor on the positive dims.
max(., floor) is 1-Lipschitz: no element near the floor is excused.

Magnitudes.  log_w[b]: the sum over t of the three per-step magnitudes plus the per-sample magnitudes of obs, prior and post from
``tail_formulas``; x = softplus(z) carries its value, and the in-kernel drift / diffusion are not leaves: the sde term is taken with
(f, G) as leaves plus, to first order, what their own rounding moves it by (``lw_formulas``).  The forward formulas of kinds 1..4
are written out on VM pairs (``coef_formulas``; the Hill / Michaelis-Menten factor of a rate law is a quotient of positive terms,
so its magnitude is its value).  The VJP of kinds 1..3 is written out (``coef_vjp_formulas``): g_theta is the sum over t of the
per-step magnitudes, g_x[t] the per-step magnitude, and g_x[T] has magnitude zero, so the kernel must write an exact zero there.
The VJP of kind 4 takes sum |g| |J| with the Jacobians J of (f, G) from autograd -- the convention ``em_adjoint`` uses for kind 4,
with its own constant for the same reason.  The forecast step's magnitude is the one ``em_step`` / ``crn_step_formula`` produce
with z_ref as a leaf: the kernel makes its normals in fp32 (logf, sqrtf, sincospif), a few ulps of z that the |G| |z| sqrt(dt) term
absorbs, which is why the forecast has constants of its own and not C_EM_STEP.

Bounds.  |got - ref| <= c 2^-24 magnitude per element; where the magnitude is zero the kernel's value must be exactly the
reference.  One c per family, 4 x the worst ratio of a correct float32 evaluation on the CPU (the written-out formulas in float32
for the log weights -- the C oracle sums the sde and gen terms of a path apart, the kernel and the formulas sum each step's
difference; float32 torch through the same SDE classes for the coefficients, which the oracle has in float64 only; for the
forecast a numpy-float32 Box-Muller on the reference Philox words feeding the float32 step of tests/sde_reference.py), over every
case of tests/test_sde_aux_ops_gpu.py, rounded up:

    family                           worst CPU ratio   c       worst ratio on an MI355X
    log weight, Gaussian               6.88             28       3.61
    log weight, count                  1.06              4.5     0.86
    coefficient forward (kinds 1..4)   3.31             13.5     3.31
    coefficient VJP (kinds 1..3)       4.46             18       5.40
    coefficient VJP (kind 4)          20.54             83      30.48
    forecast step (kinds 1..3)         6.22             25       4.81
    forecast step (kind 4)             4.41             18       4.59
    the kind-4 sweep (every <4, S, NR, KIN>, tests/sde_sweep_reference.py, on the cases of tests/test_sde_sweep_gpu.py):
    log weight                         0.37             28       0.33
    coefficient forward, mass action   3.07             13.5     3.07
    coefficient forward, rate laws     3.98             16       3.98     (C_COEF_FWD_KIN of the sweep's module)
    coefficient VJP                   12.44             83      12.95
    forecast step                      3.31             18       3.23

tests/test_sde_aux_bounds.py asserts that the CPU ratios stay within c / 4.

Inputs.  Log weights take z, means, chol (kind 0: drift, diffusion) from ``sde_reference.path_case`` -- saturated z on rows 1..5 of
path 0, NaN above the diagonals; a network's latent path stays near 1 instead (``lw_case``), and every third Lotka-Volterra path
holds z = -30 on the prey (and on the predator in its second half) so that both radicands of the factor are floored decisively; a
cell of the kind-4 sweep takes a trajectory of its own network and the quadratic form to first order (``lw_case``, ``lw_formulas``);
obs_rows holds row 0, a repeated row, row T and a row above T, which the kernel clamps to T.  Lotka-Volterra coefficient rows
cycle over t through u = 0 (with v = 1e-9 on every other such row, which floors the second radicand too), u = 1e-9 (first radicand
below half the floor) and both populations >= 1; every quantity a floor or a clamp gate tests is below half the floor or above
twice it (asserted on the float64 reference, no element is excused; the same for the Cholesky radicands of the networks).
Linear-diagonal theta holds one b_i = 25 (the softplus threshold branch) and one b_i = -25.  The clamp2 network puts its modifier
at 0 (the gradient passes), below 0 (h at u = 0, no gradient) and above.  Row T of x, which no coefficient kernel may read, is NaN,
as is the strict upper triangle of g_diffusion.  Forecast states start at U(0, 1e-3) on positive dims so that the floor is reached
(of a network: one species, see ``fc_gates_ok``), and one path of every case with more than one starts at NaN.
"""
import functools

import numpy as np
import torch

import sde_reference as R
from philox_reference import _uniform, forecast_noise, philox4x32_10
from sde_reference import C24, EM_FLOOR, F64, VM, ratio, vm_max, vm_sqrt, vm_stack

F32 = np.float32
FLOOR32 = float(np.float32(EM_FLOOR))

# c per family: 4 x the measured CPU ratio, rounded up (see the table above)
C_COEF_FWD = 13.5
C_COEF_VJP = 18.0
C_COEF_VJP_CRN = 83.0      # kind 4: the magnitudes of its VJP are |g| |J| with J from autograd, blind to the cancellation inside J
C_FC_STEP = 25.0
C_FC_STEP_CRN = 18.0
C_LW = 28.0
C_LW_COUNT = 4.5

# case name -> (kernel kind, S); the model of a name is what em_step / crn_sde know it as
class _Kinds(dict):
    """A cell of the kind-4 sweep (tests/sde_sweep_reference.py) is looked up by its name, e.g. ``sw-S5-NR4-k``, and is not listed."""

    def __missing__(self, name):
        if not R.is_sweep(name):
            raise KeyError(name)
        return R.EM_KINDS[name][:2]


KINDS = _Kinds({"ou": ("ornstein_uhlenbeck", 1), "lv": ("lotka_volterra", 2), "diag1": ("linear_diagonal", 1), "diag5": ("linear_diagonal", 5),
                "diag8": ("linear_diagonal", 8), "diag32": ("linear_diagonal", 32), "sir": ("reaction_network", 2),
                "net3": ("reaction_network", 3), "chain8": ("reaction_network", 8), "autoreg": ("reaction_network", 2),
                "repress3": ("reaction_network", 3), "chain8k": ("reaction_network", 8), "clamp2": ("reaction_network", 2)})


def model(name):
    return "diag" if name.startswith("diag") else name


def is_crn(name):
    return R.is_sweep(name) or KINDS.get(name, ("", 0))[0] == "reaction_network"


def param_dim(name):
    S = KINDS[name][1]
    return R.crn_sde(name).rate_dim if is_crn(name) else 2 * S if model(name) == "diag" else 3


def network(name):
    """What the wrappers take as ``network``: the descriptor of a mass-action network, the kinetic route of one with rate laws."""
    return R.crn_sde(name).kernel_descriptor() if is_crn(name) else None


@functools.lru_cache(maxsize=None)
def spec_sde(name):
    from viforsdes_amd.examples.sdes import LinearDiagonalSDE, LotkaVolterra, OrnsteinUhlenbeck
    if is_crn(name):
        return R.crn_sde(name)
    return {"ou": OrnsteinUhlenbeck, "lv": LotkaVolterra}[name]() if name in ("ou", "lv") else LinearDiagonalSDE(KINDS[name][1])


def _seed(name, B, T):
    return 977 * B + 13 * T + sum(map(ord, name))


def _theta(name, rng, B):
    """Parameters as ``sde_reference.em_case`` draws them; a rate-law network: its effective constants [B, 2R] in float32."""
    S = KINDS[name][1]
    if name == "ou":
        return np.stack([rng.uniform(0.5, 1.0, B), rng.standard_normal(B), rng.uniform(0.3, 0.6, B)], 1)
    if name == "lv":
        return np.array([0.8, 0.0025, 0.3]) * (1 + 0.1 * rng.random((B, 3)))
    if R.is_sweep(name):
        return R.sweep_theta(name, rng, B)
    if name in R.CRN_KINETIC:
        sde = R.crn_sde(name)
        lo, hi = (1.0, 5.0) if name in ("repress3", "chain8k") else (0.2, 1.2)
        th = torch.tensor(rng.uniform(lo, hi, (B, sde.sde_param_dim)), dtype=torch.float32)
        return sde.rates_of(th).numpy()
    if is_crn(name):
        return rng.uniform(0.3, 0.8, (B, param_dim(name)))
    return np.concatenate([rng.uniform(0.2, 0.5, (B, S)), 0.5 * rng.standard_normal((B, S))], 1)


# ========================================================================================================== coefficients
COEF_NAMES = tuple(KINDS)
COEF_TS = (1, 255, 256, 257, 600)
COEF_OUT = ("drift", "diffusion", "g_x", "g_theta")


def coef_ts(name):
    """T restricted for the S = 8 networks (44 outputs per grid point in the reference's Jacobians) to keep them quick."""
    return (1, 257) if KINDS[name][1] == 8 and is_crn(name) else COEF_TS


def coef_shapes():
    """(name, B, T) of every coefficient case of the GPU file."""
    return [(name, B, T) for name in COEF_NAMES for B in (1, 3) for T in coef_ts(name)]


@functools.lru_cache(maxsize=8)
def coef_case(name, B, T):
    """float32 inputs of the coefficient kernels (module docstring)."""
    kind, S = KINDS[name]
    rng = np.random.default_rng(_seed(name, B, T))
    theta = _theta(name, rng, B)
    t = np.arange(T + 1)
    if name == "lv":
        x = np.stack([rng.uniform(1.0, 200.0, (B, T + 1)), rng.uniform(1.0, 400.0, (B, T + 1))], -1)
        x[:, t % 3 == 0, 0] = 0.0
        x[:, t % 6 == 0, 1] = 1e-9
        x[:, t % 3 == 1, 0] = 1e-9
    elif name in ("repress3", "chain8k"):
        x = rng.uniform(2.0, 40.0, (B, T + 1, S))
    elif name in ("autoreg", "clamp2"):
        x = rng.uniform(0.5, 3.0, (B, T + 1, S))
        if name == "clamp2":
            x[:, :, 0] = np.array([0.0, -0.7, 0.0, 1.3])[t % 4]
    elif R.is_sweep(name):
        x = R.sweep_states(name, rng, (B, T + 1))
    elif is_crn(name):
        x = rng.uniform(1.6, 2.4, (B, T + 1, S))
    else:
        x = rng.standard_normal((B, T + 1, S))
    if model(name) == "diag":
        theta[0, S] = 25.0
        if B * S > 1:
            theta[B - 1, 2 * S - 1] = -25.0
    x[:, T] = np.nan
    g_diff = rng.standard_normal((B, T, S, S))
    if R.is_sweep(name):
        g_diff[..., R.sweep_zeroed(name)] = 0.0            # the columns of the floored pivots of a cell with two or more of them
    up = np.triu_indices(S, 1)
    g_diff[..., up[0], up[1]] = np.nan
    f = lambda a: np.asarray(a, F32)
    c = dict(name=name, kind=kind, S=S, B=B, T=T, P=theta.shape[1], x=f(x), theta=f(theta), g_drift=f(rng.standard_normal((B, T, S))),
             g_diffusion=f(g_diff))
    for g in coef_gates(c):
        assert ((g.v < 0.5 * EM_FLOOR) | (g.v > 2 * EM_FLOOR)).all(), "a gated quantity lies within a factor 2 of the floor: change the input"
    return c


def _lv_factor(u, v, t1, t2, t3):
    """The Lotka-Volterra Cholesky factor with its two floors as coef_fwd<2> has it: (uv, q00r, l00, c, l10, q11r, l11) as VM."""
    uv = t2 * u * v
    q00r = t1 * u + uv
    l00 = vm_sqrt(vm_max(q00r, EM_FLOOR))
    c = vm_max(l00, EM_FLOOR)
    l10 = -uv / c
    q11r = t3 * v + uv - l10 * l10
    return uv, q00r, l00, c, l10, q11r, vm_sqrt(vm_max(q11r, EM_FLOOR))


def _coef_args(c, dtype):
    return (VM(np.asarray(c["x"], dtype)[:, :-1]), VM(np.asarray(c["theta"], dtype)[:, None, :]), VM(np.asarray(c["g_drift"], dtype)),
            VM(np.nan_to_num(np.asarray(c["g_diffusion"], dtype), nan=0.0)))


def coef_gates(c):
    """float64 VM of everything a floor or a clamp gate of the case's kernels tests."""
    x, th, _, _ = _coef_args(c, F64)
    if c["name"] == "lv":
        _, q00r, l00, _, _, q11r, _ = _lv_factor(x[..., 0], x[..., 1], th[..., 0], th[..., 1], th[..., 2])
        return [q00r, l00, q11r]
    return R.crn_coef_formula(c["name"], x.v, th.v)[2] if is_crn(c["name"]) else []


def coef_formulas(c, dtype=F64):
    """Drift [B, T, S] and diffusion factor [B, T, S, S] of kinds 1..4 written out on VM pairs in ``dtype``."""
    name, S = c["name"], c["S"]
    x, th = VM(np.asarray(c["x"], dtype)[:, :-1]), VM(np.asarray(c["theta"], dtype)[:, None, :])
    zero = VM(np.zeros(x.v.shape[:2], dtype))
    G = [[zero] * S for _ in range(S)]
    if name == "ou":
        f = [th[..., 0] * (th[..., 1] - x[..., 0])]
        G[0][0] = th[..., 2] + zero
    elif name == "lv":
        u, v, t1, t3 = x[..., 0], x[..., 1], th[..., 0], th[..., 2]
        uv, _, l00, _, l10, _, l11 = _lv_factor(u, v, t1, th[..., 1], t3)
        f = [t1 * u - uv, uv - t3 * v]
        G[0][0], G[1][0], G[1][1] = l00, l10, l11
    elif is_crn(name):
        f, L, _ = R.crn_coef_formula(name, x.v, th.v, dtype)
        for i in range(S):
            for k in range(i + 1):
                G[i][k] = L[i][k]
    else:
        f = [-th[..., i] * x[..., i] for i in range(S)]
        for i in range(S):
            G[i][i] = VM(R._softplus(th.v[..., S + i])) + dtype(1e-3) + zero
    out = {"drift": vm_stack(f), "diffusion": vm_stack([vm_stack(row) for row in G], -2)}
    for k, a in out.items():
        assert a.v.dtype == dtype and a.m.dtype == dtype, (k, a.v.dtype, a.m.dtype)
    return out


COEF_DEFECTS = {"g_x_row_T_unwritten": COEF_NAMES, "rows_from_256_missing_from_g_theta": COEF_NAMES,
                "diag_last_partial_slot_dropped": ("diag5",), "diag_sigmoid_factor_missing": ("diag5",),
                "lv_q11_gate_always_open": ("lv",), "lv_d_l10_term_missing": ("lv",), "kinetic_K_gradient_one_column_low": ("autoreg",)}


def coef_vjp_formulas(c, dtype=F64, defect=None):
    """g_x [B, T + 1, S] and g_theta [B, P] of kinds 1..3 written out on VM pairs in ``dtype``, with the kernels' sum over t."""
    name, S, B, T = c["name"], c["S"], c["B"], c["T"]
    x, th, gf, gG = _coef_args(c, dtype)
    zero = VM(np.zeros((B, T), dtype))
    if name == "ou":
        gx = [-gf[..., 0] * th[..., 0]]
        gth = [gf[..., 0] * (th[..., 1] - x[..., 0]), gf[..., 0] * th[..., 0], gG[..., 0, 0] + zero]
    elif name == "lv":
        u, v, t1, t2, t3 = x[..., 0], x[..., 1], th[..., 0], th[..., 1], th[..., 2]
        uv, q00r, l00, cc, l10, q11r, l11 = _lv_factor(u, v, t1, t2, t3)
        d_l00, d_l10 = gG[..., 0, 0], gG[..., 1, 0]
        d_q11 = gG[..., 1, 1] / (2.0 * l11)
        if defect != "lv_q11_gate_always_open":
            d_q11 = d_q11.where(q11r.v >= EM_FLOOR, zero)
        d_t3, d_v, d_uv = d_q11 * v, d_q11 * t3, d_q11
        if defect != "lv_d_l10_term_missing":
            d_l10 = d_l10 + (-2.0 * l10) * d_q11
        d_uv = d_uv + (-d_l10) / cc
        d_l00 = (d_l00 + d_l10 * uv / (cc * cc)).where(l00.v >= EM_FLOOR, d_l00)
        d_q00 = (d_l00 / (2.0 * l00)).where(q00r.v >= EM_FLOOR, zero)
        d_t1, d_u, d_uv = d_q00 * u, d_q00 * t1, d_uv + d_q00
        d_t1, d_u, d_uv = d_t1 + gf[..., 0] * u, d_u + gf[..., 0] * t1, d_uv - gf[..., 0]
        d_uv, d_t3, d_v = d_uv + gf[..., 1], d_t3 - gf[..., 1] * v, d_v - gf[..., 1] * t3
        gx = [d_u + d_uv * t2 * v, d_v + d_uv * t2 * u]
        gth = [d_t1, d_uv * u * v, d_t3]
    else:
        b = th.v[..., S:]
        sg = VM(np.where(b > 20, 1.0, R._sigmoid(b)).astype(dtype))              # F.softplus passes the gradient unchanged above 20
        if defect == "diag_sigmoid_factor_missing":
            sg = VM(np.ones_like(sg.v))
        gx = [-gf[..., i] * th[..., i] for i in range(S)]
        gth = [-(gf[..., i] * x[..., i]) for i in range(S)] + [gG[..., i, i] * sg[..., i] for i in range(S)]
    keep = np.ones(T, bool)
    if defect == "rows_from_256_missing_from_g_theta":
        keep[256:] = False
    if defect == "diag_last_partial_slot_dropped":
        slots = 256 // S
        keep[(T + 1) // slots * slots:] = False
    gx = vm_stack(gx)
    last = np.full((B, 1, S), 1.0 if defect == "g_x_row_T_unwritten" else 0.0, dtype)
    out = {"g_x": VM(np.concatenate([gx.v, last], 1), np.concatenate([gx.m, np.zeros((B, 1, S), dtype)], 1)),
           "g_theta": vm_stack(gth)[:, keep].sum(1)}
    for k, a in out.items():
        assert a.v.dtype == dtype and a.m.dtype == dtype, (k, a.v.dtype, a.m.dtype)
    return out


def _coef_torch(c, dtype):
    """(x [B, T, S], theta expanded to [B, T, P]) as leaves, and (f, G) of the package's SDE class on the flattened grid."""
    sde = spec_sde(c["name"])
    B, T, S = c["B"], c["T"], c["S"]
    x = torch.tensor(np.asarray(c["x"])[:, :-1], dtype=dtype, requires_grad=True)
    th = torch.tensor(np.asarray(c["theta"]), dtype=dtype)[:, None, :].expand(B, T, -1).contiguous().requires_grad_(True)
    xf, tf = x.reshape(B * T, S), th.reshape(B * T, -1)
    return x, th, sde.drift(xf, tf).reshape(B, T, S), sde.diffusion(xf, tf).reshape(B, T, S, S)


def coef_reference(c, dtype=torch.float64, g_scale=None):
    """{drift, diffusion, g_x, g_theta} from the package's SDE classes and autograd in ``dtype`` (float32: the correct float32
    evaluation); ``g_scale`` [T] scales the upstream gradients per step (the emulation's defects)."""
    x, th, f, G = _coef_torch(c, dtype)
    gf = torch.tensor(np.asarray(c["g_drift"]), dtype=dtype)
    gG = torch.tensor(np.nan_to_num(np.asarray(c["g_diffusion"]), nan=0.0), dtype=dtype)
    if g_scale is not None:
        s = torch.tensor(g_scale, dtype=dtype)
        gf, gG = gf * s[None, :, None], gG * s[None, :, None, None]
    gx, gth = torch.autograd.grad((f * gf).sum() + (G * gG).sum(), [x, th])
    gx = torch.cat([gx, torch.zeros(c["B"], 1, c["S"], dtype=dtype)], 1)
    return {"drift": f.detach().numpy(), "diffusion": G.detach().numpy(), "g_x": gx.numpy(), "g_theta": gth.sum(1).numpy()}


def _crn_vjp_magnitudes(c):
    """Kind 4: sum over the outputs o of |g_o| |d o / d x| per step and of |g_o| |d o / d rates| over the steps."""
    x, th, f, G = _coef_torch(c, torch.float64)
    S = c["S"]
    gf = np.abs(np.asarray(c["g_drift"], F64))
    gG = np.abs(np.nan_to_num(np.asarray(c["g_diffusion"], F64), nan=0.0))
    mx, mt = np.zeros(tuple(x.shape)), np.zeros(tuple(th.shape))
    outs = [(f[..., i], gf[..., i]) for i in range(S)] + [(G[..., i, k], gG[..., i, k]) for i in range(S) for k in range(i + 1)]
    for o, g in outs:
        jx, jt = torch.autograd.grad(o.sum(), [x, th], retain_graph=True, allow_unused=True)
        if jx is not None:
            mx += g[..., None] * np.abs(jx.numpy())
        if jt is not None:
            mt += g[..., None] * np.abs(jt.numpy())
    return np.concatenate([mx, np.zeros((c["B"], 1, S))], 1), mt.sum(1)


@functools.lru_cache(maxsize=8)
def _coef_ref_mag(name, B, T):
    c = coef_case(name, B, T)
    ref = coef_reference(c)
    mag = {k: a.m for k, a in coef_formulas(c).items()}
    if is_crn(name):
        mag["g_x"], mag["g_theta"] = _crn_vjp_magnitudes(c)
    else:
        mag.update({k: a.m for k, a in coef_vjp_formulas(c).items()})
    return ref, mag


def coef_ratios(c, got):
    """(forward, VJP) worst ratios of ``got`` {name: array} against the float64 reference of case ``c``."""
    ref, mag = _coef_ref_mag(c["name"], c["B"], c["T"])
    worst = lambda names: max([ratio(got[k], ref[k], mag[k]) for k in names if k in got], default=0.0)
    return worst(COEF_OUT[:2]), worst(COEF_OUT[2:])


def coef_vjp_c(name):
    return C_COEF_VJP_CRN if is_crn(name) else C_COEF_VJP


def coef_emulated(c, defect=None):
    """A float32 emulation of the kernels' arithmetic: the written-out formulas in float32 (kind 4, which has no written-out VJP:
    float32 torch), with a defect of COEF_DEFECTS injected."""
    B, T, S, name = c["B"], c["T"], c["S"], c["name"]
    if not is_crn(name):
        out = {k: a.v for k, a in coef_formulas(c, F32).items()}
        out.update({k: a.v for k, a in coef_vjp_formulas(c, F32, defect).items()})
        return out
    scale = None
    if defect == "rows_from_256_missing_from_g_theta":
        scale = (np.arange(T) < 256).astype(F64)
    out = coef_reference(c, torch.float32, scale)
    if scale is not None:                        # g_x is written for every row: only g_theta loses the rows
        out["g_x"] = coef_reference(c, torch.float32)["g_x"]
    if defect == "g_x_row_T_unwritten":
        out["g_x"][:, T] = 1.0
    if defect == "kinetic_K_gradient_one_column_low":
        Rn = c["P"] // 2
        g = out["g_theta"].copy()
        out["g_theta"][:, Rn - 1:2 * Rn - 1] = g[:, Rn:]
        out["g_theta"][:, 2 * Rn - 1] = 0.0                 # never written; column R - 1 now holds the gradient of K_0
    return out


# ============================================================================================================== forecast
FC_TS = (1, 3, 4, 5, 8, 9)
# (name, B, positive-dim mask) of the forecast cases; "ou0": kappa = 0 from x = 0, the magnitude of step 1 is sigma sqrt(dt) |z| alone
FC_CASES = ([("ou", B, "none" if B != 255 else "all") for B in (1, 255, 256, 257)] + [("lv", B, "all") for B in (1, 255, 256, 257)]
            + [("ou0", 257, "none"), ("diag5", 51, "alt"), ("diag5", 52, "all"), ("diag32", 9, "none"), ("diag32", 9, "all"),
               ("diag32", 9, "last"), ("diag1", 257, "all"), ("sir", 65, "all"), ("net3", 65, "all"), ("chain8", 65, "all"),
               ("autoreg", 65, "all")])
FC_SUBSETS = ((9,), (1,), (1, 4, 5), (4, 4, 8), (9, 9))      # at T = 9: [T], the early exit, a block seam, duplicates on a block's
                                                             # last step, steps in the last partial block only


FC_SMALL_SPECIES = {"sir": 0, "net3": 2, "chain8": 7, "autoreg": 1}


def fc_model(name):
    return "ou" if name == "ou0" else name


def fc_shapes():
    """(name, B, T, mask) of every forecast case of the GPU file."""
    return [(name, B, T, mask) for name, B, mask in FC_CASES for T in FC_TS]


def fc_c(name):
    return C_FC_STEP_CRN if is_crn(fc_model(name)) else C_FC_STEP


@functools.lru_cache(maxsize=None)
def fc_case(name, B, T, mask):
    """float32 inputs of the forecast kernel and the float64 reference normals z_ref [B, T, S] of its key."""
    m = fc_model(name)
    kind, S = KINDS[m]
    rng = np.random.default_rng(_seed(name, B, T) + 5)
    theta = _theta(m, rng, B)
    pos = R.positive_dims(mask, S)
    if m == "lv":
        x0 = np.array([120.0, 200.0]) * (0.9 + 0.2 * rng.random((B, 2)))
    elif m in ("autoreg",):
        x0 = rng.uniform(0.5, 3.0, (B, S))
    elif R.is_sweep(m):
        x0 = R.sweep_states(m, rng, (B,))
    elif is_crn(m):
        x0 = rng.uniform(1.6, 2.4, (B, S))
    else:
        x0 = rng.standard_normal((B, S))
    small = rng.uniform(0.0, 1e-3, (B, S))
    # kinds 2 and 4: every other path starts small, and of a network only the species of FC_SMALL_SPECIES (every Cholesky radicand
    # then either stays clear of its floor or is a sum of like-signed terms: see fc_gates_ok)
    rows = np.arange(B) % 2 == 0 if (m == "lv" or is_crn(m)) else np.ones(B, bool)
    for i in ([R.sweep_hit_dim(m)] if R.is_sweep(m) else [FC_SMALL_SPECIES[m]] if is_crn(m) else pos):
        x0[rows, i] = small[rows, i]
    if name == "ou0":
        theta[:, 0], theta[:, 1], x0[:] = 0.0, 0.0, 0.0
    nan_path = B // 2 if B > 1 else None
    if nan_path is not None:
        x0[nan_path] = np.nan
    key = (0x9E3779B9 ^ (131 * B + T), (0x7F4A7C15 + sum(map(ord, name))) & 0xFFFFFFFF)
    f = lambda a: np.asarray(a, F32)
    return dict(name=name, model=m, kind=kind, S=S, B=B, T=T, P=theta.shape[1], mask=mask, pos=pos, dt=0.05 if is_crn(m) else 0.1,
                x0=f(x0), theta=f(theta), key=key, nan_path=nan_path, z_ref=forecast_noise(B, T, S, key))


def fc_check(c, traj):
    """Teacher-forced float64 one-step values from the GIVEN trajectory [B, T + 1, S] (row 0: x_start): (ref [B, T, S] after the
    floor on the positive dims, magnitude)."""
    traj = np.asarray(traj, F64)
    y = R.em_step(c["model"], traj[:, :-1], np.asarray(c["theta"], F64)[:, None, :], c["z_ref"], c["dt"])
    ref = y.v.copy()
    for i in c["pos"]:
        ref[..., i] = np.where(ref[..., i] < FLOOR32, FLOOR32, ref[..., i])
    return ref, y.m


def fc_gates_ok(c, out):
    """Whether every quantity an inner floor of the step tests (the Cholesky radicands of kinds 2 and 4), on the float64 step from
    the GIVEN states, is below half the floor, above twice it, or free of cancellation (magnitude <= 2 |value|: a sum of
    like-signed terms, whose rounding error is a few ulps of the floor itself, so that a float32 evaluation that lands on the other
    side of the floor moves the result by no more than the magnitude ``vm_max`` gives it)."""
    keep = np.arange(c["B"]) != (-1 if c["nan_path"] is None else c["nan_path"])
    x = np.concatenate([c["x0"][:, None, :], np.asarray(out)], 1)[keep][:, :-1].astype(F64)
    th = VM(np.asarray(c["theta"], F64)[keep][:, None, :])
    if c["model"] == "lv":
        _, q00r, l00, _, _, q11r, _ = _lv_factor(VM(x[..., 0]), VM(x[..., 1]), th[..., 0], th[..., 1], th[..., 2])
        gates = [q00r, l00, q11r]
    elif is_crn(c["model"]):
        gates = R.crn_coef_formula(c["model"], x, th.v)[2]
    else:
        return True
    return all(((g.v < 0.5 * EM_FLOOR) | (g.v > 2 * EM_FLOOR) | (g.m <= 2 * np.abs(g.v))).all() for g in gates)


def fc_ratio(c, out):
    """Worst ratio of the all-steps output ``out`` [B, T, S] against the teacher-forced float64 step; the path started at NaN must
    be NaN throughout and is left out of the ratio (inf otherwise)."""
    out = np.asarray(out)
    keep = np.arange(c["B"]) != (-1 if c["nan_path"] is None else c["nan_path"])
    if not np.isnan(out[~keep]).all():
        return float("inf")
    traj = np.concatenate([c["x0"][:, None, :], out], 1)[keep]
    sub = dict(c, theta=c["theta"][keep], z_ref=c["z_ref"][keep])
    ref, mag = fc_check(sub, traj)
    return ratio(traj[:, 1:], ref, mag)


def fc_noise32(c, swap_dim_and_path=False):
    """The kernel's normals in float32: Box-Muller in numpy float32 on the reference Philox words (log, sqrt and the product in
    float32; sincospi of the exact 2 u correctly rounded, as a float32 sincospif is to within an ulp)."""
    B, T, S = c["B"], c["T"], c["S"]
    k0, k1 = (int(v) & 0xFFFFFFFF for v in c["key"])
    nblk = (T + 3) // 4
    blk, i, b = np.meshgrid(np.arange(nblk), np.arange(S), np.arange(B), indexing="ij")
    w = philox4x32_10(blk, b, i, 0, k0, k1) if swap_dim_and_path else philox4x32_10(blk, i, b, 0, k0, k1)

    def pair(wa, wb):
        r = np.sqrt(F32(-2.0) * np.log(_uniform(wa)))
        ang = np.pi * (F32(2.0) * _uniform(wb)).astype(F64)
        assert r.dtype == F32
        return r * np.cos(ang).astype(F32), r * np.sin(ang).astype(F32)

    z = np.stack([*pair(w[0], w[1]), *pair(w[2], w[3])], axis=1).reshape(nblk * 4, S, B)
    assert z.dtype == F32
    return np.ascontiguousarray(z.transpose(2, 0, 1))          # [B, 4 nblk, S]: the normals of the last block's unused steps too


FC_DEFECTS = {"row_selection_off_by_one_in_block": ("ou", "lv", "diag5"), "normals_of_block_reused_for_next": ("ou", "lv", "diag5", "net3"),
              "word_pairs_swapped": ("ou", "lv", "diag5", "net3"), "dim_and_path_swapped_in_counter": ("lv", "diag5", "net3"),
              "floor_on_a_non_positive_dim": ("ou", "diag5"), "diag_b_read_at_next_dim": ("diag5",)}


def fc_simulate(c, dtype=F32, defect=None):
    """Free-running forecast in ``dtype`` from float32 Box-Muller normals: the all-steps output [B, T, S] (the kernel's
    arithmetic, vectorised over the paths), with a defect of FC_DEFECTS injected."""
    B, T, S = c["B"], c["T"], c["S"]
    z = fc_noise32(c, defect == "dim_and_path_swapped_in_counter").astype(dtype)
    n = z.shape[1]
    if defect == "normals_of_block_reused_for_next":
        z = np.tile(z[:, :4], (1, n // 4, 1))
    if defect == "word_pairs_swapped":
        z = z.reshape(B, n // 4, 4, S)[:, :, [2, 3, 0, 1]].reshape(B, n, S)
    theta = np.asarray(c["theta"], dtype).copy()
    if defect == "diag_b_read_at_next_dim":
        theta[:, S:] = np.roll(theta[:, S:], -1, axis=1)
    pos = list(range(S)) if defect == "floor_on_a_non_positive_dim" else c["pos"]
    floor = dtype(FLOOR32)
    xs = np.empty((B, n + 1, S), dtype)
    xs[:, 0] = c["x0"]
    with np.errstate(invalid="ignore"):
        for t in range(n):
            y = R.em_step(c["model"], xs[:, t], theta, z[:, t], c["dt"], dtype).v
            for i in pos:
                y[..., i] = np.where(y[..., i] < floor, floor, y[..., i])
            xs[:, t + 1] = y
    if defect == "row_selection_off_by_one_in_block":
        rows = [t + 1 if (t - 1) % 4 < 3 else t for t in range(1, T + 1)]
        return xs[:, rows]
    return xs[:, 1:T + 1]


# =========================================================================================================== log weights
# log_w[b] = obs + sum_t (sde_t - gen_t + jac_t) + prior - post.  x = softplus(z) on the positive dims and the in-kernel drift /
# diffusion are not leaves: their magnitudes (``coef_formulas``) propagate into the sde term through ``sde_reference._tri``.
LW_MODELS = {"k0": None, "diag": "linear_diagonal", "ou": "ornstein_uhlenbeck", "lv": "lotka_volterra", "sir": "reaction_network",
             "net3": "reaction_network", "chain8": "reaction_network", "autoreg": "reaction_network", "repress3": "reaction_network",
             "chain8k": "reaction_network"}
LW_OBS = ("id", "wide", "narrow")
LW_TMASKS = ("none", "all", "last")
LW_KS = (0, 1, 5)


def lw_shapes():
    """(model, S, B, T, state mask, K, obs, theta mask, lognormal, count) of every log-weight case of the GPU file."""
    vary = lambda n: (R.PATH_MASKS[n % 4], LW_KS[n % 3], LW_OBS[(n // 2) % 3], LW_TMASKS[(n // 3) % 3], n % 2)
    out = [("k0", S, 2, 257) + vary(S) + (None,) for S in range(1, 17)]
    # kind 3 has P = 2 S parameters and the tail takes P <= 16: S = 9..16 of its dispatch are refused by the host check
    out += [("diag", S, 2, 257) + vary(S + 1) + (None,) for S in range(1, 9)]
    out += [("ou", 1, 3, 257, "all", 5, "wide", "last", 0, None), ("ou", 1, 1, 600, "none", 1, "id", "none", 1, None),
            ("lv", 2, 3, 257, "all", 5, "id", "all", 1, None), ("lv", 2, 1, 600, "all", 5, "narrow", "last", 1, None)]
    for n, m in enumerate(("sir", "net3", "chain8", "autoreg", "repress3", "chain8k")):
        out.append((m, KINDS[m][1], 2, 257, "all", LW_KS[(n + 1) % 3], LW_OBS[n % 3], LW_TMASKS[(n + 1) % 3], n % 2, None))
    out += [("k0", 2, 3, 257, "alt", 5, "id", "all", 1, "poisson"), ("k0", 3, 3, 257, "none", 5, "wide16", "last", 0, "negbin"),
            ("lv", 2, 3, 257, "all", 5, "id", "all", 1, "poisson"), ("net3", 3, 2, 257, "all", 5, "wide16", "none", 0, "negbin")]
    n = 0
    for S in (1, 2, 16):
        for T in (1, 2, 255, 256, 257, 600):
            for B in (1, 3):
                out.append(("k0", S, B, T) + vary(n) + (None,))
                n += 1
    return out


def lw_rows(K, T):
    """obs_rows: row 0, a repeated row, row T, and one above T that the kernel clamps to T."""
    return {0: [], 1: [T], 5: [0, T // 2, T // 2, T, T + 3]}[K]


@functools.lru_cache(maxsize=None)
def lw_sde(model, S):
    from viforsdes_amd.examples.sdes import LinearDiagonalSDE, LotkaVolterra, OrnsteinUhlenbeck
    return (LinearDiagonalSDE(S) if model == "diag" else OrnsteinUhlenbeck() if model == "ou" else LotkaVolterra() if model == "lv"
            else R.crn_sde(model))


LW_SWEEP_NOISE = 0.5


@functools.lru_cache(maxsize=8)
def lw_case(model, S, B, T, smask, K, obs, tmask, lognormal, count):
    """float32 inputs of the log-weight kernel: z, means, chol (and for kind 0 drift, diffusion) of ``sde_reference.path_case``
    (saturated z on rows 1..5 of path 0, NaN above the diagonals); Lotka-Volterra: every third path has z = -30 on the prey
    throughout and on the predator in the second half, so both radicands of its Cholesky factor are floored decisively."""
    pc = R.path_case(S, B, T, smask)
    rng = np.random.default_rng(_seed(model, B, T) + 31 * S + K)
    z = pc["z"].copy()
    if model == "lv":
        z[::3, :, 0] = -30.0
        z[::3, (T + 1) // 2:, 1] = -30.0
    if is_crn(model):
        # a network's latent path stays near 1 (x in about [0.7, 2]), without the saturated rows (kinds 0..3 carry them): where a
        # species nearly vanishes or dwarfs the others, Sigma is close to singular, the Cholesky factor cancels for real, and the
        # magnitude of that one step would swamp the path's sum
        z = (1.0 + 0.2 * rng.standard_normal(z.shape)).astype(F32)
    rates = None
    dt = pc["dt"]
    if R.is_sweep(model):
        # the tail takes P <= 16 and reads theta for the prior / posterior terms alone: a rate-law cell's drift and diffusion read
        # ``rates``, so its theta is cut to 16 columns where the network has 17 parameters (S 2, R 16)
        sde = R.crn_sde(model)
        theta = (sde.base_theta * (1 + R.SWEEP_JITTER * rng.uniform(-1, 1, (B, len(sde.base_theta))))).astype(F32)
        full = theta
        if not sde.plain:
            rates, theta = sde.rates_of(torch.tensor(theta)).numpy(), theta[:, :16]
        # a cell of the sweep: x is a trajectory of the network itself (float64 Euler-Maruyama from the jittered start state under
        # N(0, 1) increments, dt = 0.05) and z = softplus^-1(x), so every residual lies in the span of the factor's columns and
        # its solve is of order 1 in every direction, the floored ones included (1e-3 sqrt(dt) times a unit normal).  A path drawn
        # independently per step has residuals of order 1 along a floored direction, each divided by 1e-3: log w of -1e10, a
        # magnitude 1e7 times that, and a bound that an all-zero output meets.
        dt = 0.05
        sim = dict(name=model, B=B, T=T, S=S, ch=R.EM_KINDS[model][2], dt=dt, x0=R.sweep_states(model, rng, (B,)),
                   theta=full if rates is None else rates, noise=LW_SWEEP_NOISE * rng.standard_normal((B, T, S)))
        sim["noise"][..., R.sweep_zeroed(model)] = 0.0
        x = R.em_simulate(sim, F64)
        assert (x > 0.5).all(), "a species of the latent path nearly vanishes: change the input"
        z = (x + np.log(-np.expm1(-x))).astype(F32)
    elif model == "k0":
        theta = rng.uniform(0.1, 0.9, (B, 3))
    elif model == "diag":
        theta = np.concatenate([rng.uniform(0.2, 0.5, (B, S)), rng.uniform(0.2, 1.0, (B, S))], 1)
    elif model == "ou":
        theta = np.stack([rng.uniform(0.5, 1.0, B), rng.uniform(0.5, 1.5, B), rng.uniform(0.3, 0.6, B)], 1)
    elif model in R.CRN_KINETIC:
        sde = R.crn_sde(model)
        lo, hi = (1.0, 5.0) if model in ("repress3", "chain8k") else (0.2, 1.2)
        theta = rng.uniform(lo, hi, (B, sde.sde_param_dim)).astype(F32)
        rates = sde.rates_of(torch.tensor(theta)).numpy()
    else:
        theta = _theta(model, rng, B)
    P = theta.shape[1]
    O = S if obs == "id" else 16 if obs == "wide16" else min(16, S + 3) if obs == "wide" else max(1, S - 1)
    f = lambda a: np.asarray(a, F32)
    c = dict(model=model, kind="reaction_network" if R.is_sweep(model) else LW_MODELS[model], S=S, B=B, T=T, K=K, O=O, P=P, smask=smask, pos=pc["pos"], dt=dt, z=z,
             means=pc["means"], chol=pc["chol"], drift=pc["drift"] if model == "k0" else None,
             diffusion=pc["diffusion"] if model == "k0" else None, theta=f(theta), rates=rates, obs_rows=lw_rows(K, T),
             obs_values=f(rng.integers(0, 7, (K, O))) if count else f(rng.standard_normal((K, O)) + 1.0),
             obs_matrix=None if obs == "id" else f(0.5 * rng.standard_normal((O, S))), variance=0.3, count=count,
             theta_pos=R.positive_dims(tmask, P), lognormal=int(lognormal), prior_mean=0.2, prior_std=1.3,
             post_mean=f(0.3 * rng.standard_normal(P)), post_log_std=f(0.2 * rng.standard_normal(P) - 0.5))
    return c


LW_DEFECTS = ("steps_from_256_dropped", "last_step_dropped", "partial_sum_of_wave_3_dropped", "jac_at_z0", "obs_row_minus_one",
              "obs_rows_not_clamped", "prior_minus_post_sign_flipped", "state_mask_last_bit_ignored")
LW_DEFECTS_DIAG = ("diag_without_sqrt_dt",)
LW_DEFECTS_CRN = ("last_rate_constant_read_as_zero",)


def _lw_states(c, dtype, pos):
    z = np.asarray(c["z"], dtype)
    x = z.copy()
    x[..., pos] = R._softplus(x[..., pos])
    return z, x


def _lw_tail_case(c, x, rows, dtype):
    """The per-sample tail of the log-weight kernel as a case of ``sde_reference.tail_formulas`` / ``tail_reference``."""
    B = x.shape[0]
    zero = np.zeros(B, dtype)
    return dict(B=B, K=c["K"], S=c["S"], O=c["O"], P=c["P"], x_obs=x[:, rows], obs_values=c["obs_values"], obs_matrix=c["obs_matrix"],
                variance=c["variance"], theta=c["theta"], prior_mean=c["prior_mean"], prior_std=c["prior_std"], post_mean=c["post_mean"],
                post_log_std=c["post_log_std"], pos=c["theta_pos"], lognormal=c["lognormal"], count=c["count"], sde_lp=zero, gen_lp=zero,
                jac=zero, g_out=np.asarray(R.G_OUT, dtype))


def lw_formulas(c, dtype=F64, defect=None):
    """log_w [B] written out on VM pairs in ``dtype`` with the kernel's order of sums: each step's three terms first, then the sum
    over t, then the tail."""
    S, B, T, model = c["S"], c["B"], c["T"], c["model"]
    pos = [i for i in c["pos"] if not (defect == "state_mask_last_bit_ignored" and i == S - 1)]
    z, x = _lw_states(c, dtype, pos)
    zV, xV = VM(z), VM(x)
    dt, s = float(dtype(c["dt"])), float(dtype(np.sqrt(c["dt"])))
    if model == "k0":
        drift, diff = VM(np.asarray(c["drift"], dtype)), VM(np.asarray(c["diffusion"], dtype))
    else:
        th = np.asarray(c["theta"] if c["rates"] is None else c["rates"], dtype).copy()
        if defect == "last_rate_constant_read_as_zero":
            th[:, R.crn_sde(model).num_reactions - 1] = 0
        co = coef_formulas(dict(name=model, S=S, x=x, theta=th), dtype)
        drift, diff = co["drift"], co["diffusion"]
    raw = S - 1 if defect == "diag_without_sqrt_dt" else None
    if model == "k0":
        _, _, lps = R._tri(xV[:, 1:], xV[:, :-1], drift, diff, dt, s, S, raw)
    else:
        # in-kernel coefficients: the term with (f, G) as leaves, plus to first order what their own rounding moves it by,
        # |d lp / d f_i| (m(f_i) - |f_i|) + |d lp / d G_ij| (m(G_ij) - |G_ij|) with d lp / d f = v dt and d lp / d G_ij =
        # sqrt(dt) v_i w_j - [i = j] / G_ii.  (Running the solve itself on the pairs (G, m(G)) multiplies the inflation of every
        # Cholesky level into the next -- 10^7 of the value for a 3-species network -- and the bound would see nothing.)
        w, v, lps = R._tri(xV[:, 1:], xV[:, :-1], VM(drift.v), VM(diff.v), dt, s, S, raw)
        if R.is_sweep(model):
            # a cell of the sweep: the quadratic form to first order, |w_i| m(w_i) in place of m(w_i)^2 / 2, where that is smaller.  A
            # solve through a floored pivot has m(w_i) = 16 / (1e-3 sqrt(dt)) = 1e5 against w_i of order 1: its square is 1e10 a
            # step, where a correct evaluation's w_i^2 moves by 2 |w_i| m(w_i) roundings, and a bound made from the square holds
            # the kernel to nothing
            first = np.full((B, T), 0.5 * S * R.LOG_2PI, dtype)
            for i in range(S):
                first = first + np.abs(w[i].v) * w[i].m + np.abs(np.log(np.abs(diff.v[..., i, i] * s)))
            lps = VM(lps.v, np.minimum(lps.m, first).astype(dtype))
        extra = np.zeros((B, T), dtype)
        for i in range(S):
            extra = extra + np.abs(v[i].v) * dt * (drift.m[..., i] - np.abs(drift.v[..., i]))
            for j in range(i + 1):
                d = s * v[i].v * w[j].v - (1.0 / diff.v[..., i, i] if i == j else 0.0)
                extra = extra + np.abs(d) * (diff.m[..., i, j] - np.abs(diff.v[..., i, j]))
        lps = VM(lps.v, (lps.m + extra).astype(dtype))
    _, _, lpg = R._tri(zV[:, 1:], zV[:, :-1], VM(np.asarray(c["means"], dtype)), VM(np.asarray(c["chol"], dtype)), dt, s, S)
    jac = VM(np.zeros((B, T), dtype))
    for i in pos:
        jac = jac + VM(R._log_sigmoid(z[:, :-1, i] if defect == "jac_at_z0" else z[:, 1:, i]))
    t = np.arange(T)
    keep = np.ones(T, bool)
    if defect == "steps_from_256_dropped":
        keep[256:] = False
    if defect == "last_step_dropped":
        keep[T - 1] = False
    if defect == "partial_sum_of_wave_3_dropped":
        keep[(t % 256) // 64 == 3] = False
    path = (lps - lpg + jac)[:, keep].sum(1)
    rows = np.clip(np.asarray(c["obs_rows"], int), 0, T)
    if defect == "obs_row_minus_one":
        rows = np.clip(rows - 1, 0, T)
    xr = x
    if defect == "obs_rows_not_clamped":                         # a row above T is the next path's memory (0 after the last path)
        rows = np.asarray(c["obs_rows"], int)
        flat = np.concatenate([x.reshape(B * (T + 1), S), np.zeros((T + 1, S), dtype)])
        xr = np.stack([flat[b * (T + 1):(b + 2) * (T + 1)] for b in range(B)])
    st = R.tail_formulas(_lw_tail_case(c, xr, rows, dtype), dtype)["sample_terms"]
    obs, prior, post = st[0], st[1], st[2]
    out = obs + path - prior + post if defect == "prior_minus_post_sign_flipped" else obs + path + prior - post
    assert out.v.dtype == dtype and out.m.dtype == dtype
    return out


@functools.lru_cache(maxsize=8)
def _lw_reference(*shape):
    c = lw_case(*shape)
    S, B, T, model = c["S"], c["B"], c["T"], c["model"]
    MVN = torch.distributions.MultivariateNormal
    z64, x64 = _lw_states(c, F64, c["pos"])
    z, x = torch.tensor(z64), torch.tensor(x64)
    dt, s = c["dt"], np.sqrt(c["dt"])
    if model == "k0":
        drift, diff = R._t64(c["drift"]), R._t64(np.nan_to_num(c["diffusion"], nan=0.0))
    else:
        sde = lw_sde(model, S)
        th = R._t64(c["theta"] if c["rates"] is None else c["rates"])[:, None, :].expand(B, T, -1).reshape(B * T, -1)
        xf = x[:, :-1].reshape(B * T, S)
        drift, diff = sde.drift(xf, th).reshape(B, T, S), sde.diffusion(xf, th).reshape(B, T, S, S)
    chol = R._t64(np.nan_to_num(c["chol"], nan=0.0))
    sde_lp = MVN(x[:, :-1] + drift * dt, scale_tril=torch.tril(diff) * s, validate_args=False).log_prob(x[:, 1:]).sum(1)
    gen_lp = MVN(z[:, :-1] + R._t64(c["means"]) * dt, scale_tril=torch.tril(chol) * s, validate_args=False).log_prob(z[:, 1:]).sum(1)
    jac = torch.nn.functional.logsigmoid(z[:, 1:, c["pos"]]).sum((1, 2))
    rows = np.clip(np.asarray(c["obs_rows"], int), 0, T)
    out = np.empty(B)
    for b in range(B):                                            # the batch mean of one path is that path's value
        tc = _lw_tail_case(c, x64[b:b + 1], rows, F64)
        tc.update(theta=c["theta"][b:b + 1], sde_lp=sde_lp[b:b + 1].numpy(), gen_lp=gen_lp[b:b + 1].numpy(), jac=jac[b:b + 1].numpy())
        out[b] = R.tail_reference(tc)["out"][0]
    return out, lw_formulas(c).m


def lw_reference(c_shape):
    """(float64 log_w [B] from MultivariateNormal / logsigmoid / the model's own drift and diffusion / Normal, LogNormal and the
    count likelihoods of ``sde_reference.tail_reference``, magnitude [B]) of the case with shape tuple ``c_shape``."""
    return _lw_reference(*c_shape)


def lw_ratio(shape, got):
    ref, mag = lw_reference(shape)
    return ratio(got, ref, mag)


def lw_c(shape):
    return C_LW_COUNT if shape[-1] else C_LW


# =========================================================================================================== accumulator
ACC_NS = (1, 255, 256, 257)
ACC_EDGES = ("plain", "minus_inf_chunk_first", "minus_inf_chunk_last", "plus_inf_entry")


def acc_case(n, edge):
    """Chunks of float32 log-weights for ``log_weight_accumulate``: one of n entries around -300, a second all -inf chunk before
    or after it, or a +inf entry (counted non-finite and left out of the sums) in the middle."""
    rng = np.random.default_rng(n + 17 * ACC_EDGES.index(edge))
    lw = (4.0 * rng.standard_normal(n) - 300.0).astype(F32)
    chunks = [lw]
    if edge == "minus_inf_chunk_first":
        chunks = [np.full(n, -np.inf, F32), lw]
    if edge == "minus_inf_chunk_last":
        chunks = [lw, np.full(n, -np.inf, F32)]
    if edge == "plus_inf_entry":
        chunks = [lw.copy()]
        chunks[0][n // 2] = np.inf
    return chunks


def acc_reference(chunks):
    """float64 (max, logsumexp, ESS, sum, n, n_nonfinite) of the entries that are not NaN / +inf."""
    import math
    v = np.concatenate(chunks).astype(F64)
    ok = ~(np.isnan(v) | (v == np.inf))
    fin = v[ok & np.isfinite(v)]
    m = fin.max() if fin.size else -np.inf
    w = np.exp(fin - m)
    lse = m + math.log(w.sum()) if fin.size else -np.inf
    ess = w.sum() ** 2 / (w * w).sum() if fin.size else float("nan")
    return m, lse, ess, v[ok].sum(), v.size, int((~ok).sum())
