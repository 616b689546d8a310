"""float64 reference, per-element magnitudes, bounds and test inputs of the optimizer step (csrc/vsde_optim.hip,
inference/fused_optimizer.py) and the integer bf16 cast that is the reference of the pack refresh (csrc/vsde_pack.hip).  Plain
functions on numpy arrays: tests/test_optimizer_ops_gpu.py and tests/test_pack_ops_gpu.py compare the kernels with them,
tests/test_optimizer_bounds.py checks on the CPU that the bounds hold for a correct float32 evaluation and reject one with a defect.

A case (``make_case``) is a dict of flat float32 arrays -- every tensor of the step one after the other, ``sizes`` their lengths,
``gid`` the hyper-parameter row of every element -- plus ``groups`` (float64 [G, 5]: lr, beta1, beta2, eps, weight decay), the
step count ``t``, the loss ``scale`` (None or a power of two), ``max_norm`` and ``ema_w`` (1 - decay; < 0: no EMA).  ``g`` holds the
gradients as the kernel reads them: loss-SCALED.

Values.  ``step64`` is the contract of the kernel header written out in float64: g' = g / scale; norm = sqrt(sum g'^2) over all
tensors; found_inf = not isfinite(sum); clip = min(1, max_norm / (norm + 1e-6)) when max_norm > 0, else 1; with a scale and
found_inf p, m, v and the step count stay and the EMA still lerps; otherwise p <- p - lr wd p, m <- m + (1 - b1)(clip g' - m),
v <- b2 v + (1 - b2)(clip g')^2, p <- p - lr / bc1 m / (sqrt(v) / sqrt(bc2) + eps) with the bias corrections at t + 1,
sh <- sh + w (p_new - sh), t_next = t + 1.  tests/test_optimizer_bounds.py pins it to clip_grad_norm_ + torch.optim.AdamW (not
fused) + torch.lerp in float64 to 1e-12.  ``step32`` is the same step in numpy float32 in the kernel's operation order and with its
promotions (torch's adam_math: hyper-parameters double, tensors float); it only measures the constants below and carries the
injected defects -- it is not a second oracle.

Magnitudes: of every output element, its formula with each subtraction replaced by a sum of magnitudes:

    p        |p| + lr wd |p| + |step_size m_new / denom|
    m        |m| + (1 - b1)(|clip g'| + |m|)
    v        b2 |v| + (1 - b2)(clip g')^2
    shadow   |sh| + w (|p_new| + |sh|)
    norm     the norm

Bound: |got - ref64| <= c 2^-24 magnitude per element, one c per output kind; where the magnitude is zero (a skipped step, v of a
zero gradient on a zero moment) the kernel's value must equal the reference exactly.  c = 4 x the worst ratio of ``step32`` against
``step64`` on the CPU over every class and shape of tests/test_optimizer_ops_gpu.py (``all_gpu_cases``), rounded up; the norm
constant comes from a SEQUENTIAL float32 sum of the squares, the worst order.  The factor 4 covers fused multiply-adds, v_rcp /
v_sqrt and another summation order:

    kind      worst CPU ratio   c       worst ratio on an MI355X
    p         5.34              21.5    5.34
    m         3.22              13      2.92
    v         5.30              21.5    6.15
    shadow    5.45              22      4.54
    norm      103.54            415     1.29

Every pack comparison of tests/test_pack_ops_gpu.py was bit-exact on the MI355X: the hardware conversion behind ``(__bf16)x`` rounds to
nearest even, keeps subnormals and signed zeros and turns every NaN into a NaN; neither kernel file needed a fix.

Input classes (an absolute bound on p cannot see a small relative error of the update, so each class isolates a term):

    general       p, m, g ~ N(0, 1), v = m^2 U(0.5, 2), shadow = p + 0.01 N(0, 1); |p| >= 0.1 (see below)
    zero_p        p = 0: p_new = -update, its magnitude is the update's; sign(g) = sign(m) (see below)
    zero_shadow   sh = 0: sh_new = w p_new
    tiny_grad     |g|, |m| ~ 1e-10, v ~ 1e-20, p = 0, sign(g) = sign(m): eps (1e-8 in groups 0 and 2, 1e-3 in group 1) dominates the denominator
    cold          m = v = 0 (the first step at t = 0; run at every t)
    zero_grad_v0  g = 0, v = 0: the denominator is eps alone, v_new must be exactly 0
    zero_grad     g = 0, v > 0
    large         |g|, |m| = 10^U(10, 15), v = m^2: squares up to 1e30, their sum below float32's maximum
    small_norm    m = v = 0, the gradients scaled to a global norm of 1e-5, max_norm 1e-6: clip = 1e-6 / 1.1e-5, the 1e-6 of the
                  clip denominator is 10 % of it

The magnitude of p takes the VALUE of m_new, as the formula is written, but the error of m_new is relative to ITS magnitude
|m| + (1 - b1)(|g| + |m|): where g and m have opposite signs and m_new nearly cancels, the update's error is large against the
update itself, and a correct float32 evaluation only meets the p bound because |p| covers it.  So the classes that drop |p| from
the magnitude (zero_p, tiny_grad) draw g with the sign of m -- m_new = b1 m + (1 - b1) g then has no cancellation -- and general
keeps |p| >= 0.1, two orders above the largest update (lr 1e-2); small p is zero_p's subject.

Per class: step counts t in {0, 1, 9, 999, 100000}, scales None / 1024 / 2^-10, and max_norm at 4 x the norm (no clipping), at
a quarter of it (clipping) and 0 (off); the unclamped coefficient max_norm / (norm + 1e-6) is asserted to lie outside
[0.99, 1.01], because the clip is a branch.  Three groups in every call: (1e-3, .9/.999, 1e-8, .01), (1e-2, .8/.95, 1e-3, 0),
(3e-4, .95/.9999, 1e-8, .1).
"""
import functools
import itertools

import numpy as np

F32, F64 = np.float32, np.float64
C24 = 2.0 ** -24
CHUNK = 4096                      # elements per chunk record (vsde_optim_chunk_elems)

# c per output kind: 4 x the worst CPU ratio of step32 against step64, rounded up (table in the module docstring)
C_P = 21.5
C_M = 13.0
C_V = 21.5
C_SHADOW = 22.0
C_NORM = 415.0
C = {"p": C_P, "m": C_M, "v": C_V, "sh": C_SHADOW, "norm": C_NORM}

GROUPS = np.array([(1e-3, 0.9, 0.999, 1e-8, 0.01), (1e-2, 0.8, 0.95, 1e-3, 0.0), (3e-4, 0.95, 0.9999, 1e-8, 0.1)], F64)
STEPS = (0, 1, 9, 999, 100000)
SCALES = (None, 1024.0, 2.0 ** -10)
EMA_W = 1.0 - 0.99                # the double FusedOptimizerStep hands to the kernel
CLASSES = ("general", "zero_p", "zero_shadow", "tiny_grad", "cold", "zero_grad_v0", "zero_grad", "large", "small_norm")
KINDS = ("p", "m", "v", "sh", "norm")


def max_norm_modes(cls):
    return ("fixed",) if cls == "small_norm" else ("below", "above", "off")


# ----------------------------------------------------------------------------------------------------------------- inputs
def make_case(cls, sizes, gids, t=0, scale=None, mode="below", ema_w=EMA_W, seed=0, groups=GROUPS):
    """One step's inputs: tensors of ``sizes`` elements in the groups ``gids``, drawn for the class ``cls``."""
    sizes, gids = np.asarray(sizes, np.int64), np.asarray(gids, np.int64)
    n = int(sizes.sum())
    rng = np.random.default_rng([seed, CLASSES.index(cls), n])
    randn = lambda: rng.standard_normal(n)
    sgn = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    p, m, g = randn(), randn(), randn()
    p = np.sign(p) * (0.1 + np.abs(p))
    v = m * m * rng.uniform(0.5, 2.0, n)
    sh = p + 0.01 * randn()
    if cls == "zero_p":
        p, g = np.zeros(n), np.sign(m) * np.abs(g)
    elif cls == "zero_shadow":
        sh = np.zeros(n)
    elif cls == "tiny_grad":
        p = np.zeros(n)
        g, m = 1e-10 * sgn * rng.uniform(0.5, 2.0, n), 1e-10 * sgn * rng.uniform(0.5, 2.0, n)
        v = 1e-20 * rng.uniform(0.25, 4.0, n)
    elif cls == "cold":
        m, v = np.zeros(n), np.zeros(n)
    elif cls == "zero_grad_v0":
        g, v = np.zeros(n), np.zeros(n)
    elif cls == "zero_grad":
        g = np.zeros(n)
    elif cls == "large":
        g, m = sgn * 10.0 ** rng.uniform(10, 15, n), sgn * 10.0 ** rng.uniform(10, 15, n)
        v = m * m
    elif cls == "small_norm":
        m, v = np.zeros(n), np.zeros(n)
        g = g * (1e-5 / np.sqrt((g * g).sum()))
    elif cls != "general":
        raise ValueError(cls)
    g = g.astype(F32)
    norm = float(np.sqrt((g.astype(F64) ** 2).sum()))
    if mode == "fixed":
        max_norm = 1e-6
    elif mode == "off":
        max_norm = 0.0
    else:
        max_norm = (4.0 if mode == "below" else 0.25) * norm if norm > 0 else 1.0
    max_norm = float(F32(max_norm))                                   # the kernel keeps the threshold as a float
    if max_norm > 0:
        coef = max_norm / (norm + 1e-6)
        assert not 0.99 <= coef <= 1.01, (cls, mode, coef)            # the clip is a branch: stay clear of it
    c = {"cls": cls, "sizes": sizes, "gids": gids, "gid": np.repeat(gids, sizes), "groups": np.asarray(groups, F64), "t": float(t),
         "scale": scale, "max_norm": max_norm, "ema_w": float(ema_w),
         "p": p.astype(F32), "m": m.astype(F32), "v": v.astype(F32), "sh": sh.astype(F32) if ema_w >= 0 else None,
         "g": g if scale is None else (g * F32(scale)).astype(F32)}
    assert np.isfinite(c["g"]).all()
    return c


# ------------------------------------------------------------------------------------------------------------- float64 step
def step64(c):
    """One optimizer step in float64.  Returns the values p, m, v, sh (None without EMA), norm, found_inf, t_next and, under
    "mag", the magnitude of every one of them."""
    p, m, v, g = (c[k].astype(F64) for k in ("p", "m", "v", "g"))
    scaled = c["scale"] is not None
    gp = g / c["scale"] if scaled else g
    with np.errstate(all="ignore"):
        total = float((gp * gp).sum())
        norm = float(np.sqrt(total))
    found_inf = not np.isfinite(total)
    clip = min(1.0, c["max_norm"] / (norm + 1e-6)) if c["max_norm"] > 0 else 1.0
    if scaled and found_inf:                                          # GradScaler skips the step; the EMA still moves
        p1, m1, v1, t_next = p, m, v, c["t"]
        mag = {"p": np.zeros_like(p), "m": np.zeros_like(p), "v": np.zeros_like(p)}
    else:
        lr, b1, b2, eps, wd = (c["groups"][c["gid"], i] for i in range(5))
        gh = gp * clip
        t_next = c["t"] + 1.0
        bc1, bc2 = 1.0 - b1 ** t_next, 1.0 - b2 ** t_next
        with np.errstate(all="ignore"):
            m1 = m + (1.0 - b1) * (gh - m)
            v1 = b2 * v + (1.0 - b2) * gh * gh
            update = lr / bc1 * m1 / (np.sqrt(v1) / np.sqrt(bc2) + eps)
            p1 = p - lr * wd * p - update
            mag = {"p": np.abs(p) + lr * wd * np.abs(p) + np.abs(update),
                   "m": np.abs(m) + (1.0 - b1) * (np.abs(gh) + np.abs(m)),
                   "v": b2 * np.abs(v) + (1.0 - b2) * gh * gh}
    out = {"p": p1, "m": m1, "v": v1, "sh": None, "norm": norm, "found_inf": found_inf, "t_next": t_next, "mag": mag}
    mag["norm"] = norm
    if c["ema_w"] >= 0:
        sh, w = c["sh"].astype(F64), c["ema_w"]
        out["sh"] = sh + w * (p1 - sh)
        mag["sh"] = np.abs(sh) + w * (np.abs(p1) + np.abs(sh))
    return out


# ------------------------------------------------------------------------------------------------------------- float32 step
DEFECTS = ("eps_inside_sqrt", "eps_before_bc2", "l2_weight_decay", "decay_after_update", "bias_at_t", "bc2_without_sqrt",
           "clip_without_1e-6", "clip_uncapped", "norm_of_scaled", "moments_unclipped", "ema_weight_decay", "ema_towards_old_p",
           "group_off_by_one", "chunk_last_skipped", "tail_skipped", "beta1_for_beta2")


def chunk_bounds(sizes):
    """(start, end) of every chunk record in the flat arrays: CHUNK elements, the last one of a tensor shorter."""
    out, base = [], 0
    for n in sizes:
        out += [(base + o, base + min(o + CHUNK, int(n))) for o in range(0, int(n), CHUNK)]
        base += int(n)
    return out


def step32(c, defect=None, norm_order="chunks"):
    """The step in float32 in the kernel's operation order: per element the order and promotions of torch's adam_math, the sum of
    squares as float32 partial sums per chunk added up in float32 (``norm_order`` "sequential": one float32 running sum over all
    elements, the worst order -- the norm constant).  ``defect``: one of DEFECTS."""
    assert defect is None or defect in DEFECTS, defect
    p, m, v, g = (c[k].astype(F32) for k in ("p", "m", "v", "g"))
    scaled = c["scale"] is not None
    inv = F32(1.0 / F64(F32(c["scale"]))) if scaled else F32(1.0)
    with np.errstate(all="ignore"):
        gp = g if defect == "norm_of_scaled" else g * inv
        sq = gp * gp
        if norm_order == "sequential":
            total = np.cumsum(sq, dtype=F32)[-1]
        else:
            total = np.array([sq[a:b].sum(dtype=F32) for a, b in chunk_bounds(c["sizes"])], F32).sum(dtype=F32)
        norm = np.sqrt(total)
        found_inf = not np.isfinite(total)
        clip = F32(1.0)
        if c["max_norm"] > 0:
            clip = F32(c["max_norm"]) / (norm + (F32(0.0) if defect == "clip_without_1e-6" else F32(1e-6)))
            if defect != "clip_uncapped" and not clip < 1:
                clip = F32(1.0)
        w = F32(c["ema_w"])
        if defect == "ema_weight_decay":
            w = F32(1.0 - c["ema_w"])
        sh = c["sh"]
        if scaled and found_inf:
            out = {"p": p, "m": m, "v": v, "t_next": c["t"]}
            if sh is not None:
                out["sh"] = sh + w * (p - sh)
        else:
            gid = (c["gid"] + 1) % len(c["groups"]) if defect == "group_off_by_one" else c["gid"]
            lr, b1, b2, eps, wd = (c["groups"][:, i] for i in range(5))
            step = F64(F32(c["t"]) + F32(0.0 if defect == "bias_at_t" else 1.0))
            bc1 = (1.0 - b1 ** step).astype(F32)
            bc2 = (1.0 - b2 ** step).astype(F32)
            bc2_sqrt = bc2 if defect == "bc2_without_sqrt" else np.sqrt(bc2)
            step_size = (lr / bc1.astype(F64)).astype(F32)
            lr, b1, b2, eps, wd, bc2_sqrt, step_size = (a[gid] for a in (lr, b1, b2, eps, wd, bc2_sqrt, step_size))
            grad = (g * inv) * clip
            gm = (g * inv) if defect == "moments_unclipped" else grad
            if defect == "l2_weight_decay":
                gm = (gm.astype(F64) + wd * p.astype(F64)).astype(F32)
                p1 = p
            elif defect == "decay_after_update":
                p1 = p
            else:
                p1 = (p.astype(F64) - lr * wd * p.astype(F64)).astype(F32)
            m1 = (m.astype(F64) + (1.0 - b1) * (gm - m).astype(F64)).astype(F32)
            if defect == "beta1_for_beta2":
                b2 = b1
            v1 = (b2 * v.astype(F64) + (1.0 - b2) * gm.astype(F64) * gm.astype(F64)).astype(F32)
            if defect == "eps_inside_sqrt":
                denom = np.sqrt((v1.astype(F64) + eps).astype(F32)) / bc2_sqrt
            elif defect == "eps_before_bc2":
                denom = (np.sqrt(v1).astype(F64) + eps).astype(F32) / bc2_sqrt
            else:
                denom = ((np.sqrt(v1) / bc2_sqrt).astype(F64) + eps).astype(F32)
            p1 = p1 - step_size * m1 / denom
            if defect == "decay_after_update":
                p1 = (p1.astype(F64) - lr * wd * p1.astype(F64)).astype(F32)
            out = {"p": p1, "m": m1, "v": v1, "t_next": c["t"] + 1.0}
            if sh is not None:
                out["sh"] = sh + w * ((p if defect == "ema_towards_old_p" else p1) - sh)
            if defect in ("chunk_last_skipped", "tail_skipped"):
                for a, b in chunk_bounds(c["sizes"]):
                    keep = slice(b - 1, b) if defect == "chunk_last_skipped" else slice(b - (b - a) % 4, b)
                    for k in ("p", "m", "v", "sh"):
                        if c[k] is not None:
                            out[k][keep] = c[k][keep]
    out.setdefault("sh", None)
    out.update(norm=float(norm), found_inf=found_inf)
    return out


# ----------------------------------------------------------------------------------------------------------------- scoring
def ratio(got, ref, mag):
    """Worst |got - ref| / (2^-24 magnitude); where the magnitude is zero the values must be equal."""
    got, ref, mag = (np.atleast_1d(np.asarray(a, F64)) for a in (got, ref, mag))
    if got.size == 0:
        return 0.0
    with np.errstate(all="ignore"):
        err = np.abs(got - ref)
        r = np.where(mag > 0, err / (C24 * mag), np.where(got == ref, 0.0, np.inf))
    r = np.where(np.isnan(r), np.inf, r)                              # a NaN or an inf where the reference is finite meets no bound
    return float(r.max())


def ratios(c, got, ref=None):
    """Worst ratio per output kind of ``got`` (p, m, v, sh, norm) against step64 on the case's inputs."""
    ref = step64(c) if ref is None else ref
    out = {k: ratio(got[k], ref[k], ref["mag"][k]) for k in ("p", "m", "v", "norm")}
    if ref["sh"] is not None:
        out["sh"] = ratio(got["sh"], ref["sh"], ref["mag"]["sh"])
    return out


def within(r):
    return all(v <= C[k] for k, v in r.items())


# ------------------------------------------------------------------------------------------------------- the GPU file's cases
SINGLE_CHUNK = (1, 2, 3, 4, 5, 7, 8, 255, 256, 257, 1023, 1024, 1025, 1027, 4093, 4094, 4095, 4096)
MULTI_CHUNK = (4097, 8191, 8192, 8193)
CHUNK_COUNTS = (1, 2, 255, 256, 257, 1000)
# the mixed table: 12 tensors in three groups, 4097 and 3 x 4101 among them, every n % 4 and a bias-sized one
MIXED_SIZES = (5, 231, 4097, 12303, 256, 3, 1, 1026, 4096, 682, 7, 63)
MIXED_GIDS = (0, 0, 0, 0, 0, 1, 1, 1, 2, 2, 2, 2)


def chunk_count_layout(k):
    """``k`` tensors of 5..9 elements (one chunk each); the last repeats the first tensor's size and group."""
    sizes = [5 + (i % 5) for i in range(k)]
    gids = [i % 3 for i in range(k)]
    sizes[-1], gids[-1] = sizes[0], gids[0]
    return sizes, gids


def chunk_count_case(k, **kw):
    """The first and the last tensor hold identical (p, m, v, sh, g, group): every workgroup derives the same clip, so their
    outputs must be bitwise identical."""
    sizes, gids = chunk_count_layout(k)
    c = make_case("general", sizes, gids, **kw)
    n = sizes[0]
    if k > 1:
        for key in ("p", "m", "v", "sh", "g"):
            c[key][-n:] = c[key][:n]
    return c


def cross_settings(cls):
    return list(itertools.product(SCALES, max_norm_modes(cls), STEPS))


def all_gpu_cases():
    """Every (class, shape, setting) tests/test_optimizer_ops_gpu.py runs, as thunks (the constants are measured over these)."""
    for n in SINGLE_CHUNK + MULTI_CHUNK:
        yield f"n{n}", functools.partial(make_case, "general", [n], [n % 3], t=9, scale=1024.0, mode="above")
    for k in CHUNK_COUNTS:
        yield f"chunks{k}", functools.partial(chunk_count_case, k, t=1, mode="above")
    yield "align", functools.partial(make_case, "general", ALIGN_SIZES, ALIGN_GIDS, t=9, scale=1024.0, mode="above")
    yield "no_ema", functools.partial(make_case, "general", ALIGN_SIZES, ALIGN_GIDS, t=1, mode="above", ema_w=-1.0)
    for cls in CLASSES:
        for scale, mode, t in cross_settings(cls):
            yield f"{cls}-{scale}-{mode}-{t}", functools.partial(make_case, cls, MIXED_SIZES, MIXED_GIDS, t=t, scale=scale, mode=mode)


ALIGN_SIZES = (1027, 4099, 6)      # a scalar tail in the first, a second chunk of 3 in the second
ALIGN_GIDS = (0, 1, 2)


# --------------------------------------------------------------------------------------------------------- bf16 cast, integer
def bf16_rne_bits(u):
    """float32 bit patterns (uint32) -> bfloat16 bit patterns (uint16), round to nearest even in integer arithmetic: add 0x7FFF
    plus the lowest kept bit and drop 16 bits (carries into the exponent and on to inf by themselves; subnormals are not
    flushed).  A NaN stays a NaN (quiet bit set: a payload in the dropped bits alone would otherwise round to inf)."""
    u = np.asarray(u, np.uint32).astype(np.uint64)
    nan = ((u & 0x7F800000) == 0x7F800000) & ((u & 0x007FFFFF) != 0)
    r = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    return (np.where(nan, (u >> 16) | 0x40, r) & 0xFFFF).astype(np.uint16)


def bf16_is_nan(b):
    b = np.asarray(b).astype(np.uint32) & 0xFFFF
    return ((b & 0x7F80) == 0x7F80) & ((b & 0x007F) != 0)


PACK_SENTINEL = 0x7FC1


def pack_patterns():
    """name -> uint32 float32 patterns, both signs of each: the classes the pack test demands."""
    def both(*xs):
        xs = np.array(xs, np.uint32)
        return np.concatenate([xs, xs | np.uint32(0x80000000)])
    return {
        "tie_even": both(0x3F808000, 0x40008000, 0x3F828000, 0x00028000),         # kept mantissa even: down
        "tie_odd": both(0x3F818000, 0x40018000, 0x3F838000, 0x00018000),          # kept mantissa odd: up
        "tie_plus_ulp": both(0x3F808001, 0x3F818001, 0x40008001),
        "tie_minus_ulp": both(0x3F807FFF, 0x3F817FFF, 0x40007FFF),
        "mantissa_ones": both(0x3F7FFFFF, 0x3FFFFFFF, 0x3F7F8000, 0x3F7F8001, 0x3F7F7FFF, 0x407FC000),   # carry into the exponent
        "to_bf16_max": both(0x7F7F0000, 0x7F7F0001, 0x7F7F7FFF),
        "to_inf": both(0x7F7F8000, 0x7F7F8001, 0x7F7FFFFF),
        "inf": both(0x7F800000),
        "zero": both(0x00000000),
        "subnormal": both(0x00000001, 0x00007FFF, 0x00008000, 0x00008001, 0x00010000, 0x00018000, 0x007F0000, 0x007F7FFF,
                          0x007F8000, 0x007FFFFF),
        "small_normal": both(0x00800000, 0x00800001, 0x00808000, 0x00818000, 0x00FFFFFF),
        # no NaN whose upper half is the sentinel's, before or after the quiet bit is set (0x7FC1, 0x7F81)
        "nan": both(0x7FC00000, 0x7F800001, 0x7F80FFFF, 0x7FA00000, 0x7FFFFFFF, 0x7F8F8000, 0x7FC20001),
    }


@functools.lru_cache(maxsize=None)
def pack_values(n_random=4096):
    """Every pattern of ``pack_patterns`` followed by N(0, 1) draws, as uint32."""
    rng = np.random.default_rng(7)
    special = np.concatenate(list(pack_patterns().values()))
    out = np.concatenate([special, rng.standard_normal(n_random).astype(F32).view(np.uint32)])
    out.setflags(write=False)
    return out
