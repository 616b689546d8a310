"""Every dispatch of the fused encoder elementwise kernels (csrc/vsde_encoder.hip) against float64.

Each case calls one ``viforsdes_amd._hip`` wrapper directly, so it pins one kernel, and compares every element with a
float64 torch evaluation of the operation itself (forward), or float64 autograd of the same chain against random
upstream gradients (backward).

References.  bf16 cases start from the bf16 inputs and round to bf16 exactly where the kernel does (``rnd<T>`` in the
source; each such point is marked ``# mirrors`` below).  Where the kernel's fp32 value at such a point may fall on the
other side of a bf16 rounding boundary than the float64 value, ``_round_bf16`` returns the size of that possible
one-ulp step, and the bound of every output the rounded value feeds grows by it (times the factor it is multiplied by).

Bounds, per element, never relative to a tensor's maximum:
  pointwise outputs   |got - ref| <= a * |ref| + s * (b + b32 * kappa)    s = RMS of that row of the reference
                      fp32: a = b = 1e-6 (swiglu / gate_merge a = 4e-6: __expf)   bf16: a = 2^-8 (output rounding), b = 2^-12
                      b32 = 2e-6 is the fp32 arithmetic of the kernel; kappa = RMS(x) * rstd of the normalised row (1 for
                      a centred row, 1e3 for the cancellation row) and 0 where nothing is normalised
  column sums         |got - ref| <= c * sum|terms| (+ 2^-8 |ref| in bf16)  per (batch row, channel); c = 1e-5
                      (the terms of dscale carry kappa as above).  A missing or doubled token chunk is an error of order
                      1 / nchunk of the sum, far above this bound.
Fences.  Pitched operands (scale / shift / gate in a [B, 6 depth C] modulation buffer, qkv in [B, N, 3C + 16], glog with
a row pitch d + 16) and the gradient destinations (dscale / dshift / dgate / dqkv / dglog) are column ranges at a
non-zero offset of buffers filled with a NaN sentinel: a read outside the range turns an output into NaN and fails,
and after each call every element outside the range must still be that sentinel, bit for bit.
Determinism.  Every backward with token sums (dscale, dshift, dgate, dlam) runs twice; the results must be bitwise equal.

Dispatch coverage (test id fields in brackets):
  ln_modulate / residual_ln  C 64..1024 x {f32, bf16} -> (V, LPR, NSLAB)  [v{V}l{LPR}s{NSLAB}]:
        f32   64:1,64,1  128:4,32,1  192:1,64,3  256:4,64,1  384:4,32,3  512:4,64,2  768:4,64,3  1024:4,64,4
        bf16  64:1,64,1  128:2,64,1  192:1,64,3  256:8,32,1 (two tokens per wave)  384:2,64,3  512:8,64,1
              768:8,32,3  1024:8,64,2
        token chunks per batch row [ch{n}]: (3,5) 1 chunk, (2,37) 4, (4,600) 64 with the last 4 empty, (2,1) 1 token
        grid-stride forward (more than one row per workgroup slot) [gridstride]: (512,41) f32 C 256, (1024,41) bf16 C 256
        dres / dxnew present and absent [dres|nodres], mod_pitch 0 and 6*2*C [pitch0|pitched]; every case with N >= 2
        has one constant row (var = 0, rstd = eps^-1/2) and one row of mean 1e3, std 1 (cancellation)
  gated_residual             C 68 (bf16 V = 4), 256, 1024, 2048 bf16 (256 lanes per token, the limit) at 1 / 4 / 64
                             chunks; f32 1028 / 2048 and bf16 1028 exceed 256 lanes per token [overlimit]: the backward must
                             refuse them (ValueError) or get them right
  swiglu                     H2 171 (V = 1), 170 (V = 2), 176 (full vector), 682; M = 20992, H2 = 704 f32 walks the
                             8192-workgroup grid cap more than once; |a| up to 30 (saturated sigmoid)
  gate_merge                 token_major 0 / 1 x d 4 (bf16 V = 1), 32, 64, 128 x heads 1 / 3 / 4; glog pitch d + 16
  qk_norm_rope               d 2, 4 (PV = 1, 1 and 2 lanes per head), 8 (PV = 4, one lane per head), 32, 64, 128 x heads
                             1 / 3 / 4 x token_major 0 / 1; v0 / lam absent [nov0], present [v0], present with dv0
                             accumulated onto a nonzero dv0 and dv_extra [acc]; a many-partial dlam case; every shape
                             leaves a partial last workgroup (B N heads d/2/PV not a multiple of 256)
"""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64 = torch.float64
BF = torch.bfloat16
DTYPES = {"f32": torch.float32, "bf16": BF}
SENTINEL = {torch.float32: (torch.int32, 0x7FC0DEAD), BF: (torch.int16, 0x7FDE)}   # quiet NaNs with a payload
B32 = 2e-6      # fp32 arithmetic of the kernels, scaled by the row's condition number
EPS_LN = 1e-5


def _hip():
    from viforsdes_amd import _hip
    return _hip


# ----------------------------------------------------------------------------------------------------------- helpers
def _tol(dtype, a32=1e-6):
    return (2.0 ** -8, 2.0 ** -12) if dtype == BF else (a32, 1e-6)


def _rand(g, *shape, scale=1.0, dtype=torch.float32):
    return (torch.randn(*shape, generator=g, dtype=F64) * scale).to(DEV, dtype)


def _sentinel_buffer(shape, dtype):
    idt, bits = SENTINEL[dtype]
    return torch.full(shape, bits, dtype=idt, device=DEV).view(dtype)


def _fenced(shape, dtype, ranges, values=None):
    """A sentinel-filled buffer of ``shape``; ``ranges`` are (start, stop) column ranges of its last dimension.  Returns the
    buffer and one view per range (filled from ``values`` when given)."""
    buf = _sentinel_buffer(shape, dtype)
    views = [buf[..., a:b] for a, b in ranges]
    if values is not None:
        for v, x in zip(views, values):
            v.copy_(x)
    return buf, views


def _assert_fence(name, buf, ranges):
    idt, bits = SENTINEL[buf.dtype]
    outside = torch.ones(buf.shape[-1], dtype=torch.bool, device=DEV)
    for a, b in ranges:
        outside[a:b] = False
    raw = buf.view(idt)[..., outside]
    bad = int((raw != bits).sum())
    assert bad == 0, f"{name}: {bad} elements outside the written column ranges changed"


def _row_rms(ref):
    return ref.pow(2).mean(-1, keepdim=True).sqrt()


def _check(name, got, ref, a, b, kappa=None, mag=None, extra=None):
    """|got - ref| <= a * mag + s * (b + B32 * kappa) + extra, element by element (mag defaults to |ref|, s = row RMS of ref)."""
    got = got.to(F64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    s = _row_rms(ref)
    bound = a * (ref.abs() if mag is None else mag) + s * b
    if kappa is not None:
        bound = bound + s * B32 * kappa
    if extra is not None:
        bound = bound + extra
    err = (got - ref).abs()
    bad = ~(err <= bound)
    if bool(bad.any()):
        idx = tuple(int(i) for i in bad.nonzero()[0])
        ratio = float((err / bound.clamp_min(1e-300))[~torch.isnan(err)].max()) if not bool(torch.isnan(err).all()) else float("nan")
        raise AssertionError(f"{name}: {int(bad.sum())} of {bad.numel()} elements out of bound (worst err/bound {ratio:.3g}); "
                             f"first at {idx}: got {float(got[idx])!r}, ref {float(ref[idx])!r}, bound {float(bound[idx]):.3g}")


def _check_colsum(name, got, ref, absterms, dtype, c=1e-5, extra=None):
    """Token sums per (batch row, channel): |got - ref| <= c * sum|terms| (+ one bf16 rounding of the result) + extra."""
    got = got.to(F64)
    bound = c * absterms + (2.0 ** -8 * ref.abs() if dtype == BF else 0.0) + (0.0 if extra is None else extra)
    err = (got - ref).abs()
    bad = ~(err <= bound)
    if bool(bad.any()):
        idx = tuple(int(i) for i in bad.nonzero()[0])
        raise AssertionError(f"{name}: {int(bad.sum())} of {bad.numel()} column sums out of bound; first at {idx}: "
                             f"got {float(got[idx])!r}, ref {float(ref[idx])!r}, bound {float(bound[idx]):.3g}")


def _round_bf16(t, err):
    """bf16 rounding of a float64 value the kernel forms in fp32 with an error up to ``err``: (rounded value, size of the
    one-ulp step the kernel's rounding may differ by -- 0 where the value is not within ``err`` of a rounding boundary)."""
    r = t.to(BF).to(F64)
    return r, ((t + err).to(BF).to(F64) - (t - err).to(BF).to(F64)).abs()


def _same_bits(name, a, b):
    assert torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8)), f"{name}: not bitwise reproducible"


def _chunks(B, N):
    """Token chunks per batch row of the column-sum backward (colsum_chunks in the source)."""
    c = min(max((768 + B - 1) // B, 4), 64)
    return min(c, max(N // 8, 1))


def _ln_branch(C, dtype):
    """(V, LPR, NSLAB) that ln_mod_dispatch picks for C."""
    vf = 8 if dtype == BF else 4
    for v, lpr in ((vf, 64), (vf, 32), (vf // 2, 64), (vf // 4, 64)):
        if C % (lpr * v) == 0 and C // (lpr * v) <= 4:
            return v, lpr, C // (lpr * v)
    return 1, 64, C // 64


# ------------------------------------------------------------------------------------------ LayerNorm + modulation
LN_CS = [64, 128, 192, 256, 384, 512, 768, 1024]
LN_SHAPES = [(3, 5), (2, 37), (4, 600), (2, 1)]


def _ln_inputs(g, B, N, C, dtype):
    x = torch.randn(B, N, C, generator=g, dtype=F64)
    if N >= 2:
        x[0, 0] = 2.5                                            # constant row: var = 0 (sums exact), rstd = eps^-1/2
        x[0, 1] = 1e3 + torch.randn(C, generator=g, dtype=F64)   # mean 1e3, std 1: the mean cancels in x - mu
    return x.to(DEV, dtype)


def _ln_ref(xin, sc, sh):
    """float64 LayerNorm(x) * (1 + scale) + shift with the biased variance; (y, mean, rstd, kappa)."""
    mu = xin.mean(-1, keepdim=True)
    var = (xin - mu).pow(2).mean(-1, keepdim=True)
    rstd = (var + EPS_LN).rsqrt()
    y = (xin - mu) * rstd * (1 + sc[:, None]) + sh[:, None]
    kappa = _row_rms(xin) * rstd
    return y, mu[..., 0], rstd[..., 0], kappa


def _mod_buffer(g, B, C, dtype, pitched, k):
    """k per-batch-row [B, C] vectors: column ranges C, 2C, ... of a sentinel-filled [B, 6*2*C] modulation buffer (pitched),
    or separate contiguous tensors.  Returns (buffer or None, ranges, views)."""
    vals = [_rand(g, B, C, scale=0.5, dtype=dtype) for _ in range(k)]
    if not pitched:
        return None, None, vals
    ranges = [((1 + 2 * i) * C, (2 + 2 * i) * C) for i in range(k)]
    buf, views = _fenced((B, 12 * C), dtype, ranges, vals)
    return buf, ranges, views


def _grad_buffer(B, C, dtype, pitched, k):
    if not pitched:
        return None, None, [None] * k
    ranges = [((2 + 3 * i) * C, (3 + 3 * i) * C) for i in range(k)]
    buf, views = _fenced((B, 12 * C), dtype, ranges)
    return buf, ranges, views


def _ln_cases():
    cases = []
    for dn in DTYPES:
        for i, C in enumerate(LN_CS):
            for j, (B, N) in enumerate([(2, 37), (4, 600)] + ([LN_SHAPES[0]] if i % 2 == 0 else [LN_SHAPES[3]])):
                cases.append((dn, C, B, N, (i + j) % 2 == 0, (i + j) % 3 != 0))
    cases.append(("f32", 256, 512, 41, True, True))
    cases.append(("bf16", 256, 1024, 41, False, True))
    return cases


def _ln_id(case):
    dn, C, B, N, dres, pitched = case
    v, lpr, ns = _ln_branch(C, DTYPES[dn])
    rows = "gridstride" if B * N > 4096 * (256 // lpr) else f"ch{_chunks(B, N)}"
    return f"{dn}-C{C}-v{v}l{lpr}s{ns}-{B}x{N}-{rows}-{'dres' if dres else 'nodres'}-{'pitched' if pitched else 'pitch0'}"


@pytest.mark.parametrize("case", _ln_cases(), ids=_ln_id)
def test_ln_modulate(case):
    dn, C, B, N, with_dres, pitched = case
    dtype = DTYPES[dn]
    hip = _hip()
    a, b = _tol(dtype)
    g = torch.Generator().manual_seed(C * 7 + B * N)
    x = _ln_inputs(g, B, N, C, dtype)
    mbuf, mranges, (scale, shift) = _mod_buffer(g, B, C, dtype, pitched, 2)
    mcopy = mbuf.clone() if pitched else None

    y, mean, rstd = hip.ln_modulate_fwd(x, scale, shift, EPS_LN)
    x64, sc64, sh64 = x.to(F64).requires_grad_(), scale.to(F64).requires_grad_(), shift.to(F64).requires_grad_()
    yr, mur, rsr, kappa = _ln_ref(x64, sc64, sh64)
    kd = kappa.detach()
    _check("y", y, yr.detach(), a, b, kappa=kd)
    _check("mean", mean[..., None], mur.detach()[..., None], 1e-6, 0.0, extra=1e-6 * _row_rms(x64.detach()))
    _check("rstd", rstd[..., None], rsr.detach()[..., None], 2e-6, 0.0)
    if pitched:
        _assert_fence("modulation buffer (forward)", mbuf, mranges)
        _same_bits("modulation buffer (forward)", mbuf, mcopy)

    if B * N > 4096:   # the grid-stride shapes are there for the forward
        return
    dy = _rand(g, B, N, C, dtype=dtype)
    dres = _rand(g, B, N, C, dtype=dtype) if with_dres else None
    gbuf, granges, (dsc_dst, dsh_dst) = _grad_buffer(B, C, dtype, pitched, 2)
    dx, dscale, dshift = hip.ln_modulate_bwd(x, scale, dy, mean, rstd, dres, dsc_dst, dsh_dst)
    gx, gsc, gsh = torch.autograd.grad(yr, [x64, sc64, sh64], dy.to(F64))
    dxr = gx + (dres.to(F64) if with_dres else 0)
    _check("dx", dx, dxr, a, b, kappa=kd, mag=gx.abs() + (dres.to(F64).abs() if with_dres else 0))
    xh = ((x64 - mur[..., None]) * rsr[..., None]).detach()
    dy64 = dy.to(F64)
    _check_colsum("dscale", dscale, gsc, (dy64.abs() * (xh.abs() + kd)).sum(1), dtype)
    _check_colsum("dshift", dshift, gsh, dy64.abs().sum(1), dtype)
    if pitched:
        _assert_fence("dscale/dshift buffer", gbuf, granges)
        _same_bits("modulation buffer (backward)", mbuf, mcopy)
    _, _, (d2, e2) = _grad_buffer(B, C, dtype, pitched, 2)
    again = hip.ln_modulate_bwd(x, scale, dy, mean, rstd, dres, d2, e2)
    for n, u, v in zip(["dx", "dscale", "dshift"], (dx, dscale, dshift), again):
        _same_bits(n, u, v)


@pytest.mark.parametrize("case", _ln_cases(), ids=_ln_id)
def test_residual_ln(case):
    dn, C, B, N, with_dxnew, pitched = case
    dtype = DTYPES[dn]
    hip = _hip()
    a, b = _tol(dtype)
    g = torch.Generator().manual_seed(C * 11 + B * N + 1)
    x = _ln_inputs(g, B, N, C, dtype)
    yb = _rand(g, B, N, C, dtype=dtype)
    yb[0, :2] = 0   # the constant and the cancellation row of x reach the norm unchanged
    mbuf, mranges, (gate, scale, shift) = _mod_buffer(g, B, C, dtype, pitched, 3)
    mcopy = mbuf.clone() if pitched else None

    xnew, h, mean, rstd = hip.residual_ln_fwd(x, yb, gate, scale, shift, EPS_LN)
    x64, y64, g64 = x.to(F64), yb.to(F64), gate.to(F64)
    gy = g64[:, None] * y64
    if dtype == BF:
        xnr = (x64 + gy.to(BF).to(F64)).to(BF).to(F64)   # mirrors ln_mod_fwd_kernel: v = rnd(v + rnd(rg * ry))
    else:
        xnr = x64 + gy
    _check("xnew", xnew, xnr, a, b, mag=x64.abs() + gy.abs())
    hr, mur, rsr, kappa = _ln_ref(xnr, scale.to(F64), shift.to(F64))
    _check("h", h, hr, a, b, kappa=kappa)
    _check("mean", mean.view(B, N, 1), mur[..., None], 1e-6, 0.0, extra=1e-6 * _row_rms(xnr))
    _check("rstd", rstd.view(B, N, 1), rsr[..., None], 2e-6, 0.0)
    if pitched:
        _assert_fence("modulation buffer (forward)", mbuf, mranges)
        _same_bits("modulation buffer (forward)", mbuf, mcopy)

    if B * N > 4096:
        return
    dh = _rand(g, B, N, C, dtype=dtype)
    dxnew = _rand(g, B, N, C, dtype=dtype) if with_dxnew else None
    gbuf, granges, (dg_dst, dsc_dst, dsh_dst) = _grad_buffer(B, C, dtype, pitched, 3)
    dx, dy, dgate, dscale, dshift = hip.residual_ln_bwd(xnew, yb, gate, scale, dh, dxnew, mean, rstd, dg_dst, dsc_dst, dsh_dst)
    # float64 autograd of xnew = x0 + gate * y -> LN-modulate, with x0 chosen so that xnew is the kernel's own output
    xn_k = xnew.to(F64)
    x0 = (xn_k - gy).requires_grad_()
    y64r, g64r = y64.clone().requires_grad_(), g64.clone().requires_grad_()
    sc64, sh64 = scale.to(F64).requires_grad_(), shift.to(F64).requires_grad_()
    xn = x0 + g64r[:, None] * y64r
    hh, mu2, rs2, kap2 = _ln_ref(xn, sc64, sh64)
    outs, gos = [hh], [dh.to(F64)]
    if with_dxnew:
        outs.append(xn); gos.append(dxnew.to(F64))
    gx, gy_, gg, gsc, gsh = torch.autograd.grad(outs, [x0, y64r, g64r, sc64, sh64], gos)
    kap2 = kap2.detach()
    dxnew64 = dxnew.to(F64).abs() if with_dxnew else 0
    _check("dx", dx, gx, a, b, kappa=kap2, mag=(gx - (dxnew.to(F64) if with_dxnew else 0)).abs() + dxnew64)
    sdx = _row_rms(gx)
    if dtype == BF:
        # mirrors ln_mod_bwd_kernel: t = rnd<T>(o) is the dx that feeds res_dy = gate * t and the dgate partials
        dxr, slack = _round_bf16(gx, 1e-5 * gx.abs() + sdx * (1e-5 + B32 * kap2))
        _check("dy", dy, g64[:, None] * dxr, a, b, extra=g64[:, None].abs() * slack)
        _check_colsum("dgate", dgate, (dxr * y64).sum(1), (y64.abs() * (dxr.abs() + sdx * kap2)).sum(1), dtype,
                      extra=(slack * y64.abs()).sum(1))
    else:
        _check("dy", dy, gy_, a, b, kappa=kap2)
        _check_colsum("dgate", dgate, gg, (y64.abs() * (gx.abs() + sdx * kap2)).sum(1), dtype)
    xh = ((xn_k - mu2[..., None]) * rs2[..., None]).detach()
    dh64 = dh.to(F64)
    _check_colsum("dscale", dscale, gsc, (dh64.abs() * (xh.abs() + kap2)).sum(1), dtype)
    _check_colsum("dshift", dshift, gsh, dh64.abs().sum(1), dtype)
    if pitched:
        _assert_fence("dgate/dscale/dshift buffer", gbuf, granges)
        _same_bits("modulation buffer (backward)", mbuf, mcopy)
    _, _, (d1, d2, d3) = _grad_buffer(B, C, dtype, pitched, 3)
    again = hip.residual_ln_bwd(xnew, yb, gate, scale, dh, dxnew, mean, rstd, d1, d2, d3)
    for n, u, v in zip(["dx", "dy", "dgate", "dscale", "dshift"], (dx, dy, dgate, dscale, dshift), again):
        _same_bits(n, u, v)


# ---------------------------------------------------------------------------------------------------- gated residual
def _gr_cases():
    cases = []
    for dn in DTYPES:
        for i, C in enumerate([68, 256, 1024] + ([2048] if dn == "bf16" else [])):
            for j, (B, N) in enumerate([(3, 5), (2, 37), (4, 600)]):
                cases.append((dn, C, B, N, (i + j) % 2 == 0))
    cases += [("f32", 1028, 2, 37, True), ("f32", 2048, 2, 37, False), ("bf16", 1028, 3, 5, True)]
    return cases


def _gr_id(case):
    dn, C, B, N, pitched = case
    vf = 8 if dn == "bf16" else 4
    v = vf if C % vf == 0 else 4
    lanes = C // v
    return f"{dn}-C{C}-v{v}-lanes{lanes}{'-overlimit' if lanes > 256 else ''}-{B}x{N}-ch{_chunks(B, N)}-{'pitched' if pitched else 'pitch0'}"


@pytest.mark.parametrize("case", _gr_cases(), ids=_gr_id)
def test_gated_residual(case):
    dn, C, B, N, pitched = case
    dtype = DTYPES[dn]
    hip = _hip()
    a, b = _tol(dtype)
    g = torch.Generator().manual_seed(C + B * N + 3)
    x, y = _rand(g, B, N, C, dtype=dtype), _rand(g, B, N, C, dtype=dtype)
    mbuf, mranges, (gate,) = _mod_buffer(g, B, C, dtype, pitched, 1)
    mcopy = mbuf.clone() if pitched else None
    out = hip.gated_residual_fwd(x, y, gate)
    x64, y64, g64 = x.to(F64), y.to(F64).requires_grad_(), gate.to(F64).requires_grad_()
    gy = g64[:, None] * y64
    # mirrors gated_residual_kernel: x + rnd<T>(gate * y); the product of two bf16 numbers is exact in fp32 and float64 alike
    ref = x64 + (gy.to(BF).to(F64) if dtype == BF else gy)
    _check("out", out, ref.detach(), a, b, mag=(x64.abs() + gy.abs()).detach())

    dout = _rand(g, B, N, C, dtype=dtype)
    gbuf, granges, (dg_dst,) = _grad_buffer(B, C, dtype, pitched, 1)
    vf = 8 if dtype == BF else 4
    try:
        dy, dgate = hip.gated_residual_bwd(y, gate, dout, dg_dst)
    except ValueError:
        # more lanes per token than a workgroup has (include/vsde_hip.h): refusing is allowed, a partial result is not
        if C // (vf if C % vf == 0 else 4) <= 256:
            raise
        if pitched:
            _assert_fence("dgate buffer", gbuf, [])
        return
    gyr, ggr = torch.autograd.grad(gy, [y64, g64], dout.to(F64))
    _check("dy", dy, gyr, a, b)
    _check_colsum("dgate", dgate, ggr, (dout.to(F64).abs() * y64.detach().abs()).sum(1), dtype)
    if pitched:
        _assert_fence("dgate buffer", gbuf, granges)
        _same_bits("modulation buffer", mbuf, mcopy)
    _, _, (d2,) = _grad_buffer(B, C, dtype, pitched, 1)
    again = hip.gated_residual_bwd(y, gate, dout, d2)
    _same_bits("dy", dy, again[0])
    _same_bits("dgate", dgate, again[1])


# ------------------------------------------------------------------------------------------------------------ swiglu
def _sw_cases():
    cases = [(dn, 2, 37, h2) for dn in DTYPES for h2 in (171, 170, 176, 682)]
    cases.append(("f32", 512, 41, 704))   # 20992 x 176 float4 lanes > 8192 workgroups x 256 threads
    return cases


def _sw_id(case):
    dn, B, N, H2 = case
    vf = 8 if dn == "bf16" else 4
    v = vf if H2 % vf == 0 else (2 if H2 % 2 == 0 else 1)
    grid = -(-B * N * H2 // v // 256)
    return f"{dn}-H2_{H2}-v{v}-M{B * N}" + ("-gridstride" if grid > 8192 else "")


@pytest.mark.parametrize("case", _sw_cases(), ids=_sw_id)
def test_swiglu(case):
    dn, B, N, H2 = case
    dtype = DTYPES[dn]
    hip = _hip()
    a, b = _tol(dtype, a32=4e-6)
    g = torch.Generator().manual_seed(H2 + B)
    a_ = torch.randn(B, N, H2, generator=g, dtype=F64) * 3
    a_[..., ::7] = torch.rand(B, N, len(range(0, H2, 7)), generator=g, dtype=F64) * 60 - 30   # saturated sigmoid
    u = torch.cat([a_, torch.randn(B, N, H2, generator=g, dtype=F64)], -1).to(DEV, dtype)
    out = hip.swiglu_fwd(u)
    u64 = u.to(F64).requires_grad_()
    av, bv = u64[..., :H2], u64[..., H2:]
    silu = av * torch.sigmoid(av)
    if dtype == BF:
        sr, slack = _round_bf16(silu.detach(), 4e-6 * silu.detach().abs())   # mirrors swiglu_fwd_kernel: rnd<T>(a * sigm(a)) * b
        _check("out", out, sr * bv.detach(), a, b, extra=bv.detach().abs() * slack)
    else:
        _check("out", out, (silu * bv).detach(), a, b)
    dout = _rand(g, B, N, H2, dtype=dtype)
    du = hip.swiglu_bwd(u, dout)
    (gu,) = torch.autograd.grad(silu * bv, [u64], dout.to(F64))
    with torch.no_grad():
        sg = torch.sigmoid(av)
        cancel = (dout.to(F64) * bv * sg).abs() * (1 + av.abs() * (1 - sg))   # da = g b sg (1 + a (1 - sg)) cancels near a = -1.28
    _check("da", du[..., :H2], gu[..., :H2], a, b, extra=4e-6 * cancel)
    _check("db", du[..., H2:], gu[..., H2:], a, b)


# -------------------------------------------------------------------------------------------------------- gate merge
def _gm_cases():
    return [(dn, tm, d, (1, 3, 4)[(i + tm) % 3]) for dn in DTYPES for tm in (0, 1) for i, d in enumerate((4, 32, 64, 128))]


def _gm_id(case):
    dn, tm, d, h = case
    vf = 8 if dn == "bf16" else 4
    return f"{dn}-tm{tm}-d{d}-v{vf if d % vf == 0 else 1}-h{h}-gpitch{d + 16}"


def _heads_layout(t, tm):
    """[B, N, h, d] -> the kernel's per-head layout (token-major, or [B, h, N, d])."""
    return t if tm else t.permute(0, 2, 1, 3)


@pytest.mark.parametrize("case", _gm_cases(), ids=_gm_id)
def test_gate_merge(case):
    dn, tm, d, h = case
    dtype = DTYPES[dn]
    hip = _hip()
    a, b = _tol(dtype, a32=4e-6)
    B, N = 2, 37
    g = torch.Generator().manual_seed(d * 5 + h + tm)
    attn_bnhd = _rand(g, B, N, h, d, dtype=dtype)
    attn = _heads_layout(attn_bnhd, tm).contiguous()
    rng = [(8, 8 + d)]
    gbuf, (glog,) = _fenced((B, N, d + 16), dtype, rng, [_rand(g, B, N, d, scale=2.0, dtype=dtype)])
    gcopy = gbuf.clone()
    out = hip.gate_merge_fwd(attn, glog, token_major=bool(tm))
    a64 = attn_bnhd.to(F64).requires_grad_()
    gl64 = glog.to(F64).requires_grad_()
    sg = torch.sigmoid(gl64)
    if dtype == BF:
        sr, slack = _round_bf16(sg.detach(), 4e-6 * sg.detach())   # mirrors gate_merge_fwd_kernel: av * rnd<T>(sigm(gl))
        ref = (a64.detach() * sr[:, :, None]).reshape(B, N, h * d)
        _check("out", out, ref, a, b, extra=(a64.detach().abs() * slack[:, :, None]).reshape(B, N, h * d))
    else:
        _check("out", out, (a64 * sg[:, :, None]).detach().reshape(B, N, h * d), a, b)
    _same_bits("glog buffer", gbuf, gcopy)

    dout = _rand(g, B, N, h * d, dtype=dtype)
    dbuf, (dglog_dst,) = _fenced((B, N, d + 16), dtype, rng)
    dattn, dglog = hip.gate_merge_bwd(attn, glog, dout, token_major=bool(tm), dglog=dglog_dst)
    ga, gg = torch.autograd.grad(a64 * sg[:, :, None], [a64, gl64], dout.to(F64).view(B, N, h, d))
    _check("dattn", dattn, _heads_layout(ga, tm), a, b)
    with torch.no_grad():
        ga_sum = (dout.to(F64).view(B, N, h, d) * a64).abs().sum(2)
        # 1 - sg of an fp32 sigmoid near 1 carries an absolute error of order 2^-24: relative, it grows like 1 / (1 - sg)
        slack = 4e-6 * sg * (1 - sg) * ga_sum + 2.0 ** -22 * sg * ga_sum
    _check("dglog", dglog, gg, a, b, extra=slack)
    _assert_fence("dglog buffer", dbuf, rng)
    _same_bits("glog buffer", gbuf, gcopy)


# ---------------------------------------------------------------------------------------------------- qk_norm_rope
QK_EPS = 1e-6


def _qk_cases():
    cases = []
    for dn in DTYPES:
        for i, d in enumerate((2, 4, 8, 32, 64, 128)):
            cases.append((dn, d, (1, 3, 4)[i % 3], (i + (dn == "bf16")) % 2, ("nov0", "v0", "acc")[(i + 2 * (dn == "bf16")) % 3], 2, 37))
    cases += [("f32", 64, 4, 1, "acc", 5, 333), ("bf16", 64, 4, 0, "v0", 5, 333)]   # 208+ dlam partials
    return cases


def _qk_id(case):
    dn, d, h, tm, mode, B, N = case
    pv = 4 if (d // 2) % 4 == 0 else 1
    threads = B * N * h * (d // 2 // pv)
    return f"{dn}-d{d}-pv{pv}-lanes{d // 2 // pv}-h{h}-tm{tm}-{mode}-{B}x{N}-parts{-(-threads // 256)}-tail{threads % 256}"


def _rotate(xn, cos, sin):
    """rotate-half RoPE of [B, N, h, d] rows with [N, d/2] tables"""
    half = xn.shape[-1] // 2
    lo, hi = xn[..., :half], xn[..., half:]
    c, s = cos[None, :, None, :], sin[None, :, None, :]
    return torch.cat([lo * c - hi * s, lo * s + hi * c], -1)


@pytest.mark.parametrize("case", _qk_cases(), ids=_qk_id)
def test_qk_norm_rope(case):
    dn, d, h, tm, mode, B, N = case
    dtype = DTYPES[dn]
    hip = _hip()
    a, b = _tol(dtype)
    C, half = h * d, d // 2
    g = torch.Generator().manual_seed(d * 13 + h * 3 + tm + B)
    rng = [(8, 8 + 3 * C)]
    qbuf, (qkv,) = _fenced((B, N, 3 * C + 16), dtype, rng, [_rand(g, B, N, 3 * C, dtype=dtype)])
    qcopy = qbuf.clone()
    ang = torch.arange(N, dtype=F64)[:, None] * (1e4 ** (-torch.arange(half, dtype=F64) / half))[None]
    cos, sin = torch.cos(ang).to(DEV, torch.float32), torch.sin(ang).to(DEV, torch.float32)
    wq = (1 + 0.2 * torch.randn(d, generator=g, dtype=F64)).to(DEV, torch.float32)
    wk = (1 + 0.2 * torch.randn(d, generator=g, dtype=F64)).to(DEV, torch.float32)
    with_v0 = mode != "nov0"
    lam = torch.tensor([0.3], device=DEV, dtype=torch.float32)
    v0 = _heads_layout(_rand(g, B, N, h, d, dtype=dtype), tm).contiguous() if with_v0 else None

    q, k, v = hip.qk_norm_rope_fwd(qkv, cos, sin, wq, wk, v0, lam if with_v0 else None, h, QK_EPS, token_major=bool(tm))
    x64 = qkv.to(F64).requires_grad_()
    lam64 = lam.to(F64).requires_grad_()
    v064 = v0.to(F64).requires_grad_() if with_v0 else None
    c64, s64 = cos.to(F64), sin.to(F64)
    raw = x64.view(B, N, 3, h, d)
    outs = []
    for t, w in ((0, wq), (1, wk)):
        xr = raw[:, :, t]
        xn = xr * torch.rsqrt(xr.pow(2).mean(-1, keepdim=True) + QK_EPS) * w.to(F64)   # the RMS of primitives/norm.py
        ref = _rotate(xn, c64, s64)
        outs.append(ref)
        if dtype == BF:
            # mirrors qk_norm_rope_fwd_kernel: a0 / a1 = rnd<T>(x * r * w) before the rotation
            xr_, slack = _round_bf16(xn.detach(), 2e-6 * xn.detach().abs())
            sl_lo, sl_hi = slack[..., :half], slack[..., half:]
            cc, ss = c64[None, :, None, :].abs(), s64[None, :, None, :].abs()
            extra = torch.cat([cc * sl_lo + ss * sl_hi, ss * sl_lo + cc * sl_hi], -1)
            _check("qk"[t], (q, k)[t], _heads_layout(_rotate(xr_, c64, s64), tm), a, b, extra=_heads_layout(extra, tm))
        else:
            _check("qk"[t], (q, k)[t], _heads_layout(ref.detach(), tm), a, b)
    vr = raw[:, :, 2]
    if with_v0:
        v0b = _heads_layout(v064, tm)
        vref = lam64 * vr + (1 - lam64) * v0b
        _check("v", v, _heads_layout(vref.detach(), tm), a, b, mag=_heads_layout((0.3 * vr.abs() + 0.7 * v0b.abs()).detach(), tm))
    else:
        vref = vr
        _check("v", v, _heads_layout(vref.detach(), tm), a, b)
    _same_bits("qkv buffer (forward)", qbuf, qcopy)

    dq, dk, dv = (_heads_layout(_rand(g, B, N, h, d, dtype=dtype), tm).contiguous() for _ in range(3))
    dv_extra = _heads_layout(_rand(g, B, N, h, d, dtype=dtype), tm).contiguous() if mode == "acc" else None
    dv0_init = _heads_layout(_rand(g, B, N, h, d, dtype=dtype), tm).contiguous() if mode == "acc" else None

    def bwd():
        dbuf, (dqkv_dst,) = _fenced((B, N, 3 * C + 16), dtype, rng)
        r = hip.qk_norm_rope_bwd(qkv, cos, sin, wq, wk, v0, lam if with_v0 else None, dq, dk, dv, h, QK_EPS, token_major=bool(tm),
                                 dqkv=dqkv_dst, dv0=None if dv0_init is None else dv0_init.clone(), dv_extra=dv_extra)
        return dbuf, r

    dbuf, (dqkv, dv0, dlam) = bwd()
    gvv = dv.to(F64) + (dv_extra.to(F64) if dv_extra is not None else 0)
    if dtype == BF and dv_extra is not None:
        gvv = gvv.to(BF).to(F64)   # mirrors qk_norm_rope_bwd_kernel: g0 = rnd<T>(g0 + e0), exact in fp32 for bf16 operands
    grads_out = [_heads_layout(t.to(F64), tm) for t in (dq, dk)]   # the layout map is its own inverse
    gv_bnhd = _heads_layout(gvv, tm)
    leaves = [x64] + ([v064, lam64] if with_v0 else [])
    gr = torch.autograd.grad([outs[0], outs[1], vref], leaves, grads_out + [gv_bnhd])
    with torch.no_grad():   # RMS backward r w gy - x r^3 mean(x w gy): the two terms cancel (fully along x), so bound by their sizes
        mags = []
        for t, w, go in ((0, wq, grads_out[0]), (1, wk, grads_out[1])):
            xr, c, s_ = raw[:, :, t], c64[None, :, None, :], s64[None, :, None, :]
            lo, hi = go[..., :half], go[..., half:]
            wgy = (torch.cat([lo * c + hi * s_, -lo * s_ + hi * c], -1) * w.to(F64)).abs()   # inverse rotation
            r = torch.rsqrt(xr.pow(2).mean(-1, keepdim=True) + QK_EPS)
            mags.append(r * wgy + xr.abs() * r ** 3 * (xr.abs() * wgy).mean(-1, keepdim=True))
        mags.append(gr[0].view(B, N, 3, h, d)[:, :, 2].abs())
        mag = torch.stack(mags, 2).reshape(B, N, 3 * C)
    _check("dqkv", dqkv, gr[0], a, b, mag=mag)
    _assert_fence("dqkv buffer", dbuf, rng)
    _same_bits("qkv buffer (backward)", qbuf, qcopy)
    if with_v0:
        if mode == "acc":
            y0 = dv0_init.to(F64)
            if dtype == BF:
                # mirrors qk_norm_rope_bwd_kernel: y0 + rnd<T>((1 - l) * g0), the product formed in fp32
                z = ((torch.ones_like(lam) - lam) * gvv.to(torch.float32)).to(BF).to(F64)
            else:
                z = (1 - lam64.detach()) * gvv
            _check("dv0", dv0, y0 + z, a, b, mag=y0.abs() + z.abs())
        else:
            _check("dv0", dv0, gr[1], a, b)   # v0 (and so its gradient) is in the kernel's layout
        terms = (gv_bnhd * (vr - v0b)).detach().abs().sum()
        _check_colsum("dlam", dlam.reshape(1), gr[2].reshape(1), terms.reshape(1), torch.float32)
    else:
        assert dv0 is None and dlam is None
    _, again = bwd()
    _same_bits("dqkv", dqkv, again[0])
    if with_v0:
        _same_bits("dv0", dv0, again[1])
        _same_bits("dlam", dlam, again[2])


# ---------------------------------------------------------------------------------- fused route vs norm dispatch
@pytest.mark.parametrize("dn", list(DTYPES))
def test_usable_matches_norm_dispatch(dn):
    """fused.usable() admits exactly the encoder widths the LayerNorm kernels accept (C = 64 .. 1024 in steps of 64)."""
    from viforsdes_amd.primitives import fused
    dtype = DTYPES[dn]
    hip = _hip()
    accepted = []
    for C in range(64, 1025, 64):
        x = torch.zeros(1, 2, C, device=DEV, dtype=dtype)
        sc = torch.zeros(1, C, device=DEV, dtype=dtype)
        try:
            hip.ln_modulate_fwd(x, sc, sc, EPS_LN)
            ok = True
        except ValueError:
            ok = False
        assert fused.usable(x, C, 64) == ok, (C, ok)
        if ok:
            accepted.append(C)
    assert accepted == LN_CS


def test_encoder_width_outside_norm_dispatch_takes_torch_route(monkeypatch):
    """hidden_dim 320 has no LayerNorm kernel branch: the block must take the torch chain, forward and backward."""
    from viforsdes_amd import EncoderConfig, _hip as hip
    from viforsdes_amd.models.encoder import ObservationContextEncoder
    from viforsdes_amd.primitives import fused
    torch.manual_seed(3)
    enc = ObservationContextEncoder(2, 3, EncoderConfig(hidden_dim=320, num_heads=5, depth=1)).to(DEV).train()
    calls = []
    real = hip.ln_modulate_fwd
    monkeypatch.setattr(hip, "ln_modulate_fwd", lambda *a: calls.append(1) or real(*a))
    g = torch.Generator().manual_seed(4)
    obs_t = torch.tensor([0.0, 0.7, 1.4, 2.0], device=DEV)
    obs_v = torch.randn(4, 2, generator=g).to(DEV)
    theta = (torch.rand(4, 3, generator=g) + 0.2).to(DEV)
    gout = torch.randn(4, 41, 320, generator=g).to(DEV)
    params = [p for p in enc.parameters() if p.requires_grad]

    def run():
        th = theta.clone().requires_grad_(True)
        ctx = enc(obs_v, obs_t, th, 2.0, 0.05)
        return [ctx.detach()] + list(torch.autograd.grad((ctx * gout).sum(), [th] + params))

    got = run()
    assert not calls, "the fused LayerNorm kernel was called for C = 320"
    fused.ENABLED = False
    try:
        want = run()
    finally:
        fused.ENABLED = True
    for i, (u, w) in enumerate(zip(got, want)):
        assert bool(torch.isfinite(u).all()), i
        torch.testing.assert_close(u, w, rtol=1e-5, atol=1e-5 * float(w.abs().max()) + 1e-12)
