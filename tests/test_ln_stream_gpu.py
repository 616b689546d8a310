"""The streaming form of ln_mod_fwd_kernel / ln_mod_bwd_kernel (csrc/vsde_encoder.hip) against the kernel bodies it replaced.

The tools' library keeps the earlier bodies (hand-written bf16 rounding, no look-ahead in the backward, a division per token in
the forward) behind VSDE_LN_STREAM=0.  The streaming form changes when values are loaded and how they are converted, not what is
computed or in which order it is summed, so every output must agree bit for bit: y / h, xnew, mean, rstd, dx, res_dy (dy) and
the token sums dscale / dshift / dgate.  Both backward passes read the statistics (and xnew) of one forward, so a difference in the
forward does not show up a second time in the backward's outputs; every differing output of a case is named in one failure.

Cases (B, N) at C = 256 bf16 (two tokens per wavefront): (2, 1) one token; (3, 5) one chunk, a group of 8 partly filled;
(2, 37) 4 chunks, the last one ragged (the clamped look-ahead ends there); (4, 600) 64 chunks, the last 4 empty; (1024, 41) the
grid-stride forward, the batch row changes inside one workgroup's walk.  Each with dres / dxnew present and absent and with the
per-row vectors contiguous and as column ranges of a NaN-filled [B, 6*2*C] buffer.  C = 128 and 512 bf16 and C = 256 fp32 run
(2, 37) once, and so do C = 64 (one channel per lane) and C = 192 / 768 / 1024 (two to four slabs per lane).  Every case with N >= 2 has one constant row and one row of mean 1e3, as test_encoder_ops_gpu.py builds them.
"""
import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.ablation_build]
DEV = "cuda:0"
BF = torch.bfloat16
EPS_LN = 1e-5
KNOB = "VSDE_LN_STREAM"
SENTINEL = {torch.float32: (torch.int32, 0x7FC0DEAD), BF: (torch.int16, 0x7FDE)}   # quiet NaNs with a payload

SHAPES = [(2, 1), (3, 5), (2, 37), (4, 600), (1024, 41)]
CASES = [("bf16", 256, B, N, dres, pitched) for (B, N) in SHAPES for dres in (True, False) for pitched in (False, True)]
CASES += [("bf16", 128, 2, 37, True, True), ("bf16", 512, 2, 37, True, True), ("f32", 256, 2, 37, True, True)]
# every other dispatch of the two kernels (test_encoder_ops_gpu.py lists them): which products the compiler had contracted in the
# replaced bodies depends on the vector width and on the slab, and the streaming form writes each of those choices out
CASES += [(dn, C, 2, 37, i % 2 == 0, True) for dn in ("bf16", "f32") for i, C in enumerate([64, 128, 192, 256, 384, 512, 768, 1024])
          if (dn, C) not in {(c[0], c[1]) for c in CASES}]


def _id(case):
    dn, C, B, N, dres, pitched = case
    return f"{dn}-C{C}-{B}x{N}-{'dres' if dres else 'nodres'}-{'pitched' if pitched else 'pitch0'}"


def _rand(g, *shape, scale=1.0, dtype=torch.float32):
    return (torch.randn(*shape, generator=g, dtype=torch.float64) * scale).to(DEV, dtype)


def _x(g, B, N, C, dtype):
    x = torch.randn(B, N, C, generator=g, dtype=torch.float64)
    if N >= 2:
        x[0, 0] = 2.5                                                        # constant row: var = 0
        x[0, 1] = 1e3 + torch.randn(C, generator=g, dtype=torch.float64)     # mean 1e3, std 1
    return x.to(DEV, dtype)


def _vectors(g, B, C, dtype, pitched, k, fill=True):
    """k [B, C] vectors: contiguous, or column ranges of one NaN-filled [B, 12 C] buffer."""
    if not pitched:
        return [_rand(g, B, C, scale=0.5, dtype=dtype) if fill else None for _ in range(k)]
    idt, bits = SENTINEL[dtype]
    buf = torch.full((B, 12 * C), bits, dtype=idt, device=DEV).view(dtype)
    views = [buf[:, (1 + 2 * i) * C:(2 + 2 * i) * C] for i in range(k)]
    if fill:
        for v in views:
            v.copy_(_rand(g, B, C, scale=0.5, dtype=dtype))
    return views


def _both(monkeypatch, fn):
    """fn() on the replaced kernel bodies (knob 0) and on the shipped form (knob unset)."""
    monkeypatch.setenv(KNOB, "0")
    old = fn()
    monkeypatch.delenv(KNOB)
    new = fn()
    torch.cuda.synchronize()
    return old, new


def _same(names, old, new):
    bad = []
    for n, a, b in zip(names, old, new):
        assert a.shape == b.shape and a.dtype == b.dtype, n
        assert bool(torch.isfinite(b.float()).all()), f"{n}: not finite"
        if not torch.equal(a, b):
            bad.append(f"{n}: {int((a != b).sum())} of {a.numel()}")
    assert not bad, "elements that differ from the replaced kernel's -- " + "; ".join(bad)


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_ln_modulate_streams_bit_identically(case, monkeypatch):
    from viforsdes_amd import _hip
    dn, C, B, N, with_dres, pitched = case
    dtype = BF if dn == "bf16" else torch.float32
    g = torch.Generator().manual_seed(C * 13 + B * N)
    x = _x(g, B, N, C, dtype)
    scale, shift = _vectors(g, B, C, dtype, pitched, 2)
    dy = _rand(g, B, N, C, dtype=dtype)
    dres = _rand(g, B, N, C, dtype=dtype) if with_dres else None

    monkeypatch.setenv(KNOB, "0")
    _, mean0, rstd0 = _hip.ln_modulate_fwd(x, scale, shift, EPS_LN)   # both backward passes read the same statistics

    def run():
        y, mean, rstd = _hip.ln_modulate_fwd(x, scale, shift, EPS_LN)
        dsc, dsh = _vectors(g, B, C, dtype, pitched, 2, fill=False)
        dx, dscale, dshift = _hip.ln_modulate_bwd(x, scale, dy, mean0, rstd0, dres, dsc, dsh)
        return y, mean, rstd, dx, dscale, dshift

    old, new = _both(monkeypatch, run)
    _same(["y", "mean", "rstd", "dx", "dscale", "dshift"], old, new)


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_residual_ln_streams_bit_identically(case, monkeypatch):
    from viforsdes_amd import _hip
    dn, C, B, N, with_dxnew, pitched = case
    dtype = BF if dn == "bf16" else torch.float32
    g = torch.Generator().manual_seed(C * 17 + B * N + 1)
    x = _x(g, B, N, C, dtype)
    yb = _rand(g, B, N, C, dtype=dtype)
    yb[0, :2] = 0   # the constant and the cancellation row of x reach the norm unchanged
    gate, scale, shift = _vectors(g, B, C, dtype, pitched, 3)
    dh = _rand(g, B, N, C, dtype=dtype)
    dxnew = _rand(g, B, N, C, dtype=dtype) if with_dxnew else None

    monkeypatch.setenv(KNOB, "0")
    xnew0, _, mean0, rstd0 = _hip.residual_ln_fwd(x, yb, gate, scale, shift, EPS_LN)   # what both backward passes read

    def run():
        xnew, h, mean, rstd = _hip.residual_ln_fwd(x, yb, gate, scale, shift, EPS_LN)
        dg, dsc, dsh = _vectors(g, B, C, dtype, pitched, 3, fill=False)
        dx, dy, dgate, dscale, dshift = _hip.residual_ln_bwd(xnew0, yb, gate, scale, dh, dxnew, mean0, rstd0, dg, dsc, dsh)
        return xnew, h, mean, rstd, dx, dy, dgate, dscale, dshift

    old, new = _both(monkeypatch, run)
    _same(["xnew", "h", "mean", "rstd", "dx", "res_dy", "dgate", "dscale", "dshift"], old, new)


def test_nan_inputs_give_nans_in_the_same_places(monkeypatch):
    """The packed hardware conversion and the hand-written one both turn a NaN into a quiet bf16 NaN: with NaNs in x and in the
    residual branch, the bf16 outputs of both forms are NaN at the same elements and equal everywhere else."""
    from viforsdes_amd import _hip
    B, N, C = 2, 37, 256
    g = torch.Generator().manual_seed(5)
    x, yb = _x(g, B, N, C, BF), _rand(g, B, N, C, dtype=BF)
    x[1, 3, 7] = float("nan")
    yb[0, 9, 100] = float("nan")
    gate, scale, shift = _vectors(g, B, C, BF, False, 3)
    dh, dxnew = _rand(g, B, N, C, dtype=BF), _rand(g, B, N, C, dtype=BF)

    def run():
        xnew, h, mean, rstd = _hip.residual_ln_fwd(x, yb, gate, scale, shift, EPS_LN)
        dx, dy, *_ = _hip.residual_ln_bwd(xnew, yb, gate, scale, dh, dxnew, mean, rstd)
        return xnew, h, dx, dy

    old, new = _both(monkeypatch, run)
    for n, a, b in zip(["xnew", "h", "dx", "res_dy"], old, new):
        nan = torch.isnan(a)
        assert bool(nan.any()) and torch.equal(nan, torch.isnan(b)), n
        assert torch.equal(a[~nan], b[~nan]), n
        assert bool(((b[nan].view(torch.int16) & 0x7FC0) == 0x7FC0).all()), f"{n}: a NaN that is not quiet"
