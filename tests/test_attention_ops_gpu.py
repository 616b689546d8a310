"""Every dispatch of the attention kernels against float64, element by element.

Each case calls one ``viforsdes_amd._hip`` wrapper, so it pins one kernel, and compares every element with the float64
reference of tests/attention_reference.py; the bounds (per element, never relative to a tensor's maximum) are listed and
justified in that module's docstring.  Backward kernels are teacher-forced on the kernel's own forward state (o, lse, delta,
the saved rows), so a defect cannot cancel against the same defect in a reference route.

Fences.  Pitched operands and destinations (the gate factors s, the projection gradient dy with its gate columns, the
dgate columns, x of the projection) are column ranges at a non-zero offset of buffers filled with a NaN sentinel: a read
outside the range turns an output into NaN, and every element outside the written range must still be the sentinel (or the
pre-filled gate columns), bit for bit.  Determinism: every call runs twice, and the results must be bitwise equal.

Dispatch coverage (test ids in brackets), derived from the launch code:
  attention_fwd / attention_fwd_gated (launch_attn_fwd, vsde_attention_fwd_bf16; npad = N rounded up to 32):
    [wave4]    npad <= 128: four-wave workgroups                           N 1, 31, 32, 33, 101, 128
    [wave12]   one twelve-wave workgroup per (batch, head) pair            N 129, 385, 401, 416, 417, 544 (two query rounds
               past 384), and npad <= 416 with B H < 2 x CUs
    [persist]  npad <= 416 and B H >= 2 x CUs (CU count read from the device): persistent workgroups that carry their state
               from one pair to the next                                  N 129, 385, 401, 416
    [stream]   N > 544 or head_dim 128 (vsde_attn_stream.hip)              N 545, 1001 (D 128), 101 (D 128); the online-softmax
               rescale forced by growing key norms [rescale]
    exact pass (the Cauchy-Schwarz shift would underflow): every query scaled [exact-all] and one 32-query block of one pair
    scaled [exact-block] (exact and fast waves in one workgroup); on the persistent kernel only one pair is scaled, its
    neighbours stay on the fast path
  attention_bwd: resident (dq / dk dv kernels, one or two rounds of 32-token blocks per wave: N <= 384 / > 384) and streamed,
    teacher-forced on the kernel's own o and lse; the same N table
  gate_bwd_delta: M small and M >= 65,536, s / dgate row-pitched inside sentinel buffers
  linear_gate_bwd: K 128 / 256, M small and >= 65,536 (eight-wave rows), dgate = the gate columns of a fenced dy buffer
  linear_gated_bf16: K 128 / 256 (heads 2 / 4), N 128 / 256 output columns, M small and >= 65,536
  linear_qknorm_bf16 (launch_rows_nw, 128-row stripes, 512 resident workgroups):
    [pairchunk] M 12,928: fewer stripes than resident workgroups -> column chunks of tile pairs
    [round]     M 65,536 / 103,936: one or more full rounds, no tail (last round empty, or more than half full)
    [tail]      M 205,312 (the LV shape): the last round's stripes in finer column chunks
    K 128 / 256, heads 2 / 4, with and without v0, save on and off, x a column range of a sentinel buffer
  attention_bwd_fused (vsde_attention_bwd_fused_bf16, 12 waves x 32 tokens):
    [wave4]   N 31, 101, 128                    four-wave workgroups
    [one]     N 129, 384                        one block per wave, lean instantiation
    [split]   N 385, 402, 403, 416              one block more than waves, shared by four waves (nragged 1, 18, 19, 32:
                                                dq shared; dk / dv shared only while the partial tiles fit)
    [two]     N 417, 430, 544                   two rounds; the first-round tiles parked in spare LDS where they fit
    and the LV shape (B 512, N 401, 4 heads) once.  RMS weights: unit, 1 +- 0.3 N(0, 1), and one channel (negative) at the
    limit max|w| / 16 that ``fused.norm_weights_fusable`` admits [limit]; no value mix, with or without an extra value gradient [none |
    extra], value mix [v0], value mix accumulating onto an existing dv0 with an extra value gradient [acc]
"""
import math

import pytest
import torch

import attention_reference as ar

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64 = torch.float64
BF = torch.bfloat16
SENT = (torch.int16, 0x7FDE)   # a quiet bf16 NaN with a payload
EPS = 1e-6
WORST: dict = {}


def _hip():
    from viforsdes_amd import _hip
    return _hip


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _rand(g, *shape, scale=1.0, dtype=BF):
    return (torch.randn(*shape, generator=g, dtype=F64) * scale).to(DEV, dtype)


def _sentinel(shape, dtype=BF):
    if dtype == BF:
        return torch.full(shape, SENT[1], dtype=SENT[0], device=DEV).view(BF)
    return torch.full(shape, 0x7FC0DEAD, dtype=torch.int32, device=DEV).view(torch.float32)


def _fence_ok(name, buf, lo, hi):
    raw = buf.view(SENT[0])
    bad = int((raw[:, :lo] != SENT[1]).sum()) + int((raw[:, hi:] != SENT[1]).sum())
    assert bad == 0, f"{name}: {bad} elements outside columns [{lo}, {hi}) changed"


def _same_bits(name, a, b):
    if a is None:
        assert b is None, name
        return
    assert torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8)), f"{name}: not bitwise reproducible"


def _check(kernel, name, got, ref, bound):
    n, worst, idx = ar.excess(got, ref, bound)
    key = f"{kernel}.{name}"
    WORST[key] = max(WORST.get(key, 0.0), worst if math.isfinite(worst) else float("inf"))
    print(f"RATIO {key} {worst:.3g}")
    if n:
        raise AssertionError(f"{key}: {n} of {got.numel()} elements out of bound (worst err/bound {worst:.3g}); first at {idx}: "
                             f"got {float(got[idx])!r}, ref {float(ref[idx])!r}, bound {float(bound[idx]):.3g}")


def fwd_branch(B, N, H, D):
    """The kernel launch_attn_fwd / vsde_attention_fwd_bf16 pick for this shape."""
    if D != 64 or N > 544:
        return "stream"
    npad = (N + 31) // 32 * 32
    if npad <= 128:
        return "wave4"
    if npad <= 416 and B * H >= 2 * _cus():
        return "persist"
    return "wave12"


# --------------------------------------------------------------------------------------------------- forward / backward
# (B, N, H, D); B = 0: the smallest batch that makes the launch persistent (B H >= 2 x CUs, plus a partial last sweep)
ATT_SHAPES = [(3, 1, 2, 64), (5, 31, 1, 64), (4, 32, 4, 64), (4, 33, 2, 64), (6, 101, 4, 64), (3, 128, 1, 64),
              (3, 129, 2, 64), (2, 385, 4, 64), (2, 401, 1, 64), (2, 416, 2, 64), (2, 417, 4, 64), (2, 544, 1, 64),
              (0, 129, 4, 64), (0, 385, 2, 64), (0, 401, 4, 64), (0, 416, 1, 64),
              (2, 545, 2, 64), (2, 1001, 4, 128), (3, 101, 2, 128)]
EXACT_SHAPES = [(6, 101, 4, 64), (2, 401, 4, 64), (2, 544, 1, 64), (0, 401, 4, 64), (0, 129, 4, 64)]


def _batch(B, H):
    return B if B else (2 * _cus() + H - 1) // H + 1


def _att_inputs(seed, B, N, H, D, kind="rand"):
    g = torch.Generator().manual_seed(seed)
    q, k, v = (torch.randn(B, N, H, D, generator=g, dtype=F64) for _ in range(3))
    pb, ph = min(1, B - 1), H - 1     # the pair the exact cases scale
    if kind == "exact-all":
        if B * H >= 2 * _cus():
            q[pb, :, ph] *= 6.0
        else:
            q *= 6.0
    elif kind == "exact-block":
        q[pb, 32:64, ph] *= 6.0
    elif kind == "rescale":
        k = k * torch.linspace(0.2, 3.0, N, dtype=F64).view(1, N, 1, 1)
        k[:, N - 50] = q[:, 7] * 3.0
        q[:, 7] *= 1.5
    return tuple(t.to(DEV, BF) for t in (q, k, v))


def _gate(g, M, width=96, off=16):
    """sigmoid gate factors s [M, 64] as a column range of a sentinel buffer [M, width]."""
    buf = _sentinel((M, width))
    s = buf[:, off:off + 64]
    s.copy_(torch.sigmoid(torch.randn(M, 64, generator=g, dtype=F64) * 2).to(DEV, BF))
    return buf, s


def _att_cases():
    cases = [(B, N, H, D, "rand", False) for B, N, H, D in ATT_SHAPES]
    cases += [(B, N, H, D, "rand", True) for B, N, H, D in ATT_SHAPES if D == 64 and N <= 544]
    for B, N, H, D in EXACT_SHAPES:
        cases += [(B, N, H, D, "exact-all", B == 0), (B, N, H, D, "exact-block", B != 0)]
    cases.append((2, 600, 2, 64, "rescale", False))
    return cases


def _att_id(c):
    B, N, H, D, kind, gated = c
    return f"{'P' if B == 0 else B}x{N}h{H}d{D}-{kind}{'-gated' if gated else ''}"


@pytest.mark.parametrize("case", _att_cases(), ids=_att_id)
def test_attention_fwd(case):
    B, N, H, D, kind, gated = case
    B = _batch(B, H)
    hip = _hip()
    q, k, v = _att_inputs(B * 7 + N + H, B, N, H, D, kind)
    scale = D ** -0.5
    print(f"branch {fwd_branch(B, N, H, D)}")
    if gated:
        gbuf, s = _gate(torch.Generator().manual_seed(N), B * N)
        gcopy = gbuf.clone()
        o, lse = hip.attention_fwd_gated(q, k, v, s, scale)
        o2, lse2 = hip.attention_fwd_gated(q, k, v, s, scale)
        _same_bits("gate buffer", gbuf, gcopy)
    else:
        s = None
        o, lse = hip.attention_fwd(q, k, v, scale)
        o2, lse2 = hip.attention_fwd(q, k, v, scale)
    _same_bits("o", o, o2)
    _same_bits("lse", lse, lse2)
    ref, bo, lref, bl = ar.attention_fwd_ref(q, k, v, scale, s)
    name = "attention_fwd_gated" if gated else "attention_fwd"
    _check(name, "o", o, ref, bo)
    _check(name, "lse", lse, lref, bl)


BWD_SHAPES = [(3, 1, 2, 64), (5, 31, 1, 64), (4, 33, 2, 64), (6, 101, 4, 64), (3, 128, 1, 64), (3, 129, 2, 64),
              (2, 385, 4, 64), (2, 401, 4, 64), (2, 416, 2, 64), (2, 417, 1, 64), (2, 544, 2, 64), (2, 545, 2, 64),
              (2, 1001, 4, 128), (3, 101, 2, 128), (4, 32, 4, 64)]


@pytest.mark.parametrize("B,N,H,D", BWD_SHAPES, ids=lambda *a: None)
def test_attention_bwd(B, N, H, D):
    hip = _hip()
    q, k, v = _att_inputs(B * 11 + N + D, B, N, H, D)
    dout = _rand(torch.Generator().manual_seed(N + 1), B, N, H, D)
    scale = D ** -0.5
    o, lse = hip.attention_fwd(q, k, v, scale)
    got = hip.attention_bwd(dout, q, k, v, o, lse, scale)
    again = hip.attention_bwd(dout, q, k, v, o, lse, scale)
    refs = ar.attention_bwd_ref(dout, q, k, v, lse, ar.delta_ref(dout, o), scale)
    for name, t, t2 in zip(("dq", "dk", "dv"), got, again):
        _same_bits(name, t, t2)
        ref, e = refs[name]
        _check("attention_bwd", name, t, ref, e + ar.U * ref.abs())


# ---------------------------------------------------------------------------------------------------------- the gate
@pytest.mark.parametrize("B,N,H", [(3, 37, 2), (4, 401, 4), (164, 401, 1)])
def test_gate_bwd_delta(B, N, H):
    hip = _hip()
    g = torch.Generator().manual_seed(B + N + H)
    M = B * N
    dout, og = _rand(g, B, N, H, 64), _rand(g, B, N, H, 64)
    sbuf, s = _gate(g, M, 112, 32)
    scopy = sbuf.clone()

    def run():
        dbuf = _sentinel((M, 160))
        dattn, delta = hip.gate_bwd_delta(dout, og, s, dbuf[:, 48:112])
        return dbuf, dattn, delta

    dbuf, dattn, delta = run()
    dbuf2, dattn2, delta2 = run()
    _same_bits("dgate", dbuf, dbuf2); _same_bits("dattn", dattn, dattn2); _same_bits("delta", delta, delta2)
    _same_bits("gate buffer", sbuf, scopy)
    _fence_ok("dgate buffer", dbuf, 48, 112)
    ra, ba, rd, bd, rg, bg = ar.gate_bwd_ref(dout, og, s)
    _check("gate_bwd_delta", "dattn", dattn, ra, ba)
    _check("gate_bwd_delta", "delta", delta, rd, bd)
    _check("gate_bwd_delta", "dgate", dbuf[:, 48:112], rg, bg)


@pytest.mark.parametrize("K,H,B,N", [(128, 2, 5, 37), (256, 4, 6, 401), (128, 4, 170, 401), (256, 2, 164, 401)])
def test_linear_gate_bwd(K, H, B, N):
    hip = _hip()
    g = torch.Generator().manual_seed(K + H + B + N)
    M, C = B * N, H * 64
    dy = _rand(g, M, K)
    w_t = _rand(g, C, K, scale=K ** -0.5)
    og = _rand(g, B, N, H, 64)
    sbuf, s = _gate(g, M, 112, 32)
    gcols = (3 * C + 16, 3 * C + 80)

    def run():
        dbuf = _sentinel((M, 3 * C + 96))
        fill = dbuf[:, 16:3 * C + 16]
        fill.copy_(_rand(torch.Generator().manual_seed(1), M, 3 * C))
        dattn, delta = hip.linear_gate_bwd(dy, w_t, og, s, dbuf[:, gcols[0]:gcols[1]], N)
        return dbuf, dattn, delta

    dbuf, dattn, delta = run()
    dbuf2, dattn2, delta2 = run()
    _same_bits("dy buffer", dbuf, dbuf2); _same_bits("dattn", dattn, dattn2); _same_bits("delta", delta, delta2)
    _fence_ok("dy buffer", dbuf, 16, gcols[1])
    _same_bits("dy columns outside the gate", dbuf[:, 16:3 * C + 16], _rand(torch.Generator().manual_seed(1), M, 3 * C))
    G = dy.to(F64) @ w_t.to(F64).t()
    Gr, step = ar.round_bf16(G, 2.0 ** -16 * (dy.to(F64).abs() @ w_t.to(F64).abs().t()))
    Gr, step = Gr.view(B, N, H, 64), step.view(B, N, H, 64)
    ra, ba, rd, bd, rg, bg = ar.gate_bwd_ref(Gr, og, s)
    sg = s.to(F64).view(B, N, 1, 64)
    ogm = og.to(F64).abs()
    _check("linear_gate_bwd", "dattn", dattn, ra, ba + sg * step)
    _check("linear_gate_bwd", "delta", delta, rd, bd + (ogm * step).sum(-1).permute(0, 2, 1))
    _check("linear_gate_bwd", "dgate", dbuf[:, gcols[0]:gcols[1]], rg,
           bg + ((1 - sg[:, :, 0]).abs() * (ogm * step).sum(2)).reshape(M, 64) * (1 + ar.U))


@pytest.mark.parametrize("K,Nout,M", [(128, 128, 4133), (256, 256, 4133), (256, 128, 70001), (128, 256, 65536)])
def test_linear_gated(K, Nout, M):
    hip = _hip()
    g = torch.Generator().manual_seed(K + Nout + M)
    abuf = _sentinel((M, K + 32))
    a = abuf[:, 16:16 + K]
    a.copy_(_rand(g, M, K))
    lbuf = _sentinel((M, 96))
    logit = lbuf[:, 16:80]
    logit.copy_(_rand(g, M, 64, scale=2.0))
    w = _rand(g, Nout, K, scale=K ** -0.5)
    bias = _rand(g, Nout, scale=0.1)
    y = hip.linear_gated_bf16(a, logit, w, bias)
    _same_bits("y", y, hip.linear_gated_bf16(a, logit, w, bias))
    s = torch.sigmoid(logit.to(F64)).repeat(1, K // 64)
    ae = a.to(F64) * s
    ref = ae @ w.to(F64).t() + bias.to(F64)
    mag = ae.abs() @ w.to(F64).abs().t()
    _check("linear_gated_bf16", "y", y, ref, ar.U * mag + ar.U * ref.abs() + 1e-6 * mag)


# ------------------------------------------------------------------------------------------------ projection forward
def _proj_setup(seed, B, N, K, H, with_v0, xpitched=True):
    g = torch.Generator().manual_seed(seed)
    M, C = B * N, H * 64
    if xpitched:
        xbuf = _sentinel((M, K + 64))
        x = xbuf[:, 32:32 + K]
        x.copy_(_rand(g, M, K))
    else:
        xbuf, x = None, _rand(g, M, K)
    w = _rand(g, 3 * C + 64, K, scale=K ** -0.5)
    bias = _rand(g, 3 * C + 64, scale=0.2)
    ang = torch.arange(N, dtype=F64)[:, None] * (10000.0 ** (-torch.arange(32, dtype=F64) / 32))[None]
    cos, sin = ang.cos().to(DEV, torch.float32).contiguous(), ang.sin().to(DEV, torch.float32).contiguous()
    wq = (1 + 0.3 * torch.randn(64, generator=g, dtype=F64)).to(DEV, torch.float32)
    wk = (1 - 0.3 * torch.randn(64, generator=g, dtype=F64)).to(DEV, torch.float32)
    v0 = _rand(g, M, C) if with_v0 else None
    lam = torch.tensor([0.37], device=DEV) if with_v0 else None
    return xbuf, x, w, bias, cos, sin, wq, wk, v0, lam


QK_CASES = [(101, 128, 128, 2, False, "pairchunk"), (101, 128, 256, 4, True, "pairchunk"), (128, 512, 256, 2, True, "round"),
            (259, 401, 128, 4, False, "round"), (512, 401, 256, 4, True, "tail")]


@pytest.mark.parametrize("B,N,K,H,with_v0,regime", QK_CASES, ids=lambda *a: None)
@pytest.mark.parametrize("save", [False, True])
def test_linear_qknorm(B, N, K, H, with_v0, regime, save):
    hip = _hip()
    M, C = B * N, H * 64
    xbuf, x, w, bias, cos, sin, wq, wk, v0, lam = _proj_setup(B + N + K + H, B, N, K, H, with_v0)
    xcopy = xbuf.clone()
    out = hip.linear_qknorm_bf16(x, w, bias, H, N, cos, sin, wq, wk, v0, lam, EPS, save=save)
    again = hip.linear_qknorm_bf16(x, w, bias, H, N, cos, sin, wq, wk, v0, lam, EPS, save=save)
    for i, (a, b) in enumerate(zip(out, again)):
        _same_bits(f"output {i}", a, b)
    _same_bits("x buffer", xbuf, xcopy)
    _, yr, step = ar.projection_ref(x, w, bias)
    shape = (B, N, H, 64)
    for t, (wt, name) in enumerate(((wq, "q"), (wk, "k"))):
        ref, bound, r, br = ar.qknorm_ref(yr[:, t * C:(t + 1) * C].reshape(shape), step[:, t * C:(t + 1) * C].reshape(shape),
                                          wt, cos, sin, EPS)
        _check("linear_qknorm_bf16", name, out[t].view(shape), ref, bound)
        if save:
            _check("linear_qknorm_bf16", "rinv", out[4].view(B, N, 2, H)[:, :, t], r, br)
    yv, sv = yr[:, 2 * C:3 * C], step[:, 2 * C:3 * C]
    if with_v0:
        l = float(lam)
        ref = l * yv + (1 - l) * v0.to(F64)
        _check("linear_qknorm_bf16", "v", out[2], ref, ar.U * (ref.abs() + abs(l) * sv) + abs(l) * sv + 1e-6 * (yv.abs() + v0.to(F64).abs()))
        if save:
            d = yv - v0.to(F64)
            _check("linear_qknorm_bf16", "vdiff", out[5], d, ar.U * (d.abs() + sv) + sv)
    else:
        _check("linear_qknorm_bf16", "v", out[2], yv, ar.U * (yv.abs() + sv) + sv)
        if save:
            assert out[5] is None
    yg, sg = yr[:, 3 * C:], step[:, 3 * C:]
    if save:
        ref = torch.sigmoid(yg)
        _check("linear_qknorm_bf16", "gate", out[3], ref, ar.U * (ref.abs() + sg / 4) + sg / 4 + 1e-6)
    else:
        _check("linear_qknorm_bf16", "logits", out[3], yg, ar.U * (yg.abs() + sg) + sg)


# ------------------------------------------------------------------------------------------------- fused backward
LIMIT = 16.0   # fused.NORM_WEIGHT_RATIO


def _weights(kind, g):
    if kind == "unit":
        return torch.ones(64, dtype=F64), torch.ones(64, dtype=F64)
    wq = 1 + 0.3 * torch.randn(64, generator=g, dtype=F64)
    wk = 1 - 0.3 * torch.randn(64, generator=g, dtype=F64)
    for w in (wq, wk):   # a draw the route would refuse is moved to the limit (the predicate is tested on its own)
        lo = w.abs().max() / LIMIT * 1.001
        w.copy_(torch.where(w.abs() < lo, torch.where(w < 0, -lo, lo), w))
    if kind == "limit":   # one channel of each at the smallest magnitude the route admits, negative
        wq[5] = -wq.abs().max() / LIMIT * 1.001
        wk[40] = -wk.abs().max() / LIMIT * 1.001
    return wq, wk


FUSED_CASES = [(70, 31, 4, "rand", "v0"), (9, 101, 2, "unit", "none"), (7, 128, 4, "limit", "acc"),
               (5, 129, 4, "rand", "acc"), (3, 384, 2, "limit", "v0"),
               (3, 385, 4, "unit", "acc"), (3, 402, 1, "rand", "v0"), (2, 403, 4, "limit", "none"), (3, 416, 2, "rand", "acc"),
               (2, 417, 4, "rand", "extra"), (2, 430, 2, "limit", "acc"), (2, 544, 4, "unit", "v0"),
               (512, 401, 4, "rand", "acc")]


def _fused_branch(N):
    nt = (N + 31) // 32
    return "wave4" if nt <= 4 else "one" if nt <= 12 else "split" if nt == 13 else "two"


@pytest.mark.parametrize("B,N,H,wkind,mix", FUSED_CASES, ids=lambda *a: None)
def test_attention_bwd_fused(B, N, H, wkind, mix):
    from viforsdes_amd.primitives import fused
    hip = _hip()
    print(f"branch {_fused_branch(N)}")
    K, M, C = 256, B * N, H * 64
    g = torch.Generator().manual_seed(B * N + H)
    xbuf, x, w, bias, cos, sin, _, _, v0, lam = _proj_setup(B + N + H, B, N, K, H, mix in ("v0", "acc"), xpitched=False)
    wq, wk = (t.to(DEV, torch.float32) for t in _weights(wkind, g))
    assert fused.norm_weights_fusable(wq) and fused.norm_weights_fusable(wk)
    scale = 64 ** -0.5
    shape = (B, N, H, 64)
    q, k, v, s, rinv, vdiff = hip.linear_qknorm_bf16(x, w, bias, H, N, cos, sin, wq, wk, v0, lam, EPS, save=True)
    q, k, v = q.view(shape), k.view(shape), v.view(shape)
    og, lse = hip.attention_fwd_gated(q, k, v, s, scale)
    dout = _rand(g, *shape)
    ldy = 3 * C + 64 + 16
    pre = _sentinel((M, ldy))
    dattn, delta = hip.gate_bwd_delta(dout, og, s, pre[:, 8 + 3 * C:8 + 3 * C + 64])
    acc = _rand(g, *shape) if mix == "acc" else None
    extra = _rand(g, *shape) if mix in ("acc", "extra") else None

    def run():
        dbuf = pre.clone()
        dv0, dlam = hip.attention_bwd_fused(dattn, q, k, v, lse, delta, rinv, cos, sin, wq, wk, vdiff, lam,
                                            None if acc is None else acc.clone(), extra, dbuf[:, 8:8 + 3 * C + 64], scale)
        return dbuf, dv0, dlam

    dbuf, dv0, dlam = run()
    dbuf2, dv02, dlam2 = run()
    _same_bits("dy", dbuf, dbuf2); _same_bits("dv0", dv0, dv02); _same_bits("dlam", dlam, dlam2)
    _fence_ok("dy buffer", dbuf, 8, 8 + 3 * C + 64)
    _same_bits("dy gate columns", dbuf[:, 8 + 3 * C:], pre[:, 8 + 3 * C:])

    _, yr, step = ar.projection_ref(x, w, bias)
    refs = ar.attention_bwd_ref(dattn, q, k, v, lse, delta, scale)
    dy = dbuf[:, 8:8 + 3 * C]
    for t, (wt, yh, gname) in enumerate(((wq, q, "dq"), (wk, k, "dk"))):
        gref, gb = refs[gname]
        ref, bound = ar.norm_rope_bwd_ref(gref, gb, yr[:, t * C:(t + 1) * C].reshape(shape), step[:, t * C:(t + 1) * C].reshape(shape),
                                          yh, wt, cos, sin, EPS)
        _check("attention_bwd_fused", f"dy_{'qk'[t]}", dy[:, t * C:(t + 1) * C].reshape(shape), ref, bound + ar.U * ref.abs())
    dvr, bdv = refs["dv"]
    if extra is not None:
        dvr = dvr + extra.to(F64)
    dyv = dy[:, 2 * C:].reshape(shape)
    if mix in ("none", "extra"):
        assert dv0 is None and dlam is None
        _check("attention_bwd_fused", "dy_v", dyv, dvr, bdv + ar.U * dvr.abs() + 1e-6 * dvr.abs())
        return
    l = float(lam)
    ref = l * dvr
    _check("attention_bwd_fused", "dy_v", dyv, ref, abs(l) * bdv + ar.U * ref.abs() + 1e-6 * ref.abs())
    z = (1 - l) * dvr + (acc.to(F64) if acc is not None else 0)
    zmag = (1 - l) * dvr.abs() + (acc.to(F64).abs() if acc is not None else 0)
    _check("attention_bwd_fused", "dv0", dv0, z, abs(1 - l) * bdv + ar.U * z.abs() + 1e-6 * zmag)
    dl, bl = ar.dlam_ref(dyv, l, vdiff.view(shape))
    _check("attention_bwd_fused", "dlam", dlam.reshape(1), dl, bl)


# ----------------------------------------------------------------------------------------------- the weight predicate
@pytest.mark.parametrize("small", [1e-2, 1e-3])
def test_small_norm_weight_takes_the_separate_passes(small):
    """An RMS weight far below the vector's maximum: the fused backward would divide the saved bf16 row's rounding by it, so
    attention_core_usable must refuse and the block takes the separate passes."""
    from viforsdes_amd.primitives import fused
    from viforsdes_amd.primitives.attn import Attention
    from viforsdes_amd.primitives.embeddings import RotarySpec, precompute_freq_cis
    torch.manual_seed(0)
    att = Attention(256, 4).to(DEV)
    x = torch.randn(112, 37, 256, device=DEV, dtype=BF)
    rot = RotarySpec.from_freqs(precompute_freq_cis(64, end=64)[:37].to(DEV))
    cos, _ = rot.cos_sin_tables(37)
    with torch.autocast("cuda", dtype=BF):
        att.forward_fused(x, rotary=rot, v0=None)   # builds the pack
    assert fused.attention_core_usable(x, att._proj_pack, 4, 64, att.q_norm.weight, att.k_norm.weight, cos)
    with torch.no_grad():
        att.k_norm.weight[17] = -small
    assert not fused.attention_core_usable(x, att._proj_pack, 4, 64, att.q_norm.weight, att.k_norm.weight, cos)
