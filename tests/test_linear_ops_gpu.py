"""Every dispatch of the encoder's GEMM family against float64, element by element.

Each case calls one ``viforsdes_amd._hip`` wrapper, so it pins one kernel, and compares every element with the float64
reference of tests/linear_reference.py; the bounds (per element, never relative to a tensor's maximum), the input classes
(randn | coherent | exact | scaled | saturated -- every case id ends in the class it uses) and the conditions that keep the
bounds sharp are listed and justified in that module's docstring; tests/test_linear_bounds.py shows on the CPU that each bound
rejects injected defects.

Fences.  Operands the ABI lets be pitched (x, dy, the saved u) are column ranges at a non-zero offset of buffers filled with
a NaN sentinel: a read outside the range turns an output into NaN.  Every output is pre-filled with the sentinel, so an element
a chunk or tail plan never visits fails; pitched outputs (y, u, s, du) are column ranges of sentinel buffers and everything
outside the range must still be the sentinel, bit for bit; the contiguous fp32 dW / db sit inside a one-dimensional sentinel
buffer.  Determinism: every call runs twice into fresh buffers, and the results must be bitwise equal.

Dispatch coverage (test ids in brackets), derived from the launch code.  ``linear_reference.rows_plan`` / ``cols_plan`` /
``lin_variant`` / ``wgrad_tn`` mirror that arithmetic and every case asserts the branch its id names (and
``_hip.linear_variant`` against ``lin_variant``), so a later change of a plan fails here instead of silently losing coverage.
  lin_variant:  rows kernel = K in {128, 256, 512} and N % 64 == 0, preferred for the plain epilogue when N >= K or the cols
                kernel does not fit [rows-*]; cols kernel = plain epilogue, K % 64 == 0, N % 128 == 0 [cols-*]; every SwiGLU
                epilogue is a rows launch [swiglu-*] [bwd-*]; 0 = refused (asserted for N = 64, K = 192)
  launch_rows:  K = 512 runs as two k-halves [k512]: four-wave workgroups of 128 rows below M = 65,536 [w4], eight-wave
                workgroups of 256 rows at or above it [w8]; K = 128 / 256: four waves, 256-row stripes (SwiGLU backward: 128)
  launch_rows_nw, column chunks per stripe:
    [one]       a single chunk: one pair (N = 64), odd pair counts under the doubling rule (N = 192, 832), many stripes (plain)
    [doubling]  plain epilogue, stripes < resident workgroups: chunks double while they divide the pair count (N = 256, 512)
    [uneven]    SwiGLU epilogues, stripes < resident: about one round of workgroups, the last chunk shorter
                (M = 12,928: N = 832 -> 7 chunks, the last of one pair; N = 1,408 -> 11 chunks)
    [c2|c3|c4]  SwiGLU epilogues, stripes >= resident: the chunk count with the fullest last round (512 / 1,604, 802 and 520
                stripes); N = 128 has fewer than 2 c pairs for every c and keeps the default two [pairs<2c]
  launch_rows_nw, the last round of resident workgroups:
    [first]     less than one round in all                 [round]   an exact number of rounds (M = 131,072)
    [tail]      last round at most half full: its stripe groups run in finer chunks (M = 133,000, N = 256 / 832)
    [tailcut]   plain epilogue: the equal-pairs rule reduces the tail chunks (M = 143,300, N = 768: 10 -> 6)
    [notail]    last round more than half full
    [idle]      stripe count not a multiple of 8: workgroups without a stripe;  ragged M: 1, 31, 33, stripe +- 1
  launch_cols:  [nb8] N % 256 == 0, [nb4] N = 128 / 384; K 64 (one chunk) .. 2816; M 1, 127, 128, 129, 4,264, 205,312
  wgrad2_plan:  [tn128] fewer than three 256 x 256 tiles, [tn256] three or more; [multi] the multi-round split plan of
                dW[2816, 512] (22 tiles); [few] fewer 32-row blocks than splits; N, K that are not tile multiples (8 x 16,
                264 x 520, 64 x 8); ``row_map`` with dropped rows [map]; M 1, 31, 32, 33, 100, 12,928, 205,312
  group launch: ``group_plan`` False and True, both tile-width classes in one call, each checked against float64 directly; in
                the exact class the single launches and both group plans must be identical
  mlp_fwd:      C 128 / 256, H 64, 128, 384 (341 real), 704 (682 real): padded columns of s exactly 0; M 1, 77, 256, 257, 20,000,
                205,312; want_s on and off (bitwise equal y)
"""
import ctypes
import math

import pytest
import torch

import linear_reference as lr
from linear_reference import BF, F64

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = torch.float32
SENT = (torch.int16, 0x7FDE)      # a quiet bf16 NaN with a payload
SENT32 = 0x7FC0DEAD               # the same for fp32
P, S, B = lr.EPI_PLAIN, lr.EPI_SWIGLU, lr.EPI_SWIGLU_BWD
BIG = 65536                       # from here on a case runs the classes a branch needs, not all of them
STATS: dict = {}


def _hip():
    from viforsdes_amd import _hip
    return _hip


def _gen(seed):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return g


def _sentinel(shape, dtype=BF):
    if dtype == BF:
        return torch.full(shape, SENT[1], dtype=SENT[0], device=DEV).view(BF)
    return torch.full(shape, SENT32, dtype=torch.int32, device=DEV).view(F32)


def _pitched_in(t64, off=16, tail=24):
    """A bf16 operand as columns [off, off + W) of a NaN-sentinel buffer."""
    M, W = t64.shape
    buf = _sentinel((M, off + W + tail))
    view = buf[:, off:off + W]
    view.copy_(t64.to(BF))
    return view


def _pitched_out(M, W, off=8, tail=16):
    buf = _sentinel((M, off + W + tail))
    return buf, buf[:, off:off + W]


def _fence_ok(name, buf, lo, hi):
    raw = buf.view(SENT[0])
    bad = int((raw[:, :lo] != SENT[1]).sum()) + int((raw[:, hi:] != SENT[1]).sum())
    assert bad == 0, f"{name}: {bad} elements outside columns [{lo}, {hi}) changed"


def _flat_out(shape, pad=64):
    """A contiguous fp32 output inside a one-dimensional sentinel buffer: (buffer, view)."""
    n = math.prod(shape)
    buf = _sentinel((n + 2 * pad,), F32)
    return buf, buf[pad:pad + n].view(*shape)


def _flat_fence_ok(name, buf, n, pad=64):
    raw = buf.view(torch.int32)
    bad = int((raw[:pad] != SENT32).sum()) + int((raw[pad + n:] != SENT32).sum())
    assert bad == 0, f"{name}: {bad} elements around the output changed"


def _same_bits(name, a, b):
    assert torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)), f"{name}: not bitwise reproducible"


class Tally:
    """Per-element comparison over the row slices of one output: out-of-bound count, worst ratio, ambiguous elements (bound > floor)
    and how many of them took the neighbouring value."""

    def __init__(self, key):
        self.key, self.bad, self.worst, self.first, self.n, self.amb, self.nb = key, 0, 0.0, None, 0, 0, 0

    def add(self, got, ref, bound, r0=0, amb=None):
        n, worst, idx = lr.excess(got, ref, bound)
        if n and self.first is None:
            self.first = (idx[0] + r0,) + tuple(idx[1:]), float(got[idx]), float(ref[idx]), float(bound[idx])
        self.bad += n
        self.worst = max(self.worst, worst if math.isfinite(worst) else float("inf"))
        self.n += got.numel()
        amb = (bound > 0) if amb is None else amb
        self.amb += int(amb.sum())
        self.nb += int((amb & (got.to(F64) != ref)).sum())   # (a hull's mid-point is no bf16 value: only the plain outputs' count means something)

    def share(self):
        return self.amb / max(1, self.n)

    def finish(self, limit=None):
        print(f"STAT {self.key} n={self.n} bad={self.bad} worst={self.worst:.3g} ambiguous={self.amb} ({self.share():.4f}) neighbour={self.nb}")
        STATS[self.key] = (self.n, self.bad, self.amb, self.nb)
        if self.bad:
            idx, g, r, b = self.first
            raise AssertionError(f"{self.key}: {self.bad} of {self.n} elements out of bound (worst err/bound {self.worst:.3g}); first at "
                                 f"{idx}: got {g!r}, ref {r!r}, bound {b:.3g}")
        if limit is not None:
            assert self.share() <= limit, f"{self.key}: ambiguous share {self.share():.4f} above {limit:.4f}: the check is not sharp"


def _kinds(M, small, big):
    return small if M < BIG else big


def _cases(table, small, big):
    """[(M, N, K, tags)] -> pytest params (M, N, K, kind, tags) with ids ``<tags>-MxNxK-<kind>``."""
    out = []
    for M, N, K, tags in table:
        for kind in _kinds(M, small, big):
            out.append(pytest.param(M, N, K, kind, tags, id=f"{tags}-{M}x{N}x{K}-{kind}"))
    return out


def check_tags(plan, tags):
    """Every word of a case id names a value of the mirrored plan."""
    words = {
        "w4": plan.get("nw") == 4, "w8": plan.get("nw") == 8, "k512": plan.get("rows") in (128, 256) and plan.get("k512", False),
        "one": plan.get("rule") == "one", "doubling": plan.get("rule") == "doubling", "uneven": plan.get("rule") == "uneven",
        "c2": plan.get("rule") == "c2", "c3": plan.get("rule") == "c3", "c4": plan.get("rule") == "c4",
        "pairs<2c": plan.get("pairs", 99) < 4,
        "first": plan.get("last") == "first-round", "round": plan.get("last") == "round", "tail": plan.get("last") == "tail",
        "notail": plan.get("last") == "notail",
        "tailcut": plan.get("last") == "tail" and plan.get("tail_chunks", 0) < plan.get("tc_first", 0),
        "idle": plan.get("idle", False), "ragged": plan.get("ragged", False), "short": plan.get("last_chunk_pairs", 0) < plan.get("ppc", 0),
        "nb8": plan.get("nb") == 8, "nb4": plan.get("nb") == 4, "k1": plan.get("ktiles") == 1,
        "tn128": plan.get("tn") == 128, "tn256": plan.get("tn") == 256, "multi": plan.get("multi", False), "few": plan.get("few", False),
        "edge": plan.get("edge", False), "map": True,
    }
    for word in tags.split("-")[1:]:
        assert word in words, f"unknown tag {word}"
        assert words[word], f"case tagged [{word}] no longer lands there: {plan}"


def rows_case_plan(M, N, K, epi):
    plan = lr.rows_plan(M, N, K, epi)
    plan["k512"] = K == 512
    plan["ppc"] = -(-plan["pairs"] // plan["chunks"])
    return plan


# =============================================================================================== linear_bf16, rows kernel
ROWS = [
    (1, 256, 256, "rows-w4-doubling-first-ragged-idle"), (31, 64, 128, "rows-w4-one-first-ragged"), (33, 192, 128, "rows-w4-one-first-ragged"),
    (255, 832, 256, "rows-w4-one-first-ragged"), (257, 256, 256, "rows-w4-doubling-first-ragged-idle"),
    (4264, 64, 256, "rows-w4-one-first"), (4264, 192, 256, "rows-w4-one-first-idle"), (4264, 832, 128, "rows-w4-one-first-idle"),
    (4264, 512, 256, "rows-w4-doubling-first"),
    (100000, 256, 128, "rows-w4-doubling-notail-idle"), (131072, 256, 256, "rows-w4-one-round"),
    (133000, 256, 256, "rows-w4-one-tail-ragged"), (133000, 832, 256, "rows-w4-one-tail-ragged"), (143300, 768, 256, "rows-w4-one-tailcut-ragged"),
    (127, 512, 512, "rows-k512-w4-doubling-first-ragged"), (129, 512, 512, "rows-k512-w4-doubling-first-ragged-idle"),
    (9000, 1792, 512, "rows-k512-w4-doubling-first-idle"), (65535, 512, 512, "rows-k512-w4-one-round-ragged"),
    (65536, 512, 512, "rows-k512-w8-one-round"), (66077, 512, 512, "rows-k512-w8-one-tail-ragged-idle"),
    (80000, 1024, 512, "rows-k512-w8-one-tail-idle"),
]
ALL4 = ("randn", "coherent", "exact", "scaled")


def _plain_case(key, M, N, K, kind):
    hip = _hip()
    x, w, b = lr.gemm_operands(kind, _gen(K + N), M, N, K)
    xv, wb, bb = _pitched_in(x), w.to(BF).contiguous(), b.to(BF).contiguous()
    # the call without a bias as well, where it keeps the share condition: without |b| in y the terms of randn data cancel further
    # (K = 512: 37 % ambiguous against 31 % with the bias), so there only the sharp classes run it
    nobias = M < BIG and (K <= 256 or kind in ("coherent", "exact"))
    biases = ((b, bb), (None, None)) if nobias else ((b, bb),)
    for b64, bias in biases:
        bufs = [_pitched_out(M, N) for _ in range(2)]
        for buf, y in bufs:
            assert hip.linear_bf16(xv, wb, bias, out=y) is y
        torch.cuda.synchronize()
        _same_bits(key, bufs[0][0], bufs[1][0])
        _fence_ok(key, bufs[0][0], 8, 8 + N)
        y = bufs[0][1]
        t = Tally(f"{key}.y" + ("" if bias is not None else ".nobias"))
        for r0, r1 in lr.row_slices(M, max(N, K)):
            ref, step = lr.plain_ref(x[r0:r1], w, b64, exact=(kind == "exact"))
            t.add(y[r0:r1], ref, step, r0)
        t.finish(lr.share_limit(kind, K))


@pytest.mark.parametrize("M,N,K,kind,tags", _cases(ROWS, ALL4, ("coherent", "exact", "randn")))
def test_linear_rows(M, N, K, kind, tags):
    assert lr.lin_variant(M, N, K, P) == 1 and _hip().linear_variant(M, N, K, P) == 1
    check_tags(rows_case_plan(M, N, K, P), tags)
    _plain_case(f"linear_bf16[{tags}-{M}x{N}x{K}-{kind}]", M, N, K, kind)


# =============================================================================================== linear_bf16, cols kernel
COLS = [
    (1, 128, 64, "cols-nb4-k1-ragged"), (127, 256, 192, "cols-nb8-ragged"), (128, 384, 384, "cols-nb4"), (129, 512, 768, "cols-nb8-ragged"),
    (4264, 256, 64, "cols-nb8-k1-ragged"), (4264, 384, 192, "cols-nb4-ragged"), (4264, 128, 384, "cols-nb4-ragged"),
    (4264, 256, 1408, "cols-nb8-ragged"), (4264, 128, 1536, "cols-nb4-ragged"), (4264, 512, 2816, "cols-nb8-ragged"),
    (4264, 256, 512, "cols-nb8-ragged"), (205312, 256, 768, "cols-nb8"),
]


@pytest.mark.parametrize("M,N,K,kind,tags", _cases(COLS, ALL4, ("coherent", "exact", "randn")))
def test_linear_cols(M, N, K, kind, tags):
    assert lr.lin_variant(M, N, K, P) == 2 and _hip().linear_variant(M, N, K, P) == 2
    check_tags(lr.cols_plan(M, N, K), tags)
    _plain_case(f"linear_bf16[{tags}-{M}x{N}x{K}-{kind}]", M, N, K, kind)


def test_uncovered_shapes_are_refused():
    hip = _hip()
    for M, N, K, epi in ((100, 64, 192, P), (100, 128, 192, S), (100, 96, 256, P), (100, 128, 64, B)):
        assert lr.lin_variant(M, N, K, epi) == 0 and hip.linear_variant(M, N, K, epi) == 0
    x, w = torch.zeros(100, 192, device=DEV, dtype=BF), torch.zeros(64, 192, device=DEV, dtype=BF)
    with pytest.raises(Exception):   # a missing kernel is an error, never a fall-back
        hip.linear_bf16(x, w, None)


# ====================================================================================================== linear_swiglu_bf16
# N = the width of u (two interleaved halves), s has N / 2 columns
SWIGLU = [
    (300, 128, 128, "swiglu-w4-uneven-first-ragged-idle"), (4264, 768, 128, "swiglu-w4-uneven-first-idle"),
    (12928, 832, 256, "swiglu-w4-uneven-short-first-idle"), (12928, 1408, 256, "swiglu-w4-uneven-tail-idle"),
    (200, 256, 512, "swiglu-k512-w4-uneven-first-ragged-idle"), (9000, 1408, 512, "swiglu-k512-w4-uneven-idle"),
    (66077, 1408, 512, "swiglu-k512-w8-c4-tail-ragged-idle"),
    (131072, 1408, 256, "swiglu-w4-c2-round"), (133005, 1408, 256, "swiglu-w4-c4-tail-ragged"), (205312, 1408, 256, "swiglu-w4-c3-notail-idle"),
    (133005, 128, 256, "swiglu-w4-c2-pairs<2c-notail-ragged"), (133005, 832, 128, "swiglu-w4-c4-short-tail-ragged"),
]
SW_SMALL = ("randn", "coherent", "exact", "scaled", "saturated")


@pytest.mark.parametrize("M,N,K,kind,tags", _cases(SWIGLU, SW_SMALL, ("coherent", "saturated")))
def test_linear_swiglu(M, N, K, kind, tags):
    hip = _hip()
    assert lr.lin_variant(M, N, K, S) == 1 and hip.linear_variant(M, N, K, S) == 1
    check_tags(rows_case_plan(M, N, K, S), tags)
    key = f"linear_swiglu_bf16[{tags}-{M}x{N}x{K}-{kind}]"
    x, w, b = lr.gemm_operands(kind, _gen(K + N + 1), M, N, K)
    if kind == "saturated":
        b = lr.saturate_bias(b)
    xv, wb, bb = _pitched_in(x), w.to(BF).contiguous(), b.to(BF).contiguous()
    runs = []
    for _ in range(2):
        (ubuf, u), (sbuf, s) = _pitched_out(M, N), _pitched_out(M, N // 2, off=16, tail=8)
        ru, rs = hip.linear_swiglu_bf16(xv, wb, bb, True, out_u=u, out_s=s)
        assert ru is u and rs is s
        runs.append((ubuf, u, sbuf, s))
    s3buf, s3 = _pitched_out(M, N // 2, off=16, tail=8)
    none, _ = hip.linear_swiglu_bf16(xv, wb, bb, False, out_s=s3)
    torch.cuda.synchronize()
    assert none is None
    ubuf, u, sbuf, s = runs[0]
    _same_bits(key + ".u", ubuf, runs[1][0]); _same_bits(key + ".s", sbuf, runs[1][2]); _same_bits(key + ".s(want_u=False)", sbuf, s3buf)
    _fence_ok(key + ".u", ubuf, 8, 8 + N); _fence_ok(key + ".s", sbuf, 16, 16 + N // 2)
    tu, ts = Tally(key + ".u"), Tally(key + ".s")
    amax, amin = -1e30, 1e30
    for r0, r1 in lr.row_slices(M, max(N, K)):
        ref = lr.swiglu_ref(x[r0:r1], w, b, exact=(kind == "exact"))
        tu.add(u[r0:r1], *ref["u"], r0)
        ts.add(s[r0:r1], *ref["s"], r0, amb=ref["s"][1] > 1e-30)
        a = lr.halves(ref["u"][0])[0]
        amax, amin = max(amax, float(a.max())), min(amin, float(a.min()))
    if kind == "saturated":
        assert amax > 90 and amin < -90, (amax, amin)
    tu.finish(lr.share_limit(kind, K))
    ts.finish()


# ================================================================================================== linear_swiglu_bwd_bf16
# N = H, the width of ds; u and du have 2 H interleaved columns; 128-row stripes
BWD = [
    (300, 64, 128, "bwd-w4-one-first-ragged-idle"), (4264, 384, 128, "bwd-w4-uneven-first-ragged-idle"),
    (12928, 832, 256, "bwd-w4-uneven-short-idle"), (6464, 1408, 256, "bwd-w4-uneven-idle"),
    (200, 128, 512, "bwd-k512-w4-uneven-first-ragged-idle"), (9000, 1408, 512, "bwd-k512-w4-uneven-short-tail-ragged-idle"),
    (66077, 704, 512, "bwd-k512-w8-c4-tail-ragged-idle"),
    (66560, 704, 256, "bwd-w4-c4-tail"), (102656, 704, 256, "bwd-w4-c3-notail-idle"), (205312, 704, 256, "bwd-w4-c2-tail-idle"),
    (70000, 64, 256, "bwd-w4-one-pairs<2c-notail-ragged-idle"), (66565, 128, 128, "bwd-w4-c2-pairs<2c-ragged-idle"),
]
BW_SMALL = ("randn", "coherent", "scaled", "saturated")


@pytest.mark.parametrize("M,N,K,kind,tags", _cases(BWD, BW_SMALL, ("randn", "saturated")))
def test_linear_swiglu_bwd(M, N, K, kind, tags):
    hip = _hip()
    H = N
    assert lr.lin_variant(M, H, K, B) == 1 and hip.linear_variant(M, H, K, B) == 1
    check_tags(rows_case_plan(M, H, K, B), tags)
    key = f"linear_swiglu_bwd_bf16[{tags}-{M}x{H}x{K}-{kind}]"
    g = _gen(K + H + 2)
    dy, w_t, _ = lr.gemm_operands("randn" if kind == "saturated" else kind, g, M, H, K, bias=False)
    u = torch.randn(M, 2 * H, generator=g, dtype=F32, device=DEV).to(F64) * 2
    if kind == "coherent":
        u = u.abs()
    if kind == "saturated":
        u = u + lr.saturate_bias(torch.zeros(2 * H, dtype=F64, device=DEV))
    dyv, uv, wb = _pitched_in(dy), _pitched_in(u, off=24, tail=8), w_t.to(BF).contiguous()
    bufs = [_pitched_out(M, 2 * H) for _ in range(2)]
    for buf, du in bufs:
        assert hip.linear_swiglu_bwd_bf16(dyv, wb, uv, out=du) is du
    torch.cuda.synchronize()
    _same_bits(key, bufs[0][0], bufs[1][0])
    _fence_ok(key, bufs[0][0], 8, 8 + 2 * H)
    du = bufs[0][1]
    if kind == "saturated":
        a = lr.halves(uv)[0].to(F64)
        assert float(a.max()) > 90 and float(a.min()) < -90
    t = Tally(key + ".du")
    for r0, r1 in lr.row_slices(M, max(2 * H, K)):
        ref, bound = lr.swiglu_bwd_ref(dy[r0:r1], w_t, uv[r0:r1])
        t.add(du[r0:r1], ref, bound, r0, amb=bound > 1e-30)
    t.finish()


# ================================================================================================================= wgrad
# (M, N, K, tags): dW [N, K]
WGRAD = [
    (1, 8, 16, "wgrad-tn128-few-edge"), (31, 64, 8, "wgrad-tn128-few-edge"), (32, 264, 520, "wgrad-tn256-few-edge"), (33, 256, 256, "wgrad-tn128-few"),
    (100, 832, 256, "wgrad-tn256-few"), (4264, 264, 520, "wgrad-tn256-edge"), (12928, 256, 256, "wgrad-tn128"), (12928, 1536, 256, "wgrad-tn256"),
    (12928, 256, 768, "wgrad-tn256"), (12928, 2816, 512, "wgrad-tn256"),
    (205312, 256, 256, "wgrad-tn128"), (205312, 832, 256, "wgrad-tn256"), (205312, 2816, 512, "wgrad-tn256-multi"),
]
WG_KINDS = ("randn", "coherent", "exact", "scaled")


def _wgrad_plan(hip, M, N, K):
    nbytes = hip.load().vsde_linear_wgrad_workspace_bytes(ctypes.c_int64(M), ctypes.c_int(N), ctypes.c_int(K))
    tn = lr.wgrad_tn(N, K)
    tiles = -(-N // tn) * -(-K // 256)
    nsplit = lr.wgrad_nsplit(nbytes, N, K)
    blocks = -(-M // 32)
    one_round = min(max(((256 if tn == 256 or tiles <= 2 else 512) // tiles) & ~7, 8), 256)
    return dict(tn=tn, tiles=tiles, nsplit=nsplit, blocks=blocks, few=blocks < one_round and nsplit == blocks,
                multi=tiles >= 3 and tiles * nsplit > 256, edge=(N % tn != 0 or K % 256 != 0))


def _wgrad_check(key, kind, dy, x, gW, gb, nsplit, rows=None):
    """gW [N or out_rows, K], gb against float64; ``rows``: the output row of product row n (negative: dropped)."""
    dW, mW, db, mb = lr.wgrad_ref(dy, x)
    c = lr.wgrad_depth(dy.shape[0], nsplit) * lr.ACC_C
    if rows is not None:
        keep = rows >= 0
        gW, gb = gW[rows[keep]], (None if gb is None else gb[rows[keep]])
        dW, mW, db, mb = dW[keep], mW[keep], db[keep], mb[keep]
    if kind == "exact":
        assert torch.equal(gW.to(F64), dW), f"{key}.dW differs from the exact integer result"
        assert gb is None or torch.equal(gb.to(F64), db), f"{key}.db differs from the exact integer result"
    t = Tally(key + ".dW"); t.add(gW, dW, c * mW); t.finish()
    if gb is not None:
        t = Tally(key + ".db"); t.add(gb, db, c * mb); t.finish()


@pytest.mark.parametrize("M,N,K,kind,tags", _cases(WGRAD, WG_KINDS, ("randn", "exact")))
def test_linear_wgrad(M, N, K, kind, tags):
    hip = _hip()
    plan = _wgrad_plan(hip, M, N, K)
    check_tags(plan, tags)
    key = f"linear_wgrad[{tags}-{M}x{N}x{K}-{kind}]"
    dy, x = lr.wgrad_operands(kind, _gen(N + K), M, N, K)
    dyb, xb = dy.to(BF).contiguous(), x.to(BF).contiguous()
    runs = []
    for _ in range(2):
        (wbuf, dW), (bbuf, db) = _flat_out((N, K)), _flat_out((N,))
        rW, rb = hip.linear_wgrad(dyb, xb, True, out=dW, out_bias=db)
        assert rW is dW and rb is db
        runs.append((wbuf, dW, bbuf, db))
    torch.cuda.synchronize()
    _same_bits(key + ".dW", runs[0][0], runs[1][0]); _same_bits(key + ".db", runs[0][2], runs[1][2])
    _flat_fence_ok(key + ".dW", runs[0][0], N * K); _flat_fence_ok(key + ".db", runs[0][2], N)
    _wgrad_check(key, kind, dy, x, runs[0][1], runs[0][3], plan["nsplit"])
    # without the bias gradient: the same dW
    (wbuf, dW), _ = _flat_out((N, K)), None
    hip.linear_wgrad(dyb, xb, False, out=dW)
    _same_bits(key + ".dW(no bias)", wbuf, runs[0][0])


def _row_map(N, out_rows, g):
    """A map that drops every fifth product row and scatters the others over ``out_rows`` output rows (some stay unwritten)."""
    perm = torch.randperm(out_rows, generator=g, device=DEV)[:N].to(torch.int32)
    perm[::5] = -1
    return perm.contiguous()


@pytest.mark.parametrize("M,N,K,out_rows,kind", [(4264, 264, 520, 300, "exact"), (4264, 264, 520, 300, "randn"), (33, 64, 8, 64, "exact"),
                                                 (12928, 832, 256, 1000, "exact"), (12928, 256, 256, 256, "scaled")],
                         ids=lambda v: str(v))
def test_linear_wgrad_row_map(M, N, K, out_rows, kind):
    hip = _hip()
    plan = _wgrad_plan(hip, M, N, K)
    key = f"linear_wgrad[map-{M}x{N}x{K}->{out_rows}-{kind}]"
    g = _gen(N + K + 7)
    dy, x = lr.wgrad_operands(kind, g, M, N, K)
    rows = _row_map(N, out_rows, g)
    runs = []
    for _ in range(2):
        (wbuf, dW), (bbuf, db) = _flat_out((out_rows, K)), _flat_out((out_rows,))
        hip.linear_wgrad(dy.to(BF).contiguous(), x.to(BF).contiguous(), True, row_map=rows, out_rows=out_rows, out=dW, out_bias=db)
        runs.append((wbuf, dW, bbuf, db))
    torch.cuda.synchronize()
    _same_bits(key + ".dW", runs[0][0], runs[1][0]); _same_bits(key + ".db", runs[0][2], runs[1][2])
    _flat_fence_ok(key + ".dW", runs[0][0], out_rows * K); _flat_fence_ok(key + ".db", runs[0][2], out_rows)
    dW, db = runs[0][1], runs[0][3]
    lrows = rows.long()
    _wgrad_check(key, kind, dy, x, dW, db, plan["nsplit"], rows=lrows)
    untouched = torch.ones(out_rows, dtype=torch.bool, device=DEV)
    untouched[lrows[lrows >= 0]] = False
    assert int(untouched.sum()) > 0
    assert bool((dW[untouched].view(torch.int32) == SENT32).all()) and bool((db[untouched].view(torch.int32) == SENT32).all()), \
        f"{key}: an output row no product row maps to was written"


# (M, N, K, want_bias, mapped) of one group: both tile-width classes, edge tiles, the multi-round plan, a mapped problem
GROUP = [(12928, 256, 256, True, False), (12928, 832, 256, True, False), (12928, 256, 768, False, False), (12928, 264, 520, True, True),
         (12928, 2816, 512, True, False), (12928, 64, 8, True, False), (12928, 1536, 256, True, False)]
GROUP_SMALL = [(100, 256, 256, True, False), (33, 832, 256, True, True), (1, 8, 16, True, False), (31, 256, 768, False, False)]


@pytest.mark.parametrize("kind", ["randn", "exact", "scaled"])
@pytest.mark.parametrize("table", [GROUP, GROUP_SMALL], ids=["ou", "few"])
def test_linear_wgrad_group(table, kind):
    hip = _hip()
    g = _gen(99)
    problems, data = [], []
    for M, N, K, want_bias, mapped in table:
        dy, x = lr.wgrad_operands(kind, g, M, N, K)
        out_rows = N + 40 if mapped else N
        rows = _row_map(N, out_rows, g) if mapped else None
        problems.append((dy.to(BF).contiguous(), x.to(BF).contiguous(), want_bias, rows, out_rows if mapped else None))
        data.append((dy, x, rows, out_rows))
    results = {}
    for mode in ("single", False, True):
        for rep in range(2):
            bufs = [(_flat_out((d[3], p[1].shape[1])), _flat_out((d[3],)) if p[2] else None) for p, d in zip(problems, data)]
            if mode == "single":
                for p, ((wbuf, dW), bb) in zip(problems, bufs):
                    hip.linear_wgrad(p[0], p[1], p[2], row_map=p[3], out_rows=p[4], out=dW, out_bias=None if bb is None else bb[1])
            else:
                outs = hip.linear_wgrad_group(problems, group_plan=mode, outs=[(w[1], None if bb is None else bb[1]) for w, bb in bufs])
                assert all(o[0] is w[1] for o, (w, bb) in zip(outs, bufs))
            torch.cuda.synchronize()
            if rep:
                for i, ((w0, b0), (w1, b1)) in enumerate(zip(results[mode], bufs)):
                    _same_bits(f"group[{mode}].{i}.dW", w0[0], w1[0])
                    if b0 is not None:
                        _same_bits(f"group[{mode}].{i}.db", b0[0], b1[0])
            else:
                results[mode] = bufs
    for i, ((M, N, K, want_bias, mapped), (dy, x, rows, out_rows)) in enumerate(zip(table, data)):
        plan = _wgrad_plan(hip, M, N, K)
        for mode in ("single", False, True):
            (wbuf, dW), bb = results[mode][i]
            key = f"linear_wgrad_group[{mode}].{i}[{M}x{N}x{K}-{kind}]"
            _flat_fence_ok(key, wbuf, out_rows * K)
            # group_plan=True never takes more splits than the problem's own plan and never fewer than 8 (or all blocks): the chain
            # of additions is longest at the fewest splits
            nsplit = plan["nsplit"] if mode is not True else min(plan["nsplit"], 8)
            _wgrad_check(key, kind, dy, x, dW, None if bb is None else bb[1], nsplit, rows=None if rows is None else rows.long())
            if mode is False or kind == "exact":   # group_plan=False: bit-identical to one call per problem; exact: all three
                _same_bits(key + " against the single launch", wbuf, results["single"][i][0][0])
                if bb is not None:
                    _same_bits(key + ".db against the single launch", bb[0], results["single"][i][1][0])


# =============================================================================================================== mlp_fwd
# (M, C, H padded, H real)
MLP = [(1, 128, 64, 64), (77, 256, 128, 128), (256, 128, 384, 341), (257, 256, 704, 682), (20000, 256, 704, 682), (20000, 128, 128, 128),
       (20000, 128, 384, 341), (205312, 256, 704, 682)]


def _mlp_params(kind, g, C, H, hreal):
    from viforsdes_amd.primitives import fused
    base = "randn" if kind == "saturated" else kind
    _, w_in, b_in = lr.gemm_operands(base, g, 1, 2 * hreal, C)
    _, w_out, b_out = lr.gemm_operands(base, g, 1, C, hreal)
    if kind == "saturated":
        b_in = lr.saturate_bias(b_in, interleaved=False, hreal=hreal).to(BF).to(F64)
    params = [torch.nn.Parameter(t.to(F32)) for t in (w_in, b_in, w_out, b_out)]
    pin, pout = fused.swiglu_packs(*params, H, interleave=False)
    img = fused.MlpImages(pin, pout, H)
    return (w_in, b_in, w_out, b_out), pout, img, params


MLP_CASES = [pytest.param(M, C, H, hreal, kind, id=f"mlp-{M}x{C}x{H}({hreal})-{kind}") for M, C, H, hreal in MLP
             for kind in _kinds(M, ("randn", "coherent", "scaled", "saturated"), ("randn", "coherent"))]


@pytest.mark.parametrize("M,C,H,hreal,kind", MLP_CASES)
def test_mlp_fwd(M, C, H, hreal, kind):
    hip = _hip()
    key = f"mlp_fwd[{M}x{C}x{H}({hreal})-{kind}]"
    g = _gen(C + H)
    (w_in, b_in, w_out, b_out), pout, img, params = _mlp_params(kind, g, C, H, hreal)
    x = lr.gemm_operands("randn" if kind == "saturated" else kind, g, M, 8, C)[0]
    xv = _pitched_in(x)
    w1, w2, b1 = img.operands()
    w2pad, b2 = pout.weight.to(F64), pout.bias
    assert torch.equal(w2pad[:, :hreal], w_out) and torch.equal(b2.to(F64), b_out) and float(w2pad[:, hreal:].abs().max() if H > hreal else 0) == 0
    runs = []
    for _ in range(2):
        (ybuf, y), (sbuf, s) = _pitched_out(M, C), _pitched_out(M, H, off=16, tail=8)
        ry, rs = hip.mlp_fwd(xv, w1, w2, b1, b2, H, want_s=True, out_y=y, out_s=s)
        assert ry is y and rs is s
        runs.append((ybuf, y, sbuf, s))
    y3buf, y3 = _pitched_out(M, C)
    _, none = hip.mlp_fwd(xv, w1, w2, b1, b2, H, want_s=False, out_y=y3)
    torch.cuda.synchronize()
    assert none is None
    ybuf, y, sbuf, s = runs[0]
    _same_bits(key + ".y", ybuf, runs[1][0]); _same_bits(key + ".s", sbuf, runs[1][2]); _same_bits(key + ".y(want_s=False)", ybuf, y3buf)
    _fence_ok(key + ".y", ybuf, 8, 8 + C); _fence_ok(key + ".s", sbuf, 16, 16 + H)
    if H > hreal:
        assert bool((s[:, hreal:] == 0).all()), f"{key}: padded columns of s are not exactly 0"
    ts, ty = Tally(key + ".s"), Tally(key + ".y")
    for r0, r1 in lr.row_slices(M, 2 * H):
        ref, bound = lr.mlp_s_ref(x[r0:r1], w_in, b_in, hreal)
        ts.add(s[r0:r1, :hreal], ref, bound, r0, amb=bound > 1e-30)
        # teacher-forced on the kernel's own s: the plain bound at K = H
        yref, step = lr.plain_ref(s[r0:r1].to(F64), w2pad, b2)
        ty.add(y[r0:r1], yref, step, r0)
    ts.finish()
    ty.finish(lr.share_limit("coherent" if kind == "coherent" else "randn", H))
