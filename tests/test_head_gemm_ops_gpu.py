"""GPU: the three non-recurrent GEMM stages of the fused head -- context projection, grad_context, the grouped weight / bias
gradients -- per element against float64 (tests/head_gemm_reference.py: references, derived bounds, input classes, plan mirrors),
through ``_hip.debug_head_context_projection`` / ``_hip.debug_head_backward_gemms``, which run the product's own host code on
given operands.  Every case: outputs pre-filled with NaN, row T of the context slab and of the context-gradient slab NaN (never
read, never written), two runs with equal bits, the kernel path asserted by the plan mirror, class ``exact`` (and ``onehot`` of the
projection) bit for bit.

Observed on an MI355X (recorded after the run, never used to set a bound): no element of any case out of bound, ``exact`` and the
projection's ``onehot`` bit for bit, the second run's bits equal, sentinels intact, the whole file in 4.3 s (slowest case 1.3 s: the
first launch).  Worst |error| / bound over the classes with an allowance (randn, coherent, scaled, single_row, onehot of the TN sums):
  projection      bf16 planes 0.022      gemm_nt 0.14
  grad_context    gemm_nt, f32 output 0.074; bf16 outputs (both kernels): every element equal to the rounded float64 value or,
                  among the ambiguous ones (share 0.35 - 0.37 randn, 0.17 scaled, 0.02 coherent, <= 0.007 onehot), its neighbour
  weight grads    tn_wide 0.091 (single_row 0.075)      tn_grouped 0.095
"""
import pytest
import torch

import head_gemm_reference as R
from head_gemm_reference import BF, F32, F64

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ALL = ("exact", "randn", "onehot", "coherent", "scaled")
ALL_TN = ("exact", "randn", "onehot", "coherent", "scaled", "single_row")
BASE = ("exact", "randn")


def _hip():
    from viforsdes_amd import _hip
    return _hip


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


def _dims(B, T, S=2, P=3, C=256, H=64, L=2):
    return (B, T, S, P, C, H, L)


# ------------------------------------------------------------------------------------------------------- projection
# (id, dims, ctx dtype, slab view, misaligned storage, expected path, classes)
PROJ = []
for _M, (_B, _T) in ((7, (1, 7)), (150, (6, 25)), (640, (32, 20))):
    for _H in (32, 64, 96):
        full = _M == 640 and _H == 64
        PROJ.append((f"planes-M{_M}-H{_H}", _dims(_B, _T, H=_H), BF, not (_M == 150 and _H == 64), False, "planes", ALL if full else BASE))
PROJ += [
    ("planes2-M150", _dims(6, 25, C=512), BF, True, False, "planes", BASE + ("coherent",)),
    ("planes2-M640", _dims(32, 20, C=512), BF, True, False, "planes", ("onehot", "scaled")),
    ("nt-f32-C256", _dims(6, 25), F32, True, False, "gemm_nt", ALL),
    ("nt-bf16-C128", _dims(6, 25, C=128), BF, True, False, "gemm_nt", BASE),
    ("nt-bf16-C20", _dims(6, 25, C=20), BF, True, False, "gemm_nt", BASE + ("onehot",)),
    ("nt-f32-C30", _dims(6, 25, C=30), F32, True, False, "gemm_nt", BASE + ("onehot",)),
    ("nt-H20", _dims(6, 25, H=20), BF, True, False, "gemm_nt", BASE),
    ("nt-M65", _dims(5, 13), F32, False, False, "gemm_nt", BASE),
    ("nt-misaligned", _dims(6, 25), BF, True, True, "gemm_nt", BASE + ("onehot",)),
]
PROJ_CASES = [pytest.param(*c[1:6], k, id=f"{c[0]}-{k}") for c in PROJ for k in c[6]]


@pytest.mark.parametrize("dims, dtype, slab, misalign, path, kind", PROJ_CASES)
def test_context_projection(dims, dtype, slab, misalign, path, kind):
    hip = _hip()
    B, T, S, P, C, H, L = dims
    case = R.make_case(kind, _gen(B * 1000 + C + H), dims, dtype, slab, misalign)
    ctx = case["ctx"]
    assert misalign == (ctx.data_ptr() % 16 != 0)
    assert R.proj_path(dims, ctx) == path, "the case does not reach the kernel it is meant for"
    G = hip.debug_head_context_projection(ctx, case["ws"], S, P)
    G2 = hip.debug_head_context_projection(ctx, case["ws"], S, P)
    assert torch.equal(_bits(G), _bits(G2)), "two runs differ"
    ref, A = R.proj_ref(ctx, case["ws"][0], case["ws"][2], S, planes=(path == "planes"))
    if kind in ("exact", "onehot"):
        A = torch.zeros_like(A)   # bit for bit
    nbad, worst, where = R.excess(G, ref, A)
    print(f"projection {path} {dims} {kind}: worst err/bound {worst:.3g}, out of bound {nbad}")
    assert nbad == 0, (nbad, worst, where)
    if slab:
        assert bool(torch.isnan(case["store"][:, T].float()).all())


# --------------------------------------------------------------------------------------------------------- backward
# (id, dims, ctx dtype, context gradient 'bf16-slab' | 'f32-slab' | 'f32', misaligned ctx, grad_context path, TN path, classes)
BWD = []
for _C in (64, 256, 512):
    for _M, (_B, _T) in ((7, (1, 7)), (150, (6, 25))):
        full = _C == 256 and _M == 150
        BWD.append((f"gc-planes-C{_C}-M{_M}", _dims(_B, _T, C=_C), BF, "bf16-slab", False, "planes", "grouped",
                    ("exact", "randn", "coherent", "scaled") if full else BASE))
BWD += [
    ("gc-planes-M640", _dims(32, 20), BF, "bf16-slab", False, "planes", "wide", ("onehot",)),
    ("gc-nt-f32", _dims(6, 25, C=64), BF, "f32", False, "gemm_nt", "grouped", BASE + ("onehot",)),
    ("gc-nt-f32-slab", _dims(6, 25, C=64), F32, "f32-slab", False, "gemm_nt", "grouped", BASE),
    ("gc-nt-bf16-H32", _dims(6, 25, C=64, H=32), BF, "bf16-slab", False, "gemm_nt", "grouped", BASE + ("coherent", "scaled")),
    ("gc-nt-bf16-C32", _dims(6, 25, C=32), BF, "bf16-slab", False, "gemm_nt", "grouped", BASE + ("onehot",)),
    # tn_wide: H = 64, T >= 16, B T % 16 == 0
    ("tw-1x16", (1, 16, 1, 0, 64, 64, 1), BF, "bf16-slab", False, "planes", "wide", BASE + ("single_row",)),
    ("tw-3x16", (3, 16, 2, 3, 256, 64, 2), BF, "bf16-slab", False, "planes", "wide", BASE),
    ("tw-5x16", (5, 16, 3, 16, 64, 64, 3), F32, "f32-slab", False, "gemm_nt", "wide", BASE + ("single_row",)),
    ("tw-16x17", (16, 17, 5, 3, 256, 64, 4), BF, "bf16-slab", False, "planes", "wide", BASE + ("single_row",)),
    ("tw-16x31", (16, 31, 9, 0, 64, 64, 2), F32, "f32", False, "gemm_nt", "wide", BASE + ("scaled",)),
    ("tw-48x25", (48, 25, 2, 3, 1024, 64, 1), BF, "bf16-slab", False, "planes", "wide", BASE),
    ("tw-16x272", (16, 272, 2, 3, 256, 64, 2), BF, "bf16-slab", False, "planes", "wide", ALL_TN),
    ("tw-16x272-f32", (16, 272, 1, 3, 64, 64, 1), F32, "f32", False, "gemm_nt", "wide", ("exact", "randn", "coherent", "single_row")),
    # tn_grouped
    ("tg-T15", (16, 15, 2, 3, 64, 64, 2), BF, "bf16-slab", False, "planes", "grouped", BASE),
    ("tg-3x21", (3, 21, 2, 3, 64, 64, 2), BF, "bf16-slab", False, "planes", "grouped", ALL_TN),
    ("tg-P17", (4, 16, 2, 17, 64, 64, 1), BF, "bf16-slab", False, "planes", "grouped", BASE),
    ("tg-C1280", (4, 16, 2, 3, 1280, 64, 2), BF, "bf16-slab", False, "planes", "grouped", BASE),
    ("tg-H32", (4, 16, 2, 3, 64, 32, 2), BF, "bf16-slab", False, "gemm_nt", "grouped", BASE + ("single_row",)),
    ("tg-H80", (4, 16, 3, 3, 64, 80, 1), BF, "bf16-slab", False, "gemm_nt", "grouped", BASE),
    ("tg-C30", (4, 16, 2, 3, 30, 64, 2), F32, "f32", False, "gemm_nt", "grouped", BASE),
    ("tg-misaligned", (4, 16, 2, 3, 64, 64, 2), BF, "bf16-slab", True, "planes", "grouped", BASE),
]
BWD_CASES = [pytest.param(*c[1:7], k, id=f"{c[0]}-{k}") for c in BWD for k in c[7]]


def _run_backward(hip, case, out_kind):
    B, T, S, P, C, H, L = case["dims"]
    out = None
    if out_kind != "f32":
        out = torch.full((B, T + 1, C), float("nan"), device=DEV, dtype=BF if out_kind == "bf16-slab" else F32)
    res = hip.debug_head_backward_gemms(case["ctx"], case["theta"], case["paths"], case["acts"], case["D4"], case["DO"], case["ws"],
                                        context_grad_out=out)
    return res, out


@pytest.mark.parametrize("dims, dtype, out_kind, misalign, gc_path, tn_path, kind", BWD_CASES)
def test_backward_gemms(dims, dtype, out_kind, misalign, gc_path, tn_path, kind):
    hip = _hip()
    B, T, S, P, C, H, L = dims
    case = R.make_case(kind, _gen(B * 1000 + T * 10 + C + H + L), dims, dtype, True, misalign, stage="backward")
    plan = R.tn_plan(dims, dtype == BF, ctx_aligned=not misalign)
    assert R.gctx_path(dims, out_kind == "bf16-slab") == gc_path and plan["path"] == tn_path, "the case does not reach its kernels"
    frag = hip.head_backward_workspace_bytes(1, 16, S, 0, 64, H, L) - R.backward_workspace_bytes((1, 16, S, 0, 64, H, L), 0)
    assert hip.head_backward_workspace_bytes(*dims) == R.backward_workspace_bytes(dims, frag), "the plan mirror is out of date"
    got, slab = _run_backward(hip, case, out_kind)
    got2, slab2 = _run_backward(hip, case, out_kind)
    for a, b in zip(got, got2):
        assert torch.equal(_bits(a), _bits(b)), "two runs differ"
    if slab is not None:
        assert bool(torch.isnan(slab[:, T].float()).all()), "row T of the context-gradient slab was written"
    assert bool(torch.isnan(case["store"][:, T].float()).all())

    # grad_context
    gC = (got[0][:, :T] if slab is not None else got[0]).reshape(B * T, C)
    ref, bound, A = R.gctx_ref(case["D4"], case["ws"][0], S, C, planes=(gc_path == "planes"), bf16_out=(out_kind == "bf16-slab"),
                               exact=(kind == "exact"), onehot=(kind == "onehot" and out_kind == "bf16-slab"))
    nbad, worst, where = R.excess(gC, ref, bound)
    amb = R.share(bound) if out_kind == "bf16-slab" else 0.0
    print(f"grad_context {gc_path} {dims} {kind}: out of bound {nbad}, worst err/bound {worst:.3g}, ambiguous {amb:.3f}")
    assert nbad == 0, (nbad, worst, where)
    if out_kind == "bf16-slab":
        assert amb <= R.SHARE_LIMIT[kind], amb

    # the thirteen TN sums
    worst_tn = 0.0
    for op in R.tn_operands(case):
        ref, mag = R.tn_ref(op["X"], op["Y"])
        c = 0.0 if kind == "exact" else R.tn_coefficient(plan, op["problem"], case["nonzero_rows"])
        g = got[op["idx"]][op["sel"]]
        nbad, worst, where = R.excess(g, ref, c * mag)
        worst_tn = max(worst_tn, worst if kind != "exact" else 0.0)
        assert nbad == 0, (op["name"], nbad, worst, where, c)
    print(f"weight gradients {tn_path} {dims} {kind}: worst err/bound {worst_tn:.3g}")


# ---------------------------------------------------------------------------------------- on the production operands
@pytest.mark.parametrize("B, L", [(16, 2), (32, 2), (8, 3)])
def test_debug_gemms_reproduce_head_backward_bit_for_bit(B, L):
    """D4 / DO of a real head_backward call (read back from its workspace) through debug_head_backward_gemms give that call's eleven
    GEMM outputs bit for bit: the hook launches what the product launches."""
    hip = _hip()
    T, S, P, C, H = 20, 2, 3, 64, 64
    NO = R.n_out(S)
    dims = (B, T, S, P, C, H, L)
    g = _gen(7 + B + L)
    rn = lambda *s, sc=1.0: torch.randn(*s, generator=g, device=DEV) * sc
    ws = [rn(3 * H, S + C + P, sc=.2), rn(3 * H, H, sc=.2), rn(3 * H, sc=.1), rn(3 * H, sc=.1), rn(L - 1, 3 * H, H, sc=.2),
          rn(L - 1, 3 * H, H, sc=.2), rn(L - 1, 3 * H, sc=.1), rn(L - 1, 3 * H, sc=.1), rn(NO, H, sc=.2), rn(NO, sc=.1)]
    x0, store, theta, eps = rn(B, S), rn(B, T + 1, C).to(BF), rn(B, P).abs(), rn(B, T, S)
    ctx = store[:, :T]
    gp, gm, gl = rn(B, T + 1, S), rn(B, T, S), rn(B, T, S, S)
    out = hip.head_forward(x0, ctx, theta, eps, ws, 0.05, True)
    nbytes = hip.head_backward_workspace_bytes(*dims)
    wsbuf = torch.zeros(nbytes, device=DEV, dtype=torch.uint8)
    slab = torch.full((B, T + 1, C), float("nan"), device=DEV, dtype=BF)
    grads = hip.head_backward(gp, gm, gl, ctx, theta, eps, out[0], out[3], out[4], ws, 0.05, context_grad_out=slab, workspace=wsbuf)
    lay = R.backward_workspace_layout(dims)
    D4 = wsbuf[lay["D4"]:lay["D4"] + B * T * L * 4 * H * 4].view(F32).reshape(B, T, L, 4, H).clone()
    DO = wsbuf[lay["DO"]:lay["DO"] + B * T * NO * 4].view(F32).reshape(B, T, NO).clone()
    assert bool(torch.isfinite(D4).all()) and float(D4.abs().max()) > 0
    slab2 = torch.full((B, T + 1, C), float("nan"), device=DEV, dtype=BF)
    again = hip.debug_head_backward_gemms(ctx, theta, out[0], out[4], D4, DO, ws, context_grad_out=slab2)
    want = (grads[1],) + tuple(grads[3:13])
    assert len(again) == 11
    for i, (a, b) in enumerate(zip(again, want)):
        assert torch.equal(_bits(a), _bits(b)), f"output {i} differs from head_backward's"
