"""CPU: the bounds of tests/linear_reference.py accept a faithful emulation of the GEMM kernels' arithmetic (fp32 products and
sums, bf16 rounding exactly where csrc/vsde_linear.hip, csrc/vsde_mlp.hip and csrc/vsde_wgrad.hip round) in every input class,
and reject each of nine injected defects.  Also here: the ambiguous-share conditions that keep the plain bound sharp, for every
(K, class) pair tests/test_linear_ops_gpu.py uses, and the launch-plan mirror against the figures the launch code's comments give."""
import pytest
import torch

import linear_reference as lr
from linear_reference import BF, F64

M0, N0 = 1024, 256


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def bf(t):
    return t.to(BF).float()


def trunc(t):
    return (t.float().contiguous().view(torch.int32) & -65536).view(torch.float32)


def emu_acc(x, w, drop=None, khalf=False):
    """fp32 accumulation over 16-deep k-steps, as the MFMA loop takes them.  drop: one k element left out; khalf: the first
    k-half's partial sum rounded to bf16 (the slip the two-k-half path of K = 512 invites)."""
    x32, w32 = x.float(), w.float()
    K = x.shape[1]
    if drop is not None:
        x32 = x32.clone()
        x32[:, drop] = 0
    acc = torch.zeros(x.shape[0], w.shape[0])
    for k0 in range(0, K, 16):
        acc = acc + x32[:, k0:k0 + 16] @ w32[:, k0:k0 + 16].t()
        if khalf and k0 + 16 == K // 2:
            acc = bf(acc)
    return acc


def emu_plain(x, w, b, rnd=bf, **kw):
    acc = emu_acc(x, w, **kw)
    return rnd(acc + b.float() if b is not None else acc)


def emu_swiglu(x, w, b, raw_a=False, raw_silu=False):
    u32 = emu_acc(x, w) + b.float()
    u = bf(u32)
    a, bb = lr.halves(u)
    if raw_a:
        a = lr.halves(u32)[0]
    t = a * torch.sigmoid(a)
    if not raw_silu:
        t = bf(t)
    return u, bf(t * bb)


def emu_swiglu_bwd(dy, w_t, u, wrong_factor=False):
    gs = emu_acc(dy, w_t)
    a, b = lr.halves(u.float())
    sg = torch.sigmoid(a)
    da = gs * b * sg * (1.0 + a * (sg if wrong_factor else 1.0 - sg))
    db = gs * a * sg
    return lr.interleave(bf(da), bf(db))


def emu_wgrad(dy, x, nsplit, drop_block=None, pad_garbage=False, db_skip_last=False):
    """Interleaved 32-row blocks per split, fp32 partials, fixed-order sum of the partials."""
    M = dy.shape[0]
    d32, x32 = dy.float(), x.float()
    if pad_garbage and M % 32:   # the clamped loads repeat the last row; without the zeroing those rows enter the sums
        pad = 32 - M % 32
        d32 = torch.cat([d32, d32[-1:].expand(pad, -1)])
        x32 = torch.cat([x32, x32[-1:].expand(pad, -1)])
    blocks = (d32.shape[0] + 31) // 32
    dW = torch.zeros(nsplit, dy.shape[1], x.shape[1])
    db = torch.zeros(nsplit, dy.shape[1])
    for blk in range(blocks):
        if blk == drop_block:
            continue
        d, v = d32[32 * blk:32 * blk + 32], x32[32 * blk:32 * blk + 32]
        dW[blk % nsplit] += d.t() @ v
        if not (db_skip_last and blk == blocks - 1):
            db[blk % nsplit] += d.sum(0)
    outW, outb = dW[0].clone(), db[0].clone()
    for s in range(1, nsplit):
        outW += dW[s]
        outb += db[s]
    return outW, outb


def nbad(got, ref, bound):
    return lr.excess(got, ref, bound)[0]


# ------------------------------------------------------------------------------------------------------- plain epilogue
@pytest.mark.parametrize("K", [64, 256, 512, 2816])
@pytest.mark.parametrize("kind", ["randn", "coherent", "exact", "scaled"])
def test_plain_bound_accepts_the_correct_emulation(kind, K):
    x, w, b = lr.gemm_operands(kind, _gen(K), 512, N0, K)
    ref, step = lr.plain_ref(x, w, b, exact=(kind == "exact"))
    assert nbad(emu_plain(x, w, b), ref, step) == 0
    ref, step = lr.plain_ref(x, w, None, exact=(kind == "exact"))
    assert nbad(emu_plain(x, w, None), ref, step) == 0


@pytest.mark.parametrize("K", [64, 256, 1536])
def test_truncating_output_conversion_is_rejected(K):   # defect 1
    x, w, b = lr.gemm_operands("coherent", _gen(1), M0, N0, K)
    ref, step = lr.plain_ref(x, w, b)
    assert nbad(emu_plain(x, w, b, rnd=trunc), ref, step) > 0.3 * ref.numel()
    x, w, b = lr.gemm_operands("randn", _gen(2), M0, N0, K)
    ref, step = lr.plain_ref(x, w, b)
    assert nbad(emu_plain(x, w, b, rnd=trunc), ref, step) > 0


def test_rounded_k_half_partial_sum_is_rejected():   # defect 2
    for kind in ("coherent", "randn"):
        x, w, b = lr.gemm_operands(kind, _gen(3), M0, N0, 512)
        ref, step = lr.plain_ref(x, w, b)
        assert nbad(emu_plain(x, w, b), ref, step) == 0
        assert nbad(emu_plain(x, w, b, khalf=True), ref, step) > 0.03 * ref.numel(), kind


def test_dropped_k_element_is_rejected():   # defect 3
    x, w, b = lr.gemm_operands("coherent", _gen(4), M0, N0, 2816)
    ref, step = lr.plain_ref(x, w, b)
    assert nbad(emu_plain(x, w, b, drop=1234), ref, step) > 0.01 * ref.numel()
    for K in (64, 2816):
        x, w, b = lr.gemm_operands("exact", _gen(5), M0, N0, K)
        ref, step = lr.plain_ref(x, w, b, exact=True)
        assert float(step.max()) == 0.0 and nbad(emu_plain(x, w, b), ref, step) == 0
        assert nbad(emu_plain(x, w, b, drop=K - 3), ref, step) > 0.3 * ref.numel()


# ------------------------------------------------------------------------------------------------------ SwiGLU epilogues
def _swiglu_case(kind, K, seed, M=M0, N=N0):
    x, w, b = lr.gemm_operands(kind, _gen(seed), M, N, K)
    if kind == "saturated":
        b = lr.saturate_bias(b)
    return x, w, b


@pytest.mark.parametrize("K", [128, 512])
@pytest.mark.parametrize("kind", ["randn", "coherent", "exact", "scaled", "saturated"])
def test_swiglu_bounds_accept_the_correct_emulation(kind, K):
    x, w, b = _swiglu_case(kind, K, 6)
    ref = lr.swiglu_ref(x, w, b, exact=(kind == "exact"))
    u, s = emu_swiglu(x, w, b)
    assert nbad(u, *ref["u"]) == 0 and nbad(s, *ref["s"]) == 0
    if kind == "saturated":   # the class does what it is for
        a = lr.halves(ref["u"][0])[0]
        assert float(a.max()) > 90 and float(a.min()) < -90 and int(((a.abs() > 25) & (a.abs() < 35)).sum()) > 0


@pytest.mark.parametrize("kind", ["randn", "saturated"])
def test_s_from_the_unrounded_a_is_rejected(kind):   # defect 4
    x, w, b = _swiglu_case(kind, 128, 7)
    ref = lr.swiglu_ref(x, w, b)
    assert nbad(emu_swiglu(x, w, b, raw_a=True)[1], *ref["s"]) > 0.05 * ref["s"][0].numel()


@pytest.mark.parametrize("kind", ["randn", "coherent"])
def test_unrounded_silu_is_rejected(kind):   # defect 5
    x, w, b = _swiglu_case(kind, 128, 8)
    ref = lr.swiglu_ref(x, w, b)
    assert nbad(emu_swiglu(x, w, b, raw_silu=True)[1], *ref["s"]) > 0.05 * ref["s"][0].numel()


def _bwd_case(kind, K, seed, M=M0, H=128):
    g = _gen(seed)
    dy, w_t, _ = lr.gemm_operands("randn" if kind == "saturated" else kind, g, M, H, K, bias=False)
    u = torch.randn(M, 2 * H, generator=g, dtype=torch.float32).to(F64) * 2
    if kind == "coherent":
        u = u.abs()
    if kind == "saturated":
        u = u + lr.saturate_bias(torch.zeros(2 * H, dtype=F64))
    return dy, w_t, u.to(BF)


@pytest.mark.parametrize("K", [128, 512])
@pytest.mark.parametrize("kind", ["randn", "coherent", "scaled", "saturated"])
def test_swiglu_bwd_bound_accepts_the_correct_emulation(kind, K):
    dy, w_t, u = _bwd_case(kind, K, 9)
    ref, bound = lr.swiglu_bwd_ref(dy, w_t, u)
    assert nbad(emu_swiglu_bwd(dy, w_t, u), ref, bound) == 0


@pytest.mark.parametrize("kind", ["randn", "coherent"])
def test_wrong_sigmoid_factor_in_da_is_rejected(kind):   # defect 6
    dy, w_t, u = _bwd_case(kind, 128, 10)
    ref, bound = lr.swiglu_bwd_ref(dy, w_t, u)
    assert nbad(emu_swiglu_bwd(dy, w_t, u, wrong_factor=True), ref, bound) > 0.2 * ref.numel()


# ------------------------------------------------------------------------------------------------------------- wgrad
def _wgrad_bounds(dy, x, nsplit):
    dW, mW, db, mb = lr.wgrad_ref(dy, x)
    c = lr.wgrad_depth(dy.shape[0], nsplit) * lr.ACC_C
    return dW, c * mW, db, c * mb


@pytest.mark.parametrize("M", [1, 33, 1000, 4096])
@pytest.mark.parametrize("kind", ["randn", "coherent", "exact", "scaled"])
def test_wgrad_bounds_accept_the_correct_emulation(kind, M):
    dy, x = lr.wgrad_operands(kind, _gen(11), M, 64, 48)
    nsplit = min(8, (M + 31) // 32)
    dW, bW, db, bb = _wgrad_bounds(dy, x, nsplit)
    gW, gb = emu_wgrad(dy, x, nsplit)
    if kind == "exact":
        assert torch.equal(gW.to(F64), dW) and torch.equal(gb.to(F64), db)
    assert nbad(gW, dW, bW) == 0 and nbad(gb, db, bb) == 0


@pytest.mark.parametrize("kind", ["randn", "exact", "scaled"])
@pytest.mark.parametrize("defect", ["drop_block", "pad_garbage", "db_skip_last"])   # defects 7, 8, 9
def test_wgrad_defects_are_rejected(defect, kind):
    M = 1000   # 31 whole blocks and one of 8 rows
    dy, x = lr.wgrad_operands(kind, _gen(12), M, 64, 48)
    dW, bW, db, bb = _wgrad_bounds(dy, x, 8)
    kw = {"drop_block": dict(drop_block=17), "pad_garbage": dict(pad_garbage=True), "db_skip_last": dict(db_skip_last=True)}[defect]
    gW, gb = emu_wgrad(dy, x, 8, **kw)
    bad = (nbad(gb, db, bb) if defect == "db_skip_last" else nbad(gW, dW, bW) + nbad(gb, db, bb))
    assert bad > 0.5 * (db.numel() if defect == "db_skip_last" else dW.numel())
    if kind == "exact":
        assert not (torch.equal(gW.to(F64), dW) and torch.equal(gb.to(F64), db))


# ------------------------------------------------------------------------------------------- conditions on the inputs
@pytest.mark.parametrize("K", lr.GPU_KS)
@pytest.mark.parametrize("kind", ["coherent", "randn", "scaled", "saturated", "exact"])
def test_ambiguous_share_conditions(kind, K):
    limit = lr.share_limit(kind, K)
    if limit is None:
        return   # randn-like data at K > 512: "within one ulp", no condition (every deep shape also runs coherent and exact)
    x, w, b = _swiglu_case(kind, K, 13, M=M0, N=N0)
    _, step = lr.plain_ref(x, w, b, exact=(kind == "exact"))
    sh = lr.share(step)
    print(f"SHARE {kind} K={K} {sh:.4f}")
    assert sh <= limit, (kind, K, sh)


# ------------------------------------------------------------------------------------------------------- plan mirrors
def test_plan_mirror_reproduces_the_figures_of_the_launch_code():
    P, S, B = lr.EPI_PLAIN, lr.EPI_SWIGLU, lr.EPI_SWIGLU_BWD
    # launch_rows_nw: "N = 1408 / 832 / 704: 22 / 13 / 11 pairs" at the OU example's 12.9 k tokens; 802 stripes -> 3 chunks forward;
    # the SwiGLU backward's 1,604 stripes of 128 rows -> 2 chunks; 133,000 rows = 520 stripes of 256 on 512 slots: a tail
    p = lr.rows_plan(12928, 832, 256, S)
    assert (p["stripes"], p["pairs"], p["chunks"], p["last_chunk_pairs"], p["rule"]) == (51, 13, 7, 1, "uneven")
    assert lr.rows_plan(12928, 1408, 256, S)["chunks"] == 11
    assert lr.rows_plan(205312, 1408, 256, S)["rule"] == "c3" and lr.rows_plan(205312, 704, 256, B)["rule"] == "c2"
    assert lr.rows_plan(205312, 704, 256, B)["stripes"] == 1604
    p = lr.rows_plan(133000, 256, 256, P)
    assert (p["stripes"], p["last"], p["tail_groups"], p["tail_chunks"]) == (520, "tail", 1, 4)
    assert lr.rows_plan(65535, 512, 512, P)["nw"] == 4 and lr.rows_plan(65536, 512, 512, P)["nw"] == 8
    # lin_variant: both fit -> rows for wide outputs, cols for deep reductions
    assert lr.lin_variant(100, 256, 256, P) == 1 and lr.lin_variant(100, 128, 256, P) == 2 and lr.lin_variant(100, 64, 192, P) == 0
    assert lr.lin_variant(100, 128, 192, S) == 0 and lr.lin_variant(100, 128, 512, B) == 1
    # wgrad2_plan: TN = 256 from three 256 x 256 tiles on; dW[2816, 512] = 22 tiles
    assert [lr.wgrad_tn(n, k) for n, k in ((256, 256), (832, 256), (256, 768), (512, 256), (8, 16))] == [128, 256, 256, 128, 128]
    assert lr.wgrad_nsplit(22 * 16 * (256 * 256 + 256) * 4, 2816, 512) == 16


def test_every_gpu_case_lands_in_the_branch_its_id_names():
    """The case tables of tests/test_linear_ops_gpu.py against the plan mirror (the GPU cases assert the same before they launch)."""
    import test_linear_ops_gpu as ops
    for table, epi in ((ops.ROWS, lr.EPI_PLAIN), (ops.SWIGLU, lr.EPI_SWIGLU), (ops.BWD, lr.EPI_SWIGLU_BWD)):
        for M, N, K, tags in table:
            assert lr.lin_variant(M, N, K, epi) == 1, (M, N, K)
            ops.check_tags(ops.rows_case_plan(M, N, K, epi), tags)
    for M, N, K, tags in ops.COLS:
        assert lr.lin_variant(M, N, K, lr.EPI_PLAIN) == 2, (M, N, K)
        ops.check_tags(lr.cols_plan(M, N, K), tags)
    seen = {w for t in (ops.ROWS, ops.SWIGLU, ops.BWD, ops.COLS) for c in t for w in c[3].split("-")}
    need = {"w4", "w8", "k512", "one", "doubling", "uneven", "c2", "c3", "c4", "pairs<2c", "first", "round", "tail", "tailcut", "notail",
            "idle", "ragged", "short", "nb4", "nb8", "k1"}
    assert need <= seen, need - seen
    assert {K for t in (ops.ROWS, ops.SWIGLU, ops.BWD, ops.COLS) for _, _, K, _ in t} | {H for _, _, H, _ in ops.MLP} <= set(lr.GPU_KS)
