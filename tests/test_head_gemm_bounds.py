"""CPU: the bounds, classes and plan mirrors of tests/head_gemm_reference.py against an emulation of the head's GEMM kernels' arithmetic
in torch -- the truncating three- and two-plane weight splits, the round-to-nearest operand splits with the products the kernels
keep, fp32 accumulation in the kernels' block and split order -- and against injected defects: the faithful emulation must stay
inside every bound for every class, ``exact`` and ``onehot`` must hold bit for bit, and every defect must be rejected by the class
named as catching it.  Also: the plan mirrors against the workspace queries (host only) and the ambiguous-share conditions for every
(shape, class) pair of tests/test_head_gemm_ops_gpu.py.
"""
import pytest
import torch

import head_gemm_reference as R
import test_head_gemm_ops_gpu as G
from head_gemm_reference import BF, F32, F64

NAN = float("nan")


def _gen(seed=0):
    return torch.Generator().manual_seed(seed)


def _acc(acc, add64):
    """One fp32 accumulation step: the block's products summed exactly, one rounding into the accumulator."""
    return (acc.to(F64) + add64).to(F32)


# ----------------------------------------------------------------------------------------------------- emulations
def emu_projection(case, path, defect=None):
    """proj_fwd_kernel<256[, 2]> (path 'planes') or gemm_nt_kernel: G [M, 3H] fp32, NaN where nothing is written."""
    B, T, S, P, C, H, L = case["dims"]
    M, N = B * T, 3 * H
    a = case["ctx"].reshape(M, C).to(F64)
    w = R.w_context(case["ws"][0], S, C).to(F64)
    b = case["ws"][2].to(F32)
    acc = torch.zeros(M, N, dtype=F32)
    if path == "planes":
        planes, rem = R.split_w(w, 3)
        assert float(rem.abs().max()) == 0.0          # three truncated planes hold 24 bits exactly
        if defect == "lo_dropped":
            planes[2] = torch.zeros_like(planes[2])
        if defect == "planes_swapped_k":              # the mid and lo planes indexed with neighbouring k exchanged
            perm = torch.arange(C) ^ 1
            planes[1], planes[2] = planes[1][:, perm], planes[2][:, perm]
        for kh in range(C // 256):
            if defect == "second_slice_skipped" and kh == 1:
                continue
            for pl in range(3):
                for ks in range(16):
                    k = slice(kh * 256 + ks * 16, kh * 256 + ks * 16 + 16)
                    acc = _acc(acc, a[:, k] @ planes[pl][:, k].t())
    else:
        for k0 in range(0, C, 4):                      # v_mfma_f32_16x16x4_f32: four terms per step
            acc = _acc(acc, a[:, k0:k0 + 4] @ w[:, k0:k0 + 4].t())
    out = acc if defect == "bias_omitted" else (acc + b).to(F32)
    if defect == "bias_twice":
        out = (out + b).to(F32)
    if defect == "partial_block_skipped":
        out = out.clone()
        out[M // 128 * 128:] = NAN
    return out


def emu_grad_context(case, path, bf16_out, defect=None):
    """proj_bwd_kernel<192> or gemm_nt_kernel into a [B, T+1, C] slab pre-filled with NaN; returns the slab."""
    B, T, S, P, C, H, L = case["dims"]
    M = B * T
    a, w = R.gctx_terms(case["D4"], case["ws"][0], S, C)
    acc = torch.zeros(M, C, dtype=F32)
    if path == "planes":
        (ah, al), _ = R.split_rne(a, 2)
        (wh, wl), _ = R.split_w(w.t().contiguous(), 2)
        wh, wl = wh.t(), wl.t()
        for ks in range(a.shape[1] // 16):
            k = slice(ks * 16, ks * 16 + 16)
            acc = _acc(acc, ah[:, k] @ wh[k])
            acc = _acc(acc, al[:, k] @ wh[k])
            if defect != "lo_hi_dropped":
                acc = _acc(acc, ah[:, k] @ wl[k])
    else:
        for k0 in range(0, a.shape[1], 4):
            acc = _acc(acc, a[:, k0:k0 + 4] @ w[k0:k0 + 4])
    if bf16_out:
        val = R.trunc_bf16(acc.to(F64)).to(BF) if defect == "truncated_store" else acc.to(BF)
    else:
        val = acc
    slab = torch.full((B * (T + 1) * C,), NAN, dtype=val.dtype)
    m = torch.arange(M)
    row = m * C if defect == "row_at_m_ldc" else (m // T) * (T + 1) * C + (m % T) * C
    slab[(row[:, None] + torch.arange(C)[None, :]).reshape(-1)] = val.reshape(-1)
    return slab.reshape(B, T + 1, C)


PX, PY = (2, 0, 1, 1, 0, 0), (0, 2, 1, 0, 1, 0)   # l h, h l, m m, m h, h m, h h (tw_run, smallest products first)


def _reduce4(parts):
    """tn_wide_reduce_kernel over partials [nsplit, ...]: four groups take every fourth split, each in four accumulators that chain
    every sixteenth, the rest into the first; fixed-order combines."""
    nsplit = parts.shape[0]
    groups = []
    for g in range(4):
        acc = [torch.zeros_like(parts[0]) for _ in range(4)]
        sp = g
        while sp + 12 < nsplit:
            for q in range(4):
                acc[q] = (acc[q] + parts[sp + 4 * q]).to(F32)
            sp += 16
        while sp < nsplit:
            acc[0] = (acc[0] + parts[sp]).to(F32)
            sp += 4
        groups.append(((acc[0] + acc[1]).to(F32) + (acc[2] + acc[3]).to(F32)).to(F32))
    t = groups[0]
    for q in range(1, 4):
        t = (t + groups[q]).to(F32)
    return t


def _reduce_bias(parts, defect=None):
    nsplit = parts.shape[0]
    t = [torch.zeros_like(parts[0]) for _ in range(4)]
    sp = 0
    while sp + 3 < nsplit:
        for q in range(4):
            t[q] = (t[q] + parts[sp + q]).to(F32)
        sp += 4
    while sp < nsplit and defect != "reduce_drops_tail":
        t[0] = (t[0] + parts[sp]).to(F32)
        sp += 1
    return ((t[0] + t[1]).to(F32) + (t[2] + t[3]).to(F32)).to(F32)


def emu_tile(X, Y, nsplit, mode, defect=None):
    """One tile of tn_wide_split_kernel: X [M, nx], Y [M, ny] fp32 (M % 16 == 0).  mode 'split6' (fp32 Y: six products of rounded
    pieces), 'split3' (bf16 Y), 'fp32' (the narrow tiles: v_mfma_f32_16x16x4_f32, four rows per step).  -> (dW [nx, ny], bias [nx])."""
    M, nx = X.shape
    chunks = M // 16
    Xb, Yb = X.to(F64).reshape(chunks, 16, nx), Y.to(F64).reshape(chunks, 16, -1)
    acc = torch.zeros(nsplit, nx, Yb.shape[2], dtype=F32)
    brow = torch.zeros(nsplit, 16, nx, dtype=F32)              # a thread's column sums keep their row slot from block to block
    for k in range(R._cdiv(chunks, nsplit)):
        blocks = torch.arange(k * nsplit, min(chunks, (k + 1) * nsplit))
        if defect == "block_skipped" and k == 0:
            blocks = blocks[1:]
        sp = blocks - k * nsplit
        xb, yb = Xb[blocks], Yb[blocks]
        brow[sp] = (brow[sp] + xb).to(F32)
        if mode == "fp32":
            for r0 in range(0, 16, 4):
                acc[sp] = _acc(acc[sp], torch.einsum("smn,smk->snk", xb[:, r0:r0 + 4], yb[:, r0:r0 + 4]))
            continue
        xp, xr = R.split_rne(xb, 3)
        assert float(xr.abs().max()) == 0.0                     # h + m + l == x bit for bit
        if mode == "split3":
            for p in (2, 1, 0):
                acc[sp] = _acc(acc[sp], torch.einsum("smn,smk->snk", xp[p], yb))
        else:
            yp, _ = R.split_rne(yb, 3)
            for p in range(6):
                if defect == "hl_lh_dropped" and p < 2:
                    continue
                acc[sp] = _acc(acc[sp], torch.einsum("smn,smk->snk", xp[PX[p]], yp[PY[p]]))
    bias = torch.zeros(nsplit, nx, dtype=F32)
    for r in range(16):
        bias = (bias + brow[:, r]).to(F32)
    if defect == "reduce_drops_tail":
        keep = nsplit // 4 * 4
        return _reduce4(torch.cat([acc[:keep], torch.zeros_like(acc[keep:])])), _reduce_bias(bias, defect)
    return _reduce4(acc), _reduce_bias(bias)


def emu_grouped(X, Y, rows_per_split, nsplit):
    """tn_grouped_kernel + tn_reduce_kernel: a split's rows in chunks of 64, two rows per pair of MFMA steps; splits summed in order."""
    M, nx = X.shape
    X64, Y64 = X.to(F64), Y.to(F64)
    out, bias = torch.zeros(nx, Y.shape[1], dtype=F32), torch.zeros(nx, dtype=F32)
    for s in range(nsplit):
        acc, bs = torch.zeros_like(out), torch.zeros_like(bias)
        for m in range(s * rows_per_split, min(M, (s + 1) * rows_per_split)):
            acc = _acc(acc, X64[m][:, None] * Y64[m][None, :])   # one row per MFMA (the other lane groups' rows follow in turn)
            bs = (bs + X[m]).to(F32)
        out, bias = (out + acc).to(F32), (bias + bs).to(F32)
    return out, bias


def emu_weight_gradients(case, plan, ctx_bf16, defect=None):
    """All TN sums of a case through the emulated launch; -> {name: tensor}.  Defects that live in the operand views (the h_{t-1} mask,
    the dn / dc_n remap) are applied to the operands, the others to the tile named in the defect's docstring."""
    B, T, S, P, C, H, L = case["dims"]
    ops = R.tn_operands(case)
    if defect == "hprev_from_previous_row":
        flat = case["acts"].reshape(B * T, L, 5, H)
        for op in ops:
            if op["name"].startswith("W_hh_l"):
                l = int(op["name"][6:])
                y = torch.zeros(B * T, H, dtype=F64)
                y[1:] = flat[:-1, l, 0].to(F64)                 # row m - 1 whatever its batch row
                op["Y"] = y
    if defect == "hh_reads_dn":
        for op in ops:
            if "hh" in op["name"]:
                l = int(op["name"][-1])
                op["X"] = case["D4"][:, :, l, :3].reshape(B * T, 3 * H).to(F64)
    res = {}
    for op in ops:
        kind, nsp, depth, drop = plan["problems"][op["problem"]]
        X = op["X"].to(F32)
        Y = (op["Y"] if op["Y"] is not None else torch.zeros(B * T, 1, dtype=F64)).to(F32)
        if kind < 0:
            w, b = emu_grouped(X, Y, depth - nsp[0] - 20, nsp[0])
        elif kind == 0:
            mode = "split3" if (op["problem"] == 0 and ctx_bf16) else "split6"
            tiles = [emu_tile(X, Y[:, 64 * i:64 * i + 64], nsp[i], mode, defect) for i in range(max(1, Y.shape[1] // 64))]
            w, b = torch.cat([t[0] for t in tiles], 1), tiles[0][1]
            if defect == "bias_from_tile_1" and op["problem"] == 0 and C >= 128:
                b = torch.full_like(b, NAN)   # only tile 0 of a problem writes the bias row of its partials: tile 1's is never written
        elif kind == 1:
            w, b = emu_tile(X, Y, nsp[0], "fp32", defect if defect == "reduce_drops_tail" else None)
        else:   # kind 2: out^T per 16 columns of the narrow operand (= rows of out), column sums of the narrow operand
            rows, bs = [], []
            for i in range(len(nsp)):
                xs = X[:, 16 * i:16 * i + 16]
                wt, _ = emu_tile(Y, xs, nsp[i], "fp32")
                _, bb = emu_tile(xs, torch.zeros(B * T, 1), nsp[i], "fp32")
                pad = 16 - xs.shape[1]
                rows.append(torch.cat([wt.t(), torch.zeros(pad, Y.shape[1]) if defect == "padding_rows_written" else
                                       torch.full((pad, Y.shape[1]), NAN)]))
                bs.append(bb)
            w, b = torch.cat(rows), torch.cat(bs)
        res[op["name"]] = b if op["Y"] is None else w
    return res


# ------------------------------------------------------------------------------------------------------- scoring
def projection_bad(case, path, G):
    kind = case["kind"]
    ref, A = R.proj_ref(case["ctx"], case["ws"][0], case["ws"][2], case["dims"][2], planes=(path == "planes"))
    if kind in ("exact", "onehot"):
        A = torch.zeros_like(A)
    return R.excess(G, ref, A)[0]


def grad_context_bad(case, path, bf16_out, slab):
    B, T, S, P, C, H, L = case["dims"]
    kind = case["kind"]
    ref, bound, A = R.gctx_ref(case["D4"], case["ws"][0], S, C, planes=(path == "planes"), bf16_out=bf16_out, exact=(kind == "exact"),
                               onehot=(kind == "onehot" and bf16_out))
    bad = R.excess(slab[:, :T].reshape(B * T, C), ref, bound)[0]
    return bad + int((~torch.isnan(slab[:, T].float())).sum())     # row T of the slab is never written


def weight_gradients_bad(case, plan, got):
    bad = 0
    for op in R.tn_operands(case):
        ref, mag = R.tn_ref(op["X"], op["Y"])
        c = 0.0 if case["kind"] == "exact" else R.tn_coefficient(plan, op["problem"], case["nonzero_rows"])
        g = got[op["name"]]
        if op["name"] == "out_weight":      # rows past NO are the padding of the last kind-2 tile: never written
            bad += int((~torch.isnan(g[ref.shape[0]:])).sum())
            g = g[:ref.shape[0]]
        bad += R.excess(g, ref, c * mag)[0]
    return bad


# --------------------------------------------------------------------------------------------------------- tests
PROJ_SHAPES = [((6, 25, 2, 3, 256, 64, 2), BF, "planes"), ((6, 25, 2, 3, 512, 64, 2), BF, "planes"), ((6, 25, 2, 3, 256, 64, 2), F32, "gemm_nt"),
               ((5, 13, 2, 3, 30, 20, 1), F32, "gemm_nt")]


@pytest.mark.parametrize("dims, dtype, path", PROJ_SHAPES)
@pytest.mark.parametrize("kind", G.ALL)
def test_projection_emulation_is_inside_the_bound(dims, dtype, path, kind):
    case = R.make_case(kind, _gen(1), dims, dtype)
    assert R.proj_path(dims, case["ctx"]) == path
    assert projection_bad(case, path, emu_projection(case, path)) == 0


PROJ_DEFECTS = [("lo_dropped", 256, ("onehot",)), ("planes_swapped_k", 256, ("onehot",)),
                ("second_slice_skipped", 512, ("exact", "onehot", "randn")), ("bias_omitted", 256, ("exact", "randn", "scaled")),
                ("bias_twice", 256, ("exact", "randn", "scaled")), ("partial_block_skipped", 256, ("exact", "randn", "onehot"))]


@pytest.mark.parametrize("defect, C, kinds", PROJ_DEFECTS)
def test_projection_defects_are_rejected(defect, C, kinds):
    dims = (6, 25, 2, 3, C, 64, 2) if defect != "second_slice_skipped" else (12, 25, 2, 3, C, 64, 2)   # onehot walks past k = 256
    for kind in kinds:
        case = R.make_case(kind, _gen(2), dims, BF)
        assert projection_bad(case, "planes", emu_projection(case, "planes", defect)) > 0, (defect, kind)


GC_SHAPES = [((6, 25, 2, 3, 64, 64, 2), "planes", True), ((6, 25, 2, 3, 256, 64, 1), "planes", True), ((6, 25, 2, 3, 64, 64, 2), "gemm_nt", False),
             ((6, 25, 2, 3, 32, 32, 2), "gemm_nt", True)]


@pytest.mark.parametrize("dims, path, bf16_out", GC_SHAPES)
@pytest.mark.parametrize("kind", G.ALL)
def test_grad_context_emulation_is_inside_the_bound(dims, path, bf16_out, kind):
    case = R.make_case(kind, _gen(3), dims, BF, stage="backward")
    assert R.gctx_path(dims, bf16_out) == path
    assert grad_context_bad(case, path, bf16_out, emu_grad_context(case, path, bf16_out)) == 0


def test_grad_context_split_remainders_stay_below_the_worst_case():
    """The per-term allowance the check uses (actual pieces) never exceeds the derived worst case C_SPLIT sum |a w|, and the worst
    case is attained to within 1 % by w = 2^e (1 + 2^-7 - 2^-23), a = 1 + 2^-8 - 2^-23 (its pieces: 1 and just under 2^-8)."""
    case = R.make_case("randn", _gen(4), (6, 25, 2, 3, 64, 64, 1), BF)
    a, w = R.gctx_terms(case["D4"], case["ws"][0], 2, 64)
    (ah, al), ra = R.split_rne(a, 2)
    (wh, wl), rw = R.split_w(w, 2)
    left = al.abs() @ wl.abs() + a.abs() @ rw.abs() + ra.abs() @ (wh + wl).abs()
    assert bool((left <= R.C_SPLIT * (a.abs() @ w.abs())).all())
    w1 = torch.tensor([1 + 2.0 ** -7 - 2.0 ** -23], dtype=F64)
    a1 = torch.tensor([1 + 2.0 ** -8 + 2.0 ** -9 - 2.0 ** -23], dtype=F64)
    (ah, al), ra = R.split_rne(a1, 2)
    (wh, wl), rw = R.split_w(w1, 2)
    worst = float((al * wl).abs() + (a1 * rw).abs() + (ra * (wh + wl)).abs()) / float(a1 * w1)
    assert 0.5 * R.C_SPLIT < worst <= R.C_SPLIT


GC_DEFECTS = [("lo_hi_dropped", ("onehot", "randn", "coherent")), ("row_at_m_ldc", ("exact", "randn", "onehot")),
              ("truncated_store", ("randn", "coherent"))]   # the sums of class exact stay below 256: bf16 values either way


@pytest.mark.parametrize("defect, kinds", GC_DEFECTS)
def test_grad_context_defects_are_rejected(defect, kinds):
    for kind in kinds:
        case = R.make_case(kind, _gen(5), (6, 25, 2, 3, 64, 64, 2), BF, stage="backward")
        assert grad_context_bad(case, "planes", True, emu_grad_context(case, "planes", True, defect)) > 0, (defect, kind)


TN_SHAPES = [((16, 17, 2, 3, 64, 64, 2), BF, "wide"), ((5, 16, 5, 3, 64, 64, 1), F32, "wide"), ((8, 272, 2, 0, 128, 64, 1), BF, "wide"),
             ((3, 21, 2, 3, 64, 64, 2), BF, "grouped"), ((4, 16, 2, 17, 30, 32, 1), F32, "grouped")]


@pytest.mark.parametrize("dims, dtype, path", TN_SHAPES)
@pytest.mark.parametrize("kind", G.ALL_TN)
def test_weight_gradient_emulation_is_inside_the_bound(dims, dtype, path, kind):
    case = R.make_case(kind, _gen(6), dims, dtype, stage="backward")
    plan = R.tn_plan(dims, dtype == BF)
    assert plan["path"] == path
    assert weight_gradients_bad(case, plan, emu_weight_gradients(case, plan, dtype == BF)) == 0


# (defect, dims, ctx dtype, classes that must reject it)
TN_DEFECTS = [
    ("hl_lh_dropped", (16, 17, 2, 3, 64, 64, 2), BF, ("single_row",)),
    ("block_skipped", (16, 17, 2, 3, 64, 64, 2), BF, ("exact", "randn", "coherent")),
    ("hprev_from_previous_row", (16, 17, 2, 3, 64, 64, 2), BF, ("exact", "randn", "single_row")),
    ("hh_reads_dn", (16, 17, 2, 3, 64, 64, 2), BF, ("exact", "randn")),
    ("bias_from_tile_1", (16, 17, 2, 3, 128, 64, 1), BF, ("exact", "randn")),
    ("padding_rows_written", (16, 17, 5, 3, 64, 64, 1), BF, ("exact", "randn")),
    ("reduce_drops_tail", (5, 16, 2, 3, 64, 64, 1), BF, ("exact", "randn", "coherent")),
]


@pytest.mark.parametrize("defect, dims, dtype, kinds", TN_DEFECTS)
def test_weight_gradient_defects_are_rejected(defect, dims, dtype, kinds):
    plan = R.tn_plan(dims, dtype == BF)
    assert plan["path"] == "wide"
    for kind in kinds:
        case = R.make_case(kind, _gen(7), dims, dtype, stage="backward")
        assert weight_gradients_bad(case, plan, emu_weight_gradients(case, plan, dtype == BF, defect)) > 0, (defect, kind)


def test_single_row_pieces_are_the_designed_ones():
    x = torch.tensor([1 + 2.0 ** -9 + 2.0 ** -17], dtype=F64) * 4
    (h, m, l), r = R.split_rne(x, 3)
    assert (float(h), float(m), float(l), float(r)) == (4.0, 4 * 2.0 ** -9, 4 * 2.0 ** -17, 0.0)


# -------------------------------------------------------------------------------------------- mirrors and shares
def test_plan_mirror_matches_the_workspace_query():
    from viforsdes_amd import _hip
    for L in (1, 2, 3, 4):
        for S in (1, 2, 3, 5, 9, 10):
            for H in (32, 64, 80):
                base = (1, 16, S, 0, 64, H, L)
                frag = _hip.head_backward_workspace_bytes(*base) - R.backward_workspace_bytes(base, 0)
                assert frag >= 0 and (frag == 0 or R.has_frag_block(base))
                for B, T in ((1, 16), (3, 16), (5, 16), (16, 17), (16, 31), (48, 25), (16, 272), (3, 21), (16, 15), (512, 400)):
                    for P in (0, 3, 16, 17):
                        for C in (30, 64, 256, 1024, 1280):
                            d = (B, T, S, P, C, H, L)
                            assert _hip.head_backward_workspace_bytes(*d) == R.backward_workspace_bytes(d, frag), d


def test_gpu_cases_reach_their_kernels_and_keep_the_share_conditions():
    """Every (shape, class) pair of the GPU file on the CPU: the plan mirror names the kernel the case is listed under, and the
    ambiguous share of the bf16 grad_context stays under the class's cap."""
    g = _gen(8)
    for name, dims, dtype, slab, misalign, path, kinds in G.PROJ:
        case = R.make_case(kinds[0], g, dims, dtype, slab, misalign)
        assert R.proj_path(dims, case["ctx"]) == path, name
    for name, dims, dtype, out_kind, misalign, gc_path, tn_path, kinds in G.BWD:
        B, T, S, P, C, H, L = dims
        assert R.gctx_path(dims, out_kind == "bf16-slab") == gc_path, name
        assert R.tn_plan(dims, dtype == BF, ctx_aligned=not misalign)["path"] == tn_path, name
        if out_kind != "bf16-slab":
            continue
        for kind in kinds:
            case = R.make_case(kind, g, dims, dtype, True, misalign, stage="backward")
            _, step, _ = R.gctx_ref(case["D4"], case["ws"][0], S, C, planes=(gc_path == "planes"), bf16_out=True, exact=(kind == "exact"),
                                    onehot=(kind == "onehot"))
            assert R.share(step) <= R.SHARE_LIMIT[kind], (name, kind, R.share(step))


def test_debug_entry_points_check_their_arguments_before_any_hip_call():
    """No GPU here: a refusal can only come from the host-side checks.  The pointers are never dereferenced."""
    import ctypes
    from viforsdes_amd import _hip
    lib = _hip.load()
    fake = ctypes.c_void_p(4096)
    d = _hip._Dims(4, 16, 2, 3, 64, 64, 2)
    w = _hip._Weights(*[fake] * 10)
    view = _hip._CtxView(fake, 1, 17 * 64, 64)
    fwd = lambda dims, v, ws_bytes, G=fake: lib.vsde_debug_head_context_projection(
        ctypes.byref(dims), ctypes.byref(v), ctypes.byref(w), G, fake, ctypes.c_size_t(ws_bytes), None)
    assert fwd(d, view, 0) < 0 and b"workspace too small" in lib.vsde_last_error()
    assert fwd(d, view, 1 << 30, None) < 0 and b"NULL" in lib.vsde_last_error()
    assert fwd(d, _hip._CtxView(fake, 7, 17 * 64, 64), 1 << 30) < 0 and b"context dtype" in lib.vsde_last_error()
    assert fwd(_hip._Dims(4, 16, 2, 3, 64, 64, 5), view, 1 << 30) < 0 and b"num_layers" in lib.vsde_last_error()
    grads = lambda dtype, stride: _hip._Grads(*[fake] * 13, dtype, stride)
    bwd = lambda g, ws_bytes, D4=fake: lib.vsde_debug_head_backward_gemms(
        ctypes.byref(d), ctypes.byref(view), fake, fake, fake, D4, fake, ctypes.byref(w), ctypes.byref(g), fake,
        ctypes.c_size_t(ws_bytes), None)
    assert bwd(grads(0, 0), 0) < 0 and b"workspace too small" in lib.vsde_last_error()
    assert bwd(grads(0, 0), 1 << 30, None) < 0 and b"NULL" in lib.vsde_last_error()
    assert bwd(grads(2, 0), 1 << 30) < 0 and b"context_dtype" in lib.vsde_last_error()
    assert bwd(grads(1, 16 * 64 - 8), 1 << 30) < 0 and b"context_batch_stride" in lib.vsde_last_error()
