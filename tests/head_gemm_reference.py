"""float64 references, per-element error bounds, input classes and launch-plan mirrors of the three non-recurrent GEMM stages of the
fused head, as ``_hip.debug_head_context_projection`` / ``_hip.debug_head_backward_gemms`` run them on given operands:

  context projection   G = ctx W_c^T + b_ih0                csrc/vsde_proj.hip split_planes_kernel<3>, proj_fwd_kernel<256>, <256, 2>
                                                             or csrc/vsde_gemm.hip gemm_nt_kernel
  grad_context         gC = dpre0 W_c                        split_planes_kernel<2>, proj_bwd_kernel<192>, or gemm_nt_kernel
  weight / bias grads  dW = X^T Y over all m = (b, t)        csrc/vsde_tn_wide.hip tn_wide_split_kernel + tn_wide_reduce_kernel, or
                                                             csrc/vsde_gemm.hip tn_grouped_kernel + tn_reduce_kernel
with W_c = W_ih_l0[:, S:S+C].  Plain functions on torch tensors of any device, in the style of tests/linear_reference.py:
tests/test_head_gemm_ops_gpu.py runs them on the GPU against the kernels, tests/test_head_gemm_bounds.py on the CPU against an
emulation of the kernels' arithmetic with injected defects.

Operand layouts (build_tn of csrc/vsde_head.hip)
  D4[b, t, l]   4H floats [dr | du | dn | dc_n]: the ih problems (and grad_context, l = 0) read columns [0, 3H), the hh problems
                [0, 2H) u [3H, 4H) (RowView col_split 2H, col_skip H)
  acts[b, t, l, 0] = h^l_t; a shift of -1 gives h^l_{t-1}, which is ZERO at t = 0 (not the previous batch row's last state)
  theta         [B, P] read with row stride 0: the same row for every t
  ctx           the [:, :T] view of a [B, T+1, C] slab (or any [B, T, C] view); paths [B, T+1, S], rows [:, :T] are read
  the thirteen sums: dW_ih_l0 = [X0^T paths | X0^T ctx | X0^T theta] (column blocks S | C | P), b_ih_l0 = colsum X0;
  dW_hh_l0 = Xh0^T h^0_{t-1}, b_hh_l0 = colsum Xh0; layers l >= 1: dW_ih = X_l^T h^{l-1}_t, dW_hh = Xh_l^T h^l_{t-1} and their
  column sums; out_weight = DO^T h^{L-1}_t, out_bias = colsum DO.

Bounds: per element, never relative to a tensor's maximum; ACC_C = 2^-24 is the fp32 unit round-off, every fp32 accumulation
(MFMA or VALU) is taken as no worse than round-to-nearest term by term (the assumption tests/linear_reference.py measured).
  projection, bf16 planes   split_planes_kernel<3> cuts W into three TRUNCATED bf16 planes (8 + 8 + 8 bits: hi + mid + lo == W exactly, all
                 of W's sign, so sum_p |plane_p| = |W|); ctx is bf16, so every product is exact in fp32; an output is one chain of
                 3 K products (three planes x K / 16 MFMA steps of 16, the k-slices of C = 512 continue the same accumulator) and
                 the bias add:  A = (3 K + 2) ACC_C (sum_k |a w| + |b|).
  gemm_nt        fp32 MFMA (16x16x4, fma chain) over K terms and the bias:  A = (K + 2) ACC_C (sum + |b|); a bf16 output is
                 round_bf16(y64, A) (round-to-nearest-even in the epilogue).
  grad_context, two planes   proj_bwd_kernel: a = ah + al + ra with ah = rne_bf16(a), al = rne_bf16(a - ah): |a - ah| <= 2^-8 |a|,
                 |al| <= 2^-8 (1 + 2^-8) |a|, |ra| <= 2^-16 |a|.  split_planes_kernel<2>: w = wh + wl + rw TRUNCATED: |w - wh| < 2^-7 |w|
                 (one ulp of 8 bits), the remainder's leading bit is at most 2^-8 |w|, so |rw| < 2^-15 |w|.  The kernel sums
                 wh ah + wh al + wl ah; what it leaves out is wl al + rw a + (wh + wl) ra:
                     C_SPLIT = 2^-15 (1 + 2^-8) + 2^-15 + 2^-16 = 5 * 2^-16 + 2^-23      (the header's "2^-16" is the typical size)
                 worst case, all three attained together by w = 2^e (1 + 2^-7 - 2^-23).  The check uses the SAME three terms per
                 (m, k, n) with the actual pieces instead of their worst case -- split_a2 / split_w2 below are the kernel's splits in
                 float64 -- which is never larger (tests/test_head_gemm_bounds.py asserts it) and on average about a quarter:
                     A = sum_k (|wl al| + |rw a| + |(wh + wl) ra|) + (3 K + 1) ACC_C (1 + 2^-6) sum_k |a w|
                 (a chain of 3 K exact bf16 products; 1 + 2^-6 covers |wh ah| + |wh al| + |wl ah| <= (1 + 2^-8)(1 + 2^-7) |a w|);
                 the bf16 output is round_bf16(y64, A).
  TN             |got - ref| <= c sum_m |x y|, c = D ACC_C + c_drop, D the longest chain of fp32 additions a term passes through:
                   192 x 64 split tiles  16 NP ceil(chunks / nsplit) + nsplit / 4 + 20: a split's 16-row blocks, NP = 6 (fp32 Y) or 3
                                     (bf16 Y) MFMAs of 16 products per block; the reduction chains every fourth split; 20 for the
                                     combines.  c_drop: x = h + m + l ROUNDED pieces, |m| <= 2^-8 (1 + 2^-8) |x|, |l| <= 2^-16 |x|;
                                     the dropped m l + l m + l l <= (2 * 2^-24 (1 + 2^-8) + 2^-32) |x y| < C_DROP = 2^-23 (1 + 2^-7);
                                     0 for a bf16 Y (one exact piece, all three pieces of X are multiplied)
                   narrow fp32 tiles (kinds 1, 2)  16 ceil(chunks / nsplit) + nsplit / 4 + 20, c_drop = 0
                   tn_grouped        rows_per_split + nsplit + 20 (a split's rows in one chain, the splits summed in order), c_drop = 0
                 nsplit from ``tn_plan``, the mirror of tw_splits / tn_plan at default knobs, which ``backward_workspace_bytes``
                 checks against vsde_head_backward_workspace_bytes.  Biases: c sum_m |x| with the same D (their chains are shorter).
                 Adding an exact zero commits no rounding: with R non-zero rows (class single_row) D = 6 R + R + 8.

Input classes (``make_case``); every value is one its operand's dtype holds exactly:
  exact       small integers: ctx, W_ih_l0 in {-1, 0, 1}, b_ih_l0 and every other operand in [-8, 8]; M 64 <= 2^24.  Every product and
              partial sum is exact in fp32 in any order and every split is exact: ZERO allowance, bit for bit (a bf16 grad_context is
              the one rounding of the exact integer)
  onehot      the left operand of the projection / of grad_context has ONE non-zero +-2^e per row, at column m mod K.  Projection: G
              must equal a W[n][k] + 0 (bias zero) bit for bit -- all three planes and their k indexing.  grad_context: W_c holds 16
              significant bits there (the two truncated planes are exact; the projection's W_c keeps all 24), so gC = rne_bf16(a w): round_bf16 with A = 2^-16 |term| covers it
  single_row  (TN) a handful of non-zero rows m -- the first, a t = 0 row, the last row, a row of the last 16-row group -- with
              full 24-bit mantissas +-(1 + 2^-9 + 2^-17) 2^e (pieces 1, 2^-9, 2^-17): sum |x y| has R terms, c = (7 R + 8) ACC_C + c_drop
              is far below the 2^-16 a dropped h l + l h costs
  coherent    all operands positive;  randn;  scaled: W row n (D4 column n) times 2^-(n mod 12), rows of D4 / DO times 10^(-3 u)

Ambiguous share of the bf16 grad_context (step > 0), asserted by the CPU test for every case of the GPU file: exact 0, onehot <= 2 %,
coherent <= 5 %, randn / scaled <= 1/2.
"""
import numpy as np
import torch

from linear_reference import ACC_C, BF, F64, SCALE_PERIOD, excess, round_bf16, row_slices, share  # noqa: F401  (re-exported)

F32 = torch.float32
C_SPLIT = 5 * 2.0 ** -16 + 2.0 ** -23
C_DROP = 2.0 ** -23 * (1 + 2.0 ** -7)
SHARE_LIMIT = {"exact": 0.0, "onehot": 0.02, "coherent": 0.05, "randn": 0.5, "scaled": 0.5, "single_row": 0.5}


def _cdiv(a, b):
    return (a + b - 1) // b


def n_out(S):
    return S + S * (S + 1) // 2


# ------------------------------------------------------------------------------------------------------------ splits
def trunc_bf16(x):
    """float64 tensor of fp32 values -> the value with the low 16 bits of its fp32 pattern cleared (split_planes_kernel)."""
    i = x.to(F32).contiguous().view(torch.int32)
    return (i & -65536).view(F32).to(F64)


def rne_bf16(x):
    return x.to(F32).to(BF).to(F64)


def split_w(w, planes):
    """split_planes_kernel<planes>: (pieces..., remainder), truncating; every remainder is exact in fp32."""
    out, r = [], w.to(F64)
    for _ in range(planes):
        p = trunc_bf16(r)
        out.append(p)
        r = r - p
    return out, r


def split_rne(x, pieces):
    """tw_split2 / the A split of proj_bwd_kernel: round-to-nearest-even pieces, (pieces..., remainder)."""
    out, r = [], x.to(F64)
    for _ in range(pieces):
        p = rne_bf16(r)
        out.append(p)
        r = r - p
    return out, r


# --------------------------------------------------------------------------------------------------------- references
def w_context(W_ih0, S, C):
    return W_ih0[:, S:S + C]


def proj_ref(ctx, W_ih0, b_ih0, S, planes):
    """(G64, A) [M, 3H] for ctx [B, T, C]; ``planes``: the bf16-plane kernel (chain of 3 K) or gemm_nt (K)."""
    B, T, C = ctx.shape
    a, w, b = ctx.reshape(B * T, C).to(F64), w_context(W_ih0, S, C).to(F64), b_ih0.to(F64)
    y = a @ w.t() + b
    mag = a.abs() @ w.abs().t() + b.abs()
    return y, ((3 * C if planes else C) + 2) * ACC_C * mag


def gctx_terms(D4, W_ih0, S, C):
    B, T, L, _, H = D4.shape
    return D4[:, :, 0].reshape(B * T, 4 * H)[:, :3 * H].to(F64), w_context(W_ih0, S, C).to(F64)


def gctx_ref(D4, W_ih0, S, C, planes, bf16_out, exact=False, onehot=False):
    """(ref, allowance-or-step, A) [M, C] of gC = dpre0 W_c; a bf16 output goes through round_bf16 (then the second value is the
    one-ulp step), an fp32 output is checked with |got - ref| <= A directly."""
    a, w = gctx_terms(D4, W_ih0, S, C)
    K = a.shape[1]
    y = a @ w
    mag = a.abs() @ w.abs()
    if planes:
        (ah, al), ra = split_rne(a, 2)
        (wh, wl), rw = split_w(w.t().contiguous(), 2)     # the planes are cut from WcT [C][3H]
        wh, wl, rw = wh.t(), wl.t(), rw.t()
        left = al.abs() @ wl.abs() + a.abs() @ rw.abs() + ra.abs() @ (wh + wl).abs()
        A = left + (3 * K + 1) * ACC_C * (1 + 2.0 ** -6) * mag
    else:
        A = (K + 2) * ACC_C * mag
    if exact:
        A = torch.zeros_like(A)
    if onehot:
        A = 2.0 ** -16 * mag
    if bf16_out:
        ref, step = round_bf16(y, A)
        return ref, step, A
    return y, A, A


def _rows(t, B, T):
    return t.reshape(B * T, -1).to(F64)


def tn_operands(case):
    """The thirteen TN sums of a case as a list of dicts: name, X [M, NX], Y [M, NY] or None (bias), key = (output index in the tuple
    ``debug_head_backward_gemms`` returns, row / column selection), problem = index into ``tn_plan``'s problems."""
    B, T, S, P, C, H, L = case["dims"]
    D4, DO, acts = case["D4"], case["DO"], case["acts"]
    M = B * T
    h = lambda l: acts[:, :, l, 0]
    def hprev(l):
        z = torch.zeros_like(acts[:, :, l, 0])
        z[:, 1:] = acts[:, :-1, l, 0]      # h^l_{t-1}: zero at t = 0
        return z
    x_ih = lambda l: _rows(D4[:, :, l, :3].reshape(B, T, 3 * H), B, T)
    x_hh = lambda l: _rows(torch.cat([D4[:, :, l, :2].reshape(B, T, 2 * H), D4[:, :, l, 3]], -1), B, T)
    ctx = case["ctx"]
    out, prob = [], 0
    sl = slice(None)
    out.append(dict(name="W_ih_l0[ctx]", X=x_ih(0), Y=_rows(ctx, B, T), idx=1, sel=(sl, slice(S, S + C)), problem=prob))
    out.append(dict(name="b_ih_l0", X=x_ih(0), Y=None, idx=3, sel=(sl,), problem=prob)); prob += 1
    out.append(dict(name="W_ih_l0[state]", X=x_ih(0), Y=_rows(case["paths"][:, :T], B, T), idx=1, sel=(sl, slice(0, S)), problem=prob)); prob += 1
    if P > 0:
        th = case["theta"][:, None, :].expand(B, T, P)
        out.append(dict(name="W_ih_l0[theta]", X=x_ih(0), Y=_rows(th, B, T), idx=1, sel=(sl, slice(S + C, S + C + P)), problem=prob)); prob += 1
    out.append(dict(name="W_hh_l0", X=x_hh(0), Y=_rows(hprev(0), B, T), idx=2, sel=(sl, sl), problem=prob))
    out.append(dict(name="b_hh_l0", X=x_hh(0), Y=None, idx=4, sel=(sl,), problem=prob)); prob += 1
    for l in range(1, L):
        out.append(dict(name=f"W_ih_l{l}", X=x_ih(l), Y=_rows(h(l - 1), B, T), idx=5, sel=(l - 1, sl, sl), problem=prob))
        out.append(dict(name=f"b_ih_l{l}", X=x_ih(l), Y=None, idx=7, sel=(l - 1, sl), problem=prob)); prob += 1
        out.append(dict(name=f"W_hh_l{l}", X=x_hh(l), Y=_rows(hprev(l), B, T), idx=6, sel=(l - 1, sl, sl), problem=prob))
        out.append(dict(name=f"b_hh_l{l}", X=x_hh(l), Y=None, idx=8, sel=(l - 1, sl), problem=prob)); prob += 1
    out.append(dict(name="out_weight", X=_rows(DO, B, T), Y=_rows(h(L - 1), B, T), idx=9, sel=(sl, sl), problem=prob))
    out.append(dict(name="out_bias", X=_rows(DO, B, T), Y=None, idx=10, sel=(sl,), problem=prob))
    return out


def tn_ref(X, Y):
    """(ref, mag) of X^T Y [NX, NY], or of the column sums of X when Y is None."""
    ref = mag = None
    for r0, r1 in row_slices(X.shape[0], max(X.shape[1], 1 if Y is None else Y.shape[1]), budget=2 ** 22):
        x = X[r0:r1]
        part = (x.sum(0), x.abs().sum(0)) if Y is None else (x.t() @ Y[r0:r1], x.abs().t() @ Y[r0:r1].abs())
        ref, mag = part if ref is None else (ref + part[0], mag + part[1])
    return ref, mag


# ------------------------------------------------------------------------------------------------------ plan mirrors
def proj_path(dims, ctx):
    """Which kernel the context projection takes: 'planes' (launch_proj_fwd_bf16) or 'gemm_nt'."""
    B, T, S, P, C, H, L = dims
    N = 3 * H
    ok = (ctx.dtype == BF and C in (256, 512) and N % 32 == 0 and N <= 512 and ctx.data_ptr() % 16 == 0
          and ctx.stride(0) % 8 == 0 and ctx.stride(1) % 8 == 0)
    return "planes" if ok else "gemm_nt"


def gctx_path(dims, out_bf16):
    """launch_proj_bwd_bf16 takes a bf16 output at 3H = 192 and C % 64 == 0 (torch allocations are 16-byte aligned)."""
    B, T, S, P, C, H, L = dims
    return "planes" if (out_bf16 and 3 * H == 192 and C % 64 == 0) else "gemm_nt"


def tn_problem_shapes(dims):
    """(NX, NY) of build_tn's problems, in its order."""
    B, T, S, P, C, H, L = dims
    pr = [(3 * H, C), (3 * H, S)] + ([(3 * H, P)] if P > 0 else []) + [(3 * H, H)]
    for _ in range(1, L):
        pr += [(3 * H, H), (3 * H, H)]
    return pr + [(n_out(S), H)]


def _tw_kind(nx, ny):
    if nx == 192 and ny > 0 and ny % 64 == 0:
        return 0
    if nx == 192 and 0 < ny <= 16:
        return 1
    if 0 < nx <= 64 and ny == 64:
        return 2
    return -1


def _tw_splits(kinds, chunks):
    """tw_splits of csrc/vsde_tn_wide.hip at the split form's default knobs (512 workgroups, weights 1 / 0.7 / 0.4), in its float32."""
    f = np.float32
    wgs, w = 512, [f(1.0), f(0.01) * f(70), f(0.01) * f(40)]
    tot, narrow, nwide = f(0), f(0), 0
    for k in kinds:
        tot = f(tot + w[k])
        if k == 0:
            nwide += 1
        else:
            narrow = f(narrow + w[k])
    wide_n = (int(f(wgs) / tot) & ~7) if nwide else 0
    left = wgs - nwide * wide_n
    last_narrow = max([i for i, k in enumerate(kinds) if k != 0], default=-1)
    out = []
    for i, k in enumerate(kinds):
        if k == 0:
            n = wide_n
        elif i == last_narrow:
            n = left & ~7
        else:
            n = int(f(f(f(left) * w[k]) / narrow) + f(4.0)) & ~7
            left -= n
            narrow = f(narrow - w[k])
        n = max(n, 8)
        out.append(min(n, chunks))
    return out


def tn_plan(dims, ctx_bf16, ctx_aligned=True):
    """The weight-gradient launch of a shape at default knobs.  -> dict(path 'wide' | 'grouped', per PROBLEM: list of (kind, nsplit,
    depth D, c_drop) -- the loosest over the problem's tiles --, wide_bytes, grouped_bytes)."""
    B, T, S, P, C, H, L = dims
    M = B * T
    shapes = tn_problem_shapes(dims)
    # generic plan (tn_plan of csrc/vsde_gemm.hip)
    tiles = sum(_cdiv(nx, 64) * _cdiv(ny, 64) for nx, ny in shapes)
    chunks64 = _cdiv(M, 64)
    nsplit = max(1, 2048 // tiles)
    nsplit = min(nsplit, chunks64, 256)
    cps = _cdiv(chunks64, nsplit)
    g_rows, g_nsplit = cps * 64, _cdiv(chunks64, cps)
    grouped_bytes = tiles * g_nsplit * (64 * 64 + 64) * 4
    # wide plan (tw_plan_shapes / tw_splits of csrc/vsde_tn_wide.hip)
    kinds = [_tw_kind(nx, ny) for nx, ny in shapes]
    wide_bytes, per_problem = 0, None
    if min(kinds) >= 0 and 0 in kinds:
        ntile = [ny // 64 if k == 0 else (_cdiv(nx, 16) if k == 2 else 1) for (nx, ny), k in zip(shapes, kinds)]
        if sum(ntile) <= 24:
            chunks = _cdiv(M, 16)
            tile_kinds = [k for k, n in zip(kinds, ntile) for _ in range(n)]
            ns = _tw_splits(tile_kinds, chunks)
            wide_bytes = sum(ns) * (192 * 64 + 192) * 4
            per_problem, at = [], 0
            for i, (k, n) in enumerate(zip(kinds, ntile)):
                nsp = ns[at:at + n]
                at += n
                np_ = (3 if (i == 0 and ctx_bf16) else 6) if k == 0 else 1
                depth = max(16 * np_ * _cdiv(chunks, s) + s // 4 + 20 for s in nsp)
                per_problem.append((k, nsp, depth, C_DROP if (k == 0 and np_ == 6) else 0.0))
    wide = per_problem is not None and T >= 16 and M % 16 == 0 and ctx_aligned
    if not wide:
        per_problem = [(-1, [g_nsplit], g_rows + g_nsplit + 20, 0.0) for _ in shapes]
    return dict(path="wide" if wide else "grouped", problems=per_problem, wide_bytes=wide_bytes, grouped_bytes=grouped_bytes,
                tn_bytes=max(wide_bytes, grouped_bytes))


def _a256(n):
    return (n + 255) & ~255


def backward_workspace_layout(dims):
    """bwd_layout of csrc/vsde_head.hip without the multi-path kernels' fragment block (H = 64, L = 2, S <= 2 only; a constant of
    csrc/vsde_head_mp.hip that ``frag_bytes`` reads back): offsets of D4 and DO, the bytes before the TN workspace, the TN bytes."""
    B, T, S, P, C, H, L = dims
    off = _a256((2 * L - 1) * 16 * 3 * 64 * 16) + _a256(3 * H * C * 4)
    d4 = off
    off += _a256(B * T * L * 4 * H * 4)
    do = off
    off += _a256(B * T * n_out(S) * 4)
    return dict(D4=d4, DO=do, fixed=off)


def has_frag_block(dims):
    B, T, S, P, C, H, L = dims
    return H == 64 and L == 2 and 1 <= S <= 2


def backward_workspace_bytes(dims, frag_bytes=0):
    """The mirror's total: what vsde_head_backward_workspace_bytes must return (both plans enter: the fast path may still decline)."""
    return backward_workspace_layout(dims)["fixed"] + (frag_bytes if has_frag_block(dims) else 0) + _a256(tn_plan(dims, True)["tn_bytes"])


def tn_coefficient(plan, problem, nonzero_rows=None):
    k, nsp, depth, drop = plan["problems"][problem]
    if nonzero_rows is not None:
        depth = min(depth, 7 * nonzero_rows + 8)
    return depth * ACC_C + drop


# ------------------------------------------------------------------------------------------------------ input classes
def _randn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=F32, device=g.device).to(F64)


def _ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g, device=g.device).to(F64)


def _pow2(g, *shape):
    """+-2^e, e in [-3, 3]."""
    e = torch.randint(-3, 4, shape, generator=g, device=g.device).to(F64)
    s = torch.randint(0, 2, shape, generator=g, device=g.device).to(F64) * 2 - 1
    return s * 2.0 ** e


def _full24(g, *shape):
    """+-(1 + 2^-9 + 2^-17) 2^e: rne pieces 1, 2^-9, 2^-17 (times 2^e)."""
    return _pow2(g, *shape) * (1 + 2.0 ** -9 + 2.0 ** -17)


def single_rows(B, T):
    """The non-zero rows m of class single_row: the first row, a t = 0 row and its predecessor (the last step of the batch row before
    it: what a wrong h_{t-1} mask would read), the last row, a row of the last 16-row group."""
    M = B * T
    rows = {0, M - 1, max(0, M - 9)}
    if B > 1:
        rows |= {(B // 2) * T, (B // 2) * T - 1, (B - 1) * T}
    return sorted(rows)


def make_case(kind, g, dims, ctx_dtype=BF, slab=True, misalign=False, stage="projection"):
    """All operands of one (shape, class) case on the generator's device.  ctx is a [B, T, C] view (of a [B, T+1, C] slab whose row T is
    NaN when ``slab``; ``misalign``: of storage that starts 2 bytes past a 16-byte boundary); the ten weights ``ws`` are fp32.  ``stage``
    "backward" cuts the W_c of class onehot to 16 significant bits (grad_context's two planes then hold it exactly); the projection
    gets all 24."""
    B, T, S, P, C, H, L = dims
    dev, NO, I = g.device, n_out(S), S + C + P
    q = (lambda t: t.to(BF).to(F64)) if ctx_dtype == BF else (lambda t: t.to(F32).to(F64))
    rn, nz = (lambda *s: _randn(g, *s)), None
    if kind == "exact":
        assert B * T * 64 <= 2 ** 24
        it = lambda *s: _ints(g, -8, 8, *s)
        ctx, Wih0, b0 = _ints(g, -1, 1, B, T, C), _ints(g, -1, 1, 3 * H, I), it(3 * H)
        D4, DO, acts, paths, theta = it(B, T, L, 4, H), it(B, T, NO), it(B, T, L, 5, H), it(B, T + 1, S), it(B, P)
    elif kind in ("randn", "coherent", "scaled"):
        ctx, Wih0, b0 = rn(B, T, C), rn(3 * H, I) * C ** -0.5, rn(3 * H)
        D4, DO, acts, paths, theta = rn(B, T, L, 4, H), rn(B, T, NO), rn(B, T, L, 5, H), rn(B, T + 1, S), rn(B, P)
        if kind == "coherent":
            ctx, Wih0, b0, D4, DO, acts, paths, theta = (t.abs() for t in (ctx, Wih0, b0, D4, DO, acts, paths, theta))
        if kind == "scaled":
            sc = 2.0 ** -(torch.arange(3 * H, device=dev) % SCALE_PERIOD).to(F64)
            Wih0, b0 = Wih0 * sc[:, None], b0 * sc
            sc4 = 2.0 ** -(torch.arange(4 * H, device=dev) % SCALE_PERIOD).to(F64).reshape(4, H)
            u = 10.0 ** (-3.0 * torch.randint(0, 3, (B, T), generator=g, device=dev).to(F64))
            D4 = D4 * sc4 * u[:, :, None, None, None]
            DO = DO * 2.0 ** -(torch.arange(NO, device=dev) % SCALE_PERIOD).to(F64) * u[:, :, None]
    elif kind == "onehot":
        m = torch.arange(B * T, device=dev)
        ctx = torch.zeros(B * T, C, dtype=F64, device=dev)
        ctx[m, m % C] = _pow2(g, B * T)
        ctx = ctx.reshape(B, T, C)
        Wih0, b0 = rn(3 * H, I), torch.zeros(3 * H, dtype=F64, device=dev)
        if stage == "backward":
            Wih0[:, S:S + C] = trunc16(Wih0[:, S:S + C])
        D4 = torch.zeros(B * T, L, 4 * H, dtype=F64, device=dev)
        D4[m, :, m % (3 * H)] = _pow2(g, B * T)[:, None]
        D4 = D4.reshape(B, T, L, 4, H)
        DO, acts, paths, theta = rn(B, T, NO), rn(B, T, L, 5, H), rn(B, T + 1, S), rn(B, P)
    elif kind == "single_row":
        nz = single_rows(B, T)
        keep = torch.zeros(B * T, dtype=F64, device=dev)
        keep[torch.tensor(nz, device=dev)] = 1.0
        keep = keep.reshape(B, T)
        f24 = lambda *s: _full24(g, *s)
        ctx, Wih0, b0 = (_pow2(g, B, T, C) if ctx_dtype == BF else f24(B, T, C)), rn(3 * H, I), rn(3 * H)
        D4 = f24(B, T, L, 4, H) * keep[:, :, None, None, None]
        DO = f24(B, T, NO) * keep[:, :, None]
        acts, paths, theta = f24(B, T, L, 5, H), f24(B, T + 1, S), f24(B, P)
    else:
        raise ValueError(kind)
    ctx = q(ctx)
    f32 = lambda t: t.to(F32)
    T1 = T + 1 if slab else T
    if misalign:
        flat = torch.zeros(B * T1 * C + 8, dtype=ctx_dtype, device=dev)
        store = flat[1:1 + B * T1 * C].view(B, T1, C)
    else:
        store = torch.zeros(B, T1, C, dtype=ctx_dtype, device=dev)
    store[:, :T] = ctx.to(ctx_dtype)
    if slab:
        store[:, T] = float("nan")
    z = lambda *s: torch.zeros(*s, dtype=F32, device=dev)
    ws = [f32(Wih0), z(3 * H, H), f32(b0), z(3 * H), z(L - 1, 3 * H, H), z(L - 1, 3 * H, H), z(L - 1, 3 * H), z(L - 1, 3 * H),
          z(NO, H), z(NO)]
    return dict(kind=kind, dims=dims, ctx=store[:, :T], store=store, ws=ws, D4=f32(D4), DO=f32(DO), acts=f32(acts), paths=f32(paths),
                theta=f32(theta), nonzero_rows=(len(nz) if nz else None))


def trunc16(w):
    """fp32 values cut to 16 significant bits: two truncated bf16 planes hold them exactly."""
    (a, b), _ = split_w(w.to(F32).to(F64), 2)
    return a + b
