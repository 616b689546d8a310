"""float64 references, per-element error bounds, input classes and launch-plan mirrors of the encoder's GEMM family:
``vsde_linear_bf16`` (plain, SwiGLU and SwiGLU-backward epilogues on the rows and cols kernels of csrc/vsde_linear.hip), the
weight / bias gradients of csrc/vsde_wgrad.hip and the fused MLP forward of csrc/vsde_mlp.hip.  Plain functions on torch tensors
of any device: tests/test_linear_ops_gpu.py runs them on the GPU against the kernels, tests/test_linear_bounds.py on the CPU
against an emulation of the kernels' arithmetic (with injected defects that each bound must reject).

Every reference takes a ROW SLICE of its operands (``row_slices``): at M = 205,312 and N = 1,408 one float64 tensor is 2.3 GB.

Bounds, per element, never relative to a tensor's maximum.  U = 2^-8 is the bf16 unit round-off, ACC_C = 2^-24 the fp32 one.
  plain          y = rnd(x W^T + b).  A = (K + 2) ACC_C (sum_k |x_k w_k| + |b|) is the worst case of a round-to-nearest fp32
                 accumulation over K terms and the bias add (derived, not measured).  ref, step = round_bf16(y64, A): an element
                 passes iff |got - ref| <= step, i.e. bit-exact except where float64 lies within A of a rounding boundary; there
                 the neighbouring bf16 value is accepted too.  ``share`` = the fraction of such ambiguous elements.
  SwiGLU         u as above; s = rnd(rnd(silu(a)) b) from the ROUNDED a, b.  The one-ulp allowance of u is carried into s: s is
                 evaluated for each admissible (a, b) and for both roundings of silu(a) within SIGM_C = 4e-6 relative (sigm_f:
                 __expf + fast_rcp; the constant tests/test_encoder_ops_gpu.py uses for |a| <= 30), and the hull is accepted.
                 The product of two bf16 values is exact in fp32, so nothing else enters.  Floor: TINY (1 + |b|), TINY = 2^-126
                 the smallest normal bf16 -- a flushed denormal silu(a) (error < TINY) times b, and a flushed denormal output.
  SwiGLU bwd     acc = ds = dy w_t^T stays fp32; a, b are the given bf16 u.  da = rnd(ds b sg (1 + a (1 - sg))), db = rnd(ds a sg):
                 round_bf16 of the float64 value with allowance |d out / d ds| A_ds + 1e-5 |terms| + floor, A_ds as in the plain
                 case without bias, |terms| = |ds b sg| (1 + |a (1 - sg)|) resp. |ds a sg|, floor = TINY (1 + |d out / d sg|):
                 a sigmoid below the smallest normal fp32 (a < -87) may be flushed, and so may a denormal output.
  fused MLP      s as in the SwiGLU epilogue (the kernel's u never leaves it; its bias is an fp32 accumulator initialiser, the
                 same K + 1 additions); y = rnd(s W2^T + b2) is checked teacher-forced on the kernel's OWN s with the plain bound
                 at K = H.
  wgrad          dW, db fp32: |got - ref| <= c sum_m |dy_mn x_mk| (c sum_m |dy_mn| for db), c = D ACC_C with D the longest chain of
                 fp32 additions a term passes through: D = 2 ceil(blocks / nsplit) + nsplit / 4 + 20 (a split's 32-row blocks,
                 two 16-deep MFMA steps each; the fixed-order reduction, which chains every fourth split; 20 for the sums
                 inside an MFMA step and the final combines).  nsplit is read back from ``vsde_linear_wgrad_workspace_bytes`` (``wgrad_nsplit``).  Sound but loose: the
                 sharp check of these kernels is the ``exact`` class.

Input classes (``gemm_operands`` / ``wgrad_operands``):
  randn      x ~ N(0, 1), W ~ N(0, 1 / K), b ~ N(0, 1): terms cancel, A is large against |y|
  coherent   all operands positive (|randn|, weights scaled by 1 / K): sum |x w| = |y|, A stays far below one ulp at any K
  exact      small integers: every product and partial sum is exact in fp32 in any order.  GEMMs: x, W dense in {-1, 0, 1},
             bias integers in [-8, 8]: NO allowance at any K.  wgrad: integers in [-8, 8] (M 64 <= 2^24): dW, db equal float64 exactly
  scaled     randn with row n of W (column n of dy) multiplied by 2^-(n mod 12)
  saturated  (SwiGLU) randn with bias +-30 and +-100 on some ``a`` columns: saturated sigmoid, overflowing __expf

Ambiguous share (step > 0), measured on the CPU with this module alone (M = 1024, N = 256; tests/test_linear_bounds.py asserts
the conditions for every (K, class) pair of the GPU file): coherent <= 10 % at every K (0.1 % at K = 64, 1.2 % at 512, 6.3 % at
2816); randn, scaled and saturated <= 1/3 at K <= 512 (2.9 % at K = 64, 14 % at 256, 31 % at 512; scaled, exponents n mod 12,
has exactly the share of randn -- a power of two on a column moves y and A alike; without a bias randn reaches 37 % at K = 512,
so the GPU file runs that variant at K = 512 in the sharp classes only); randn at K > 512 degenerates to "within one ulp",
which is why every deep shape also runs coherent and exact.

MFMA rounding.  The constant ACC_C = 2^-24 assumes that v_mfma_f32_32x32x16_bf16 accumulates no worse than round-to-nearest fp32
term by term.  Measured on an MI355X: it held -- no element of any case of tests/test_linear_ops_gpu.py left its bound (rows and
cols kernels, K 64 .. 2816, all classes), and of the ambiguous elements only about one in a thousand took the neighbouring value
at all.  torch's own bf16 matmul (hipBLASLt, the same instruction) through the same check, M = 4,264 / 133,000, K 64 .. 2816:
0 elements out of bound with 2^-24 as well (coherent K = 2816: 137,927 of 2.2 M ambiguous, 46 at the neighbour; randn K = 512:
664,986 ambiguous, 202 at the neighbour; exact: bit for bit).  The constant was therefore not widened.
"""
import torch

from attention_reference import BF, F64, U, excess, round_bf16  # noqa: F401  (re-exported for the tests)

ACC_C = 2.0 ** -24
SIGM_C = 4e-6
TERM_C = 1e-5
TINY = 2.0 ** -126
EPI_PLAIN, EPI_SWIGLU, EPI_SWIGLU_BWD = 0, 1, 2
SCALE_PERIOD = 12


def row_slices(M, width, budget=2 ** 25):
    """Row ranges whose [rows, width] float64 tensors stay within ``budget`` elements."""
    step = max(1, budget // max(1, width))
    return [(r0, min(M, r0 + step)) for r0 in range(0, M, step)]


# --------------------------------------------------------------------------------------------------------- references
def gemm64(x, w, bias=None, c=ACC_C):
    """(y64, A) of y = x W^T + b: A = (K + 2) c (sum_k |x_k w_k| + |b|)."""
    x64, w64 = x.to(F64), w.to(F64)
    y = x64 @ w64.t()
    mag = x64.abs() @ w64.abs().t()
    if bias is not None:
        y = y + bias.to(F64)
        mag = mag + bias.to(F64).abs()
    return y, (x.shape[1] + 2) * c * mag


def plain_ref(x, w, bias=None, exact=False, c=ACC_C):
    """(ref, step): the bf16 output of the plain epilogue and its one-ulp allowance; ``exact``: no allowance at all."""
    y, A = gemm64(x, w, bias, c)
    if exact:
        A = torch.zeros_like(A)
    # mirrors stage_block: pack_bf16x2(acc + bias) -- the one rounding of the plain epilogue
    return round_bf16(y, A)


def halves(u):
    """(a, b) [m, N / 2] of an interleaved [m, N] matrix: blocks of 16 columns, a then b."""
    m, N = u.shape
    v = u.reshape(m, N // 32, 2, 16)
    return v[:, :, 0].reshape(m, N // 2), v[:, :, 1].reshape(m, N // 2)


def interleave(a, b):
    m, H = a.shape
    return torch.stack([a.reshape(m, H // 16, 16), b.reshape(m, H // 16, 16)], 2).reshape(m, 2 * H)


def _silu_candidates(a):
    t = a * torch.sigmoid(a)
    e = SIGM_C * t.abs()
    # mirrors swiglu_stage: t = pack_bf16x2(a0 * sigm_f(a0), ..) -- silu rounded to bf16 before the product with b
    return (t - e).to(BF).to(F64), (t + e).to(BF).to(F64)


def swiglu_s_ref(ya, Aa, yb, Ab):
    """(ref, bound) of s = rnd(rnd(silu(a)) b) with a = rnd(ya), b = rnd(yb) known up to the allowances Aa, Ab: the hull over the
    admissible (a, b) and over both roundings of silu, as (mid-point, half-width + floor)."""
    # mirrors swiglu_stage / swiglu_quads: a, b are the ROUNDED u (the packed words that go to the staging row)
    a_c = ((ya - Aa).to(BF).to(F64), (ya + Aa).to(BF).to(F64))
    b_c = ((yb - Ab).to(BF).to(F64), (yb + Ab).to(BF).to(F64))
    lo = hi = None
    for a in a_c:
        for t in _silu_candidates(a):
            for b in b_c:
                # mirrors out = pack_bf16x2(bf_lo(t) * b0, ..): the fp32 product of two bf16 values is exact, one rounding
                s = (t * b).to(BF).to(F64)
                lo = s if lo is None else torch.minimum(lo, s)
                hi = s if hi is None else torch.maximum(hi, s)
    floor = TINY * (1.0 + torch.maximum(b_c[0].abs(), b_c[1].abs()))
    return (lo + hi) / 2, (hi - lo) / 2 + floor


def swiglu_ref(x, w, bias=None, exact=False, c=ACC_C):
    """The SwiGLU epilogue for the interleaved-packed w [N, K]: {"u": (ref, step) [m, N], "s": (ref, bound) [m, N / 2]}."""
    y, A = gemm64(x, w, bias, c)
    if exact:
        A = torch.zeros_like(A)
    ya, yb = halves(y)
    Aa, Ab = halves(A)
    return {"u": round_bf16(y, A), "s": swiglu_s_ref(ya, Aa, yb, Ab)}


def swiglu_bwd_ref(dy, w_t, u, exact=False, c=ACC_C):
    """(ref, bound) of du [m, 2 H] (interleaved like u) from dy [m, K], w_t [H, K] and the saved bf16 u [m, 2 H]."""
    ds, A = gemm64(dy, w_t, None, c)          # mirrors the EPI_SWIGLU_BWD block: gs = acc stays fp32
    if exact:
        A = torch.zeros_like(A)
    a, b = halves(u.to(F64))
    sg = torch.sigmoid(a)
    one = 1.0 + a * (1.0 - sg)
    da = ds * b * sg * one                    # mirrors da[i] = gs * b[i] * sg * (1.0f + a[i] * (1.0f - sg))
    db = ds * a * sg                          # mirrors db[i] = gs * a[i] * sg
    ta = (ds * b * sg).abs() * (1.0 + (a * (1.0 - sg)).abs())
    tb = db.abs()
    fa = TINY * (1.0 + (ds * b).abs() * (1.0 + a.abs()))
    fb = TINY * (1.0 + (ds * a).abs())
    # mirrors pack_bf16x2(da[0], da[1]) / pack_bf16x2(db[0], db[1]): one rounding each
    ra, sa = round_bf16(da, (b * sg * one).abs() * A + TERM_C * ta + fa)
    rb, sb = round_bf16(db, (a * sg).abs() * A + TERM_C * tb + fb)
    return interleave(ra, rb), interleave(sa + fa, sb + fb)


def mlp_s_ref(x, w_in, b_in, hreal, exact=False, c=ACC_C):
    """(ref, bound) of the fused MLP's s [m, hreal] for w_in [2 hreal, C] = [a rows | b rows], b_in [2 hreal] (both as bf16 values)."""
    # mirrors gemm1: uacc starts as the fp32 copy of the bf16 bias, then C / 16 MFMA steps; swiglu8: pack2 of u, of silu, of the product
    y, A = gemm64(x, w_in, b_in, c)
    if exact:
        A = torch.zeros_like(A)
    return swiglu_s_ref(y[:, :hreal], A[:, :hreal], y[:, hreal:], A[:, hreal:])


def wgrad_partial(dy, x):
    """Float64 sums of one row slice: (dy^T x, |dy|^T |x|, colsum dy, colsum |dy|); the caller adds the slices up."""
    d, v = dy.to(F64), x.to(F64)
    return d.t() @ v, d.abs().t() @ v.abs(), d.sum(0), d.abs().sum(0)


def wgrad_ref(dy, x):
    """(dW, magW, db, magb) in float64 over all rows, accumulated in row slices."""
    acc = None
    for r0, r1 in row_slices(dy.shape[0], max(dy.shape[1], x.shape[1])):
        part = wgrad_partial(dy[r0:r1], x[r0:r1])
        acc = part if acc is None else tuple(p + q for p, q in zip(acc, part))
    return acc


# ------------------------------------------------------------------------------------------------------ plan mirrors
def lin_variant(M, N, K, epi):
    """csrc/vsde_linear.hip lin_variant of the product build: 1 = rows kernel, 2 = cols kernel, 0 = not covered."""
    rows_ok = K in (128, 256, 512) and N % 64 == 0
    cols_ok = K % 64 == 0 and N % 128 == 0 and epi == EPI_PLAIN
    if epi != EPI_PLAIN:
        return 1 if rows_ok else 0
    if rows_ok and (not cols_ok or N >= K):
        return 1
    return 2 if cols_ok else (1 if rows_ok else 0)


def _cdiv(a, b):
    return (a + b - 1) // b


def rows_plan(M, N, K, epi):
    """launch_rows / launch_rows_nw of csrc/vsde_linear.hip for the three epilogues of ``vsde_linear_bf16`` (default knobs):
    waves per workgroup, stripe height, column chunks, the tail groups and their chunks, and the name of the chunk rule taken."""
    nkh = 2 if K == 512 else 1
    nw = 8 if (nkh > 1 and M >= 256 * 256) else 4
    rb = 1 if (epi == EPI_SWIGLU_BWD or nkh > 1) else 2
    rows, resident = 32 * nw * rb, (512 if nw == 4 else 256)
    stripes, pairs = _cdiv(M, rows), N // 64
    chunks, rule = 1, "one"
    if epi != EPI_PLAIN and stripes < resident and pairs >= 2:
        c = min(_cdiv(resident, stripes), pairs)
        ppc = _cdiv(pairs, c)
        chunks = _cdiv(pairs, ppc)
        rule = "uneven" if chunks > 1 else "one"
    else:
        while stripes * chunks < resident and chunks * 2 <= pairs and pairs % (chunks * 2) == 0:
            chunks *= 2
        rule = "doubling" if chunks > 1 else "one"
    uneven_ok = epi != EPI_PLAIN
    want = 1 if epi == EPI_PLAIN else 2
    if uneven_ok:
        best = 0.0
        for c in (2, 3, 4):
            if pairs < 2 * c:
                break
            rounds = stripes * c / resident
            eff = rounds / float(int(rounds + 0.999999)) - 0.05 * c
            if eff > best:
                best, want = eff, c
    if stripes >= resident and want > 1 and (pairs % want == 0 or (uneven_ok and pairs >= 2 * want)):
        chunks, rule = want, f"c{want}"
    groups = _cdiv(stripes, 8)
    wg_main = groups * 8 * chunks
    full = wg_main // resident * resident
    rest = wg_main - full
    tail_groups, tail_chunks, tc_first = 0, chunks, 0
    if full > 0 and rest >= 8 * chunks and rest * 2 <= resident:
        tg = (rest // chunks + 7) // 8
        tc = tc_first = min(resident // (tg * 8), pairs)
        while tc > chunks and epi == EPI_PLAIN and pairs % tc != 0:
            tc -= 1
        if tc > chunks:
            tail_groups, tail_chunks = tg, tc
    if full == 0:
        last = "first-round"
    elif rest == 0:
        last = "round"
    elif tail_groups:
        last = "tail"
    else:
        last = "notail"
    ppc = _cdiv(pairs, chunks)
    return dict(nw=nw, rows=rows, stripes=stripes, pairs=pairs, chunks=chunks, rule=rule, last=last, tail_groups=tail_groups,
                tail_chunks=tail_chunks, tc_first=tc_first, last_chunk_pairs=pairs - (chunks - 1) * ppc,
                idle=(groups * 8 != stripes), ragged=(M % rows != 0))


def cols_plan(M, N, K):
    """launch_cols: column blocks per workgroup (NB 8 at N % 256 == 0, else 4), 128-row stripes, 64-deep K chunks."""
    nb = 8 if N % 256 == 0 else 4
    return dict(nb=nb, stripes=_cdiv(M, 128), ktiles=K // 64, col_tiles=N // (32 * nb), ragged=(M % 128 != 0))


def wgrad_tn(N, K):
    """Tile height of wgrad2_plan: 256 when the output has at least three 256 x 256 tiles."""
    return 256 if _cdiv(N, 256) * _cdiv(K, 256) >= 3 else 128


def wgrad_nsplit(workspace_bytes, N, K):
    """The plan's split count, read back from the workspace size: bytes / (tiles x PART x 4)."""
    tn = wgrad_tn(N, K)
    tiles = _cdiv(N, tn) * _cdiv(K, 256)
    part = tn * 256 + tn
    assert workspace_bytes % (tiles * part * 4) == 0, (workspace_bytes, tiles, part)
    return workspace_bytes // (tiles * part * 4)


def wgrad_depth(M, nsplit):
    """D: the longest chain of fp32 additions a term of dW passes through."""
    return 2 * _cdiv(_cdiv(M, 32), nsplit) + nsplit // 4 + 20


# ------------------------------------------------------------------------------------------------------ input classes
def _randn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float32, device=g.device).to(F64)


def _ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g, device=g.device).to(F64)


def gemm_operands(kind, g, M, N, K, bias=True):
    """(x [M, K], w [N, K], b [N] or None) as float64 tensors holding bf16 values, on the generator's device."""
    if kind == "exact":
        x, w, b = _ints(g, -1, 1, M, K), _ints(g, -1, 1, N, K), _ints(g, -8, 8, N)
    elif kind == "coherent":
        x, w, b = _randn(g, M, K).abs(), _randn(g, N, K).abs() / K, _randn(g, N).abs()
    elif kind in ("randn", "scaled", "saturated"):
        x, w, b = _randn(g, M, K), _randn(g, N, K) * K ** -0.5, _randn(g, N)
        if kind == "scaled":
            sc = 2.0 ** -(torch.arange(N, device=g.device) % SCALE_PERIOD).to(F64)
            w, b = w * sc[:, None], b * sc
    else:
        raise ValueError(kind)
    q = lambda t: t.to(BF).to(F64)
    return q(x), q(w), (q(b) if bias else None)


SAT_VALUES = (30.0, -30.0, 100.0, -100.0)


def saturate_bias(b, interleaved=True, hreal=None):
    """Put +-30 / +-100 on some ``a`` columns of a SwiGLU bias: a-column j of every 7th unit, the four values in turn."""
    b = b.clone()
    H = b.numel() // 2 if hreal is None else hreal
    for n, j in enumerate(range(3, H, 7)):
        col = 32 * (j // 16) + j % 16 if interleaved else j
        b[col] = SAT_VALUES[n % 4]
    return b


def wgrad_operands(kind, g, M, N, K):
    """(dy [M, N], x [M, K]) as float64 tensors holding bf16 values."""
    if kind == "exact":
        assert M * 64 <= 2 ** 24
        dy, x = _ints(g, -8, 8, M, N), _ints(g, -8, 8, M, K)
    elif kind == "coherent":
        dy, x = _randn(g, M, N).abs(), _randn(g, M, K).abs()
    elif kind in ("randn", "scaled"):
        dy, x = _randn(g, M, N), _randn(g, M, K)
        if kind == "scaled":
            dy = dy * 2.0 ** -(torch.arange(N, device=g.device) % SCALE_PERIOD).to(F64)
    else:
        raise ValueError(kind)
    return dy.to(BF).to(F64), x.to(BF).to(F64)


def share(step):
    """Fraction of ambiguous elements (step > 0)."""
    return float((step > 0).to(F64).mean())


# K values of tests/test_linear_ops_gpu.py (rows kernel 128 / 256 / 512, cols kernel the others, fused MLP 128 / 256 and H = 64 / 704)
GPU_KS = (64, 128, 192, 256, 384, 512, 704, 768, 1408, 1536, 2816)


def share_limit(kind, K):
    """The ambiguous share a case of this class may have at most (None: no condition)."""
    if kind == "exact":
        return 0.0
    if kind == "coherent":
        return 0.10
    return 1.0 / 3.0 if K <= 512 else None
