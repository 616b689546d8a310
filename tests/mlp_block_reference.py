"""float64 stage references, operand classes, an fp32 / bf16 emulation and the shared check driver of the fused MLP's two BLOCK forms
(csrc/vsde_mlp.hip, ``mlp_fwd_kernel<C, 0, 0, BLK>``): ``vsde_mlp_block_fwd_bf16`` (BLK == 1) and ``vsde_mlp_attn_block_fwd_bf16``
(BLK == 2), the instantiations every no-grad sampling call runs.  tests/test_mlp_block_ops_gpu.py drives the kernels through
``check_case``, tests/test_mlp_block_bounds.py the emulation below (with injected defects that the checks must reject).

The block forms output only ``tok`` and ``hnext``; x1, h, s and y never leave the kernel.  An end-to-end float64 check with the
allowances carried through h -> u -> s -> y -> tok is sound but almost empty (measured with this module: ambiguous share of tok
23 % at C = 128, H = 64, but 55 % at (256, 128) and 80 % at (256, 704), half of those wider than one bf16 ulp).  The sharp checks
therefore come from operand classes that make ONE internal stage observable exactly.  The kernel is deterministic and its prologue
depends neither on the MLP weights nor on gm, so several launches on the same activations see the same x1 and h:

  gm0      gm = 0: tok = rnd(x1 + rnd(0 y)) = x1 bit for bit -> ``x1k``.
           BLK == 1: x1 = rnd(x + rnd(ga yin)).  The product of two bf16 values is exact in fp32; the sum is exact in fp32 wherever
           float32(x + t) == x + t: NO allowance there, 2 |x + t - float32(x + t)| elsewhere -> bit-exact, ambiguous share 0.
           BLK == 2: yin = rnd(og W_o^T + b_o), og = rnd(o rnd(sigmoid(glog[:, k % 64]))).  The gate logits are drawn by rejection so
           that no rnd(sigmoid) is ambiguous within SIGM_C: og is known exactly; yin gets the plain allowance of ``gemm64`` at K = C
           (what ``plain_ref`` rounds with) and x1k must lie in the hull over the yin candidates.
  probe    (BLK == 2) gm = 0, W_o a permutation matrix, b_o = 0: yin == og, x1 bit-exact.  Pins the k % 64 gate column, the W_o chunk
           order (2 chunks at C = 128, 4 at C = 256, the last re-using region 0) and the fragment -> row-segment transposition.
  select   an identity MLP (H >= C): C of the hidden units, unit u_j picks channel pi(j) (b-row weight 1), every a-row is 0 with bias
           32, W_out[pi(j), u_j] = 1/32, b_out = 0.  rnd(silu(32)) = 32 for any sigmoid within SIGM_C, s = 32 h exactly, y == h exactly:
           tok in hull{ rnd(x1k + rnd(gm hc)) : hc in candidates of rnd(LN(x1k)(1 + sc) + sh) } -- the prologue LayerNorm per element,
           and known data through every tile group, the per-workgroup tile rotation and both weight images.
  scm1     sc = -1: (x1 - mu) rs (1 + (-1)) + sh = sh exactly in fp32 -> the MLP input is the known bf16 vector sh[b]; real weights;
           ``mlp_s_ref`` gives s, A_y = (H + 2) ACC_C mag + |W_out| halfwidth(s), tok in the hull over the y candidates from x1k.
  full     all operands random.  tok against the end-to-end hull from x1k ONLY at C = 128, H = 64 (see the shares above: deeper shapes
           are left to the three launches before).
  hnext    in EVERY launch with a next norm: rnd(LN(tok)(1 + sn) + hs) with eps_next, teacher-forced on the kernel's OWN tok.

LayerNorm allowance (derived, not measured; U = 2^-8, ACC_C = 2^-24).  errmu = C ACC_C mean|x| bounds the error of the fp32 mean (at most
C additions of partial sums below sum|x|); d = x - mu; the variance is a sum of C non-negative terms (chain C / 8 + 3 long in the
kernel, bounded by C here), each with the relative error of d squared, and rs = rsqrt(var + eps) halves it:
    rel = (C / 2 + 4) ACC_C + errmu mean|d| / (var + eps)
    A   = |d rs (1 + sc)| (rel + RSQRT_C ACC_C) + errmu rs |1 + sc| + ACC_C |sh|
RSQRT_C = 4 covers rsqrtf and the three fp32 operations of the affine part.  ``eps`` enters as the fp32 value the host passes.

Conditions on the ambiguous share (caps, not tolerances; ``CAPS``): x1 BLK == 1 and the probe 0; select tok <= 2 %; hnext <= 5 %; x1
BLK == 2 with a real W_o, scm1 tok and the end-to-end tok <= 1/3 (``linear_reference.share_limit``).

rsqrtf and MFMA rounding.  Nobody had measured rsqrtf's error on gfx950 before these tests; RSQRT_C = 4 and ACC_C = 2^-24 are the derived
constants.  Measured on an MI355X: they held -- no element of any check of tests/test_mlp_block_ops_gpu.py left its bound (20 cases, both
entry points, lowvar rows included); of 15,928 ambiguous select elements 13 took the neighbouring value, of 142,550 ambiguous hnext
elements 137, of 25,503 ambiguous x1(W_o) elements 10.  The constants were therefore not widened.

Activation classes (``build_case``): randn; lowvar (every third row of x and yin / attn scaled by 2^-9: eps is comparable to the
variance, an eps mix-up becomes a gross error; BLK == 2 also scales b_o); scaled (columns times 2^-(n mod 12)).  Modulation vectors:
0.5 randn, another vector per batch row.  MLP weights: ``weight_class`` (randn at H <= 512, coherent at H = 704, where randn put
35 - 49 % of the scm1 tok elements over the 1/3 cap: 14 % of u is ambiguous at K = 256 and 682 such units feed every y).
"""
import torch

import linear_reference as lr
from linear_reference import ACC_C, BF, F64, SIGM_C, excess, gemm64, gemm_operands, mlp_s_ref, share, swiglu_s_ref

F32 = torch.float32
STRIPE, WAVE_ROWS, MODB, MIN_TOKENS = 256, 32, 4, 86   # csrc/vsde_mlp.hip: NW * 32 rows per workgroup, MODB batch rows per stripe
EPS, EPS_NEXT = 1e-5, 1e-3
RSQRT_C = 4.0
VECS = ("ga", "sc", "sh", "gm", "sn", "hs")            # the order of the kernel's LDS table [MODB][6][C]
CAPS = {"x1": 0.0, "x1(W_o)": 1.0 / 3.0, "probe": 0.0, "select": 0.02, "hnext": 0.05, "scm1": 1.0 / 3.0, "e2e": 1.0 / 3.0}
E2E_SHAPE = (128, 64)                                   # the only (C, H) at which the end-to-end hull of tok means something

# (B, N): the smallest shapes at which each piece of row / batch-row bookkeeping has its edge
#   (3, 86)  M = 258: a second stripe of two rows -- seven of its eight waves lie wholly past M, the M - 1 clamp is live
#   (7, 86)  M = 602: stripe 1 = rows 256..511 = batch rows 2, 3, 4, 5: all four MODB slots at the minimum sequence length; blast clamp in stripe 2
#   (3, 256) M = 768: whole stripes, stripe = batch row;  (2, 401) M = 802: the LV token count;  (5, 101) M = 505
# per case: (B, N, C, H, hreal, activation class, last block, (H, hreal) of the select launch)
_ROWS = [((3, 86), (64, 64), "randn", False), ((7, 86), (128, 100), "lowvar", False), ((3, 256), (704, 682), "scaled", True),
         ((2, 401), (704, 682), "randn", False), ((5, 101), (128, 100), "lowvar", True)]
CASES = [(B, N, C, H, hreal, kind, last, (704, 682) if (C == 256 and i in (1, 2)) else (C, C))
         for C in (128, 256) for i, ((B, N), (H, hreal), kind, last) in enumerate(_ROWS)]


def weight_class(H):
    """Class of the real MLP weights (linear_reference.gemm_operands): randn up to the depth at which its allowance still means
    something (share_limit: K <= 512), coherent beyond -- there the scm1 launch also takes |sh|, so that u, s and y are coherent sums."""
    return "randn" if H <= 512 else "coherent"


def case_id(blk, case):
    B, N, C, H, hreal, kind, last, sel = case
    return f"blk{blk}-{B}x{N}x{C}-H{H}({hreal})-{kind}-{'last' if last else 'next'}-sel{sel[0]}"


def q(t):
    """Round to bf16, back in float64."""
    return t.to(BF).to(F64)


def f32_value(v):
    return float(torch.tensor(v, dtype=F32))


def row_map(M, N):
    """(stripe, wave, batch row, slot) of every row m: slot = batch row - first batch row of the stripe (``brow`` in the kernel)."""
    m = torch.arange(M)
    stripe, b = m // STRIPE, m // N
    return stripe, (m % STRIPE) // WAVE_ROWS, b, b - (stripe * STRIPE) // N


# ---------------------------------------------------------------------------------------------------------- references
def residual_hull(x, g, ycands):
    """(lo, hi, nominal) of rnd(x + rnd(g y)) over the candidates y (the first one is the nominal value of y); x, g, y bf16 values."""
    lo = hi = nom = None
    for y in ycands:
        # mirrors t = pack2(bf_lo(gv) * bf_lo(yv), ..): the fp32 product of two bf16 values is exact, one rounding
        t = q(g * y)
        # mirrors x1 = pack2(bf_lo(xv) + bf_lo(t), ..): one fp32 addition (exact wherever float32(x + t) == x + t), one rounding
        s = x + t
        A = 2.0 * (s - s.to(F32).to(F64)).abs()
        a, b = q(s - A), q(s + A)
        if nom is None:
            nom = q(s)
        lo = a if lo is None else torch.minimum(lo, a)
        hi = b if hi is None else torch.maximum(hi, b)
    return lo, hi, nom


def ln_ref(x, sc, sh, eps):
    """(h64, A) of LN(x)(1 + sc) + sh before its rounding, for x [m, C] of bf16 values and per-row sc, sh [m, C]."""
    C = x.shape[1]
    eps = f32_value(eps)
    # mirrors mu = t * (1.0f / C) after the three xor_lane steps; qq = sum (x1 - mu)^2; rs = rsqrtf(qq * (1.0f / C) + p.eps)
    mu = x.mean(1, keepdim=True)
    d = x - mu
    var = (d * d).mean(1, keepdim=True)
    rs = (var + eps).rsqrt()
    errmu = C * ACC_C * x.abs().mean(1, keepdim=True)
    rel = (C / 2 + 4) * ACC_C + errmu * d.abs().mean(1, keepdim=True) / (var + eps)
    # mirrors pack2((bf_lo(x1) - mu) * rs * (1.0f + bf_lo(cv)) + bf_lo(hv), ..)
    core = d * rs * (1.0 + sc)
    A = core.abs() * (rel + RSQRT_C * ACC_C) + errmu * rs * (1.0 + sc).abs() + ACC_C * sh.abs()
    return core + sh, A


def candidates(v, A):
    """(nominal, low, high) bf16 candidates of a value known up to A."""
    return q(v), q(v - A), q(v + A)


def sigmoid_ambiguous(gl):
    s = torch.sigmoid(gl)
    return q(s * (1.0 - SIGM_C)) != q(s * (1.0 + SIGM_C))


def gated_o(o, glog):
    """og = rnd(o rnd(sigmoid(glog[:, k % 64]))), exact for logits that passed the rejection."""
    assert not bool(sigmoid_ambiguous(glog).any())
    # mirrors sg = pack2(sigm(bf_lo(gl)), ..) and xfr[ks] = pack2(bf_lo(a) * bf_lo(g), ..) with g = sg[ks & 3]: column k takes gate k % 64
    sg = q(torch.sigmoid(glog))
    return q(o * sg.repeat(1, o.shape[1] // 64))


def y_from_s(s_mid, s_half, w_out, b_out, H):
    """(nominal, low, high) candidates of y = rnd(s W_out^T + b_out) for s in [s_mid - s_half, s_mid + s_half]; H: the padded depth."""
    # mirrors gemm2 (H / 16 k-steps into yacc) and the epilogue's pack2(a + bf_lo(bb.x), ..)
    w = w_out.to(F64)
    y = s_mid @ w.t() + b_out
    spread = s_half @ w.abs().t()
    mag = s_mid.abs() @ w.abs().t() + spread + b_out.abs()
    return candidates(y, (H + 2) * ACC_C * mag + spread)


def s_from_h(h_mid, h_half, w_in, b_in, hreal):
    """(mid, half) of s for the MLP input h in [h_mid - h_half, h_mid + h_half] (h_half may be None: h exact)."""
    if h_half is None:
        return mlp_s_ref(h_mid, w_in, b_in, hreal)
    w = w_in.to(F64)
    u = h_mid @ w.t() + b_in
    spread = h_half @ w.abs().t()
    A = (h_mid.shape[1] + 2) * ACC_C * (h_mid.abs() @ w.abs().t() + spread + b_in.abs()) + spread
    return swiglu_s_ref(u[:, :hreal], A[:, :hreal], u[:, hreal:], A[:, hreal:])


# ------------------------------------------------------------------------------------------------------ operand classes
def _randn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=F32, device=g.device).to(F64)


def gate_logits(g, M, scale=2.0):
    """bf16 gate logits [M, 64] none of whose rnd(sigmoid) is ambiguous within SIGM_C (drawn by rejection)."""
    gl = q(scale * _randn(g, M, 64))
    for _ in range(64):
        bad = sigmoid_ambiguous(gl)
        if not bool(bad.any()):
            return gl
        gl = torch.where(bad, q(scale * _randn(g, M, 64)), gl)
    raise AssertionError("gate logits: rejection did not converge")


def mlp_weights(kind, g, C, hreal):
    """(w_in [2 hreal, C] = [a rows | b rows], b_in, w_out [C, hreal], b_out) of class ``kind`` (linear_reference.gemm_operands)."""
    _, w_in, b_in = gemm_operands(kind, g, 1, 2 * hreal, C)
    _, w_out, b_out = gemm_operands(kind, g, 1, C, hreal)
    return w_in, b_in, w_out, b_out


def select_weights(g, C, hreal):
    """The identity MLP of the ``select`` launch: y == h exactly (see the module docstring)."""
    assert hreal >= C
    dev = g.device
    units = torch.randperm(hreal, generator=g, device=dev)[:C]
    pi = torch.randperm(C, generator=g, device=dev)
    w_in = torch.zeros(2 * hreal, C, dtype=F64, device=dev)
    b_in = torch.zeros(2 * hreal, dtype=F64, device=dev)
    b_in[:hreal] = 32.0
    w_in[hreal + units, pi] = 1.0
    w_out = torch.zeros(C, hreal, dtype=F64, device=dev)
    w_out[pi, units] = 1.0 / 32.0
    return w_in, b_in, w_out, torch.zeros(C, dtype=F64, device=dev)


def build_case(blk, case, seed, device="cpu", wkind=None):
    """All operands of one case as float64 tensors holding bf16 values, and its launches.  A launch is a dict
    {mods: {name: [B, C] or None}, mlp: (w_in, b_in, w_out, b_out, H, hreal), wo, bo} -- what changes between launches."""
    B, N, C, H, hreal, kind, last, (Hs, hs_real) = case
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    M = B * N
    x, y = _randn(g, M, C), _randn(g, M, C)
    if kind == "lowvar":
        x[::3] *= 2.0 ** -9
        y[::3] *= 2.0 ** -9
    elif kind == "scaled":
        col = 2.0 ** -(torch.arange(C, device=device) % lr.SCALE_PERIOD).to(F64)
        x, y = x * col, y * col
    else:
        assert kind == "randn", kind
    ops = dict(blk=blk, B=B, N=N, C=C, M=M, last=last, eps=EPS, eps_next=EPS_NEXT, x=q(x), y=q(y), kind=kind)
    mods = {name: q(0.5 * _randn(g, B, C)) for name in VECS}
    if last:
        mods["sn"] = mods["hs"] = None
    wo = bo = wperm = None
    if blk == 2:
        ops["glog"] = gate_logits(g, M)
        wo, bo = q(_randn(g, C, C) * C ** -0.5), q(0.1 * _randn(g, C) * (2.0 ** -9 if kind == "lowvar" else 1.0))
        wperm = torch.zeros(C, C, dtype=F64, device=device)
        wperm[torch.arange(C, device=device), torch.randperm(C, generator=g, device=device)] = 1.0
    wkind = wkind or weight_class(H)
    real = mlp_weights(wkind, g, C, hreal) + (H, hreal)
    sel = select_weights(g, C, hs_real) + (Hs, hs_real)
    zero = torch.zeros(B, C, dtype=F64, device=device)
    launches = {
        "gm0": dict(mods={**mods, "gm": zero}, mlp=real, wo=wo, bo=bo),
        "select": dict(mods=mods, mlp=sel, wo=wo, bo=bo),
        "scm1": dict(mods={**mods, "sc": zero - 1.0, "sh": (mods["sh"].abs() if wkind == "coherent" else mods["sh"])}, mlp=real, wo=wo, bo=bo),
        "full": dict(mods=mods, mlp=real, wo=wo, bo=bo),
    }
    if blk == 2:
        launches["probe"] = dict(mods={**mods, "gm": zero}, mlp=real, wo=wperm, bo=torch.zeros(C, dtype=F64, device=device))
    ops["launches"] = launches
    return ops


# ---------------------------------------------------------------------------------------------------------- emulation
def _bf(t):
    return t.to(BF).float()


def _acc(x, w, order=None):
    """fp32 accumulation in 16-deep k-steps as the MFMA loops take them; ``order``: the sequence of k-steps."""
    ks = x.shape[1] // 16
    parts = x.reshape(x.shape[0], ks, 16).permute(1, 0, 2).contiguous() @ w.reshape(w.shape[0], ks, 16).permute(1, 2, 0).contiguous()
    acc = torch.zeros(x.shape[0], w.shape[0])
    for k in (range(ks) if order is None else order):
        acc = acc + parts[k]
    return acc


DEFECTS = ("ga_next_row", "eps_swapped", "sn_hs_swapped", "stats_unrounded", "gy_unrounded", "mean_lane_step", "slot3_alias",
           "tile_group_twice", "gate_col_mod32", "bo_dropped", "wo_chunk3_from_0", "x1_from_parked_tok")


def emulate(ops, launch, defect=None):
    """(tok, hnext) as bf16 tensors: the arithmetic of mlp_fwd_kernel<C, 0, 0, BLK> in fp32 with bf16 roundings exactly where the
    kernel packs.  ``defect``: one of DEFECTS (tests/test_mlp_block_bounds.py names the check that rejects each)."""
    assert defect is None or defect in DEFECTS, defect
    blk, N, C, M = ops["blk"], ops["N"], ops["C"], ops["M"]
    stripe, _, b, slot = row_map(M, N)
    eps, eps_next = f32_value(ops["eps"]), f32_value(ops["eps_next"])
    if defect == "eps_swapped":
        eps, eps_next = eps_next, eps
    bsrc = b.clone()
    if defect == "slot3_alias":                        # LDS table entry of slot 3 never filled: it reads slot 2's vectors
        bsrc = torch.where(slot == 3, b - 1, b)
    vec = {k: (None if v is None else v.float()[bsrc]) for k, v in launch["mods"].items()}
    if defect == "sn_hs_swapped" and vec["sn"] is not None:
        vec["sn"], vec["hs"] = vec["hs"], vec["sn"]
    ga = vec["ga"]
    if defect == "ga_next_row":                        # brow of a stripe's last row taken from the row after it
        last_rows = (torch.arange(M) % STRIPE == STRIPE - 1)
        bn = torch.clamp(b + 1, max=ops["B"] - 1)
        ga = torch.where(last_rows[:, None], launch["mods"]["ga"].float()[bn], ga)
    x = ops["x"].float()
    if blk == 2:
        # mirrors the BLK == 2 prologue: sg = pack2(sigm(..)); og = pack2(o * g); gemm0_chunk over W_o's k-steps; yin = pack2(acc + b_o)
        sg = _bf(torch.sigmoid(ops["glog"].float()))
        gate = sg[:, :32].repeat(1, C // 32) if defect == "gate_col_mod32" else sg.repeat(1, C // 64)
        og = _bf(ops["y"].float() * gate)
        wo = launch["wo"].float()
        if defect == "wo_chunk3_from_0" and C == 256:  # the chunk that re-uses region 0 is multiplied before it landed
            wo = wo.clone()
            wo[:, 192:256] = wo[:, 0:64]
        yin = _acc(og, wo)
        yin = _bf(yin if defect == "bo_dropped" else yin + launch["bo"].float())
    else:
        yin = ops["y"].float()
    # mirrors t = pack2(ga * yin); x1 = pack2(x + t)
    raw = x + ga * yin if defect == "gy_unrounded" else x + _bf(ga * yin)
    x1 = _bf(raw)

    def ln(v, sc, sh, e, stats=None, lane_step=False):
        # mirrors the row statistics (fp32 sums over the lane's chunks and the 8 lanes of a row) and the modulated affine part
        sv = v if stats is None else stats
        if lane_step:   # xor_lane<4> missing: a lane only sees the sum over its own half of the 8 lanes of a row
            lanes = (torch.arange(C) // 8) % 8 // 4
            part = torch.stack([(sv * (lanes == k)).sum(1) for k in (0, 1)], 1)
            mu = part[:, lanes] * (1.0 / C)
        else:
            mu = sv.sum(1, keepdim=True) * (1.0 / C)
        dd = sv - mu
        rs = torch.rsqrt((dd * dd).sum(1, keepdim=True) * (1.0 / C) + e)
        return _bf((v - mu) * rs * (1.0 + sc) + sh)

    h = ln(x1, vec["sc"], vec["sh"], eps, stats=(raw if defect == "stats_unrounded" else None), lane_step=(defect == "mean_lane_step"))
    w_in, b_in, w_out, b_out, H, hreal = launch["mlp"]
    # mirrors gemm1 (bias, then C / 16 k-steps), swiglu8 (pack2 of u, of silu, of the product), gemm2 (one k-step per tile, tiles
    # in the order rotated per workgroup: rot = 4 ((blockIdx * 5) % (T / 4))) and the epilogue's pack2(acc + b_out)
    u = _bf(_acc(h, w_in.float()) + b_in.float())
    a, bb = u[:, :hreal], u[:, hreal:]
    s = torch.zeros(M, H)
    s[:, :hreal] = _bf(_bf(a * torch.sigmoid(a)) * bb)
    w2 = torch.zeros(C, H)
    w2[:, :hreal] = w_out.float()
    T = H // 16
    yv = torch.empty(M, C)
    for st in range((M + STRIPE - 1) // STRIPE):
        rot = 4 * ((st * 5) % (T // 4))
        order = [(t + rot) % T for t in range(T)]
        if defect == "tile_group_twice" and rot:       # under rotation group 1 is visited twice, group 0 not at all
            order = [t + 4 if t < 4 else t for t in order]
        rows = slice(st * STRIPE, min(M, (st + 1) * STRIPE))
        yv[rows] = _bf(_acc(s[rows], w2, order) + b_out.float())
    x1e = x1
    if defect == "x1_from_parked_tok" and blk == 2:    # the epilogue treats the parked x1 as x and applies the gated residual again
        x1e = _bf(x1 + _bf(ga * yin))
    # mirrors gm = pack2(mv * ml); t = pack2(x1 + gm) and the next block's LayerNorm with eps_next
    tok = _bf(x1e + _bf(vec["gm"] * yv))
    hnext = None if vec["sn"] is None else ln(tok, vec["sn"], vec["hs"], eps_next)
    return tok.to(BF), (None if hnext is None else hnext.to(BF))


# ------------------------------------------------------------------------------------------------------- check driver
class Check:
    """Outcome of one check: elements, out of bound, worst |err| / bound, ambiguous share, ambiguous elements off the nominal value."""

    def __init__(self, name, got, lo, hi, nominal, N):
        mid, half = (lo + hi) / 2, (hi - lo) / 2
        self.name, self.n = name, got.numel()
        self.nbad, self.worst, self.first = excess(got, mid, half)
        self.share = share(half)
        amb = half > 0
        self.ambiguous = int(amb.sum())
        self.moved = int((amb & (got.to(F64) != nominal)).sum())
        self.where = ""
        if self.first is not None:
            m = self.first[0]
            stripe, wave, b, slot = (int(t[m]) for t in row_map(got.shape[0], N))
            self.where = f" first bad [{m}, {self.first[1]}]: stripe {stripe}, wave {wave}, batch row {b} = slot {slot}"

    def __str__(self):
        return (f"{self.name}: {self.nbad} of {self.n} out of bound, worst err/bound {self.worst:.3g}, ambiguous {self.ambiguous} "
                f"({self.share:.4f}), {self.moved} of them off the nominal value{self.where}")


def cap_of(name):
    return CAPS[name.split(".")[-1] if not name.startswith("hnext") else "hnext"]


def check_case(ops, run, out=print, key=""):
    """Run every launch of a case through ``run(ops, launch) -> (tok, hnext)`` and check it: {check name: Check}.  The checks use
    the kernel's own x1 (gm0 launch) and, for hnext, its own tok: each one isolates a single stage."""
    blk, N, C, M = ops["blk"], ops["N"], ops["C"], ops["M"]
    _, _, b, _ = row_map(M, N)
    b = b.to(ops["x"].device)
    res, L = {}, ops["launches"]
    rows = lambda v: v[b]

    def note(name, got, lo, hi, nominal):
        res[name] = c = Check(name, got, lo, hi, nominal, N)
        out(f"BLOCKCHECK {key} {c}")

    def hnext_check(name, launch, tok, hn):
        mods = launch["mods"]
        assert (hn is None) == (mods["sn"] is None), f"{key} {name}: hnext returned / missing against sn"
        if hn is None:
            return
        hv, A = ln_ref(tok.to(F64), rows(mods["sn"]), rows(mods["hs"]), ops["eps_next"])
        nom, lo, hi = candidates(hv, A)
        note(f"hnext.{name}", hn, lo, hi, nom)

    def x1_hull(launch):
        ga = rows(launch["mods"]["ga"])
        if blk == 1:
            return residual_hull(ops["x"], ga, [ops["y"]])
        # yin = rnd(og W_o^T + b_o) with the plain allowance at K = C: its float64 rounding and, where ambiguous, the neighbour
        return residual_hull(ops["x"], ga, candidates(*gemm64(gated_o(ops["y"], ops["glog"]), launch["wo"], launch["bo"])))

    # gm0: x1 observed
    tok, hn = run(ops, L["gm0"])
    note("x1" if blk == 1 else "x1(W_o)", tok, *x1_hull(L["gm0"]))
    hnext_check("gm0", L["gm0"], tok, hn)
    x1k = tok.to(F64)
    if blk == 2:
        tok, hn = run(ops, L["probe"])
        note("probe", tok, *x1_hull(L["probe"]))
        hnext_check("probe", L["probe"], tok, hn)

    def tok_hull(launch, ycands):
        return residual_hull(x1k, rows(launch["mods"]["gm"]), ycands)

    def h_cands(launch):
        mods = launch["mods"]
        return candidates(*ln_ref(x1k, rows(mods["sc"]), rows(mods["sh"]), ops["eps"]))

    # select: h observed through the identity MLP
    tok, hn = run(ops, L["select"])
    note("select", tok, *tok_hull(L["select"], h_cands(L["select"])))
    hnext_check("select", L["select"], tok, hn)
    # sc = -1: the MLP input is sh[b] exactly
    la = L["scm1"]
    w_in, b_in, w_out, b_out, H, hreal = la["mlp"]
    tok, hn = run(ops, la)
    s_mid, s_half = s_from_h(la["mods"]["sh"], None, w_in, b_in, hreal)          # one MLP input per batch row
    note("scm1", tok, *tok_hull(la, [rows(v) for v in y_from_s(s_mid, s_half, w_out, b_out, H)]))
    hnext_check("scm1", la, tok, hn)
    # full: everything random
    la = L["full"]
    tok, hn = run(ops, la)
    hnext_check("full", la, tok, hn)
    if (C, H) == E2E_SHAPE:
        _, hlo, hhi = h_cands(la)
        s_mid, s_half = s_from_h((hlo + hhi) / 2, (hhi - hlo) / 2, w_in, b_in, hreal)
        note("e2e", tok, *tok_hull(la, y_from_s(s_mid, s_half, w_out, b_out, H)))
    else:
        assert bool(torch.isfinite(tok.float()).all()), f"{key} full: tok not finite"
    return res


def assert_case(res, key=""):
    """Zero elements out of bound and every share within its cap."""
    bad = [str(c) for c in res.values() if c.nbad]
    assert not bad, f"{key}: " + " | ".join(bad)
    over = [f"{c.name} share {c.share:.4f} > {cap_of(c.name):.4f}" for c in res.values() if c.share > cap_of(c.name)]
    assert not over, f"{key}: " + " | ".join(over)
