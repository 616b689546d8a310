"""float64 references, per-element error bounds, an fp32 emulation (with injectable defects) and the dispatch mirror of the recurrent
kernels of the fused head: the GRU path sampler's time loop and its reverse-time sweep (csrc/vsde_head.hip, csrc/vsde_head_mp.hip).
Plain numpy: tests/test_head_step_ops_gpu.py scores the kernels with it, tests/test_head_step_bounds.py checks on the CPU that a
correct fp32 implementation stays inside every bound and that each injected defect leaves it.

Forward: one step, teacher-forced per layer (``forward_ref``)
  Every input of step t is the KERNEL's own: z_t = paths[:, t], h^l_{t-1} = acts[:, t-1, l, 0] (zero at t = 0), the input of layer l > 0
  is acts[:, t, l-1, 0], the emission reads acts[:, t, L-1, 0], layer 0's context term is the kernel's projected record G
  (``_hip.debug_head_context_projection``: vsde_head.hip:2116-2128 calls ``context_projection`` (:1613-1633), the function
  ``vsde_head_forward`` calls at :1726 with the same dims, view and weights -- the same kernel on the same operands; its ``save``
  argument only switches the profiling marks).  Inside one GRU cell the float64 values are chained (r and c_n enter n, u and n enter h)
  and their bounds are propagated, so a bound never relies on which of its registers a kernel stored.
  Returned per quantity: (float64 value, bound), for acts (h, r, u, n, c_n), means, chol_raw, chol and z_{t+1}.  Bit-for-bit
  identities that need no bound (``chol_identities``): diag(chol) == max(chol_raw diag, float32(diag_min)) (vsde_head.hip:275, :828, :859,
  :1377; vsde_head_mp.hip emission block), strict upper triangle of chol == 0 (:288-292, :686/:830, :881-883, :1391-1394).

  U = 2^-24 (fp32 unit round-off; every fp32 accumulation, VALU fma chain or MFMA, is taken as no worse than round-to-nearest term by
  term, the assumption tests/linear_reference.py measured).  A dot product of n terms, summed in ANY order, is off by at most
  (n - 1) U sum |w x| to first order; the kernels' orders differ (v1: one fma chain over 4-float chunks, vsde_head.hip:123-130, :251-268;
  v2: 16-term chains per quad lane then two DPP adds, :783-820, :497-501; wide: one chain over H, :1342-1353, :1371-1372; multi-path:
  two 32-deep MFMA steps, vsde_head_mp.hip:146-160), so the depth used is the full reduction length n plus SLACK = 8 roundings for what
  rides on the sum in one kernel or another: the exp2-domain pre-scaling of each weight / bias / record by -log2(e) or 2 log2(e)
  (vsde_head.hip:580-593, :614-623, :681; vsde_head_mp.hip:87-92) and of c_n back by 1 / (2 log2 e) (:767, vsde_head_mp.hip:283), the
  constants' own rounding, the add of the two halves a + c, the fold of the second accumulator (vsde_head_mp.hip:181).
    layer 0   a = G + theta W_theta^T + z_t W_z^T           n_a = 1 + P + S        c = b_hh + h_{t-1} W_hh^T     n_c = H + 1
    layer l   a = b_ih + h^{l-1}_t W_ih^T                    n_a = H + 1
    d(a + c) = (n_a + n_c + SLACK) U (mag_a + mag_c) [+ split]        d c_n = (n_c + SLACK) U mag_c [+ split]
    r, u      sigmoid: d = d(a + c) / 4 + E_sig                  (Lipschitz 1/4)
    n         x = a_n + r c_n: dx = d a_n + r d c_n + |c_n| dr + dr d c_n + 3 U (mag_a + r mag_c);  dn = dx + E_tanh   (Lipschitz 1)
    h         (1 - u) n + u h_{t-1}: dh = |h_{t-1} - n| du + (1 - u) dn + du dn + 4 U (|n| + |h_{t-1}|)
              (4 U (|n| + |h|) covers both forms: (1 - u) n + u h, :235/:1361, and fma(u, h - n, n), :758, vsde_head_mp.hip:295)
    emission  o = b_o + h^{L-1}_t W_o^T: (H + 1 + SLACK) U mag_o [+ split]; chol: the entry's own bound (max(., m) is 1-Lipschitz)
    z_{t+1}   z + mu dt + sqdt sum_j L_ij eps_j with dt, sqdt the kernel's float32 values (:1735): dt d mu + sqdt sum_j |eps_j| d L_ij +
              (S + 6) U (|z| + |mu dt| + sqdt sum |L eps|)
  every bound + FLOOR = 2^-120 (flushed fp32 denormals).

  Activations (vsde_common.h:91-94): sigmoid(x) = rcp(1 + exp2(-log2e x)), tanh(x) = 1 - 2 rcp(1 + exp2(2 log2e x)).  v_exp_f32 and
  v_rcp_f32 are specified to 1 ulp ("AMD Instruction Set Architecture, CDNA3 / CDNA4", VOP1 opcodes V_EXP_F32, V_RCP_F32: "1ULP
  accuracy"; vsde_common.h:90 relies on the same figure), i.e. a relative error of at most 2^-23.  With s = sigmoid(x), e = exp(-x),
  y = fl(c x): |dy| <= 2 U |y| (the constant and the product), e's relative error <= 2^-23 + ln2 |dy| = 2^-23 (1 + |x|), the add 1 + e
  costs U, rcp 2^-23, and d log s = (1 - s) d log e + ...:
      E_sig(x)  = 2^-23 s ((1 - s)(1 + |x|) + 1.5)                      (<= 2 * 2^-23 everywhere)
      E_tanh(x) = 2 E_sig(-2 x) + U |tanh x|                             (q = sigmoid(-2x), tanh = 1 - 2 q, the subtraction rounds once)
  Checked on the CPU against numpy float64 for the same formula in float32 (tests/test_head_step_bounds.py).

  f16 split of the multi-path kernels (vsde_head_mp.hip:44-66): x = hi + lo' / 2048, hi = f16(x), lo' = f16((x - hi) 2048).
  |x - hi| <= 2^-11 |x|, the rounding of lo' leaves <= 2^-22 |x|.  A value whose hi would be an f16 subnormal goes to lo' alone
  (mp_split: the compare at :53; mp_split_fast under the flushed denormal mode, :57-66), and a lo' below 2^-14 is itself flushed, so an
  operand is off by at most 2^-22 |x| + 2^-25 (2^-25 = 2^-14 / 2048: the smallest normal lo').  A product keeps hi hi + (hi lo' + lo' hi) /
  2048 and drops lo lo (:132-160, :181):
      split = sum_k 3 * 2^-22 |w_k x_k| + 2^-25 (|w_k| + |x_k|)
  (3 = the two operand remainders and the dropped term; in the exp2 domain w is 1.44 or 2.89 times larger and the result is divided by
  that again, which only shrinks the |x_k| part).  It applies to every H-long product of those kernels: W_hh h, W_ih h, W_o h; the
  state and theta terms are fp32 VALU (:26).

Backward: the reverse-time sweep on the kernel's saved tensors (``sweep_ref``)
  backward.py:208-624 as vsde_head.hip:367-476 / oracle/vsde_oracle_impl.h:184-264 state it, in float64, from the kernel's chol_raw and
  acts, the upstream gradients and the weights: D4 [B, T, L, 4, H], DO [B, T, NO], grad_x0 [B, S], grad_theta [B, P].  The clamp
  pass-through (keep dL on a diagonal iff raw >= diag_min or dL < 0) reads the kernel's saved chol_raw; where the SIGN of dL differs
  between float64 and the kernel (one keeps dL, the other writes zero), the error is |dL| of the one that kept it, which is below the
  UNMASKED bound b of dL.  So on a diagonal below the floor whose float64 |dL| <= b the sign is ambiguous and b is added as an
  absolute error source (track F below) to that element and, carried on, to everything downstream; on every other diagonal the
  kernel must take the float64 branch and a zeroed element's bound is FLOOR.  No element is excluded.
  Given the saved tensors the sweep is linear in the upstream gradients.  The same recurrence is run again on absolute values --
  |upstream|, |W|, |eps| and the gate-derivative coefficients, with (1 - n^2) replaced by 1 = |1 - n^2| + n^2, the magnitude its
  rounding error is relative to (fl(n n) is rounded before the subtraction; every other coefficient is a product of single roundings of
  exact fp32 inputs) -- which gives a per-element magnitude M that includes the carry through time.  An element of step t has passed
  through T - t steps; one step's longest chain of roundings is
      D_STEP = (NO + 4) + L (3 H + C_COEF + 2) + (S + 4)
  (the chain d z_{t+1} -> dO: 4 (:372, :382-385); out_proj^T dO: NO (:392); per layer the add d = dcur + dh, the C_COEF = 10 roundings of
  the coefficient products of dr_pre (:403-409) and a 3 H-term product: W_ih^T pi down to the next layer (:418-438), at layer 0 the state
  columns' 3 H products with their wave / LDS sum into d z_t (:447-462, S + 4); the chain through W_hh^T ph + carry (3 H + 1, :418-445)
  is the shorter one).  grad_theta adds T (the sum over t of pi_0, :447, :469-476) + 3 H + 2.
      bound(t) = M(t) n (1 + n) ,  n = (T - t) (D_STEP U [+ N_SPLIT 3 * 2^-22])  +  F(t)  +  FLOOR
  multi-path sweep (head_bwd_mp_kernel / head_bwd_mps_kernel, vsde_head_mp.hip:637-649, :683-707, :765-833): every product of a step is a
  split product, N_SPLIT = 2 L + 2 stages per step (out_proj^T, W_hh^T and W_ih^T per layer, W_z^T); the sweep runs on g / Sg with
  Sg = 2^(1 + exponent of max |g|) (:569-573, :669-673) so the operands' absolute floor is 2^-25 Sg; F is that floor, 2^-25 sum_k (Sg
  |w_k| + |d_k|) at every product, carried through the same absolute recurrence, plus the clamp's ambiguity sources above (the only
  part of F the fp32 kernels have).

Dispatch mirror (``route_forward`` / ``route_backward``), copied from vsde_head_forward (vsde_head.hip:1737-1807) and vsde_head_backward
(:1981-2108): the generic test H > kHP || NO > kWave (:1737, :1991); use_mp / mp_auto (:1565-1581: hidden 64, L <= 2, S <= 2, from 32
paths on, hook 0 = never, > 0 = always), group size (vsde_head_mp.hip:1388 and :1410-1413: 2 / 4 spread with one unit per lane, 8 / 16
side by side); use_mp_bwd (:1586-1594, L == 2 only) and launch_head_bwd_mp's choice (vsde_head_mp.hip:1292-1331: groups of 2 / 4 the
spread sweep, 8 (and 16 -> 8) head_bwd_mp_kernel); v2 forward CH / MODE (:1762-1779, ``fwd_v2_lds`` :512-526); v2 backward: wide variant
(:1997-2022), SM variant (:2027-2061), fallback (:2065-2091) with ``bwd_v2_lds`` (:934-947), kMaxSRegV2 = 4 (:118); v1 with ``pick_wpb``
(:1596-1602, :1794-1805, :2096-2107).  ``FORWARD_KERNELS`` / ``BACKWARD_KERNELS`` list every instantiation a launch can reach at
H <= 64 / S <= 9 or beyond (found by sweeping the mirror over all dims, asserted by the CPU test):
  forward   head_fwd_kernel<L, SAVE> L = 1..4 (L <= 2 only through debug_force_v1)                                        :1800-1805
            head_fwd_v2_kernel<L, SAVE, 16, MODE> L = 1, 2, MODE = 1..4; <2, true, 8, 4> (S >= 5 at H = 64: 80 KB exceeded)   :1781-1787
            head_fwd_wide_kernel<SAVE>                                                                                    :1740-1741
            head_fwd_mp_kernel<L, SAVE, S, NP, UPL> L, S = 1, 2, (NP, UPL) = (2, 1), (4, 1), (8, 4), (16, 4)              mp:1410-1422
  backward  head_bwd_kernel<L> L = 1..4                                                                                   :2102-2107
            head_bwd_wide_kernel                                                                                           :1994
            head_bwd_v2_kernel<L, CH, 0, true, true>  (L, CH) = (1, 16), (1, 10), (2, 16), (2, 10), (2, 8)                    :2013
            head_bwd_v2_kernel<L, CH, SM, true>       SM = 1, 2, 0 at (L, CH) = (1, 16), (2, 16), (2, 10); <2, 8, 0, true>    :2046
            head_bwd_v2_kernel<L, CH, 0, false>       H % 4 != 0: (L, CH) = (1, 16), (2, 16), (2, 15)                     :2074
            head_bwd_mps_kernel<S, NP> S = 1, 2, NP = 2, 4; head_bwd_mp_kernel<S, 8>                                 mp:1304-1331
"""
import math

import numpy as np

F8, F4, F2 = np.float64, np.float32, np.float16
U = 2.0 ** -24
SLACK = 8
FLOOR = 2.0 ** -120
ULP_T = 2.0 ** -23          # v_exp_f32 / v_rcp_f32: 1 ulp
C_COEF = 10
C_SPLIT = 3 * 2.0 ** -22
C_SUB = 2.0 ** -25
LOG2E = 1.4426950408889634
DIAG_MIN = 1e-2
K_HP, K_WAVE, K_MAX_SREG_V2 = 64, 64, 4


def n_out(S):
    return S + S * (S + 1) // 2


def _f8(a):
    return np.asarray(a, F8)


# ----------------------------------------------------------------------------------------------------------- activations
def sig64(x):
    return 1.0 / (1.0 + np.exp(-x))


def e_sig(x):
    s = sig64(x)
    return ULP_T * s * ((1.0 - s) * (1.0 + np.abs(x)) + 1.5)


def e_tanh(x):
    return 2.0 * e_sig(-2.0 * x) + U * np.abs(np.tanh(x))


def sigmoid32(x):
    """vsde_common.h:93 in float32 (numpy's exp2 / division stand in for v_exp_f32 / v_rcp_f32)."""
    x = np.asarray(x, F4)
    with np.errstate(over="ignore"):
        return (F4(1) / (F4(1) + np.exp2(F4(-LOG2E) * x))).astype(F4)


def tanh32(x):
    x = np.asarray(x, F4)
    with np.errstate(over="ignore"):
        return (F4(1) - F4(2) * (F4(1) / (F4(1) + np.exp2(F4(2 * LOG2E) * x)))).astype(F4)


# ------------------------------------------------------------------------------------------------------------- forward
def _dot(x, W):
    """(x W^T, |x| |W|^T, split allowance) for x [..., K], W [N, K] in float64."""
    ax, aw = np.abs(x), np.abs(W)
    mag = ax @ aw.T
    split = C_SPLIT * mag + C_SUB * (aw.sum(1) + ax.sum(-1, keepdims=True))
    return x @ W.T, mag, split


def forward_ref(ws, theta, eps, G, paths, acts, dt, mp=False, diag_min=DIAG_MIN):
    """dict name -> (float64 value, bound) of every output of the forward time loop, step by step on the kernel's own history.
    ws: the ten weights (nn.GRU layout), G [B, T, 3H] the kernel's projected record, paths [B, T+1, S], acts [B, T, L, 5, H]."""
    W = [_f8(a) for a in ws]
    theta, eps, G, paths, acts = _f8(theta), _f8(eps), _f8(G), _f8(paths), _f8(acts)
    B, T, L, _, H = acts.shape
    S, P = paths.shape[2], theta.shape[1]
    C = W[0].shape[1] - S - P
    dt32, sq32, dm = float(F4(dt)), float(F4(math.sqrt(dt))), float(F4(diag_min))
    sp = 1.0 if mp else 0.0
    hprev = np.concatenate([np.zeros((B, 1, L, H)), acts[:, :-1, :, 0]], axis=1)
    z = paths[:, :-1]
    ref, bnd = np.empty((B, T, L, 5, H)), np.empty((B, T, L, 5, H))
    for l in range(L):
        if l == 0:
            th, mth, _ = _dot(theta, W[0][:, S + C:])
            zz, mz, _ = _dot(z, W[0][:, :S])
            a, mag_a, n_a, sp_a = G + th[:, None] + zz, np.abs(G) + mth[:, None] + mz, 1 + P + S, 0.0
            Wh, bh = W[1], W[3]
        else:
            ai, mai, spi = _dot(acts[:, :, l - 1, 0], W[4][l - 1])
            a, mag_a, n_a, sp_a = ai + W[6][l - 1], mai + np.abs(W[6][l - 1]), H + 1, sp * spi
            Wh, bh = W[5][l - 1], W[7][l - 1]
        ch, mch, sph = _dot(hprev[:, :, l], Wh)
        c, mag_c, n_c, sp_c = ch + bh, mch + np.abs(bh), H + 1, sp * sph
        d_ac = (n_a + n_c + SLACK) * U * (mag_a + mag_c) + sp_a + sp_c
        d_a = (n_a + SLACK) * U * mag_a + sp_a
        d_c = (n_c + SLACK) * U * mag_c + sp_c
        x_r, x_u = a[..., :H] + c[..., :H], a[..., H:2 * H] + c[..., H:2 * H]
        r, u = sig64(x_r), sig64(x_u)
        d_r, d_u = d_ac[..., :H] / 4 + e_sig(x_r), d_ac[..., H:2 * H] / 4 + e_sig(x_u)
        cn, d_cn = c[..., 2 * H:], d_c[..., 2 * H:]
        x_n = a[..., 2 * H:] + r * cn
        d_xn = d_a[..., 2 * H:] + r * d_cn + np.abs(cn) * d_r + d_r * d_cn + 3 * U * (mag_a[..., 2 * H:] + r * mag_c[..., 2 * H:])
        n = np.tanh(x_n)
        d_n = d_xn + e_tanh(x_n)
        hp = hprev[:, :, l]
        h = (1.0 - u) * n + u * hp
        d_h = np.abs(hp - n) * d_u + (1.0 - u) * d_n + d_u * d_n + 4 * U * (np.abs(n) + np.abs(hp))
        for k, (v, d) in enumerate(((h, d_h), (r, d_r), (u, d_u), (n, d_n), (cn, d_cn))):
            ref[:, :, l, k], bnd[:, :, l, k] = v, d + FLOOR
    oo, mo, spo = _dot(acts[:, :, L - 1, 0], W[8])
    o, d_o = oo + W[9], (H + 1 + SLACK) * U * (mo + np.abs(W[9])) + sp * spo + FLOOR
    means, raw = o[..., :S], o[..., S:]
    ii, jj = np.tril_indices(S)
    Lm, dL = np.zeros((B, T, S, S)), np.zeros((B, T, S, S))
    Lm[..., ii, jj], dL[..., ii, jj] = raw, d_o[..., S:]
    dg = np.arange(S)
    Lm[..., dg, dg] = np.maximum(Lm[..., dg, dg], dm)
    le = np.einsum("btij,btj->bti", Lm, eps)
    nxt = z + means * dt32 + le * sq32
    d_nxt = (dt32 * d_o[..., :S] + sq32 * np.einsum("btij,btj->bti", dL, np.abs(eps))
             + (S + 6) * U * (np.abs(z) + np.abs(means * dt32) + sq32 * np.einsum("btij,btj->bti", np.abs(Lm), np.abs(eps))) + FLOOR)
    return dict(acts=(ref, bnd), means=(means, d_o[..., :S]), chol_raw=(raw, d_o[..., S:]), chol=(Lm, dL), next=(nxt, d_nxt))


def chol_identities(chol, chol_raw, diag_min=DIAG_MIN):
    """The chol a kernel must have written, bit for bit, given its own chol_raw: the lower triangle copied, the diagonal floored at
    float32(diag_min), the strict upper triangle zero."""
    chol, raw = np.asarray(chol), np.asarray(chol_raw)
    S = chol.shape[-1]
    ii, jj = np.tril_indices(S)
    want = np.zeros_like(chol)
    want[..., ii, jj] = raw
    dg = np.arange(S)
    d = want[..., dg, dg]
    want[..., dg, dg] = np.where(d < F4(diag_min), F4(diag_min), d)      # NaN propagates like the kernels' select
    return want


def excess(got, ref, bound):
    """(number of elements out of bound, worst |error| / bound, index of the worst) -- every element counts, NaN is out of bound."""
    err = np.abs(_f8(got) - ref)
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf))
    ratio = np.where(np.isfinite(ratio), ratio, np.inf)
    bad = ~(err <= bound)
    k = int(np.argmax(ratio)) if ratio.size else 0
    return int(bad.sum()), (float(ratio.reshape(-1)[k]) if ratio.size else 0.0), (np.unravel_index(k, ratio.shape) if ratio.size else ())


# -------------------------------------------------------------------------------------------------------------- sweep
def upstream_scale(gp, gm, gl):
    """Sg of the multi-path sweep: 2^(1 + exponent of max |g|) (vsde_head_mp.hip:669-673)."""
    m = max(float(np.abs(a).max()) if a.size else 0.0 for a in (gp, gm, gl))
    if m == 0.0 or not np.isfinite(m):
        return 1.0
    return 2.0 ** (math.floor(math.log2(m)) + 1)


def _sweep(ws, eps, chol_raw, acts, gp, gm, gl, dt, diag_min, keep=None, floor_sg=None, per_step=0.0):
    """One pass of the reverse-time recurrence.  keep is None: the float64 values (also returns the clamp masks and the unmasked dL of
    every diagonal); otherwise keep = (masks, unmasked dL) and the pass runs on absolute values, with a second track F of absolute error
    sources carried through the same recurrence: the clamp's sign ambiguity (below) and, with floor_sg, the multi-path split floor."""
    absolute = keep is not None
    A = np.abs if absolute else (lambda v: v)
    W = [A(_f8(a)) for a in ws]
    eps, raw, acts = A(_f8(eps)), _f8(chol_raw), _f8(acts)
    gp, gm, gl = A(_f8(gp)), A(_f8(gm)), A(_f8(gl))
    B, T, L, _, H = acts.shape
    S = gp.shape[2]
    NO = n_out(S)
    dt32, sq32, dm = float(F4(dt)), float(F4(math.sqrt(dt))), float(F4(diag_min))
    tril = [(i, j) for i in range(S) for j in range(i + 1)]
    D4, DO = np.zeros((B, T, L, 4, H)), np.zeros((B, T, NO))
    track_f = absolute
    F4_, FO = (np.zeros_like(D4), np.zeros_like(DO)) if track_f else (None, None)
    dx, dh, spi = np.zeros((B, S)), [np.zeros((B, H)) for _ in range(L)], np.zeros((B, 3 * H))
    fx, fh, fspi = np.zeros((B, S)), [np.zeros((B, H)) for _ in range(L)], np.zeros((B, 3 * H))
    masks, vun = np.ones((B, T, S), bool), np.zeros((B, T, S))

    def fl(d, Wm):      # the split floor a product x @ Wm adds: 2^-25 sum_k (Sg |w_k| + |d_k|)
        return C_SUB * (floor_sg * Wm.sum(0) + d.sum(1, keepdims=True)) if floor_sg is not None else 0.0

    for t in range(T - 1, -1, -1):
        dx = dx + gp[:, t + 1]
        dO, fO = np.zeros((B, NO)), np.zeros((B, NO))
        dO[:, :S] = dx * dt32 + gm[:, t]
        fO[:, :S] = fx * dt32
        for k, (i, j) in enumerate(tril):
            v = dx[:, i] * eps[:, t, j] * sq32 + gl[:, t, i, j]
            f = fx[:, i] * eps[:, t, j] * sq32
            if i == j:
                if not absolute:
                    m = (raw[:, t, k] >= dm) | (v < 0)
                    masks[:, t, i], vun[:, t, i] = m, v
                    v = np.where(m, v, 0.0)
                else:
                    # Below the floor the rule turns on the SIGN of dL.  Where the float64 |dL| is within the unmasked bound b of dL the
                    # kernel's sign may differ: one side keeps a value of at most b, the other writes zero -- an absolute error of
                    # up to b here and, carried on, downstream.  Everywhere else the kernel must take the float64 branch.
                    n = (T - t) * per_step
                    b = v * n * (1 + n) + f
                    amb = (raw[:, t, k] < dm) & (np.abs(keep[1][:, t, i]) <= b)
                    m = keep[0][:, t, i]
                    v, f = np.where(m, v, 0.0), np.where(m, f, 0.0) + np.where(amb, b, 0.0)
            dO[:, S + k], fO[:, S + k] = v, f
        DO[:, t] = dO
        dcur = dO @ W[8]
        if track_f:
            FO[:, t] = fO
            fcur = fO @ W[8] + fl(dO, W[8])
        for l in range(L - 1, -1, -1):
            r, u, n, cn = acts[:, t, l, 1], acts[:, t, l, 2], acts[:, t, l, 3], acts[:, t, l, 4]
            hp = acts[:, t - 1, l, 0] if t > 0 else np.zeros((B, H))
            c_n = 1.0 - u                                   # coefficients of d in dn, du, dn_pre, ...
            c_u = A(hp - n)
            k_n = np.ones_like(n) if absolute else 1.0 - n * n
            k_u, k_r = u * (1.0 - u), r * (1.0 - r)
            cn_ = A(cn)

            def gates(d):
                dn_pre = c_n * d * k_n
                du_pre = c_u * d * k_u
                return dn_pre * cn_ * k_r, du_pre, dn_pre, dn_pre * r
            d = dcur + dh[l]
            dr, du, dn, dcn = gates(d)
            D4[:, t, l] = np.stack([dr, du, dn, dcn], 1)
            pi, ph = np.concatenate([dr, du, dn], 1), np.concatenate([dr, du, dcn], 1)
            Wh = W[1] if l == 0 else W[5][l - 1]
            dh[l] = u * d + ph @ Wh
            if track_f:
                fd = fcur + fh[l]
                fr, fu, fn, fcn = gates(fd)
                F4_[:, t, l] = np.stack([fr, fu, fn, fcn], 1)
                fpi, fph = np.concatenate([fr, fu, fn], 1), np.concatenate([fr, fu, fcn], 1)
                fh[l] = u * fd + fph @ Wh + fl(ph, Wh)
            if l > 0:
                Wi = W[4][l - 1]
                dcur = pi @ Wi
                if track_f:
                    fcur = fpi @ Wi + fl(pi, Wi)
            else:
                Wz = W[0][:, :S]
                dx = dx + pi @ Wz
                spi = spi + pi
                if track_f:
                    fx = fx + fpi @ Wz + fl(pi, Wz)
                    fspi = fspi + fpi
    return D4, DO, dx, spi, (masks, vun), (F4_, FO, fx, fspi)


def sweep_ref(ws, theta_dim, eps, chol_raw, acts, gp, gm, gl, dt, mp=False, diag_min=DIAG_MIN):
    """dict name -> (float64 value, bound) for D4, DO, grad_x0, grad_theta of the reverse-time sweep on the kernel's saved tensors."""
    B, T, L, _, H = np.asarray(acts).shape
    S, P = np.asarray(gp).shape[2], theta_dim
    NO = n_out(S)
    Wi0 = _f8(ws[0])
    Wth = Wi0[:, Wi0.shape[1] - P:] if P else np.zeros((3 * H, 0))
    D4, DO, dx, spi, keep, _ = _sweep(ws, eps, chol_raw, acts, gp, gm, gl, dt, diag_min)
    masks = keep[0]
    sg = upstream_scale(np.asarray(gp), np.asarray(gm), np.asarray(gl)) if mp else None
    d_step = (NO + 4) + L * (3 * H + C_COEF + 2) + (S + 4)
    per_step = d_step * U + ((2 * L + 2) * C_SPLIT if mp else 0.0)
    M4, MO, mx, mspi, _, (F4_, FO, fx, fspi) = _sweep(ws, eps, chol_raw, acts, gp, gm, gl, dt, diag_min, keep=keep, floor_sg=sg, per_step=per_step)
    gx0, mx0 = dx + _f8(gp)[:, 0], mx + np.abs(_f8(gp)[:, 0])
    gth, mth = spi @ Wth, mspi @ np.abs(Wth)

    def rel(steps, extra=0):
        n = steps * per_step + extra * U
        return n * (1 + n)
    steps = (T - np.arange(T)).astype(F8)                        # element of step t: T - t steps of the chain
    b4 = M4 * rel(steps)[None, :, None, None, None] + FLOOR
    bo = MO * rel(steps)[None, :, None] + FLOOR
    bx = mx0 * rel(T + 1) + FLOOR + fx
    bt = mth * rel(T + 1, T + 3 * H + 2) + FLOOR + fspi @ np.abs(Wth)
    b4, bo = b4 + F4_, bo + FO
    return dict(D4=(D4, b4), DO=(DO, bo), grad_x0=(gx0, bx), grad_theta=(gth, bt)), masks


# ------------------------------------------------------------------------------------------------ fp32 emulation, with defects
FORWARD_FAULTS = ("no_cross", "flush_sub", "skip_index", "wrong_layer", "cn_no_bias")
SWEEP_FAULTS = ("no_cross", "flush_sub", "skip_index", "drop_carry", "ignore_clamp")
F16_MIN = 2.0 ** -14


def split16(v, fault=None):
    """mp_split / mp_split_fast under the flushed denormal mode, on float32 arrays: (hi, lo') as float32 holding f16 values.
    fault 'flush_sub': the historical defect -- hi = f16(v) is taken as is, the matrix pipe then reads a subnormal hi as zero."""
    v = np.asarray(v, F4)
    with np.errstate(over="ignore", under="ignore"):
        if fault == "flush_sub":
            hi = v.astype(F2).astype(F4)
        else:
            hi = np.where(np.abs(v) < F4(F16_MIN), F4(0), v.astype(F2).astype(F4)).astype(F4)
        lo = ((v - hi) * F4(2048)).astype(F2).astype(F4)
    lo = np.where(np.abs(lo) < F4(F16_MIN), F4(0), lo).astype(F4)
    if fault == "flush_sub":
        hi = np.where(np.abs(hi) < F4(F16_MIN), F4(0), hi).astype(F4)
    return hi, lo


def dot32(x, W, bias=None, mp=False, fault=None):
    """x [B, K] @ W [K, N] (+ bias) in float32, plain left-to-right summation; mp: the three-product f16 split form."""
    x, W = np.asarray(x, F4), np.asarray(W, F4)
    K = x.shape[1]
    skip = K // 2 if fault == "skip_index" else -1
    acc = np.zeros((x.shape[0], W.shape[1]), F4) if bias is None else np.broadcast_to(np.asarray(bias, F4), (x.shape[0], W.shape[1])).copy()
    if not mp:
        for k in range(K):
            if k != skip:
                acc = acc + x[:, k:k + 1] * W[k]
        return acc
    xh, xl = split16(x, fault)
    wh, wl = split16(W, fault)
    a1, a2 = np.zeros_like(acc), np.zeros_like(acc)
    for k in range(K):
        if k != skip:
            a1 = a1 + xh[:, k:k + 1] * wh[k]
            a2 = a2 + (xh[:, k:k + 1] * wl[k] + xl[:, k:k + 1] * wh[k])
    return acc + (a1 if fault == "no_cross" else a1 + a2 * F4(1.0 / 2048))


def project32(ctx, ws, S):
    """G = ctx W_c^T + b_ih0 in float32 (an input of the time loop; the projection kernels have their own tests)."""
    ctx = np.asarray(ctx, F4)
    C = ctx.shape[2]
    Wc = np.asarray(ws[0], F4)[:, S:S + C]
    return (ctx.astype(F8) @ Wc.astype(F8).T + np.asarray(ws[2], F8)).astype(F4)


def emulate_forward(ws, x0, theta, eps, G, dt, mp=False, fault=None, diag_min=DIAG_MIN):
    """Free-running float32 forward: (paths, means, chol, chol_raw, acts), the tensors a kernel returns."""
    W = [np.asarray(a, F4) for a in ws]
    x0, theta, eps, G = (np.asarray(a, F4) for a in (x0, theta, eps, G))
    B, S = x0.shape
    T, P = eps.shape[1], theta.shape[1]
    H = W[1].shape[1]
    L = 1 + (W[4].shape[0] if W[4].size else 0)
    C = W[0].shape[1] - S - P
    NO = n_out(S)
    dt32, sq32, dm = F4(dt), F4(math.sqrt(dt)), F4(diag_min)
    dflt = fault if fault in ("no_cross", "flush_sub", "skip_index") else None
    paths, means = np.zeros((B, T + 1, S), F4), np.zeros((B, T, S), F4)
    chol, raws, acts = np.zeros((B, T, S, S), F4), np.zeros((B, T, NO - S), F4), np.zeros((B, T, L, 5, H), F4)
    gth = dot32(theta, W[0][:, S + C:].T)
    h = [np.zeros((B, H), F4) for _ in range(L)]
    z = x0.copy()
    paths[:, 0] = z
    ii, jj = np.tril_indices(S)
    for t in range(T):
        a = (G[:, t] + gth) + dot32(z, W[0][:, :S].T)
        hold = [v.copy() for v in h]
        for l in range(L):
            Wh, bh = (W[1], W[3]) if l == 0 else (W[5][l - 1], W[7][l - 1])
            hp = hold[(l + 1) % L] if fault == "wrong_layer" else hold[l]
            c = dot32(hp, Wh.T, bh, mp, dflt)
            cn = c[:, 2 * H:]
            cn_used = (cn - bh[2 * H:]) if fault == "cn_no_bias" else cn
            r, u = sigmoid32(a[:, :H] + c[:, :H]), sigmoid32(a[:, H:2 * H] + c[:, H:2 * H])
            n = tanh32(a[:, 2 * H:] + r * cn_used)
            hn = ((F4(1) - u) * n + u * hold[l]).astype(F4)
            acts[:, t, l] = np.stack([hn, r, u, n, cn], 1)
            h[l] = hn
            if l < L - 1:
                a = dot32(hn, W[4][l].T, W[6][l], mp, dflt)
        o = dot32(h[L - 1], W[8].T, W[9], mp, dflt)
        means[:, t], raws[:, t] = o[:, :S], o[:, S:]
        Lm = np.zeros((B, S, S), F4)
        Lm[:, ii, jj] = o[:, S:]
        dg = np.arange(S)
        Lm[:, dg, dg] = np.where(Lm[:, dg, dg] < dm, dm, Lm[:, dg, dg])
        chol[:, t] = Lm
        acc = np.zeros((B, S), F4)
        for j in range(S):
            acc = acc + Lm[:, :, j] * eps[:, t, j:j + 1]
        z = (z + o[:, :S] * dt32 + acc * sq32).astype(F4)
        paths[:, t + 1] = z
    return paths, means, chol, raws, acts


def emulate_sweep(ws, theta_dim, eps, chol_raw, acts, gp, gm, gl, dt, mp=False, fault=None, fault_step=None, diag_min=DIAG_MIN):
    """Float32 reverse-time sweep on given saved tensors: (D4, DO, grad_x0, grad_theta).  mp: on g / Sg with split products."""
    W = [np.asarray(a, F4) for a in ws]
    eps, raw, acts, gp, gm, gl = (np.asarray(a, F4) for a in (eps, chol_raw, acts, gp, gm, gl))
    B, T, L, _, H = acts.shape
    S, P = gp.shape[2], theta_dim
    NO = n_out(S)
    dt32, sq32, dm = F4(dt), F4(math.sqrt(dt)), F4(diag_min)
    sg = F4(upstream_scale(gp, gm, gl)) if mp else F4(1)
    inv = F4(1) / sg
    dflt = fault if fault in ("no_cross", "flush_sub", "skip_index") else None
    fault_step = T - 1 if fault_step is None else fault_step
    tril = [(i, j) for i in range(S) for j in range(i + 1)]
    D4, DO = np.zeros((B, T, L, 4, H), F4), np.zeros((B, T, NO), F4)
    dx, dh, spi = np.zeros((B, S), F4), [np.zeros((B, H), F4) for _ in range(L)], np.zeros((B, 3 * H), F4)
    for t in range(T - 1, -1, -1):
        dx = dx + gp[:, t + 1] * inv
        dO = np.zeros((B, NO), F4)
        dO[:, :S] = dx * dt32 + gm[:, t] * inv
        for k, (i, j) in enumerate(tril):
            v = (dx[:, i] * eps[:, t, j]) * sq32 + gl[:, t, i, j] * inv
            if i == j and fault != "ignore_clamp":
                v = np.where((raw[:, t, k] >= dm) | (v < 0), v, F4(0))
            dO[:, S + k] = v
        DO[:, t] = dO * sg
        dcur = dot32(dO, W[8], None, mp, dflt)
        for l in range(L - 1, -1, -1):
            r, u, n, cn = acts[:, t, l, 1], acts[:, t, l, 2], acts[:, t, l, 3], acts[:, t, l, 4]
            hp = acts[:, t - 1, l, 0] if t > 0 else np.zeros((B, H), F4)
            d = dcur + dh[l]
            dn_pre = ((F4(1) - u) * d) * (F4(1) - n * n)
            du_pre = ((hp - n) * d) * (u * (F4(1) - u))
            dcn = dn_pre * r
            dr_pre = (dn_pre * cn) * (r * (F4(1) - r))
            D4[:, t, l] = np.stack([dr_pre, du_pre, dn_pre, dcn], 1) * sg
            pi, ph = np.concatenate([dr_pre, du_pre, dn_pre], 1), np.concatenate([dr_pre, du_pre, dcn], 1)
            Wh = W[1] if l == 0 else W[5][l - 1]
            carry = np.zeros_like(d) if (fault == "drop_carry" and t == fault_step) else u * d
            dh[l] = dot32(ph, Wh, None, mp, dflt) + carry
            if l > 0:
                dcur = dot32(pi, W[4][l - 1], None, mp, dflt)
            else:
                dx = dx + dot32(pi, W[0][:, :S], None, mp, dflt)
                spi = spi + pi
    gx0 = (dx + gp[:, 0] * inv) * sg
    Wth = W[0][:, W[0].shape[1] - P:] if P else np.zeros((3 * H, 0), F4)
    return D4, DO, gx0, dot32(spi, Wth) * sg


# ------------------------------------------------------------------------------------------------------ dispatch mirror
def _take(off, n):
    return off + ((n + 3) & ~3)


def fwd_v2_lds(H, S, L, CH, save):
    """Total floats of fwd_v2_lds (vsde_head.hip:512-526)."""
    ntril = S * (S + 1) // 2
    off = 0
    for n in (L * 64, 64, S * 3 * 64, (S + ntril + 1) * 68, 3 * 64, 2 * CH * 3 * H, 2 * CH * S, CH * S, CH * S, CH * S * S,
              CH * ntril if save else 0, CH * L * 5 * 64 if save else 0, L * 5 * 64 if save else 0):
        off = _take(off, n)
    return off


def bwd_v2_lds(H, S, L, CH, two_act_buffers=False, wide=False):
    """Total floats of bwd_v2_lds (vsde_head.hip:934-947)."""
    ntril = S * (S + 1) // 2
    NO = S + ntril
    off = 0
    for n in ((2 if two_act_buffers else 1) * (CH + 1) * L * 5 * H, CH * L * 4 * H, CH * NO, CH * S, CH * S, CH * S * S, CH * ntril, CH * S,
              256 * 20 if wide else NO * 64, 64 if wide else 0, 16 * 16 if wide else 4 * 16, S * 3 * 64 if wide else 0):
        off = _take(off, n)
    return off


def pick_wpb(B, lds_fixed, lds_per_wave):
    wpb = min(max((B + 255) // 256, 1), 8)
    while wpb > 1 and lds_fixed + wpb * lds_per_wave > 160 * 1024:
        wpb -= 1
    return wpb


def v1_wpb(dims, backward=False):
    """Waves per workgroup of the v1 kernels (vsde_head.hip:1794-1799, :2096-2101)."""
    B, T, S, P, C, H, L = dims
    NO = n_out(S)
    mats = min(2 * L - 1, 3) * (16 * 3 * 64) * 16
    if backward:
        return pick_wpb(B, mats + NO * 64 * 4, (4 * 64 + 3 * 64) * 4)
    return pick_wpb(B, mats + 16 * NO * 16, 3 * 64 * 4)


def wide_block(dims):
    B, T, S, P, C, H, L = dims
    return min((max(H, n_out(S)) + 63) // 64 * 64, 1024)


ERROR_CODES = {"VSDE_E_BADARG": -1, "VSDE_E_LAYERS": -2, "VSDE_E_HIDDEN": -3, "VSDE_E_WORKSPACE": -4, "VSDE_E_STATE": -5}


def check_dims(dims):
    """check_dims (vsde_head.hip:1519-1532): None, or the name of the refusal (``ERROR_CODES``: include/vsde_hip.h:45-49)."""
    B, T, S, P, C, H, L = dims
    if not (B > 0 and T > 0 and S > 0 and P >= 0 and C > 0 and H > 0):
        return "VSDE_E_BADARG"
    if not 1 <= L <= 4:
        return "VSDE_E_LAYERS"
    if H > 1024:
        return "VSDE_E_HIDDEN"
    if S > 32:
        return "VSDE_E_STATE"
    if (L * H + 2 * H + 4 * H + (S + 2) * (S + H + 4)) * 4 > 150 * 1024:
        return "VSDE_E_HIDDEN"
    return None


def _generic(H, S):
    return H > K_HP or n_out(S) > K_WAVE


def mp_applicable(H, L, S):
    return H == 64 and 1 <= L <= 2 and 1 <= S <= 2


def mp_bwd_applicable(H, L, S):
    return H == 64 and L == 2 and 1 <= S <= 2


def _use_mp(applicable, B, mp_mode):
    if not applicable or mp_mode == 0:
        return False
    return True if mp_mode > 0 else B >= 32            # mp_auto / use_mp_bwd: from 32 paths on


def _b(v):
    return "true" if v else "false"


def route_forward(dims, save, mp_mode=-1, force_v1=False):
    """The forward time-loop kernel vsde_head_forward launches (shipped library, default knobs, sticky overflow flag clear)."""
    B, T, S, P, C, H, L = dims
    assert check_dims(dims) is None
    NO = n_out(S)
    if _generic(H, S):
        return f"head_fwd_wide_kernel<{_b(save)}>"
    if not force_v1 and _use_mp(mp_applicable(H, L, S), B, mp_mode):
        np_ = mp_mode if mp_mode in (2, 4, 8, 16) else (2 if B <= 512 else 4 if B <= 1024 else 8 if B <= 2048 else 16)
        return f"head_fwd_mp_kernel<{L}, {_b(save)}, {S}, {np_}, {1 if np_ <= 4 else 4}>"
    if L <= 2 and not force_v1:
        ch = 8 if fwd_v2_lds(H, S, L, 16, save) * 4 > 80 * 1024 else 16
        assert fwd_v2_lds(H, S, L, ch, save) * 4 <= 160 * 1024
        mode = 1 if (S == 1 and ch == 16) else 2 if (S == 2 and ch == 16) else 3 if NO <= 16 else 4
        return f"head_fwd_v2_kernel<{L}, {_b(save)}, {ch}, {mode}>"
    return f"head_fwd_kernel<{L}, {_b(save)}>"


def route_backward(dims, mp_mode=-1, force_v1=False):
    """The reverse-time sweep kernel vsde_head_backward launches."""
    B, T, S, P, C, H, L = dims
    assert check_dims(dims) is None
    NO = n_out(S)
    if not force_v1 and _use_mp(mp_bwd_applicable(H, L, S), B, mp_mode):
        np_ = mp_mode if mp_mode in (2, 4, 8) else 8 if mp_mode == 16 else (2 if B <= 512 else 4 if B <= 1024 else 8)
        return f"head_bwd_mps_kernel<{S}, {np_}>" if np_ in (2, 4) else f"head_bwd_mp_kernel<{S}, 8>"
    if _generic(H, S):
        return "head_bwd_wide_kernel"
    if L <= 2 and H % 4 == 0 and (NO > 16 or S > K_MAX_SREG_V2) and S <= 16 and not force_v1:
        ch = 0
        for limit in (80, 156):
            for c in (16, 10, 8):
                if not ch and bwd_v2_lds(H, S, L, c, True, True) * 4 <= limit * 1024:
                    ch = c
        assert ch
        return f"head_bwd_v2_kernel<{L}, {ch}, 0, true, true>"
    if L <= 2 and NO <= 16 and S <= K_MAX_SREG_V2 and not force_v1:
        ch = 0
        if H % 4 == 0:
            for c in (16, 10, 8):
                if not ch and bwd_v2_lds(H, S, L, c, True) * 4 <= 80 * 1024:
                    ch = c
        if ch:
            return f"head_bwd_v2_kernel<{L}, {ch}, {S if S <= 2 else 0}, true>"
        ch = 16
        while ch > 4 and bwd_v2_lds(H, S, L, ch) * 4 > 80 * 1024:
            ch -= 1
        if ch < 12:
            ch = 8
        return f"head_bwd_v2_kernel<{L}, {ch}, 0, false>"
    return f"head_bwd_kernel<{L}>"


# every instantiation a launch can reach (the CPU test sweeps the mirror over all dims and hook values and compares)
FORWARD_KERNELS = tuple(sorted(
    [f"head_fwd_kernel<{L}, {s}>" for L in (1, 2, 3, 4) for s in ("true", "false")]
    + [f"head_fwd_v2_kernel<{L}, {s}, 16, {m}>" for L in (1, 2) for s in ("true", "false") for m in (1, 2, 3, 4)]
    + ["head_fwd_v2_kernel<2, true, 8, 4>", "head_fwd_wide_kernel<true>", "head_fwd_wide_kernel<false>"]
    + [f"head_fwd_mp_kernel<{L}, {s}, {S}, {n}, {u}>" for L in (1, 2) for s in ("true", "false") for S in (1, 2)
       for n, u in ((2, 1), (4, 1), (8, 4), (16, 4))]))
BACKWARD_KERNELS = tuple(sorted(
    [f"head_bwd_kernel<{L}>" for L in (1, 2, 3, 4)] + ["head_bwd_wide_kernel"]
    + [f"head_bwd_v2_kernel<{L}, {c}, 0, true, true>" for L, c in ((1, 16), (1, 10), (2, 16), (2, 10), (2, 8))]
    + [f"head_bwd_v2_kernel<1, 16, {m}, true>" for m in (0, 1, 2)]
    + [f"head_bwd_v2_kernel<2, {c}, {m}, true>" for c, m in ((16, 0), (16, 1), (16, 2), (10, 0), (10, 1), (10, 2), (8, 0))]
    + [f"head_bwd_v2_kernel<{L}, {c}, 0, false>" for L, c in ((1, 16), (2, 16), (2, 15))]
    + [f"head_bwd_mps_kernel<{S}, {n}>" for S in (1, 2) for n in (2, 4)] + ["head_bwd_mp_kernel<1, 8>", "head_bwd_mp_kernel<2, 8>"]))


# ------------------------------------------------------------------------------------------------------ cases and inputs
def _case(name, B, T, S, H, L, P=3, C=16, mp=-1, v1=False, kind="randn"):
    return dict(id=name, dims=(B, T, S, P, C, H, L), mp=mp, v1=v1, kind=kind)


KINDS = ("randn", "sub", "sat", "clamp", "eps0", "onegrad")
T_SET = (1, 2, 3, 15, 16, 17, 33)
CASES = (
    # v2, default dispatch: 17 paths cross all 16 phases of the staggered first chunk (vsde_head.hip:689)
    [_case(f"v2-L2-S2-T{T}", 17, T, 2, 64, 2) for T in T_SET]
    + [_case("v2-L1-S1-T17", 5, 17, 1, 64, 1), _case("v2-L2-S1-P1-T33", 5, 33, 1, 64, 2, P=1), _case("v2-L1-S2-T3", 5, 3, 2, 64, 1),
       _case("v2-L1-S3-T16", 5, 16, 3, 64, 1), _case("v2-L2-S3-H32-T33", 5, 33, 3, 32, 2), _case("v2-L2-S4-T17", 5, 17, 4, 64, 2),
       _case("v2-L2-S4-H40-T15", 5, 15, 4, 40, 2), _case("v2-L2-S1-H32-T3", 5, 3, 1, 32, 2), _case("v2-L2-S2-H32-T17", 5, 17, 2, 32, 2),
       _case("v2-L1-S5-T17", 5, 17, 5, 64, 1), _case("v2-L2-S5-ch8-T33", 5, 33, 5, 64, 2), _case("v2-L2-S9-ch8-T16", 5, 16, 9, 64, 2),
       _case("v2-L1-S9-H32-T2", 5, 2, 9, 32, 1), _case("v2-L2-S8-H24-T15", 5, 15, 8, 24, 2), _case("v2-L2-S8-H40-T17", 5, 17, 8, 40, 2),
       _case("v2-L1-S9-H44-T1", 5, 1, 9, 44, 1),
       _case("v2-L2-S2-H30-T17", 5, 17, 2, 30, 2), _case("v2-L1-S3-H30-T16", 5, 16, 3, 30, 1), _case("v2-L2-S4-H63-T33", 5, 33, 4, 63, 2),
       _case("v2-L1-S5-H30-T3", 5, 3, 5, 30, 1), _case("v2-L2-S5-H30-T15", 5, 15, 5, 30, 2)]
    # the backward's wide variant and its fallback at the short step counts too
    + [_case(f"v2-L2-S5-T{T}", 5, T, 5, 64, 2) for T in (1, 2, 3)] + [_case(f"v2-L2-S2-H30-T{T}", 5, T, 2, 30, 2) for T in (1, 2, 3, 15)]
    # v1: L = 3, 4 by default dispatch, L = 1, 2 forced (H <= 64, NO <= 64), two waves per workgroup at B > 256
    + [_case("v1-L3-T17", 3, 17, 2, 64, 3), _case("v1-L4-H48-T3", 3, 3, 3, 48, 4), _case("v1-L1-forced-T2", 3, 2, 2, 64, 1, v1=True),
       _case("v1-L2-forced-H20-T33", 5, 33, 1, 20, 2, v1=True), _case("v1-L3-B300-T2", 300, 2, 2, 64, 3), _case("v1-L4-S5-T16", 3, 16, 5, 64, 4)]
    # generic wide kernels
    + [_case("wide-H80-L2-T17", 4, 17, 3, 80, 2), _case("wide-H130-L1-S10-T3", 3, 3, 10, 130, 1), _case("wide-H96-L4-T2", 3, 2, 2, 96, 4),
       _case("wide-H128-L1-T15", 3, 15, 2, 128, 1), _case("wide-H40-S10-L1-T3", 3, 3, 10, 40, 1), _case("wide-H65-L3-T33", 3, 33, 1, 65, 3)]
    # multi-path forward (and, at L = 2, backward): B = one full group, one group + 1, 3
    + [_case(f"mp{n}-L2-S{S}-B{B}-T{T}", B, T, S, 64, 2, mp=n) for S, n, T, B in (
        (1, 2, 1, 3), (1, 4, 2, 5), (1, 8, 3, 8), (1, 16, 17, 17), (2, 2, 33, 2), (2, 4, 17, 4), (2, 8, 33, 9), (2, 16, 1, 16),
        (2, 2, 3, 3), (2, 4, 1, 3), (2, 8, 2, 3), (1, 2, 17, 3), (1, 4, 33, 5), (2, 8, 17, 8), (1, 16, 2, 3), (2, 4, 3, 5), (1, 8, 1, 9))]
    + [_case(f"mp{n}-L1-S{S}-B{B}-T{T}", B, T, S, 64, 1, mp=n) for S, n, T, B in (
        (1, 2, 2, 3), (1, 4, 3, 4), (1, 8, 17, 9), (1, 16, 33, 16), (2, 2, 17, 2), (2, 4, 33, 5), (2, 8, 1, 8), (2, 16, 2, 17))]
    # default dispatch on both sides of the mp_auto threshold
    + [_case("auto-B31", 31, 17, 2, 64, 2), _case("auto-B32", 32, 17, 2, 64, 2)]
    # input classes on one representative of each family
    + [_case(f"v2-{k}", 17, 17, 2, 64, 2, kind=k) for k in KINDS[1:]]
    + [_case(f"v1-{k}", 3, 17, 2, 64, 3, kind=k) for k in KINDS[1:]]
    + [_case(f"wide-{k}", 4, 17, 3, 80, 2, kind=k) for k in KINDS[1:]]
    + [_case(f"mp4-{k}", 5, 17, 2, 64, 2, mp=4, kind=k) for k in KINDS[1:]]
    + [_case(f"mp8-{k}", 9, 17, 2, 64, 2, mp=8, kind=k) for k in ("sub", "sat", "clamp", "onegrad")]
    + [_case("mp16-L1-sub", 17, 3, 2, 64, 1, mp=16, kind="sub"), _case("mp2-L1-sat", 3, 17, 1, 64, 1, mp=2, kind="sat")]
    # theta with P = 1 in every family (v2: v2-L2-S1-P1-T33 above)
    + [_case("v1-L3-P1-T17", 3, 17, 2, 64, 3, P=1), _case("v1-L1-forced-P1-T3", 3, 3, 1, 64, 1, P=1, v1=True),
       _case("wide-H80-L2-P1-T17", 4, 17, 3, 80, 2, P=1), _case("mp4-L2-S2-P1-T17", 5, 17, 2, 64, 2, P=1, mp=4),
       _case("mp8-L2-S1-P1-T17", 9, 17, 1, 64, 2, P=1, mp=8), _case("mp16-L1-S2-P1-T3", 17, 3, 2, 64, 1, P=1, mp=16)]
)


def is_mp(name):
    return "_mp" in name


def make_inputs(case, seed=0):
    """Inputs of a case as float32 numpy arrays: ws (ten weights at the scales of tests/test_head_gpu.py), x0, ctx [B, T, C] fp32, theta, eps,
    the upstream gradients gp, gm, gl, dt.  Classes:
      sub      a quarter of the recurrent / emission weights drawn from [2^-26, 2^-14): the f16 subnormal rule of the split
      sat      a quarter of the gate rows x 30, another quarter with a bias of +-30: pre-activations around +-30, |W| 2.89 < 150 (f16 range)
      clamp    (S >= 2) first diagonal's emission row scaled down around a bias of diag_min, so the floor binds on about half the steps;
               last diagonal's row zero with bias float32(diag_min): raw == diag_min exactly
      eps0     no noise;  onegrad  upstream gradients zero except one (b, t) pair, the last step of the middle path"""
    B, T, S, P, C, H, L = case["dims"]
    kind, NO = case["kind"], n_out(S)
    g = np.random.default_rng(1000 * S + 100 * L + 10 * T + H + 7 * B + seed)
    rn = lambda *s, sc=1.0: (g.standard_normal(s) * sc).astype(F4)
    ws = [rn(3 * H, S + C + P, sc=.15), rn(3 * H, H, sc=.15), rn(3 * H, sc=.1), rn(3 * H, sc=.1), rn(L - 1, 3 * H, H, sc=.15),
          rn(L - 1, 3 * H, H, sc=.15), rn(L - 1, 3 * H, sc=.1), rn(L - 1, 3 * H, sc=.1), rn(NO, H, sc=.2), rn(NO, sc=.3)]
    x0, ctx, theta, eps = rn(B, S), rn(B, T, C), np.abs(rn(B, P)), rn(B, T, S)
    gp, gm, gl = rn(B, T + 1, S), rn(B, T, S), rn(B, T, S, S)
    if kind == "sub":
        for i in (1, 4, 5, 8):
            w = ws[i]
            tiny = (2.0 ** g.uniform(-26, -14, w.shape) * g.choice([-1.0, 1.0], w.shape)).astype(F4)
            ws[i] = np.where(g.random(w.shape) < 0.25, tiny, w).astype(F4)
    if kind == "sat":
        for wi, bi in ((1, 3), (5, 7)):
            if ws[wi].size:
                rows = g.random(ws[bi].shape)
                ws[wi] = (ws[wi] * np.where(rows < 0.25, 30.0, 1.0)[..., None]).astype(F4)
                ws[bi] = np.where(rows > 0.75, np.where(g.random(rows.shape) < 0.5, -30.0, 30.0), ws[bi]).astype(F4)
    if kind == "clamp":
        d0, dl = S, S + S * (S + 1) // 2 - 1          # emission rows of the first and the last diagonal entry
        ws[8][d0] *= F4(0.05)
        ws[9][d0] = F4(DIAG_MIN)
        if S >= 2:
            ws[8][dl] = 0
            ws[9][dl] = F4(DIAG_MIN)
    if kind == "eps0":
        eps = np.zeros_like(eps)
    if kind == "onegrad":
        b0 = B // 2
        keep_p, keep_t = np.zeros((B, T + 1, 1), F4), np.zeros((B, T, 1), F4)
        keep_p[b0, T], keep_t[b0, T - 1] = 1, 1
        gp, gm, gl = gp * keep_p, gm * keep_t, gl * keep_t[..., None]
    return dict(ws=ws, x0=x0, ctx=ctx, theta=theta, eps=eps, gp=gp, gm=gm, gl=gl, dt=0.05)
