"""float64 references and per-element error bounds of the attention kernels (csrc/vsde_attn.hip, csrc/vsde_attn_stream.hip and
the attention epilogues of csrc/vsde_linear.hip).  Plain functions on torch tensors of any device: tests/test_attention_ops_gpu.py
runs them on the GPU against the kernels, tests/test_attention_bounds.py on the CPU against an emulation of the kernels' rounding
(with injected defects that each bound must reject).

Layouts as in the kernels: q, k, v, o token-major [B, N, H, 64] (or D = 128), lse / delta [B, H, N], projection rows [M = B N, ...].
Every reference works in batch slices (``slices``): the LV shape's probabilities alone are 2.6 GB in float64.

Bounds, per element, never relative to a tensor's maximum.  U = 2^-8 is the bf16 unit round-off (half an ulp, relative): U |ref|
is exactly one rounding of the output, so an output whose only error is its own rounding reaches err / bound up to 1 by
construction; the roundings inside the sums (P, dS) get 2 U, a factor 2 to spare for the fp32 work around them:
  attention_fwd           o_i    2 U sum_j p_ij |v_j| + U |o_i|                       (P rounded for the PV product; the output)
  attention_fwd_gated     og_i   s_i (2 U sum_j p_ij |v_j|) + U |og_i|                (s = the bf16 gate factor, applied in fp32)
  lse                     |lse_i - ref| <= 1e-5 (|lse_i| + scale |q_i| max_j |k_j|)   (fp32 scores, shift and log)
  attention_bwd           dq_i   2 U scale sum_j |dS_ij| |k_j| + U |dq_i|            (dS rounded for the second product)
  (teacher-forced on the  dk_j   2 U scale sum_i |dS_ij| |q_i| + U |dk_j|
   kernel's own o, lse)   dv_j   2 U sum_i P_ij |dO_i| + U |dv_j|                     (P rounded)
                          P = exp(scale q k^T - lse), delta_i = <dO_i, o_i>, dS = P (dO v^T - delta); 2 U |dS| in dq / dk
                          grows by 2^-20 P (|dO| |v|^T + sum_j P_ij |dO_i| |v_j|): the fp32 error of dP - delta, which is
                          all there is where the two cancel (N = 1: dP = delta)
  gate_bwd_delta          dattn  U |ref|;  delta  1e-5 sum_c |dout og|;  dlogit  U |ref| + |1 - s| 1e-5 sum |dout og|
  linear_gate_bwd         the same from G = rnd(dy w_t^T) (fp32 accumulation: one-ulp allowance of G propagated)
  linear_gated_bf16       y  U sum_k |a_k s_k w_k| + U |y| + 1e-6 sum |a s w|         (rnd(sigmoid), rnd(a s), output)
  linear_qknorm_bf16      y = rnd(x W^T + b) with the one-ulp allowance (fp32 GEMM error 2^-16 sum |x w|); a = rnd(y r w);
                          an output rounded after an allowance A entered is bounded by U (|ref| + A) + A;
                          q / k = rnd(R a): U (|ref| + A) + A, A = the allowances of a propagated through R; gate s = rnd(sigmoid(y)):
                          U |s| + |y-step| / 4; logits / v (no v0) = rnd(y); v = rnd(lam y + (1 - lam) v0); vdiff = rnd(y - v0);
                          rinv = r (1e-6 + sum_k |y_k| dy_k / (64 ms))
  attention_bwd_fused     g = scale dS k (fp32, not rounded): E_g = 2 U scale sum_j |dS_ij| |k_j|; with n = y r (RAW y),
                          dn = w (R^T g), cc = <dn, n> / 64, the reference is dy = r (dn - n cc) and its bound, channel j with
                          rotary partner p (j +- 32):
                            r (|w_j| (|c| E_g,j + |s| E_g,p) + |n_j| sum_k |yhat_k| E_g,k / 64)      g's error, carried
                            + U r cc_abs (|n_j| + (|yhat_j| + |yhat_p|) / |w_j|)                       the saved bf16 yhat,
                                                                                                       divided by w_j
                            + U |ref| + 1e-5 r (|w_j| |u_j| + |n_j| cc_abs) + the allowance of raw y
                          The backward rebuilds n_j = (R^T yhat)_j / w_j from the saved bf16 rotated row: yhat's rounding
                          (U of |yhat_j| + |yhat_p|) is divided by |w_j|.  That term is the reason for the weight limit of
                          ``fused.norm_weights_fusable``: with |w_j| >= max|w| / 16 it stays within 16 x the
                          rounding the separate passes make.
                          values: dv = P^T dattn (+ dv_extra): dy_v = rnd(lam dv): |lam| E_dv + U |ref|; dv0 = rnd((1 - lam) dv
                          (+ dv0)): |1 - lam| E_dv + U |ref|; dlam = sum dv vdiff, teacher-forced on the kernel's own
                          dv = dy_v / lam (rounded once, U |dv|): 1e-5 sum |dv vdiff| + U sum |dv vdiff|
"""
import torch

F64 = torch.float64
BF = torch.bfloat16
U = 2.0 ** -8
LSE_C = 1e-5
SUM_C = 1e-5
FP32_C = 2.0 ** -20   # fp32 arithmetic of a short sum, relative to the sum of its terms' magnitudes


def slices(B, rows_per_pair, budget=2 ** 27):
    """Batch slices whose [b, H, N, N] float64 products stay within ``budget`` elements."""
    step = max(1, budget // max(1, rows_per_pair))
    return [(b0, min(B, b0 + step)) for b0 in range(0, B, step)]


def round_bf16(t, err):
    """bf16 rounding of a float64 value the kernel forms in fp32 with an error up to ``err``: (rounded value, size of the one-ulp
    step the kernel's rounding may differ by -- 0 where the value is not within ``err`` of a rounding boundary)."""
    r = t.to(BF).to(F64)
    return r, ((t + err).to(BF).to(F64) - (t - err).to(BF).to(F64)).abs()


def excess(got, ref, bound):
    """(number of elements out of bound, worst |err| / bound, index of the first bad element or None).  NaN counts as out."""
    err = (got.to(F64) - ref).abs()
    bad = ~(err <= bound)
    ratio = err / bound.clamp_min(1e-300)
    worst = float(ratio[~torch.isnan(ratio)].max()) if bool((~torch.isnan(ratio)).any()) else float("nan")
    nbad = int(bad.sum())
    return nbad, worst, (tuple(int(i) for i in bad.nonzero()[0]) if nbad else None)


def _heads(t):
    return t.to(F64).permute(0, 2, 1, 3)   # [b, N, H, D] -> [b, H, N, D]


def _tok(t):
    return t.permute(0, 2, 1, 3)           # [b, H, N, D] -> [b, N, H, D]


# ------------------------------------------------------------------------------------------------------------ forward
def attention_fwd_ref(q, k, v, scale, gate=None):
    """o (or og = o s), lse and their bounds for bf16 q, k, v [B, N, H, D]; gate: the bf16 factors s [B N, >= 64] (D = 64).
    Returns (o, bound_o, lse, bound_lse), o in token-major layout."""
    B, N, H, D = q.shape
    o = torch.empty(B, N, H, D, dtype=F64, device=q.device)
    bo = torch.empty_like(o)
    lse = torch.empty(B, H, N, dtype=F64, device=q.device)
    blse = torch.empty_like(lse)
    for b0, b1 in slices(B, H * N * N):
        qh, kh, vh = _heads(q[b0:b1]), _heads(k[b0:b1]), _heads(v[b0:b1])
        s = scale * qh @ kh.transpose(-1, -2)
        l = torch.logsumexp(s, -1)
        p = torch.exp(s - l[..., None])
        oh = p @ vh
        mag = p @ vh.abs()
        if gate is not None:
            sg = gate[b0 * N:b1 * N, :64].to(F64).reshape(b1 - b0, 1, N, 64)
            oh, mag = oh * sg, mag * sg
        o[b0:b1] = _tok(oh)
        bo[b0:b1] = _tok(2 * U * mag + U * oh.abs())
        lse[b0:b1] = l
        kmax = kh.norm(dim=-1).amax(-1, keepdim=True)
        blse[b0:b1] = LSE_C * (l.abs() + scale * qh.norm(dim=-1) * kmax)
    return o, bo, lse, blse


# ----------------------------------------------------------------------------------------------------------- backward
def attention_bwd_ref(dout, q, k, v, lse, delta, scale, need=("dq", "dk", "dv")):
    """Teacher-forced attention backward: P = exp(scale q k^T - lse) with the kernel's lse, dS = P (dout v^T - delta).  ``delta``
    [B, H, N] (e.g. <dout, o> of the kernel's own o).  Returns {name: (ref [B, N, H, D], error bound without output rounding)}."""
    B, N, H, D = q.shape
    out = {n: (torch.empty(B, N, H, D, dtype=F64, device=q.device), torch.empty(B, N, H, D, dtype=F64, device=q.device)) for n in need}
    for b0, b1 in slices(B, 2 * H * N * N):
        qh, kh, vh, dh = _heads(q[b0:b1]), _heads(k[b0:b1]), _heads(v[b0:b1]), _heads(dout[b0:b1])
        p = torch.exp(scale * qh @ kh.transpose(-1, -2) - lse[b0:b1].to(F64)[..., None])
        ds = p * (dh @ vh.transpose(-1, -2) - delta[b0:b1].to(F64)[..., None])
        # |dS| plus the fp32 error of dP - delta (both sums of |dO| |v|-sized terms; |o| <= sum_j p_j |v_j|): where they cancel
        # (N = 1: dP = delta exactly) the kernel's difference is rounding noise, not zero
        pa = dh.abs() @ vh.abs().transpose(-1, -2)
        dsa = 2 * U * ds.abs() + FP32_C * p * (pa + (p * pa).sum(-1, keepdim=True))
        res = {}
        if "dq" in need:
            res["dq"] = (scale * ds @ kh, scale * dsa @ kh.abs())
        if "dk" in need:
            res["dk"] = (scale * ds.transpose(-1, -2) @ qh, scale * dsa.transpose(-1, -2) @ qh.abs())
        if "dv" in need:
            pt = p.transpose(-1, -2)
            res["dv"] = (pt @ dh, 2 * U * pt @ dh.abs())
        for n, (r, e) in res.items():
            out[n][0][b0:b1] = _tok(r)
            out[n][1][b0:b1] = _tok(e)
    return out


def delta_ref(dout, o):
    """<dout_i, o_i> per (batch, head, token) -> [B, H, N] float64."""
    return (dout.to(F64) * o.to(F64)).sum(-1).permute(0, 2, 1)


# ---------------------------------------------------------------------------------------------------------- the gate
def gate_bwd_ref(dout, og, s):
    """Backward of og = o s (s [B N, >= 64] bf16 gate factors shared by the heads): (dattn, b_dattn, delta, b_delta, dlogit, b_dlogit);
    dout, og [B, N, H, 64] (dout may be float64 with its own allowance folded in by the caller)."""
    B, N, H, D = og.shape
    d, o = dout.to(F64), og.to(F64)
    sg = s[:, :64].to(F64).reshape(B, N, 1, 64)
    dattn = d * sg
    prod = d * o
    delta = prod.sum(-1).permute(0, 2, 1)
    bdelta = SUM_C * prod.abs().sum(-1).permute(0, 2, 1)
    acc = prod.sum(2)                                   # [B, N, 64]
    dlogit = (acc * (1 - sg[:, :, 0])).reshape(B * N, 64)
    bdlogit = U * dlogit.abs() + ((1 - sg[:, :, 0]).abs() * SUM_C * prod.abs().sum(2)).reshape(B * N, 64)
    return dattn, U * dattn.abs(), delta, bdelta, dlogit, bdlogit


# ------------------------------------------------------------------------------------------------- projection forward
def projection_ref(x, w, bias):
    """y = x W^T + b in float64 and its bf16 rounding with the one-ulp allowance: (y64, y_bf16_as_f64, step)."""
    x64, w64 = x.to(F64), w.to(F64)
    y = x64 @ w64.t()
    err = 2.0 ** -16 * (x64.abs() @ w64.abs().t())
    if bias is not None:
        y = y + bias.to(F64)
        err = err + 2.0 ** -24 * bias.to(F64).abs()
    yr, step = round_bf16(y, err)
    return y, yr, step


def rope(a, cos, sin):
    """Rotate the half-split head rows a [..., N, H, 64] by the token's (cos, sin) [N, 32]: (a0 c - a1 s, a0 s + a1 c)."""
    c, s = cos.to(F64)[:, None, :], sin.to(F64)[:, None, :]
    a0, a1 = a[..., :32], a[..., 32:]
    return torch.cat([a0 * c - a1 * s, a0 * s + a1 * c], -1)


def rope_t(g, cos, sin):
    """R^T g (inverse rotation)."""
    c, s = cos.to(F64)[:, None, :], sin.to(F64)[:, None, :]
    g0, g1 = g[..., :32], g[..., 32:]
    return torch.cat([g0 * c + g1 * s, g1 * c - g0 * s], -1)


def qknorm_ref(yr, step, w, cos, sin, eps):
    """One q or k block: yr, step [B, N, H, 64] (raw bf16 projection and its allowance), w [64] fp32 -> (qhat ref, bound, r [B, N, H],
    bound of r).  a = rnd(y r w) with its allowance, then the rotation and the output rounding."""
    w64 = w.to(F64)
    ms = yr.pow(2).mean(-1) + eps
    r = ms.rsqrt()
    br = r * (1e-6 + (yr.abs() * step).sum(-1) / (64 * ms))
    a64 = yr * r[..., None] * w64
    aerr = 2.0 ** -20 * a64.abs() + w64.abs() * (r[..., None] * step + yr.abs() * br[..., None])
    a, astep = round_bf16(a64, aerr)
    da = astep + aerr
    ref = rope(a, cos, sin)
    c, s = cos.to(F64)[:, None, :].abs(), sin.to(F64)[:, None, :].abs()
    prop = torch.cat([c * da[..., :32] + s * da[..., 32:], s * da[..., :32] + c * da[..., 32:]], -1)
    mag = torch.cat([c * a[..., :32].abs() + s * a[..., 32:].abs(), s * a[..., :32].abs() + c * a[..., 32:].abs()], -1)
    allow = prop + 2.0 ** -20 * mag
    return ref, U * (ref.abs() + allow) + allow, r, br


# ------------------------------------------------------------------------------------ RMS-norm + RoPE backward (fused)
def norm_rope_bwd_ref(g, bg, yraw, ystep, yhat, w, cos, sin, eps):
    """Gradient of the raw projection head rows from the gradient g [B, N, H, 64] of the rotated normalised rows (bound bg), the
    RAW rows yraw (bf16 values, allowance ystep), the saved bf16 rotated rows yhat and the fp32 weights w [64].
    Returns (ref, bound without output rounding)."""
    w64 = w.to(F64)
    yh = yhat.to(F64)
    ms = yraw.pow(2).mean(-1, keepdim=True) + eps
    r = ms.rsqrt()
    n = yraw * r
    u = rope_t(g, cos, sin)
    dn = w64 * u
    cc = (dn * n).sum(-1, keepdim=True) / 64
    ref = r * (dn - n * cc)
    c, s = cos.to(F64)[:, None, :].abs(), sin.to(F64)[:, None, :].abs()
    swap = lambda t: torch.cat([t[..., 32:], t[..., :32]], -1)   # the rotary partner channel
    cs = torch.cat([c, c], -1)
    sn = torch.cat([s, s], -1)
    cc_abs = (g.abs() * yh.abs()).sum(-1, keepdim=True) / 64
    u_abs = cs * g.abs() + sn * swap(g.abs())
    carried = r * (w64.abs() * (cs * bg + sn * swap(bg)) + n.abs() * (yh.abs() * bg).sum(-1, keepdim=True) / 64)
    rebuilt = U * r * cc_abs * (n.abs() + (yh.abs() + swap(yh.abs())) / w64.abs())
    fp32 = SUM_C * r * (w64.abs() * u_abs + n.abs() * cc_abs)
    dn_abs = w64.abs() * u_abs
    raw = r * r * (ystep * cc_abs + n.abs() * (dn_abs * ystep).sum(-1, keepdim=True) / 64) * 2
    return ref, carried + rebuilt + fp32 + raw


def dlam_ref(dyv, lam, vdiff):
    """d lambda = sum dv (v_raw - v0) from the kernel's own value gradient dv = dy_v / lam: (ref, bound), both shape [1]."""
    dv = dyv.to(F64) / lam
    t = dv * vdiff.to(F64)
    return t.sum().reshape(1), (SUM_C * t.abs().sum() + U * t.abs().sum()).reshape(1)
