"""CPU: the float64 references and error bounds of tests/attention_reference.py (used by tests/test_attention_ops_gpu.py) against
an emulation of the attention kernels' rounding at small shapes.  The correct emulation must pass every bound; each injected
defect must be rejected by at least one of them -- so the bounds' sensitivity is checked on machines without a GPU.

Emulation (fp32 arithmetic, bf16 rounding where csrc/vsde_attn.hip rounds):
  forward   scores in fp32, p = exp(scale (s - max)), the row sum from the fp32 p, P rounded to bf16 for the PV product,
            o = rnd(PV / sum), lse = scale max + log(sum)
  backward  P = exp(scale s - lse), delta = <dO, o>, dS = P (dO v^T - delta); dq = rnd(scale rnd(dS) k), dk = rnd(scale
            rnd(dS)^T q), dv = rnd(rnd(P)^T dO)
  QK-norm   forward a = rnd(y r w), yhat = rnd(R a); backward (staged_norm_rope_bwd) u = R^T g, cc = <g, yhat> / 64,
            dy = rnd(r (w u - (R^T yhat) cc / w))
  d lambda  sum dv (v_raw - v0) in fp32 over the values' gradient dv
Defects: lse + 0.03; the ragged last key tile dropped; the - delta missing for the first query block; a RoPE sign flip in the
second half of the inverse rotation; the inverse RMS of the next head; d lambda off by 1 %.
"""
import pytest
import torch

import attention_reference as ar

F32, F64, BF = torch.float32, torch.float64, torch.bfloat16
B, N, H, D = 2, 45, 2, 64          # two key tiles, the last one ragged (13 keys)
SCALE = D ** -0.5
EPS = 1e-6
DEFECTS = [None, "lse", "ragged", "delta", "rope", "rinv", "dlam"]


def rb(t):
    return t.to(BF).to(F32)


def _heads(t):
    return t.to(F32).permute(0, 2, 1, 3)


def _tok(t):
    return t.permute(0, 2, 1, 3)


def emu_fwd(q, k, v, defect):
    qh, kh, vh = _heads(q), _heads(k), _heads(v)
    s = qh @ kh.transpose(-1, -2)
    if defect == "ragged":
        s[..., (N // 32) * 32:] = -float("inf")
    mx = s.amax(-1, keepdim=True)
    p = torch.exp(SCALE * (s - mx))
    l = p.sum(-1, keepdim=True)
    o = rb((rb(p) @ vh) / l)
    lse = (SCALE * mx + torch.log(l))[..., 0]
    if defect == "lse":
        lse = lse + 0.03
    return _tok(o).to(BF), lse


def emu_bwd(dout, q, k, v, o, lse, defect):
    qh, kh, vh, dh, oh = (_heads(t) for t in (q, k, v, dout, o))
    p = torch.exp(SCALE * qh @ kh.transpose(-1, -2) - lse[..., None])
    delta = (dh * oh).sum(-1, keepdim=True)
    dp = dh @ vh.transpose(-1, -2)
    ds = p * (dp - delta)
    if defect == "delta":
        ds[:, :, :32] = (p * dp)[:, :, :32]
    dq = rb(SCALE * rb(ds) @ kh)
    dk = rb(SCALE * rb(ds).transpose(-1, -2) @ qh)
    dv = rb(rb(p).transpose(-1, -2) @ dh)
    return [_tok(t).to(BF) for t in (dq, dk, dv)]


def _rope(a, c, s):
    return torch.cat([a[..., :32] * c - a[..., 32:] * s, a[..., :32] * s + a[..., 32:] * c], -1)


def emu_qknorm(y, w, cos, sin):
    """(yhat bf16, r fp32 [B, N, H]) from the raw bf16 rows y [B, N, H, 64]."""
    yf = y.to(F32)
    r = torch.rsqrt(yf.pow(2).mean(-1) + EPS)
    a = rb(yf * r[..., None] * w)
    c, s = cos[:, None, :], sin[:, None, :]
    return _rope(a, c, s).to(BF), r


def emu_norm_bwd(g, yhat, r, w, cos, sin, defect):
    c, s = cos[:, None, :], sin[:, None, :]
    g0, g1 = g[..., :32], g[..., 32:]
    y = yhat.to(F32)
    y0, y1 = y[..., :32], y[..., 32:]
    u = torch.cat([g0 * c + g1 * s, (g1 * c + g0 * s) if defect == "rope" else (g1 * c - g0 * s)], -1)
    a = torch.cat([y0 * c + y1 * s, y1 * c - y0 * s], -1)
    cc = (g * y).sum(-1, keepdim=True) / 64
    rr = torch.roll(r, 1, dims=-1) if defect == "rinv" else r
    return rb(rr[..., None] * (w * u - a * (cc / w))).to(BF)


def _inputs(seed):
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s, scale=1.0: (torch.randn(*s, generator=g, dtype=F64) * scale).to(BF)
    q, k, v, dout = rnd(B, N, H, D), rnd(B, N, H, D), rnd(B, N, H, D), rnd(B, N, H, D)
    # raw projection rows: the heads at different magnitudes (their inverse RMS differ by 2x)
    y = rnd(B, N, H, 64) * torch.tensor([1.0, 2.0], dtype=BF).view(1, 1, H, 1)
    w = (1 + 0.3 * torch.randn(64, generator=g, dtype=F64)).to(F32)
    ang = torch.arange(N, dtype=F64)[:, None] * (10000.0 ** (-torch.arange(32, dtype=F64) / 32))[None]
    cos, sin = ang.cos().to(F32), ang.sin().to(F32)
    return q, k, v, dout, y, w, cos, sin


def _fails(got, ref, bound):
    return ar.excess(got, ref, bound)[0] > 0


def _run_checks(defect, seed=0):
    """{check name: rejected?} of the emulation with ``defect``."""
    q, k, v, dout, y, w, cos, sin = _inputs(seed)
    out = {}
    o, lse = emu_fwd(q, k, v, defect)
    ref, bo, lref, bl = ar.attention_fwd_ref(q, k, v, SCALE)
    out["o"] = _fails(o, ref, bo)
    out["lse"] = _fails(lse, lref, bl)
    dq, dk, dv = emu_bwd(dout, q, k, v, o, lse, defect)
    refs = ar.attention_bwd_ref(dout, q, k, v, lse, ar.delta_ref(dout, o), SCALE)
    for name, t in (("dq", dq), ("dk", dk), ("dv", dv)):
        r_, e = refs[name]
        out[name] = _fails(t, r_, e + ar.U * r_.abs())
    # fused QK-norm backward: g is the (unrounded) gradient of the rotated rows, exact here up to fp32
    yhat, r = emu_qknorm(y, w, cos, sin)
    gq = refs["dq"][0]
    dy = emu_norm_bwd(gq.to(F32), yhat, r, w, cos, sin, defect)
    ref, bound = ar.norm_rope_bwd_ref(gq, 1e-7 * gq.abs(), y.to(F64), torch.zeros_like(gq), yhat, w, cos, sin, EPS)
    out["dy_q"] = _fails(dy, ref, bound + ar.U * ref.abs())
    # d lambda over value gradients correlated with v_raw - v0 (a sum that does not cancel)
    lam = 0.37
    dvf = refs["dv"][0].to(F32)
    vdiff = (dvf + 0.3 * torch.randn(dvf.shape, generator=torch.Generator().manual_seed(seed + 1))).to(BF)
    dyv = rb(lam * dvf).to(BF)
    dl = (dvf * vdiff.to(F32)).sum()
    if defect == "dlam":
        dl = dl * 1.01
    ref, bound = ar.dlam_ref(dyv, lam, vdiff)
    out["dlam"] = _fails(dl.reshape(1), ref, bound)
    return out


def test_correct_emulation_passes_every_bound():
    for seed in range(3):
        res = _run_checks(None, seed)
        assert not any(res.values()), (seed, res)


@pytest.mark.parametrize("defect,check", [("lse", "lse"), ("ragged", "o"), ("delta", "dq"), ("rope", "dy_q"),
                                          ("rinv", "dy_q"), ("dlam", "dlam")])
def test_injected_defect_is_rejected(defect, check):
    res = _run_checks(defect)
    assert res[check], (defect, res)


def test_norm_weight_limit():
    """The fused core admits RMS weights down to max|w| / NORM_WEIGHT_RATIO and refuses anything smaller (or zero)."""
    from viforsdes_amd.primitives import fused
    w = torch.ones(64)
    assert fused.norm_weights_fusable(w)
    assert fused.norm_weights_fusable(1 + 0.3 * torch.randn(64, generator=torch.Generator().manual_seed(0)).clamp(-2, 2))
    lim = float(w.max()) / fused.NORM_WEIGHT_RATIO
    for val, ok in ((lim, True), (-lim, True), (lim * 0.999, False), (-1e-2, False), (1e-3, False), (0.0, False)):
        w2 = w.clone()
        w2[17] = val
        assert fused.norm_weights_fusable(w2) == ok, (val, ok)
    w3 = w.clone() * 3.0
    w3[3] = -3.0 / fused.NORM_WEIGHT_RATIO   # relative to the maximum, not to 1
    assert fused.norm_weights_fusable(w3)
    w3[3] = -2.9 / fused.NORM_WEIGHT_RATIO
    assert not fused.norm_weights_fusable(w3)
