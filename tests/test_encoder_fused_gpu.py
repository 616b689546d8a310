"""GPU parity of the fused encoder operators against the unfused torch chains (which themselves are
pinned against the reference's encoder by tests/test_host_logic.py::test_encoder_matches_reference...).

fp32: forward 2e-5, gradients 2e-4 (relative to max).  bf16: both sides round at different points,
tolerance 3e-2 relative to max (bf16 eps = 7.8e-3)."""
import numpy as np
import pytest
import torch

from helpers import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _block(dim=128, heads=4, cond=32, residual_v=True, seed=0):
    from viforsdes_amd.primitives.sit import SiTBlock
    torch.manual_seed(seed)
    blk = SiTBlock(dim=dim, num_heads=heads, mlp_hidden_dim=int(dim * 8 / 3), cond_dim=cond, attn_residual_v=residual_v).to(DEV)
    with torch.no_grad():
        for n, p in blk.named_parameters():
            if p.requires_grad and (p.abs().sum() == 0 or "lambda" in n):
                p.add_(torch.randn_like(p) * 0.2)
    return blk


def _run(blk, x, cond, rot, v0, fused_on, dtype):
    from viforsdes_amd.primitives import fused
    fused.ENABLED = fused_on
    try:
        xs = x.clone().requires_grad_(True); cs = cond.clone().requires_grad_(True)
        v0s = v0.clone().requires_grad_(True) if v0 is not None else None
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=dtype == torch.bfloat16):
            xin = xs.to(dtype) if dtype == torch.bfloat16 else xs
            out, vals = blk(xin, cond=cs, rotary=rot, v0=v0s.to(dtype) if v0s is not None and dtype == torch.bfloat16 else v0s)
        g = torch.Generator(device="cpu").manual_seed(1)
        go = torch.randn(out.shape, generator=g).to(DEV)
        gv = torch.randn(vals.shape, generator=g).to(DEV)
        loss = (out.float() * go).sum() + (vals.float() * gv).sum()
        params = [p for p in blk.parameters() if p.requires_grad]
        grads = torch.autograd.grad(loss, [xs, cs] + ([v0s] if v0s is not None else []) + params)
        return out.float().detach(), vals.float().detach(), grads
    finally:
        fused.ENABLED = True


@pytest.mark.parametrize("dtype,ftol,gtol", [(torch.float32, 2e-5, 2e-4), (torch.bfloat16, 3e-2, 6e-2)])
@pytest.mark.parametrize("residual_v", [False, True])
def test_fused_block_matches_unfused(dtype, ftol, gtol, residual_v):
    from viforsdes_amd.primitives.embeddings import RotarySpec, precompute_freq_cis
    B, N, C, h = 3, 37, 128, 4
    blk = _block(C, h, 32, residual_v)
    g = torch.Generator().manual_seed(4)
    x = torch.randn(B, N, C, generator=g).to(DEV)
    cond = torch.randn(B, 32, generator=g).to(DEV)
    v0 = torch.randn(B, h, N, C // h, generator=g).to(DEV) if residual_v else None
    rot = RotarySpec.from_freqs(precompute_freq_cis(C // h, end=64).to(DEV)[:N])
    o1, v1, g1 = _run(blk, x, cond, rot, v0, False, dtype)
    o2, v2, g2 = _run(blk, x, cond, rot, v0, True, dtype)
    assert rel_err(o2.cpu().numpy(), o1.cpu().numpy()) < ftol
    assert rel_err(v2.cpu().numpy(), v1.cpu().numpy()) < ftol
    names = ["x", "cond"] + (["v0"] if residual_v else []) + [n for n, p in blk.named_parameters() if p.requires_grad]
    for n, a, b_ in zip(names, g2, g1):
        assert rel_err(a.float().cpu().numpy(), b_.float().cpu().numpy()) < gtol, n


def test_fused_ops_individually_fp32():
    from viforsdes_amd.primitives import fused
    g = torch.Generator().manual_seed(2)
    rn = lambda *s: torch.randn(*s, generator=g).to(DEV)
    B, N, C = 4, 19, 256
    x, sc, sh, gate, y = rn(B, N, C).requires_grad_(), rn(B, C).requires_grad_(), rn(B, C).requires_grad_(), rn(B, C).requires_grad_(), rn(B, N, C).requires_grad_()
    ref = torch.nn.functional.layer_norm(x, (C,), eps=1e-5) * (1 + sc[:, None]) + sh[:, None]
    got = fused.ln_modulate(x, sc, sh, 1e-5)
    assert torch.allclose(got, ref, rtol=1e-5, atol=1e-5)
    go = rn(B, N, C)
    for a, b_ in zip(torch.autograd.grad((got * go).sum(), [x, sc, sh]), torch.autograd.grad((ref * go).sum(), [x, sc, sh])):
        assert rel_err(a.cpu().numpy(), b_.cpu().numpy()) < 1e-5
    ref = x + gate[:, None] * y
    got = fused.gated_residual(x, y, gate)
    assert torch.allclose(got, ref, rtol=1e-6, atol=1e-6)
    for a, b_ in zip(torch.autograd.grad((got * go).sum(), [x, y, gate]), torch.autograd.grad((ref * go).sum(), [x, y, gate])):
        assert rel_err(a.cpu().numpy(), b_.cpu().numpy()) < 1e-5
    u = rn(B, N, 2 * 170).requires_grad_()
    a_, b2 = u.chunk(2, -1)
    ref = torch.nn.functional.silu(a_) * b2
    got = fused.swiglu(u)
    assert torch.allclose(got, ref, rtol=1e-5, atol=1e-6)
    go2 = rn(B, N, 170)
    assert rel_err(torch.autograd.grad((got * go2).sum(), u)[0].cpu().numpy(), torch.autograd.grad((ref * go2).sum(), u)[0].cpu().numpy()) < 1e-5


def test_encoder_fused_vs_unfused_full_module_bf16_autocast():
    """Whole ObservationContextEncoder at the benchmark width (C=256, 4 heads) under bf16 autocast."""
    from viforsdes_amd import EncoderConfig
    from viforsdes_amd.models.encoder import ObservationContextEncoder
    from viforsdes_amd.primitives import fused
    torch.manual_seed(0)
    enc = ObservationContextEncoder(2, 3, EncoderConfig(hidden_dim=256, num_heads=4, depth=2)).to(DEV)
    with torch.no_grad():
        for n, p in enc.named_parameters():
            if p.requires_grad and p.abs().sum() == 0:
                p.add_(torch.randn_like(p) * 0.05)
    obs_t, obs_v = torch.tensor([0.0, 1.0, 2.0], device=DEV), torch.randn(3, 2, device=DEV)
    theta = torch.rand(6, 3, device=DEV) + 0.2
    outs = []
    for on in (False, True):
        fused.ENABLED = on
        with torch.autocast("cuda", dtype=torch.bfloat16):
            outs.append(enc(obs_v, obs_t, theta, 2.0, 0.05).float().detach())
    fused.ENABLED = True
    assert outs[0].shape == (6, 41, 256)
    assert rel_err(outs[1].cpu().numpy(), outs[0].cpu().numpy()) < 3e-2


def test_nograd_block_kernel_routes_agree_and_follow_the_optimizer():
    """Posterior sampling at >= 32768 token rows runs each block's second half -- and the attention branch's gate + out projection --
    as ONE kernel (csrc/vsde_mlp.hip block forms).  Whole encoder, bf16 autocast, no grad: the three routes (separate kernels |
    block form | block form with the out projection) agree to bf16 round-off, and after a parameter update followed by the trainer's
    pack refresh (which is all a captured step replays) every route sees the new weights through its derived tile images."""
    from viforsdes_amd import EncoderConfig
    from viforsdes_amd.models.encoder import ObservationContextEncoder
    from viforsdes_amd.primitives import fused
    torch.manual_seed(0)
    enc = ObservationContextEncoder(2, 3, EncoderConfig(hidden_dim=256, num_heads=4, depth=2)).to(DEV)
    with torch.no_grad():
        for n, p in enc.named_parameters():
            if p.requires_grad and p.abs().sum() == 0:
                p.add_(torch.randn_like(p) * 0.05)
    obs_t, obs_v = torch.tensor([0.0, 1.0, 2.0, 4.0], device=DEV), torch.randn(4, 2, device=DEV)
    theta = torch.rand(400, 3, device=DEV) + 0.2   # 400 x 101 tokens = 40400 rows

    def run(block, outp):
        old = fused.BLOCK_MLP, fused.BLOCK_OUT_PROJ
        fused.BLOCK_MLP, fused.BLOCK_OUT_PROJ = block, outp
        try:
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
                return enc(obs_v, obs_t, theta, 5.0, 0.05).float()
        finally:
            fused.BLOCK_MLP, fused.BLOCK_OUT_PROJ = old

    calls = {"block": 0, "attn_block": 0}
    from viforsdes_amd import _hip
    real = _hip.mlp_block_fwd, _hip.mlp_attn_block_fwd

    def spy(name, fn):
        def wrapped(*a, **k):
            calls[name] += 1
            return fn(*a, **k)
        return wrapped
    _hip.mlp_block_fwd, _hip.mlp_attn_block_fwd = spy("block", real[0]), spy("attn_block", real[1])
    try:
        base = run(False, False)
        assert calls == {"block": 0, "attn_block": 0}
        blk = run(True, False)
        assert calls == {"block": 2, "attn_block": 0}          # one launch per block (depth 2)
        both = run(True, True)
        assert calls == {"block": 2, "attn_block": 2}
    finally:
        _hip.mlp_block_fwd, _hip.mlp_attn_block_fwd = real
    assert base.shape == (400, 101, 256) and torch.isfinite(both).all()
    assert rel_err(blk.cpu().numpy(), base.cpu().numpy()) < 2e-2
    assert rel_err(both.cpu().numpy(), blk.cpu().numpy()) < 2e-2
    params = [p for p in enc.parameters() if p.requires_grad]
    with torch.no_grad():
        for p in params:
            p.mul_(0.7)
    fused.note_parameters_changed()
    fused.PackedWeight.refresh_all(force=True, params={id(p) for p in params})
    base2, both2 = run(False, False), run(True, True)
    assert rel_err(both2.cpu().numpy(), base2.cpu().numpy()) < 2e-2
    assert rel_err(base2.cpu().numpy(), base.cpu().numpy()) > 5e-2


@pytest.mark.parametrize("M,N,K", [(8192 + 37, 768, 256), (5000, 64, 256), (4100, 256, 768), (20000, 1536, 256), (4096, 8, 16),
                                   # tile counts that underfill one round of workgroups: finer splits in several rounds
                                   (20000 + 13, 2816, 512), (9000, 512, 1408)])
def test_linear_wgrad_kernel(M, N, K):
    """dW = dy^T x, db = colsum(dy): bf16 inputs, fp32 accumulation; reference in float64 on the same bf16 values."""
    from viforsdes_amd import _hip
    g = torch.Generator().manual_seed(M)
    dy = torch.randn(M, N, generator=g).to(torch.bfloat16).to(DEV)
    x = torch.randn(M, K, generator=g).to(torch.bfloat16).to(DEV)
    dW, db = _hip.linear_wgrad(dy, x, True)
    ref_w = dy.double().t() @ x.double()
    ref_b = dy.double().sum(0)
    assert rel_err(dW.cpu().numpy(), ref_w.cpu().numpy()) < 2e-5
    assert rel_err(db.cpu().numpy(), ref_b.cpu().numpy()) < 2e-5
    dW2, none = _hip.linear_wgrad(dy, x, False)
    assert none is None and torch.equal(dW, dW2)  # deterministic


def test_fused_linear_autograd_matches_f_linear():
    from viforsdes_amd.primitives import fused
    g = torch.Generator().manual_seed(9)
    x = torch.randn(6, 700, 256, generator=g).to(torch.bfloat16).to(DEV).requires_grad_()
    w = (torch.randn(768, 256, generator=g) * 0.05).to(DEV).requires_grad_()
    b = (torch.randn(768, generator=g) * 0.05).to(DEV).requires_grad_()
    go = torch.randn(6, 700, 768, generator=g).to(DEV)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y1 = fused.linear(x, w, b)
        y2 = torch.nn.functional.linear(x, w, b)
    assert y1.dtype == torch.bfloat16 and torch.equal(y1, y2)
    g1 = torch.autograd.grad((y1.float() * go).sum(), [x, w, b])
    g2 = torch.autograd.grad((y2.float() * go).sum(), [x, w, b])
    assert rel_err(g1[0].float().cpu().numpy(), g2[0].float().cpu().numpy()) < 1e-2
    assert rel_err(g1[1].cpu().numpy(), g2[1].cpu().numpy()) < 1e-2   # torch's own wgrad is rounded to bf16
    assert rel_err(g1[2].cpu().numpy(), g2[2].cpu().numpy()) < 1e-2
    assert g1[1].dtype == torch.float32


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_head_layouts_agree(dtype):
    """qk_norm_rope / gate_merge give the same values in the [B,h,N,d] and the token-major [B,N,h,d] layout."""
    from viforsdes_amd.primitives import fused
    g = torch.Generator().manual_seed(5)
    rn = lambda *s: torch.randn(*s, generator=g).to(DEV, dtype)
    B, N, h, d = 3, 21, 4, 64
    ang = torch.arange(N, device=DEV, dtype=torch.float32)[:, None] * torch.linspace(0.1, 1.0, d // 2, device=DEV)
    cos, sin = torch.cos(ang).contiguous(), torch.sin(ang).contiguous()
    wq, wk = (1 + 0.1 * rn(d)).float(), (1 + 0.1 * rn(d)).float()
    qkv0, v00, glog0 = rn(B, N, 3 * h * d), rn(B, h, N, d), rn(B, N, d)
    outs = {}
    for tm in (False, True):
        qkv, v0, glog = (t.clone().requires_grad_() for t in (qkv0, v00, glog0))
        lam = torch.tensor(0.7, device=DEV, requires_grad=True)
        v0_in = v0.transpose(1, 2).contiguous() if tm else v0
        q, k, v = fused.qk_norm_rope(qkv, cos, sin, wq, wk, v0_in, lam, h, 1e-6, token_major=tm)
        a = q * 0.5 + k * 0.25 + v  # stand-in for attention, same layout as its inputs
        merged = fused.gate_merge(a, glog, token_major=tm)
        go = torch.linspace(-1, 1, merged.numel(), device=DEV).reshape(merged.shape)
        grads = torch.autograd.grad((merged.float() * go).sum(), [qkv, v0, glog, lam])
        std = (lambda t: t.transpose(1, 2)) if tm else (lambda t: t)
        outs[tm] = [std(q), std(k), std(v), merged, *grads[:3]]
        lam_grad = grads[3]
        outs[tm].append(lam_grad)
    for a, b_ in zip(outs[False][:-1], outs[True][:-1]):
        assert torch.equal(a.contiguous(), b_.contiguous())
    # d(lambda) is a block-partial sum whose grouping follows the layout
    assert abs(float(outs[False][-1]) - float(outs[True][-1])) <= 1e-3 * (1 + abs(float(outs[False][-1])))


@pytest.mark.parametrize("C", [64, 128, 192, 256, 384, 512, 768, 1024])
@pytest.mark.parametrize("dtype,tol", [(torch.float32, 2e-5), (torch.bfloat16, 2e-2)])
def test_ln_modulate_and_gated_residual_channel_counts(C, dtype, tol):
    """Every vector-width / lanes-per-token dispatch of the norm and residual kernels, incl. the fused column sums and the
    residual-gradient hand-off (GradLink), against the torch chain evaluated in fp32."""
    from viforsdes_amd.primitives import fused
    g = torch.Generator().manual_seed(C)
    rn = lambda *s: torch.randn(*s, generator=g).to(DEV, dtype)
    B, N = 3, 37
    leaves = [rn(B, N, C), rn(B, C) * 0.3, rn(B, C) * 0.3, rn(B, C), rn(B, N, C)]
    go = rn(B, N, C).float()

    def run(use_fused):
        x, sc, sh, gate, w = (t.clone().float().requires_grad_() if not use_fused else t.clone().requires_grad_() for t in leaves)
        if use_fused:
            link = fused.GradLink()
            h = fused.ln_modulate(x, sc, sh, 1e-5, link)
            out = fused.gated_residual(x, h * w, gate, link)
        else:
            h = torch.nn.functional.layer_norm(x, (C,), eps=1e-5) * (1 + sc[:, None]) + sh[:, None]
            out = x + gate[:, None] * (h * w)
        grads = torch.autograd.grad((out.float() * go).sum(), [x, sc, sh, gate, w])
        return [out.detach().float()] + [t.float() for t in grads]

    for name, a, b_ in zip(["out", "dx", "dscale", "dshift", "dgate", "dw"], run(True), run(False)):
        assert rel_err(a.cpu().numpy(), b_.cpu().numpy()) < tol, name


@pytest.mark.parametrize("B,N,H", [(2, 1, 2), (2, 31, 4), (3, 32, 1), (2, 101, 4), (2, 401, 4), (1, 544, 2)])
def test_attention_kernel_vs_fp32_softmax(B, N, H):
    """vsde_attention_fwd_bf16 (token-major, K/V resident in LDS) vs an fp32 softmax(q k^T) v of the same bf16 inputs; the
    backward (library kernel fed with our output and log-sum-exp) vs autograd through the fp32 chain."""
    from viforsdes_amd import _hip
    from viforsdes_amd.primitives import fused
    g = torch.Generator().manual_seed(N)
    q, k, v = (torch.randn(B, N, H, 64, generator=g).to(DEV, torch.bfloat16).requires_grad_() for _ in range(3))
    go = torch.randn(B, N, H, 64, generator=g).to(DEV, torch.bfloat16)
    assert fused.attention_usable(q)
    o = fused.attention(q, k, v, 0.125)
    dq, dk, dv = torch.autograd.grad((o.float() * go.float()).sum(), [q, k, v])
    qf, kf, vf = (t.detach().float().transpose(1, 2).requires_grad_() for t in (q, k, v))
    s = (qf @ kf.transpose(-1, -2)) * 0.125
    ref = (torch.softmax(s, -1) @ vf).transpose(1, 2)
    rq, rk, rv = torch.autograd.grad((ref * go.float()).sum(), [qf, kf, vf])
    assert rel_err(o.detach().float().cpu().numpy(), ref.detach().cpu().numpy()) < 1e-2
    _, lse = _hip.attention_fwd(q.detach(), k.detach(), v.detach(), 0.125)
    assert torch.allclose(lse, torch.logsumexp(s.detach(), -1), atol=1e-4, rtol=1e-5)
    for a, r in ((dq, rq), (dk, rk), (dv, rv)):  # absolute floor: at N = 1 dq and dk are exactly 0
        a, r = a.float().cpu().numpy(), r.transpose(1, 2).cpu().numpy()
        assert np.abs(a - r).max() <= 2e-2 * np.abs(r).max() + 1e-2


@pytest.mark.parametrize("B,N,H", [(150, 401, 4), (300, 37, 2), (131, 416, 4), (140, 385, 4), (600, 101, 1)])
def test_persistent_attention_forward_many_pairs(B, N, H):
    """>= 2 (batch, head) pairs per CU and at most 13 query blocks: the forward runs as persistent workgroups that walk the pairs
    and request the next pair's K / V behind the current pair's last query block (attn_fwd_kernel<true>).  Against the
    one-workgroup-per-pair kernel (VSDE_ATTN_PERSIST=0 in a child process would be another library load: compared with the fp32
    softmax instead, per pair, plus the gated store)."""
    from viforsdes_amd import _hip
    g = torch.Generator().manual_seed(B + N)
    q, k, v = (torch.randn(B, N, H, 64, generator=g).to(DEV, torch.bfloat16) for _ in range(3))
    o, lse = _hip.attention_fwd(q, k, v, 0.125)
    gate = torch.sigmoid(torch.randn(B * N, 64, generator=g)).to(DEV, torch.bfloat16)
    og, lse_g = _hip.attention_fwd_gated(q, k, v, gate, 0.125)
    assert torch.equal(lse, lse_g)
    for b0 in range(0, B, 50):   # fp32 reference in slices (memory)
        qf, kf, vf = (t[b0:b0 + 50].float().transpose(1, 2) for t in (q, k, v))
        s = (qf @ kf.transpose(-1, -2)) * 0.125
        ref = (torch.softmax(s, -1) @ vf).transpose(1, 2)
        assert rel_err(o[b0:b0 + 50].float().cpu().numpy(), ref.cpu().numpy()) < 1e-2, b0
        assert torch.allclose(lse[b0:b0 + 50], torch.logsumexp(s, -1), atol=1e-4, rtol=1e-5), b0
        refg = ref * gate[b0 * N:(b0 + 50) * N].float().view(-1, N, 1, 64)
        assert rel_err(og[b0:b0 + 50].float().cpu().numpy(), refg.cpu().numpy()) < 1e-2, b0


def test_attention_kernel_large_scores_take_the_exact_path():
    """|q||k| scale far above the Cauchy-Schwarz-shift limit: the kernel must fall back to true row maxima (no NaN/underflow)."""
    from viforsdes_amd import _hip
    g = torch.Generator().manual_seed(3)
    q, k, v = (torch.randn(2, 77, 2, 64, generator=g).to(DEV, torch.bfloat16) for _ in range(3))
    q, k = q * 6, k * 6
    o, lse = _hip.attention_fwd(q, k, v, 0.125)
    qf, kf, vf = (t.float().transpose(1, 2) for t in (q, k, v))
    s = (qf @ kf.transpose(-1, -2)) * 0.125
    ref = (torch.softmax(s, -1) @ vf).transpose(1, 2)
    assert torch.isfinite(o.float()).all() and torch.isfinite(lse).all()
    assert rel_err(o.float().cpu().numpy(), ref.cpu().numpy()) < 1e-2
    assert torch.allclose(lse, torch.logsumexp(s, -1), atol=1e-3, rtol=1e-5)


def test_packed_weights_follow_parameter_updates():
    """PackedWeight (cached bf16 GEMM operands) must never serve stale weights: in-place parameter updates are picked up
    lazily (version check) and by refresh_all(); gradients come back per parameter piece."""
    from viforsdes_amd.primitives import fused
    from viforsdes_amd.primitives.mlp import SwiGLU
    torch.manual_seed(0)
    mlp = SwiGLU(256, 682).to(DEV)
    x = torch.randn(16, 300, 256, device=DEV, dtype=torch.bfloat16)

    def reference(inp):
        with torch.autocast("cuda", dtype=torch.bfloat16):
            a, b_ = mlp.input_proj(inp).chunk(2, dim=-1)
            return mlp.output_proj(torch.nn.functional.silu(a) * b_)

    with torch.autocast("cuda", dtype=torch.bfloat16):
        y0 = mlp(x)
    assert hasattr(mlp, "_packs"), "large bf16 inputs should take the packed route"
    assert rel_err(y0.float().detach().cpu().numpy(), reference(x).float().detach().cpu().numpy()) < 3e-2
    with torch.no_grad():  # optimizer-style in-place update, no explicit refresh: the version check must catch it
        mlp.input_proj.weight.mul_(0.5)
        mlp.output_proj.bias.add_(1.0)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y1 = mlp(x)
    assert rel_err(y1.float().detach().cpu().numpy(), reference(x).float().detach().cpu().numpy()) < 3e-2
    assert (y1 - y0).abs().max() > 0.5
    with torch.no_grad():
        mlp.output_proj.weight.mul_(2.0)
    assert any(pk.stale() for pk in mlp._packs)
    fused.PackedWeight.refresh_all()
    assert not any(pk.stale() for pk in mlp._packs)
    xg = x.clone().requires_grad_()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y2 = mlp(xg)
    ref = reference(xg)
    assert rel_err(y2.float().detach().cpu().numpy(), ref.float().detach().cpu().numpy()) < 3e-2
    params = [mlp.input_proj.weight, mlp.input_proj.bias, mlp.output_proj.weight, mlp.output_proj.bias]
    go = torch.randn_like(y2)
    g_fused = torch.autograd.grad((y2.float() * go.float()).sum(), [xg] + params)
    g_ref = torch.autograd.grad((ref.float() * go.float()).sum(), [xg] + params)
    for name, a, b_ in zip(["x", "w_in", "b_in", "w_out", "b_out"], g_fused, g_ref):
        assert a.shape == b_.shape, name
        assert rel_err(a.float().cpu().numpy(), b_.float().cpu().numpy()) < 6e-2, name


@pytest.mark.parametrize("C", [64, 192, 256, 512])
@pytest.mark.parametrize("dtype,tol", [(torch.float32, 3e-5), (torch.bfloat16, 3e-2)])
def test_residual_norm_fused_op(C, dtype, tol):
    """gated residual fused with the following LayerNorm-modulate (forward and the five gradients, including the gradient
    that reaches xnew from another consumer) vs the torch chain in fp32."""
    from viforsdes_amd.primitives import fused
    g = torch.Generator().manual_seed(C + 1)
    rn = lambda *s: torch.randn(*s, generator=g).to(DEV, dtype)
    B, N = 3, 41
    leaves = [rn(B, N, C), rn(B, N, C), rn(B, C), rn(B, C) * 0.3, rn(B, C) * 0.3]
    go_x, go_h = rn(B, N, C).float(), rn(B, N, C).float()

    def run(use_fused):
        x, y, gate, sc, sh = (t.clone().requires_grad_() if use_fused else t.clone().float().requires_grad_() for t in leaves)
        if use_fused:
            xnew, h = fused.residual_norm(x, y, gate, sc, sh, 1e-5)
        else:
            xnew = x + gate[:, None] * y
            h = torch.nn.functional.layer_norm(xnew, (C,), eps=1e-5) * (1 + sc[:, None]) + sh[:, None]
        grads = torch.autograd.grad((xnew.float() * go_x).sum() + (h.float() * go_h).sum(), [x, y, gate, sc, sh])
        return [xnew.detach().float(), h.detach().float()] + [t.float() for t in grads]

    for name, a, b_ in zip(["xnew", "h", "dx", "dy", "dgate", "dscale", "dshift"], run(True), run(False)):
        assert rel_err(a.cpu().numpy(), b_.cpu().numpy()) < tol, name


@pytest.mark.parametrize("residual_v", [False, True])
@pytest.mark.parametrize("B,N", [(112, 37), (40, 130)])   # >= 4096 rows: below that the packed projection is not taken at all
def test_nograd_projection_kernel_matches_the_training_path(residual_v, B, N):
    """Posterior sampling (no grad) runs the [q | k | v | gate] projection with the QK-norm / RoPE / value-mix epilogue in ONE
    kernel (vsde_linear_qknorm_bf16); the training path runs the same arithmetic with the same rounding points as GEMM ->
    qk_norm_rope.  Same block, same inputs: outputs and value heads must agree to bf16 round-off (the RMS sums are formed in a
    different order, so a few elements may move by one bf16 ulp)."""
    from viforsdes_amd.primitives.embeddings import RotarySpec, precompute_freq_cis
    from viforsdes_amd.primitives import fused
    blk = _block(dim=256, heads=4, cond=32, residual_v=residual_v, seed=3)
    att = blk.self_attn
    g = torch.Generator().manual_seed(B * N)
    x = torch.randn(B, N, 256, generator=g).to(DEV, torch.bfloat16)
    rot = RotarySpec.from_freqs(precompute_freq_cis(64, end=256)[:N].to(DEV))
    v0 = (torch.randn(B, N, 4, 64, generator=g).to(DEV, torch.bfloat16)).transpose(1, 2) if residual_v else None
    assert att.fusable(x, rot)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        fused.ATTN_FUSED_TRAIN = False   # the separate-pass training chain (the fused training core has its own tests: test_attention_core_gpu.py)
        try:
            out_t, val_t = att.forward_fused(x, rotary=rot, v0=v0)      # grad mode: GEMM, then qk_norm_rope
        finally:
            fused.ATTN_FUSED_TRAIN = True
        with torch.no_grad():
            pack = att._proj_pack
            cos, sin = rot.cos_sin_tables(N)
            assert fused.projection_split_nograd_usable(x, pack, 4, 64, att.q_norm.weight, cos)
            out_n, val_n = att.forward_fused(x, rotary=rot, v0=v0)      # the fused-epilogue kernel
    for a, b_ in ((out_n, out_t), (val_n, val_t)):
        a, b_ = a.float(), b_.float()
        assert torch.isfinite(a).all()
        assert float((a - b_).abs().max()) <= 2.0 ** -6 * float(b_.abs().max())
        assert float((a != b_).float().mean()) < 0.05


@pytest.mark.parametrize("M,N,K", [(31, 832, 256), (1, 64, 8), (20000, 832, 256), (3000, 264, 520)])
def test_linear_wgrad_edge_shapes_and_row_map(M, N, K):
    """Fewer rows than one 32-row block, one row, the [q|k|v|gate] width (6.5 tiles of 128), sizes that are no multiple of the
    tile edges; and the row-mapped form: product row n stored at row_map[n] (negative = dropped), bias likewise."""
    from viforsdes_amd import _hip
    g = torch.Generator().manual_seed(M + N)
    dy = torch.randn(M, N, generator=g).to(torch.bfloat16).to(DEV)
    x = torch.randn(M, K, generator=g).to(torch.bfloat16).to(DEV)
    ref_w = (dy.double().t() @ x.double()).cpu().numpy()
    ref_b = dy.double().sum(0).cpu().numpy()
    dW, db = _hip.linear_wgrad(dy, x, True)
    assert rel_err(dW.cpu().numpy(), ref_w) < 2e-5 and rel_err(db.cpu().numpy(), ref_b) < 2e-5
    perm = torch.randperm(N, generator=g)
    keep = perm[: N - N // 8]                      # one eighth of the rows is dropped
    row_map = torch.full((N,), -1, dtype=torch.int32)
    row_map[keep] = torch.arange(keep.numel(), dtype=torch.int32)
    dWm, dbm = _hip.linear_wgrad(dy, x, True, row_map.to(DEV), keep.numel())
    assert dWm.shape == (keep.numel(), K)
    assert torch.equal(dWm, dW[keep.to(DEV)]) and torch.equal(dbm, db[keep.to(DEV)])
