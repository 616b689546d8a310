"""GPU: the fused MLP's two block forms -- ``vsde_mlp_block_fwd_bf16`` (BLK == 1) and ``vsde_mlp_attn_block_fwd_bf16`` (BLK == 2),
csrc/vsde_mlp.hip -- per element against the float64 stage references of tests/mlp_block_reference.py (see its docstring for the
observation trick of each launch, the bounds and the share conditions).  Every case runs the launches gm0 / probe / select / scm1 /
full through ``_hip.mlp_block_fwd`` / ``_hip.mlp_attn_block_fwd`` on the same activations, with the images built the way
primitives/fused.py builds them (``swiglu_packs`` + ``MlpImages``, ``plain_pack`` + ``OutProjImage``), the modulation vectors as six
column ranges of one pitched [B, 8 C + 64] buffer and the gate logits as a column range of a wider buffer, both NaN-sentinel filled
around the ranges.  The operands are drawn on the CPU with the seeds of tests/test_mlp_block_bounds.py, so the share conditions that
file asserts for the reference alone are re-asserted here on the same data.  x and yin / attn must come back unchanged bit for bit.

The wrappers allocate tok and hnext themselves; ``test_outputs_stay_inside_their_buffers`` therefore calls the two entry points
directly with outputs inside sentinel-filled buffers, and the host-guard tests do the same to see that a refused call writes nothing.

Shapes (tests/mlp_block_reference.py ``CASES``): (B, N) = (3, 86), (7, 86), (3, 256), (2, 401), (5, 101) at C = 128 and 256, H = 64, 128
(100 real), 704 (682 real); select at H = C and at (256, 704); last block and not; eps = 1e-5, eps_next = 1e-3.
"""
import ctypes

import pytest
import torch

import mlp_block_reference as br
from mlp_block_reference import BF, F64

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = torch.float32
SENT = (torch.int16, 0x7FDE)      # a quiet bf16 NaN with a payload
ALL = [pytest.param(blk, case, id=br.case_id(blk, case)) for blk in (1, 2) for case in br.CASES]


def _hip():
    from viforsdes_amd import _hip
    return _hip


def _sentinel(*shape):
    return torch.full(shape, SENT[1], dtype=SENT[0], device=DEV).view(BF)


def _is_sentinel(t):
    return bool((t.view(SENT[0]) == SENT[1]).all())


def _to_dev(ops):
    """The case's float64 operands on the device (launches included)."""
    mv = lambda v: v.to(DEV) if torch.is_tensor(v) else v
    out = {k: mv(v) for k, v in ops.items() if k != "launches"}
    seen = {}

    def once(v):           # launches share tensors (and weight tuples): keep them shared, the image cache goes by identity
        if v is None or not (torch.is_tensor(v) or isinstance(v, tuple)):
            return v
        if id(v) not in seen:
            seen[id(v)] = (v, tuple(once(e) for e in v) if isinstance(v, tuple) else v.to(DEV))
        return seen[id(v)][1]

    out["launches"] = {name: dict(mods={k: once(v) for k, v in la["mods"].items()}, mlp=once(la["mlp"]), wo=once(la["wo"]), bo=once(la["bo"]))
                       for name, la in ops["launches"].items()}
    return out


class Runner:
    """``run(ops, launch) -> (tok, hnext)`` on the kernels; keeps the device operands, the images and the buffers of one case."""

    def __init__(self, ops):
        B, N, C, M = ops["B"], ops["N"], ops["C"], ops["M"]
        self.ops, self.blk = ops, ops["blk"]
        self.x = ops["x"].to(BF).view(B, N, C).contiguous()
        self.y = ops["y"].to(BF).view(B, N, C).contiguous()
        self.x0, self.y0 = self.x.clone(), self.y.clone()
        self.mbuf = _sentinel(B, 8 * C + 64)
        self.views = [self.mbuf[:, i * C:(i + 1) * C] for i in range(6)]
        if self.blk == 2:
            self.gbuf = _sentinel(M, 96)
            self.glog = self.gbuf[:, 16:80]
            self.glog.copy_(ops["glog"].to(BF))
        self.images, self.keep = {}, []

    def mods(self, launch):
        """The six vectors as views of the pitched buffer (None for a missing next norm)."""
        out = []
        for name, view in zip(br.VECS, self.views):
            v = launch["mods"][name]
            if v is None:
                view.copy_(_sentinel(*view.shape))
                out.append(None)
            else:
                view.copy_(v.to(BF))
                out.append(view)
        return out

    def mlp(self, launch):
        from viforsdes_amd.primitives import fused
        key = id(launch["mlp"])
        if key not in self.images:
            w_in, b_in, w_out, b_out, H, hreal = launch["mlp"]
            params = [torch.nn.Parameter(t.to(F32)) for t in (w_in, b_in, w_out, b_out)]
            pin, pout = fused.swiglu_packs(*params, H, interleave=False)
            img = fused.MlpImages(pin, pout, H)
            w1, w2, b1 = img.operands()
            assert torch.equal(pout.weight.to(F64)[:, :hreal], w_out) and torch.equal(pout.bias.to(F64), b_out)
            self.keep.append((params, pin, pout, img))
            self.images[key] = (w1, w2, b1, pout.bias, H)
        return self.images[key]

    def out_proj(self, launch):
        from viforsdes_amd.primitives import fused
        key = id(launch["wo"])
        if key not in self.images:
            wo, bo = torch.nn.Parameter(launch["wo"].to(F32)), torch.nn.Parameter(launch["bo"].to(F32))
            po = fused.plain_pack(wo, bo)
            wo_b, bo_b = po.operands()
            oimg = fused.OutProjImage(po)
            assert torch.equal(wo_b.to(F64), launch["wo"]) and torch.equal(bo_b.to(F64), launch["bo"])
            self.keep.append((wo, bo, po, oimg))
            self.images[key] = (oimg.operand(), bo_b)
        return self.images[key]

    def __call__(self, ops, launch):
        hip = _hip()
        ga, sc, sh, gm, sn, hs = self.mods(launch)
        w1, w2, b1, b2, H = self.mlp(launch)
        eps, eps_next = ops["eps"], ops["eps_next"]
        if self.blk == 1:
            tok, hn = hip.mlp_block_fwd(self.x, self.y, ga, sc, sh, gm, sn, hs, eps, eps_next, w1, w2, b1, b2, H)
        else:
            wo_img, bo = self.out_proj(launch)
            tok, hn = hip.mlp_attn_block_fwd(self.x, self.y, self.glog, wo_img, bo, ga, sc, sh, gm, sn, hs, eps, eps_next, w1, w2, b1, b2, H)
        torch.cuda.synchronize()
        M, C = ops["M"], ops["C"]
        return tok.view(M, C), (None if hn is None else hn.view(M, C))

    def inputs_unchanged(self, key):
        assert torch.equal(self.x.view(torch.int16), self.x0.view(torch.int16)), f"{key}: x changed"
        assert torch.equal(self.y.view(torch.int16), self.y0.view(torch.int16)), f"{key}: yin / attn changed"
        C = self.ops["C"]
        assert _is_sentinel(self.mbuf[:, 6 * C:]), f"{key}: the modulation buffer changed past its six ranges"
        if self.blk == 2:
            assert _is_sentinel(self.gbuf[:, :16]) and _is_sentinel(self.gbuf[:, 80:]), f"{key}: the gate buffer changed around the logits"


def _seed(blk, case):
    return 1000 * blk + br.CASES.index(case)   # the seeds of tests/test_mlp_block_bounds.py


@pytest.mark.parametrize("blk,case", ALL)
def test_block_form_stages_against_float64(blk, case):
    key = br.case_id(blk, case)
    ops = _to_dev(br.build_case(blk, case, seed=_seed(blk, case)))
    run = Runner(ops)
    res = br.check_case(ops, run, key=key)
    run.inputs_unchanged(key)
    br.assert_case(res, key)
    # bitwise reproducible: the full launch once more
    tok, hn = run(ops, ops["launches"]["full"])
    tok2, hn2 = run(ops, ops["launches"]["full"])
    assert torch.equal(tok.view(torch.int16), tok2.view(torch.int16)) and (hn is None or torch.equal(hn.view(torch.int16), hn2.view(torch.int16)))


# ------------------------------------------------------------------------------------- direct calls: fences and host guards
PAD = 64


def _direct(run, launch, N=None, tok=None, hnext="own", drop_hs=False):
    """Call the entry point of the case directly with outputs inside flat sentinel buffers: (rc message or None, tok buffer, hnext buffer)."""
    hip = _hip()
    lib = hip.load()
    ops = run.ops
    B, C, M = ops["B"], ops["C"], ops["M"]
    N = ops["N"] if N is None else N
    rows = B * N
    ga, sc, sh, gm, sn, hs = run.mods(launch)
    if drop_hs:
        hs = None
    w1, w2, b1, b2, H = run.mlp(launch)
    tbuf, hbuf = _sentinel(2 * PAD + M * C), _sentinel(2 * PAD + M * C)
    tok_ptr = hip._ptr(tbuf[PAD:]) if tok is None else hip._ptr(tok)
    hn_ptr = hip._ptr(hbuf[PAD:]) if (hnext == "own" and sn is not None) else hip._ptr(None)
    tail = (hip._i64(run.mbuf.stride(0)), ctypes.c_int(N), ctypes.c_double(ops["eps"]), ctypes.c_double(ops["eps_next"]), hip._ptr(w1), hip._ptr(w2),
            hip._ptr(b1), hip._ptr(b2), tok_ptr, hn_ptr, hip._i64(rows), ctypes.c_int(C), ctypes.c_int(H), hip._stream(torch.device(DEV)))
    vecs = tuple(hip._ptr(v) for v in (ga, sc, sh, gm, sn, hs))
    msg = None
    try:
        with torch.cuda.device(DEV):
            if run.blk == 1:
                hip._call(lib.vsde_mlp_block_fwd_bf16, hip._ptr(run.x), hip._ptr(run.y), *vecs, *tail)
            else:
                wo_img, bo = run.out_proj(launch)
                hip._call(lib.vsde_mlp_attn_block_fwd_bf16, hip._ptr(run.x), hip._ptr(run.y), hip._ptr(run.glog), hip._i64(run.glog.stride(0)),
                          hip._ptr(wo_img), hip._ptr(bo), *vecs, *tail)
    except ValueError as e:
        msg = str(e)
    torch.cuda.synchronize()
    return msg, tbuf, hbuf


def _runner(blk, B, N, C):
    case = next(c for c in br.CASES if (c[0], c[1], c[2]) == (B, N, C))
    ops = _to_dev(br.build_case(blk, case, seed=_seed(blk, case)))
    return Runner(ops), ops, br.case_id(blk, case)


@pytest.mark.parametrize("blk", [1, 2])
@pytest.mark.parametrize("C", [128, 256])
def test_outputs_stay_inside_their_buffers(blk, C):
    """M = 258: the second stripe holds two rows, seven of its waves lie past M -- nothing may be written around tok and hnext, and the
    fenced outputs equal the wrapper's bit for bit."""
    run, ops, key = _runner(blk, 3, 86, C)
    la = ops["launches"]["full"]
    n = ops["M"] * C
    msg, tbuf, hbuf = _direct(run, la)
    assert msg is None
    tok, hn = run(ops, la)
    for name, buf, ref in (("tok", tbuf, tok), ("hnext", hbuf, hn)):
        assert _is_sentinel(buf[:PAD]) and _is_sentinel(buf[PAD + n:]), f"{key}: elements around {name} changed"
        assert torch.equal(buf[PAD:PAD + n].view(torch.int16), ref.reshape(-1).view(torch.int16)), f"{key}: {name} differs from the wrapper's"
    run.inputs_unchanged(key)


@pytest.mark.parametrize("blk", [1, 2])
def test_host_guards_refuse_and_write_nothing(blk):
    hip = _hip()
    run, ops, key = _runner(blk, 3, 86, 128)
    la = ops["launches"]["full"]
    B, C = ops["B"], ops["C"]
    # sequences below 86 tokens: a 256-row stripe would touch more than MODB batch rows
    msg, tbuf, hbuf = _direct(run, la, N=85)
    assert msg is not None and "86" in msg, msg
    assert _is_sentinel(tbuf) and _is_sentinel(hbuf), f"{key}: a refused call wrote to its outputs"
    # ... and through the wrappers
    ga, sc, sh, gm, sn, hs = run.mods(la)
    w1, w2, b1, b2, H = run.mlp(la)
    x85, y85 = run.x[:, :85].contiguous(), run.y[:, :85].contiguous()
    with pytest.raises(ValueError, match="86"):
        if blk == 1:
            hip.mlp_block_fwd(x85, y85, ga, sc, sh, gm, sn, hs, br.EPS, br.EPS_NEXT, w1, w2, b1, b2, H)
        else:
            wo_img, bo = run.out_proj(la)
            hip.mlp_attn_block_fwd(x85, y85, run.glog[:B * 85], wo_img, bo, ga, sc, sh, gm, sn, hs, br.EPS, br.EPS_NEXT, w1, w2, b1, b2, H)
    # sn without hs
    msg, tbuf, hbuf = _direct(run, la, drop_hs=True)
    assert msg is not None and "go together" in msg, msg
    assert _is_sentinel(tbuf) and _is_sentinel(hbuf), f"{key}: a refused call wrote to its outputs"
    with pytest.raises(ValueError, match="go together"):
        if blk == 1:
            hip.mlp_block_fwd(run.x, run.y, ga, sc, sh, gm, sn, None, br.EPS, br.EPS_NEXT, w1, w2, b1, b2, H)
        else:
            wo_img, bo = run.out_proj(la)
            hip.mlp_attn_block_fwd(run.x, run.y, run.glog, wo_img, bo, ga, sc, sh, gm, sn, None, br.EPS, br.EPS_NEXT, w1, w2, b1, b2, H)
    if blk == 2:
        # the attention form parks x1 in tok: tok must not be x
        msg, tbuf, hbuf = _direct(run, la, tok=run.x)
        assert msg is not None and "alias" in msg, msg
        assert _is_sentinel(hbuf), f"{key}: a refused call wrote to hnext"
    torch.cuda.synchronize()
    run.inputs_unchanged(key)
