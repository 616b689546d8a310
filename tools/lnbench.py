"""Time the fused norm / residual kernels at the LV encoder shape (GPU only): us per call and the rate over the [M, C] streams each
kernel has to move (the per-row vectors and mean / rstd are under 1 % of that), next to the ~6.3 TB/s a plain copy reaches."""
import os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch
from viforsdes_amd import _hip

B, N, C = 512, 401, 256
dev = torch.device("cuda:0")
bf = torch.bfloat16
x = torch.randn(B, N, C, device=dev, dtype=bf); dy = torch.randn_like(x); dres = torch.randn_like(x); y = torch.randn_like(x)
sc = torch.randn(B, C, device=dev, dtype=bf); sh = torch.randn_like(sc); gate = torch.randn_like(sc)
_, mean, rstd = _hip.ln_modulate_fwd(x, sc, sh, 1e-5)

def t(fn, n=30):
    for _ in range(3): fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3

mb = B * N * C * 2 / 1e6

def line(name, fn, streams):
    us = t(fn)
    print(f"{name:17s} {us:7.1f} us  ({streams * mb:.0f} MB, {streams * mb / us:5.2f} TB/s)")

line("ln_fwd", lambda: _hip.ln_modulate_fwd(x, sc, sh, 1e-5), 2)
line("ln_bwd (+dres)", lambda: _hip.ln_modulate_bwd(x, sc, dy, mean, rstd, dres), 4)
line("ln_bwd", lambda: _hip.ln_modulate_bwd(x, sc, dy, mean, rstd), 3)
line("gres_fwd", lambda: _hip.gated_residual_fwd(x, y, gate), 3)
line("gres_bwd", lambda: _hip.gated_residual_bwd(y, gate, dy), 3)
xn, h, mean2, rstd2 = _hip.residual_ln_fwd(x, y, gate, sc, sh, 1e-5)
line("residual_ln_fwd", lambda: _hip.residual_ln_fwd(x, y, gate, sc, sh, 1e-5), 4)
# the training step's form: dxnew present (4 streams in, dx and dy out); the call includes the small colsum_finish launch
line("residual_ln_bwd", lambda: _hip.residual_ln_bwd(xn, y, gate, sc, dy, dres, mean2, rstd2), 6)
