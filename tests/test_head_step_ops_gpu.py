"""GPU: the recurrent kernels of the fused head -- the GRU path sampler's time loop and its reverse-time sweep, every instantiation
``vsde_head_forward`` / ``vsde_head_backward`` can launch -- per element against float64 (tests/head_step_reference.py: teacher-forced
references, derived bounds, case table, dispatch mirror; tests/test_head_step_bounds.py checks all of them on the CPU).

Every case: the training launch (saved activations), the no-grad launch (bit for bit the same paths / means / chol), the projected
context record G of the same view (``_hip.debug_head_context_projection``), then ``head_backward`` in a caller-owned workspace from
which D4 / DO are read back (``head_gemm_reference.backward_workspace_layout``).  Scored, every element, |kernel - float64| <= bound:
the five saved slots of every unit, means, chol_raw, chol, z_{t+1}; D4, DO, grad_x0, grad_theta.  Bit for bit: paths[:, 0] == x0,
diag(chol) == max(chol_raw, float32(diag_min)), the strict upper triangle of chol == 0.  Kernels are forced only through
``debug_head_mp`` / ``debug_force_v1`` at shapes their host guards admit; the fixture restores both.

Observed on an MI355X (recorded after the run, never used to set a bound): 108 tests in 3 s, no element of any case out of bound, the
no-grad launch bit-equal everywhere.  Worst |error| / bound over all cases of a kernel family:
  forward   acts / means / chol_raw, chol / z_{t+1}:  v2 0.25 / 0.076 / 0.10 / 0.13;  v1 0.23 / 0.058 / 0.085 / 0.20;
            generic wide 0.15 / 0.065 / 0.061 / 0.058;  multi-path 0.20 / 0.016 / 0.017 / 0.10
  sweep     D4 / DO / grad_x0 / grad_theta:  v2 0.023 / 0.0062 / 7.4e-4 / 4.1e-4;  v1 0.019 / 0.0059 / 7.7e-5 / 1.4e-4;
            generic wide 0.0084 / 0.0054 / 9.2e-6 / 5.6e-6;  head_bwd_mps_kernel 0.037 / 0.0022 / 2.6e-4 / 3.1e-4;
            head_bwd_mp_kernel 0.043 / 0.0019 / 5.0e-4 / 5.9e-4
  P = 1 (one case or more per family): grad_theta at most 3.8e-5 of its bound, everything else inside the figures above
"""
import numpy as np
import pytest
import torch

import head_gemm_reference as RG
import head_step_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _hip():
    from viforsdes_amd import _hip
    return _hip


@pytest.fixture()
def forced(request):
    """Applies a case's kernel hooks (multi-path group size / v1) and restores the defaults."""
    hip = _hip()
    case = request.param
    hip.debug_head_mp(case["mp"])
    hip.debug_force_v1(case["v1"])
    yield case
    hip.debug_head_mp(-1)
    hip.debug_force_v1(False)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _run(hip, case, inp):
    """One case on the device -> dict of numpy arrays (the kernels' outputs, G, D4, DO) and the no-grad launch's tensors."""
    B, T, S, P, C, H, L = case["dims"]
    NO = R.n_out(S)
    ws = [_t(w) for w in inp["ws"]]
    x0, ctx, theta, eps = _t(inp["x0"]), _t(inp["ctx"]), _t(inp["theta"]), _t(inp["eps"])
    gp, gm, gl = _t(inp["gp"]), _t(inp["gm"]), _t(inp["gl"])
    G = hip.debug_head_context_projection(ctx, ws, S, P)
    out = hip.head_forward(x0, ctx, theta, eps, ws, inp["dt"], True)
    ev = hip.head_forward(x0, ctx, theta, eps, ws, inp["dt"], False)
    nbytes = hip.head_backward_workspace_bytes(*case["dims"])
    buf = torch.zeros(nbytes, device=DEV, dtype=torch.uint8)
    grads = hip.head_backward(gp, gm, gl, ctx, theta, eps, out[0], out[3], out[4], ws, inp["dt"], workspace=buf)
    torch.cuda.synchronize()
    lay = RG.backward_workspace_layout(case["dims"])
    D4 = buf[lay["D4"]:lay["D4"] + B * T * L * 4 * H * 4].view(torch.float32).reshape(B, T, L, 4, H)
    DO = buf[lay["DO"]:lay["DO"] + B * T * NO * 4].view(torch.float32).reshape(B, T, NO)
    n = lambda t: t.cpu().numpy()
    res = dict(paths=n(out[0]), means=n(out[1]), chol=n(out[2]), chol_raw=n(out[3]), acts=n(out[4]), G=n(G).reshape(B, T, 3 * H),
               D4=n(D4), DO=n(DO), grad_x0=n(grads[0]), grad_theta=n(grads[2]))
    return res, out, ev


@pytest.mark.parametrize("forced", R.CASES, indirect=True, ids=[c["id"] for c in R.CASES])
def test_time_loop_and_reverse_sweep_per_element(forced):
    hip, case = _hip(), forced
    B, T, S, P, C, H, L = case["dims"]
    fwd_name, bwd_name = R.route_forward(case["dims"], True, case["mp"], case["v1"]), R.route_backward(case["dims"], case["mp"], case["v1"])
    inp = R.make_inputs(case)
    res, out, ev = _run(hip, case, inp)
    # the no-grad launch: same bits, no saved tensors
    for a, b in zip(ev[:3], out[:3]):
        assert torch.equal(a, b), "the no-grad launch differs from the training launch"
    assert ev[3] is None and ev[4] is None
    # with the sticky f16-range flag up the host serves every multi-path shape with the v2 kernels, silently: the case would not reach its kernel
    if case["kind"] == "sat" or R.is_mp(fwd_name) or R.is_mp(bwd_name):
        assert not hip.head_mfma_range_exceeded(), "the sticky f16-range flag is up: the multi-path kernels were not launched"
    # identities that need no bound
    assert np.array_equal(res["paths"][:, 0], inp["x0"])
    assert np.array_equal(R.chol_identities(res["chol"], res["chol_raw"]), res["chol"])
    if case["kind"] == "clamp":
        raw = res["chol_raw"]
        assert (raw[..., 0] < np.float32(R.DIAG_MIN)).any() and (raw[..., 0] >= np.float32(R.DIAG_MIN)).any()
        assert S < 2 or (raw[..., -1] == np.float32(R.DIAG_MIN)).all()
    # forward, one step at a time on the kernel's own history
    ref = R.forward_ref(inp["ws"], inp["theta"], inp["eps"], res["G"], res["paths"], res["acts"], inp["dt"], mp=R.is_mp(fwd_name))
    got = dict(acts=res["acts"], means=res["means"], chol_raw=res["chol_raw"], chol=res["chol"], next=res["paths"][:, 1:])
    score = {k: R.excess(got[k], *ref[k]) for k in got}
    # the sweep on the kernel's own saved tensors
    sref, _ = R.sweep_ref(inp["ws"], P, inp["eps"], res["chol_raw"], res["acts"], inp["gp"], inp["gm"], inp["gl"], inp["dt"], mp=R.is_mp(bwd_name))
    score.update({k: R.excess(res[k], *sref[k]) for k in ("D4", "DO", "grad_x0", "grad_theta")})
    print(f"{case['id']} | {fwd_name} | {bwd_name} | worst err/bound: " + " ".join(f"{k} {v[1]:.3g}" for k, v in score.items()))
    assert float(np.abs(res["D4"]).max()) > 0 and np.isfinite(res["D4"]).all()
    for k, (nbad, worst, where) in score.items():
        assert nbad == 0, (k, nbad, worst, where)


@pytest.mark.parametrize("B, hook", [(31, 0), (32, 2)], ids=["B31-v2", "B32-mp"])
def test_default_dispatch_lands_on_the_kernel_the_mirror_names(B, hook):
    """On either side of the mp_auto threshold the default dispatch gives, bit for bit, what the hook value the mirror names gives
    (31 paths: the v2 kernels, hook 0; 32 paths: groups of two on the matrix cores, hook 2) -- and not what the other family gives."""
    hip = _hip()
    dims = (B, 17, 2, 3, 16, 64, 2)
    named = (R.route_forward(dims, True), R.route_backward(dims))
    assert named == (R.route_forward(dims, True, hook), R.route_backward(dims, hook))
    case = dict(id=f"auto-B{B}", dims=dims, mp=-1, v1=False, kind="randn")
    inp = R.make_inputs(case)
    keys = ("paths", "means", "chol", "chol_raw", "acts", "D4", "DO", "grad_x0", "grad_theta")
    try:
        assert not hip.head_mfma_range_exceeded()
        default, _, _ = _run(hip, case, inp)
        hip.debug_head_mp(hook)
        same, _, _ = _run(hip, case, inp)
        hip.debug_head_mp(0 if hook else 2)
        other, _, _ = _run(hip, case, inp)
    finally:
        hip.debug_head_mp(-1)
    for k in keys:
        assert np.array_equal(default[k], same[k]), k
    assert not np.array_equal(default["acts"], other["acts"]) and not np.array_equal(default["D4"], other["D4"])
