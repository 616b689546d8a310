"""GPU: every kind-4 instantiation ``<4, S, NR, KIN>`` of the simulator, coefficient, forecast and log-weight kernels
(csrc/vsde_sde.hip, csrc/vsde_elbo.hip) against float64, per element: one test per case of tests/sde_sweep_reference.py (the 48
cells of ``crn_dispatch`` and the lower-edge points R = 5, 9), six launches each, scored with |got - ref| <= c 2^-24 magnitude by
the references, magnitudes and constants of tests/sde_reference.py / tests/sde_aux_reference.py.

  launch       shape                                   what the shape reaches
  em_fwd       B 65, T 2 CH + 3                        a full 64-path group and a group of one path; two chunk seams and a partial
                                                       chunk of the LDS staging (row stride CH S + 1); teacher-forced per step on the
                                                       kernel's own trajectory; every clamp site clamps
  em_bwd       the same                                the (CH + 1) S + 1 stride, g_x0, g_theta of R < NR and R = NR (crn_store_rates)
  coef_fwd/bwd B 1, T 257                              258 grid points cross one 256-thread block
  forecast     B 65, T 9, rows (1, 4, 5) and (9, 9)    a Philox block seam and a duplicated row; the floor is reached
  log_weight   B 2, T 257, the 5 rows of lw_rows       the 256 seam, row 0, a shared row, the clamped row

Inputs travel as in tests/test_sde_ops_gpu.py (views at offset 64 of NaN-filled buffers, NaN in row T of x and above the
diagonal of g_diffusion), every kernel runs twice and must give the same bits."""
import numpy as np
import pytest
import torch

import sde_aux_reference as A
import sde_reference as R
import sde_sweep_reference as W
from test_sde_ops_gpu import guarded, same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _np(t):
    return t.cpu().numpy()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _simulator(name, net):
    from viforsdes_amd import _hip
    c = R.em_case(name, *W.em_shape(name))
    x0, theta, noise, g_traj = (guarded(c[k]) for k in ("x0", "theta", "noise", "g_traj"))
    run = lambda: _hip.euler_maruyama_fwd(c["kind"], x0, theta, noise, c["dt"], c["pos"], network=net)
    traj = run()
    back = lambda: _hip.euler_maruyama_bwd(c["kind"], theta, noise, traj, g_traj, c["dt"], c["pos"], network=net)
    grads = back()
    assert same_bits((traj,), (run(),)) and same_bits(grads, back())
    tr = _np(traj)
    assert R.em_clamped_at_sites(c, tr)                             # the clamp is exercised at every site
    return R.em_ratios(c, tr, _np(grads[0]), _np(grads[1]))


def _coefficients(name, net):
    from viforsdes_amd import _hip
    B, T = W.COEF_SHAPE
    c = A.coef_case(name, B, T)
    x, th, gf, gG = (guarded(c[k]) for k in ("x", "theta", "g_drift", "g_diffusion"))
    fwd = lambda: _hip.sde_coefficients_fwd(c["kind"], x, th, network=net)
    bwd = lambda: _hip.sde_coefficients_bwd(c["kind"], x, th, gf, gG, network=net)
    out, grads = fwd(), bwd()
    assert same_bits(out, fwd()) and same_bits(grads, bwd())
    got = dict(zip(A.COEF_OUT, [_np(t) for t in tuple(out) + tuple(grads)]))
    up = np.triu_indices(c["S"], 1)
    assert (got["diffusion"][..., up[0], up[1]] == 0).all()
    assert (got["g_x"][:, T] == 0).all()
    return A.coef_ratios(c, got)


def _forecast(name, net):
    from viforsdes_amd import _hip
    B, T, mask = W.FC_SHAPE
    c = A.fc_case(name, B, T, mask)
    x0, th = guarded(c["x0"]), guarded(c["theta"])
    key = torch.from_numpy(np.array(c["key"], dtype=np.uint32).view(np.int32)).to(DEV)

    def run(steps):
        steps = torch.tensor(steps, dtype=torch.int32, device=DEV)
        return _hip.forecast(c["kind"], x0, th, T, steps, key, c["dt"], c["pos"], network=net)

    every = list(range(1, T + 1))
    out = run(every)
    assert same_bits((out,), (run(every),))
    o = _np(out)
    assert A.fc_gates_ok(c, o)
    assert (o == np.float32(A.FLOOR32)).any()                         # the floor is reached
    for sub in W.FC_SUBSETS:
        assert torch.equal(_bits(run(list(sub))), _bits(out[:, [s - 1 for s in sub]])), sub
    return A.fc_ratio(c, o)


def _log_weights(name, net):
    from viforsdes_amd import _hip
    shape = W.lw_shape(name)
    c = A.lw_case(*shape)
    t = {k: guarded(c[k]) for k in ("z", "means", "chol", "theta", "rates", "obs_values", "obs_matrix", "post_mean", "post_log_std")}
    rows = torch.tensor(c["obs_rows"], dtype=torch.int32, device=DEV)
    run = lambda: _hip.log_weights(c["kind"], t["z"], t["means"], t["chol"], None, None, t["theta"], rows, t["obs_values"],
                                   t["obs_matrix"], c["variance"], c["lognormal"], c["prior_mean"], c["prior_std"], t["post_mean"],
                                   t["post_log_std"], c["pos"], c["theta_pos"], c["dt"], network=net, rates=t["rates"])
    out = run()
    assert same_bits((out,), (run(),))
    return A.lw_ratio(shape, _np(out))


@pytest.mark.parametrize("name", W.NAMES)
def test_cell(name):
    net = A.network(name)
    step, adj = _simulator(name, net)
    fwd, vjp = _coefficients(name, net)
    fc = _forecast(name, net)
    lw = _log_weights(name, net)
    print(f"RATIO {name} em_step {step:.4f} em_adj_crn {adj:.4f} coef_fwd {fwd:.4f} coef_vjp_crn {vjp:.4f} fc_step_crn {fc:.4f} lw {lw:.4f}")
    assert step <= W.em_step_c(name) and adj <= R.C_EM_ADJ_CRN, (step, adj)
    assert fwd <= W.coef_fwd_c(name) and vjp <= A.C_COEF_VJP_CRN, (fwd, vjp)
    assert fc <= A.C_FC_STEP_CRN, fc
    assert lw <= A.C_LW, lw
