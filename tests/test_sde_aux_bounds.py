"""CPU: the bounds of tests/sde_aux_reference.py (log-weight, coefficient and forecast kernels) are sound and sensitive.

* the written-out formulas behind the magnitudes equal the float64 references to 1e-12 of the magnitude;
* a correct float32 evaluation (float32 torch through the package's SDE classes for the coefficients; a numpy-float32 Box-Muller
  on the reference Philox words feeding the float32 step for the forecast) stays within c / 4 of every bound at every shape of
  tests/test_sde_aux_ops_gpu.py -- this is where the c values are asserted to hold;
* a float32 emulation of each kernel's arithmetic passes, and is rejected by at least one bound once a defect is injected.

Two defects a reader of the kernels might expect are not in the catalogues because no input can show them: the `b > 20` branch of
the linear-diagonal softplus derivative (1 / (1 + exp(-b)) is exactly 1 in float32 from b = 17 on), and a Lotka-Volterra gate on
l00 tested against q00r (l00 = sqrt(max(q00r, 1e-6)) >= 1e-3 always passes its gate, and where q00r is floored the adjoint of l00
is dropped by the q00r gate anyway).  In their place: the sigmoid factor missing from g_theta (seen at b = -25), and the gate on
q11r left open."""
import numpy as np
import pytest
import torch

import sde_aux_reference as A
import sde_reference as R

F32 = np.float32


# =========================================================================================================== log weights
LW_DEFECT_CASE = ("k0", 3, 3, 257, "all", 5, "id", "all", 1, None)       # two stride rounds, every observation-row edge, mask bit S - 1
LW_DIAG_CASE = ("diag", 5, 2, 257, "alt", 5, "wide", "none", 0, None)
LW_CRN_CASE = ("net3", 3, 2, 257, "all", 5, "wide", "last", 1, None)


@pytest.mark.parametrize("shape", [LW_DEFECT_CASE, LW_DIAG_CASE, LW_CRN_CASE, *A.lw_shapes()[::7], *A.lw_shapes()[-44:-36]], ids=lambda s: "-".join(map(str, s)))
def test_log_weight_formula_equals_the_float64_reference(shape):
    ref, mag = A.lw_reference(shape)
    f = A.lw_formulas(A.lw_case(*shape))
    assert np.isfinite(R.conditioning(ref, mag)) and R.ratio(f.v, ref, f.m) * R.C24 <= 1e-12


def lw_cpu_ratios():
    """Worst (Gaussian, count) ratio of the written-out formulas in float32 over every log-weight case of the GPU file."""
    worst = [0.0, 0.0]
    for shape in A.lw_shapes():
        k = int(bool(shape[-1]))
        worst[k] = max(worst[k], A.lw_ratio(shape, A.lw_formulas(A.lw_case(*shape), F32).v))
    return worst


def test_log_weight_bounds_hold_for_a_correct_float32_evaluation_at_every_gpu_shape():
    gauss, count = lw_cpu_ratios()
    print(f"log weights, formulas in float32: Gaussian {gauss:.3f}, count {count:.3f}")
    assert gauss <= A.C_LW / 4 and count <= A.C_LW_COUNT / 4, (gauss, count)


def test_log_weight_cases_floor_both_radicands_of_the_lotka_volterra_factor_decisively():
    c = A.lw_case("lv", 2, 3, 257, "all", 5, "id", "all", 1, None)
    _, x = A._lw_states(c, np.float64, c["pos"])
    th = R.VM(c["theta"].astype(np.float64)[:, None, :])
    _, q00r, _, _, _, q11r, _ = A._lv_factor(R.VM(x[:, :-1, 0]), R.VM(x[:, :-1, 1]), th[..., 0], th[..., 1], th[..., 2])
    for q in (q00r.v, q11r.v):
        assert ((q < 0.5 * R.EM_FLOOR) | (q > 2 * R.EM_FLOOR)).all() and (q < R.EM_FLOOR).any() and (q > R.EM_FLOOR).any()


@pytest.mark.parametrize("shape,defects", [(LW_DEFECT_CASE, A.LW_DEFECTS), (LW_DIAG_CASE, A.LW_DEFECTS_DIAG), (LW_CRN_CASE, A.LW_DEFECTS_CRN)],
                         ids=["kind0", "kind3", "kind4"])
def test_log_weight_emulation_passes_and_defects_are_rejected(shape, defects):
    c = A.lw_case(*shape)
    assert A.lw_ratio(shape, A.lw_formulas(c, F32).v) <= A.lw_c(shape)
    for defect in defects:
        assert A.lw_ratio(shape, A.lw_formulas(c, F32, defect).v) > A.lw_c(shape), defect


# ========================================================================================================== coefficients
@pytest.mark.parametrize("name,B,T", [("ou", 3, 257), ("lv", 3, 600), ("lv", 1, 1), ("diag1", 3, 257), ("diag5", 3, 257), ("diag32", 1, 256),
                                      ("sir", 3, 255), ("net3", 3, 257), ("chain8", 1, 257), ("autoreg", 3, 257), ("repress3", 3, 256),
                                      ("chain8k", 1, 257), ("clamp2", 3, 257)])
def test_coefficient_formulas_equal_autograd(name, B, T):
    c = A.coef_case(name, B, T)
    ref = A.coef_reference(c)
    f = A.coef_formulas(c)
    if not A.is_crn(name):
        f.update(A.coef_vjp_formulas(c))
    for k, a in f.items():
        assert R.ratio(a.v, ref[k], a.m) * R.C24 <= 1e-12, k
    up = np.triu_indices(c["S"], 1)
    assert (ref["diffusion"][..., up[0], up[1]] == 0).all() and (f["diffusion"].m[..., up[0], up[1]] == 0).all()
    assert (ref["g_x"][:, T] == 0).all()


@pytest.mark.parametrize("name", ["autoreg", "repress3", "chain8k"])
def test_hill_factor_derivatives_equal_the_packages_autograd(name):
    """The written-out derivatives of the Hill factor (sde_reference._HillFactor) against autograd through the package's own
    propensities, modifiers away from 0, to 1e-12 of sum |g| |J|."""
    c = A.coef_case(name, 3, 257 if name == "chain8k" else 255)
    sde = R.crn_sde(name)
    ref, mag = A._coef_ref_mag(name, c["B"], c["T"])
    patched = sde._propensities
    sde._propensities = sde.autograd_propensities
    try:
        pkg = A.coef_reference(c)
    finally:
        sde._propensities = patched
    for k in A.COEF_OUT:
        assert R.ratio(pkg[k], ref[k], mag[k]) * R.C24 <= 1e-12, k


def coef_cpu_ratios():
    """Worst (forward, VJP kinds 1..3, VJP kind 4) ratio of float32 torch over every coefficient case of the GPU file."""
    worst = [0.0, 0.0, 0.0]
    for shape in A.coef_shapes():
        c = A.coef_case(*shape)
        f, v = A.coef_ratios(c, A.coef_reference(c, torch.float32))
        worst[0] = max(worst[0], f)
        worst[2 if A.is_crn(shape[0]) else 1] = max(worst[2 if A.is_crn(shape[0]) else 1], v)
    return worst


def test_coefficient_bounds_hold_for_a_correct_float32_evaluation_at_every_gpu_shape():
    fwd, vjp, vjp4 = coef_cpu_ratios()
    print(f"coefficients, float32 torch: forward {fwd:.3f}, VJP kinds 1..3 {vjp:.3f}, VJP kind 4 {vjp4:.3f}")
    assert fwd <= A.C_COEF_FWD / 4 and vjp <= A.C_COEF_VJP / 4 and vjp4 <= A.C_COEF_VJP_CRN / 4, (fwd, vjp, vjp4)


def _coef_passes(c, got):
    f, v = A.coef_ratios(c, got)
    return f <= A.C_COEF_FWD and v <= A.coef_vjp_c(c["name"])


COEF_DEFECT_T = 257          # two rows in the second stride round; diag5: 51 slots, rows 255 and 256 in a partial sixth round


@pytest.mark.parametrize("name", A.COEF_NAMES)
def test_coefficient_emulation_passes(name):
    for B, T in ((3, COEF_DEFECT_T), (1, 1)):
        c = A.coef_case(name, B, T)
        assert _coef_passes(c, A.coef_emulated(c)), (name, B, T)


@pytest.mark.parametrize("defect,name", [(d, n) for d, names in A.COEF_DEFECTS.items() for n in names])
def test_coefficient_defect_is_rejected(defect, name):
    c = A.coef_case(name, 3, COEF_DEFECT_T)
    assert not _coef_passes(c, A.coef_emulated(c, defect))


# ============================================================================================================== forecast
def fc_cpu_ratios():
    """Worst (kinds 1..3, kind 4) ratio of the float32 forecast over every forecast case of the GPU file; every case's inner floors
    are decisive or free of cancellation (``fc_gates_ok``)."""
    worst = [0.0, 0.0]
    for shape in A.fc_shapes():
        c = A.fc_case(*shape)
        out = A.fc_simulate(c)
        assert A.fc_gates_ok(c, out), shape
        if c["pos"] and c["B"] > 1:
            assert (out == F32(R.EM_FLOOR)).any(), shape                    # the floor is reached
        k = int(A.is_crn(c["model"]))
        worst[k] = max(worst[k], A.fc_ratio(c, out))
    return worst


@pytest.mark.parametrize("name,B,mask", [("ou", 257, "none"), ("lv", 257, "all"), ("diag5", 52, "all"), ("diag32", 9, "last")])
def test_forecast_step_formula_equals_autograd(name, B, mask):
    """The step the forecast is scored with (sde_reference.em_step on the reference normals) against the float64 torch statement
    x + f dt + G z sqrt(dt) of the package's SDE class, from small and large states."""
    c = A.fc_case(name, B, 9, mask)
    keep = np.arange(B) != c["nan_path"]
    x = np.concatenate([c["x0"][:, None, :], A.fc_simulate(c)], 1)[keep][:, :-1].astype(np.float64)
    th = np.broadcast_to(c["theta"][keep].astype(np.float64)[:, None, :], x.shape[:2] + (c["P"],))
    z = c["z_ref"][keep]
    sde = A.spec_sde(c["model"])
    xt, tt = torch.tensor(x).reshape(-1, c["S"]), torch.tensor(np.ascontiguousarray(th)).reshape(-1, c["P"])
    y = xt + sde.drift(xt, tt) * c["dt"] + torch.einsum("nik,nk->ni", sde.diffusion(xt, tt), torch.tensor(z).reshape(-1, c["S"])) * c["dt"] ** 0.5
    step = R.em_step(c["model"], x, th, z, c["dt"])
    assert R.ratio(step.v, y.reshape(x.shape).numpy(), step.m) * R.C24 <= 1e-12


def test_forecast_noise_in_float32_is_the_reference_stream():
    """The float32 Box-Muller of the emulation against tests/philox_reference.py: a few ulps of |z| per normal."""
    c = A.fc_case("diag5", 52, 9, "all")
    z32, z = A.fc_noise32(c)[:, :9].astype(np.float64), c["z_ref"]
    assert (np.abs(z32 - z) <= 4 * R.C24 * np.abs(z)).all()


def test_forecast_bounds_hold_for_a_correct_float32_evaluation_at_every_gpu_shape():
    step, step4 = fc_cpu_ratios()
    print(f"forecast, float32 Box-Muller and step: kinds 1..3 {step:.3f}, kind 4 {step4:.3f}")
    assert step <= A.C_FC_STEP / 4 and step4 <= A.C_FC_STEP_CRN / 4, (step, step4)


FC_DEFECT_SHAPE = {"ou": ("ou", 257, 9, "none"), "lv": ("lv", 257, 9, "all"), "diag5": ("diag5", 51, 9, "alt"), "net3": ("net3", 65, 9, "all")}


@pytest.mark.parametrize("name", sorted(FC_DEFECT_SHAPE))
def test_forecast_emulation_passes(name):
    c = A.fc_case(*FC_DEFECT_SHAPE[name])
    assert A.fc_ratio(c, A.fc_simulate(c)) <= A.fc_c(name)


def test_forecast_of_ou_without_drift_from_zero_pins_each_normal():
    """kappa = 0 from x = 0: the magnitude of step 1 is sigma sqrt(dt) |z| alone, so the bound holds z to c ulps."""
    c = A.fc_case("ou0", 257, 9, "none")
    keep = np.arange(257) != c["nan_path"]
    ref, mag = A.fc_check(dict(c, theta=c["theta"][keep], z_ref=c["z_ref"][keep]),
                          np.concatenate([c["x0"][:, None, :], A.fc_simulate(c)], 1)[keep])
    want = c["theta"][keep, 2].astype(np.float64) * np.sqrt(c["dt"]) * np.abs(c["z_ref"][keep, 0, 0])
    assert np.allclose(mag[:, 0, 0], want, rtol=1e-12, atol=0)
    assert A.fc_ratio(c, A.fc_simulate(c)) <= A.C_FC_STEP


@pytest.mark.parametrize("defect,name", [(d, n) for d, names in A.FC_DEFECTS.items() for n in names])
def test_forecast_defect_is_rejected(defect, name):
    c = A.fc_case(*FC_DEFECT_SHAPE[name])
    assert A.fc_ratio(c, A.fc_simulate(c, defect=defect)) > A.fc_c(name)


# =========================================================================================================== accumulator
def test_accumulator_reference_is_logsumexp():
    for n in A.ACC_NS:
        for edge in A.ACC_EDGES:
            chunks = A.acc_case(n, edge)
            m, lse, ess, total, count, bad = A.acc_reference(chunks)
            v = torch.tensor(np.concatenate(chunks), dtype=torch.float64)
            v = v[v != float("inf")]
            assert count == sum(len(ch) for ch in chunks) and bad == (edge == "plus_inf_entry")
            if v.numel() == 0:                                  # n = 1 with its only entry +inf: nothing is summed
                assert lse == float("-inf")
                continue
            assert abs(float(torch.logsumexp(v, 0)) - lse) <= 1e-12 * abs(lse) and 1.0 - 1e-12 <= ess <= n
