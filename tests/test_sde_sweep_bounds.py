"""CPU: the conditions of the kind-4 sweep (tests/test_sde_sweep_gpu.py) on the references alone.

* the mirror of ``crn_dispatch`` maps exactly one case to each of the 48 cells, the lower-edge points land in the bins above;
  every network is served by the kernels, and a rate-law cell has a Hill law, a Michaelis-Menten law (S > 1) and a shared constant;
* the floored pivots per cell are what tests/sde_sweep_reference.py tabulates, the same at every state of the case, columns are
  zeroed only with two or more of them, and two cells keep exactly one with full noise;
* every gate of ``crn_coef_formula`` is at least a factor 2 from the floor on the states of the simulator, coefficient and
  log-weight launches (the forecast's through ``fc_gates_ok``), every clamp site clamps;
* the log-weight bound holds the kernel to something in every case: an all-zero output, a row read past T and (in all cases but
  one) a rate constant read as zero miss C_LW;
* a correct float32 evaluation (float32 torch through the package's classes; the written-out formulas for the log weights) of the
  full case of all six launches of every case stays within c / 4 -- where the constants are asserted to hold;
* the two constants of the sweep's own still reject injected defects, in every cell of their family;
* the reverse step of a rate-law cell (``sde_reference._crn_step_bwd`` on the ``_HillFactor`` copy) equals the package's autograd."""
import numpy as np
import pytest
import torch

import reaction_networks as rn
import sde_aux_reference as A
import sde_reference as R
import sde_sweep_reference as W

F32 = np.float32


# ------------------------------------------------------------------------------------------------------------------ cells
def test_one_case_per_cell_and_the_edge_points():
    cases = W.cases()
    assert len(W.CELLS) == 48 and len(set(W.CELLS)) == 48 and len(cases) == 48 + 2 * len(W.EDGE_POINTS) == len(set(W.NAMES))
    hits = {cell: [c for c in cases[:48] if W.dispatch(*c) == cell] for cell in W.CELLS}
    assert all(len(v) == 1 for v in hits.values())
    for S, R_, kin in cases[:48]:
        assert R_ == (W.dispatch(S, R_, kin)[1] if S % 2 == 0 else rn.SWEEP_REACTIONS[W.dispatch(S, R_, kin)[1]])
    assert [W.dispatch(*c) for c in cases[48:]] == [(6, 8, False), (6, 8, True), (7, 16, False), (7, 16, True)]
    assert [c[1] for c in cases[48:]] == [5, 5, 9, 9]                           # the first count of the bins of 8 and 16
    assert isinstance(W.dispatch(9, 3, False), str) and isinstance(W.dispatch(3, 17, False), str) and isinstance(W.dispatch(3, 0, True), str)
    for name, c in zip(W.NAMES, cases):
        S, NR, kin, R_ = rn.sweep_cell(name)
        assert (S, R_, kin) == c and (S, NR, kin) == W.dispatch(*c)
        assert R.EM_KINDS[name] == ("reaction_network", S, 32 if S <= 2 else 16 if S <= 4 else 8) and A.KINDS[name] == ("reaction_network", S)
        assert R.is_crn(name) and A.is_crn(name) and name not in R.EM_KINDS and name not in A.KINDS


@pytest.mark.parametrize("name", W.NAMES)
def test_network_of_the_case(name):
    S, NR, kin, R_ = rn.sweep_cell(name)
    sde = R.crn_sde(name)
    assert sde.kernel_compatible() and sde.state_dim == S and sde.num_reactions == R_ and sde.plain == (not kin)
    assert sde.rate_dim == (2 * R_ if kin else R_) and len(sde.base_theta) == sde.sde_param_dim
    if kin:
        laws = [law for law in sde.laws if law is not None]
        kw = rn.sweep_network(S, NR, True, R_)[0]
        assert tuple(sde.laws[0][:3]) == (2, S - 1, 2)                      # Hill repression by the last species, n = 2, on the feed
        assert S == 1 or tuple(sde.laws[1][:3]) == (1, 0, 1)                # Michaelis-Menten in X_0 on the conversion
        assert len(laws) == (1 if S == 1 else 2)
        # a shared constant, as sweep_network builds it: the first round of decays, wherever there are two of them
        assert (len(set(kw["rate_constants"])) < R_) == (min(R_, 3 + S) - 3 >= 2)


# ---------------------------------------------------------------------------------------------------------- floored pivots
FLOORED = {5: (3, 4), 6: (4, 5), 7: (3, 4, 5, 6), 8: (4, 5, 6, 7)}          # NR 4 (R 3 or 4): S -> pivots


def test_floored_pivots_and_what_is_zeroed():
    one = []
    for name in W.NAMES:
        S, NR, kin, R_ = rn.sweep_cell(name)
        want = FLOORED.get(S, ()) if NR == 4 else (5,) if (S, R_) == (6, 5) else ()
        assert R.sweep_floored(name) == want, name
        assert R.sweep_zeroed(name) == (list(want) if len(want) >= 2 else [])
        assert R.sweep_hit_dim(name) == (2 if want else S - 1)
        one += [name] * (len(want) == 1)
    assert one == ["sw-S6-NR8-R5", "sw-S6-NR8-k-R5"]                        # exactly one floored pivot: full noise, nothing zeroed


def _gates_clear(name, x, th):
    """Every gate a factor 2 from the floor, and the floored pivots those of ``sweep_floored``, at the states x."""
    gates = R.crn_coef_formula(name, np.asarray(x, np.float64), np.asarray(th, np.float64))[2]
    fl = R.sweep_floored(name)
    for j in range(len(gates) // 2):
        rad, piv = gates[2 * j].v, gates[2 * j + 1].v
        assert ((rad < 0.5 * R.EM_FLOOR) | (rad > 2 * R.EM_FLOOR)).all() and (piv > 2 * R.EM_FLOOR).all(), (name, j)
        assert (rad < R.EM_FLOOR).all() if j in fl else (rad > R.EM_FLOOR).all(), (name, j)


# ------------------------------------------------------------------------------------------- float32 within c / 4, per case
@pytest.mark.parametrize("name", W.NAMES)
def test_bounds_hold_for_a_correct_float32_evaluation_of_the_case(name):
    # simulator: float32 torch step, float32 reverse recursion with float32 Jacobians, on its own trajectory
    c = R.em_case(name, *W.em_shape(name))
    assert (c["noise"][..., R.sweep_zeroed(name)] == 0).all()
    traj = R.em_simulate(c, F32)
    assert R.em_clamped_at_sites(c, traj)
    a, gth = R.em_adjoint(c, traj, F32)
    step, adj = R.em_ratios(c, traj, a.v, gth.v)                    # asserts that no one-step value is within a factor 2 of the floor
    _gates_clear(name, traj[:, :-1], c["theta"][:, None, :])
    # coefficients
    cc = A.coef_case(name, *W.COEF_SHAPE)                           # asserts the gates of its grid
    up = np.triu_indices(cc["S"], 1)
    g = np.nan_to_num(cc["g_diffusion"], nan=0.0)
    assert (g[..., R.sweep_zeroed(name)] == 0).all() and np.isnan(cc["g_diffusion"][..., up[0], up[1]]).all()
    _gates_clear(name, cc["x"][:, :-1], cc["theta"][:, None, :])
    fwd, vjp = A.coef_ratios(cc, A.coef_reference(cc, torch.float32))
    # forecast
    fcase = A.fc_case(name, *W.FC_SHAPE)
    o = A.fc_simulate(fcase)
    assert A.fc_gates_ok(fcase, o) and (o == F32(A.FLOOR32)).any()
    fc = A.fc_ratio(fcase, o)
    # log weights
    shape = W.lw_shape(name)
    lc = A.lw_case(*shape)
    _gates_clear(name, A._lw_states(lc, np.float64, lc["pos"])[1][:, :-1], (lc["theta"] if lc["rates"] is None else lc["rates"])[:, None, :])
    lw = A.lw_ratio(shape, A.lw_formulas(lc, F32).v)
    # the log-weight bound holds the kernel to something in every case: an all-zero output and a row read past T miss it
    ref, mag = A.lw_reference(shape)
    assert A.lw_ratio(shape, np.zeros_like(ref)) > A.C_LW and R.conditioning(ref, mag) < 2e5
    assert A.lw_ratio(shape, A.lw_formulas(lc, F32, "obs_rows_not_clamped").v) > A.C_LW
    print(f"CPU {name} em_step {step:.3f} em_adj {adj:.3f} coef_fwd {fwd:.3f} coef_vjp {vjp:.3f} fc {fc:.3f} lw {lw:.3f}")
    assert step <= W.em_step_c(name) / 4 and adj <= R.C_EM_ADJ_CRN / 4, (step, adj)
    assert fwd <= W.coef_fwd_c(name) / 4 and vjp <= A.C_COEF_VJP_CRN / 4, (fwd, vjp)
    assert fc <= A.C_FC_STEP_CRN / 4 and lw <= A.C_LW / 4, (fc, lw)


@pytest.mark.parametrize("name", ["sw-S4-NR8", "sw-S8-NR16-k", "sw-S7-NR4", "sw-S6-NR8-R5"])
def test_formulas_of_the_case_equal_the_float64_references(name):
    """The written-out step and log weight (where the magnitudes come from) against the torch statements, to 1e-12."""
    c = R.em_case(name, *W.em_shape(name))
    traj = R.em_simulate(c, np.float64)
    for t in (0, c["ch"], c["ch"] + 1):
        args = (name, traj[:, t], c["theta"], c["noise"][:, t], c["dt"])
        f = R.crn_step_formula(*args)
        assert R.ratio(f.v, R.em_step(*args).v, f.m) * R.C24 <= 1e-12
    shape = W.lw_shape(name)
    ref, mag = A.lw_reference(shape)
    f = A.lw_formulas(A.lw_case(*shape))
    assert np.isfinite(R.conditioning(ref, mag)) and R.ratio(f.v, ref, f.m) * R.C24 <= 1e-12


def test_first_order_factor_magnitude_is_the_smaller_one_and_finite():
    """The sweep's magnitude of the diffusion factor never exceeds the recursion's and stays within 1e9 of the entry's size
    (largest: the entries of a floored column, noise over 1e-3), where the recursion's alone reaches 1e120."""
    for name in ("sw-S8-NR8", "sw-S8-NR4-k", "sw-S7-NR16-k"):
        cc = A.coef_case(name, *W.COEF_SHAPE)
        m = A.coef_formulas(cc)["diffusion"]
        lo = np.tril_indices(cc["S"])
        assert np.isfinite(m.m).all() and (m.m[..., lo[0], lo[1]] >= (1 - 1e-12) * np.abs(m.v[..., lo[0], lo[1]])).all()
        scale = np.abs(m.v).max(axis=(-1, -2))[..., None, None]
        assert (m.m <= 1e9 * scale).all(), name


# ------------------------------------------------------------------------------------------------- the sweep's own constants
@pytest.mark.parametrize("name", [n for n in W.NAMES if rn.sweep_cell(n)[0] == 2])
def test_step_constant_of_the_two_species_cells_rejects_the_injected_defects(name):
    B, T = 130, W.em_shape(name)[1]                                 # a partial third group, as tests/test_sde_bounds.py
    c = R.em_case(name, B, T)

    def passes(fwd=None, bwd=None):
        traj = R.em_simulate(c, F32, fwd)
        a, gth = R.em_adjoint(c, traj, F32, bwd)
        step, adj = R.em_ratios(c, traj, a.v, gth.v)
        return step <= W.em_step_c(name) and adj <= R.C_EM_ADJ_CRN

    assert W.em_step_c(name) == W.C_EM_STEP_S2 and passes()
    for defect in R.EM_DEFECTS_FWD:
        assert not passes(fwd=defect), defect
    for defect in R.EM_DEFECTS_BWD:
        assert not passes(bwd=defect), defect


@pytest.mark.parametrize("name", [n for n in W.NAMES if rn.sweep_cell(n)[2]])
def test_coefficient_constant_of_the_rate_law_cells_rejects_injected_defects(name):
    cc = A.coef_case(name, *W.COEF_SHAPE)
    good = A.coef_reference(cc, torch.float32)
    assert W.coef_fwd_c(name) == W.C_COEF_FWD_KIN and A.coef_ratios(cc, good)[0] <= W.C_COEF_FWD_KIN
    Rn = cc["P"] // 2
    for col, what in ((Rn - 1, "the last rate constant read as 1"), (Rn, "the Hill constant read as 1")):
        bad = dict(cc, theta=cc["theta"].copy())
        bad["theta"][:, col] = 1.0
        assert A.coef_ratios(cc, A.coef_reference(bad, torch.float32))[0] > W.C_COEF_FWD_KIN, what
    shifted = {k: v.copy() for k, v in good.items()}
    shifted["diffusion"][:, 256] = good["diffusion"][:, 255]        # the grid point past the first 256-thread block repeats its neighbour
    assert A.coef_ratios(cc, shifted)[0] > W.C_COEF_FWD_KIN


def test_log_weight_bound_rejects_a_rate_constant_read_as_zero():
    """``last_rate_constant_read_as_zero`` (sde_aux_reference.LW_DEFECTS_CRN) misses C_LW in every case but one, whose last
    reaction is a repeated decay with the smallest constant of its network (26.9 against 28)."""
    passing = []
    for name in W.NAMES:
        shape = W.lw_shape(name)
        if A.lw_ratio(shape, A.lw_formulas(A.lw_case(*shape), F32, A.LW_DEFECTS_CRN[0]).v) <= A.C_LW:
            passing.append(name)
    assert passing == ["sw-S7-NR16"], passing


# ------------------------------------------------------------------------------------------------------ rate-law reverse step
@pytest.mark.parametrize("name", ["sw-S1-NR4-k", "sw-S4-NR8-k", "sw-S8-NR16-k", "sw-S6-NR8-k-R5"])
def test_reverse_step_of_a_rate_law_cell_equals_the_packages_autograd(name):
    """``_crn_step_bwd`` differentiates the copy whose Hill factor has written-out derivatives; here against autograd through the
    package's own propensities, to 1e-12 of |a| |J|."""
    c = R.em_case(name, 65, 5)
    sde = R.crn_sde(name)
    a = R.VM(c["g_traj"][:, 1].astype(np.float64))
    args = (name, c["x0"], c["theta"], c["noise"][:, 0], a, c["dt"], np.float64)
    ax, gth = R._crn_step_bwd(*args)
    patched = sde._propensities
    sde._propensities = sde.autograd_propensities
    try:
        pax, pgth = R._crn_step_bwd(*args)
    finally:
        sde._propensities = patched
    assert R.ratio(pax.v, ax.v, ax.m) * R.C24 <= 1e-12 and R.ratio(pgth.v, gth.v, gth.m) * R.C24 <= 1e-12
    assert np.abs(gth.v[:, sde.num_reactions:]).max() > 0           # the half-saturation constants do carry gradient
