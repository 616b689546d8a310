"""CPU: the bounds of tests/sde_reference.py are sound and sensitive.

* the written-out formulas behind the magnitudes equal the autograd references to 1e-12 of the magnitude;
* a correct float32 evaluation (the C oracle's f32 instantiation; float32 torch autograd for the tail's gradients) stays within
  c / 4 of every bound at every shape of tests/test_sde_ops_gpu.py -- this is where the c values are asserted to hold;
* a float32 emulation of each kernel's arithmetic passes, and is rejected by at least one bound once a defect is injected."""
import numpy as np
import pytest
import torch

import sde_reference as R
from oracle import vsde_oracle as vo

F32 = np.float32


def _vals(d):
    return {k: a.v for k, a in d.items()}


# ============================================================================================================ path terms
def oracle_path(c):
    """The oracle's float32 instantiation on the case's inputs."""
    args = [c[k] for k in ("z", "x", "means", "chol", "drift", "diffusion")]
    got = dict(zip(R.PATH_NAMES, vo.elbo_path_terms(*args, c["pos"], c["dt"], F32)))
    got.update(zip(R.PATH_GRADS, vo.elbo_path_terms_bwd(*args, c["pos"], c["dt"], c["g_sde"], c["g_gen"], c["g_jac"], F32)))
    return got


def path_cpu_ratios():
    """Worst (forward, backward) ratio of the oracle's f32 instantiation over every path-term case of the GPU file."""
    worst = [0.0, 0.0]
    for shape in R.path_shapes():
        c = R.path_case(*shape)
        worst = [max(w, r) for w, r in zip(worst, R.path_ratios(c, oracle_path(c)))]
    return worst


@pytest.mark.parametrize("S,B,T,mask", [(1, 3, 257, "all"), (3, 3, 257, "alt"), (16, 3, 257, "last"), (8, 1, 600, "all"),
                                        (2, 3, 2, "none"), (16, 1, 1, "all")])
def test_path_formulas_equal_autograd(S, B, T, mask):
    c = R.path_case(S, B, T, mask)
    ref, f = R.path_reference(c), R.path_formulas(c)
    for k in ref:
        assert R.ratio(f[k].v, ref[k], f[k].m) * R.C24 <= 1e-12, k
    up = np.triu_indices(S, 1)
    for k in ("g_chol", "g_diffusion"):
        assert (ref[k][..., up[0], up[1]] == 0).all() and (f[k].m[..., up[0], up[1]] == 0).all()


def test_path_bounds_hold_for_a_correct_float32_evaluation_at_every_gpu_shape():
    fwd, bwd = path_cpu_ratios()
    print(f"path terms, oracle f32: forward {fwd:.3f}, backward {bwd:.3f}")
    assert fwd <= R.C_PATH_FWD / 4 and bwd <= R.C_PATH_BWD / 4, (fwd, bwd)


PATH_DEFECT_CASE = (3, 3, 257, "all")


def _path_passes(got, c):
    fwd, bwd = R.path_ratios(c, got)
    return fwd <= R.C_PATH_FWD and bwd <= R.C_PATH_BWD


def test_path_emulation_passes():
    for shape in (PATH_DEFECT_CASE, (16, 3, 257, "last"), (1, 1, 600, "all"), (8, 3, 1, "alt")):
        c = R.path_case(*shape)
        assert _path_passes(_vals(R.path_formulas(c, F32)), c), shape


@pytest.mark.parametrize("defect", R.PATH_DEFECTS)
@pytest.mark.parametrize("shape", [PATH_DEFECT_CASE, (16, 3, 257, "last")], ids=["S3", "S16"])
def test_path_defect_is_rejected(defect, shape):
    c = R.path_case(*shape)
    assert not _path_passes(_vals(R.path_formulas(c, F32, defect)), c)


# ================================================================================================================== tail
def correct_tail(c):
    """out [6] from the oracle's f32 observation / prior / posterior sums and float32 batch means; gradients from float32 torch."""
    got = R.tail_reference(c, torch.float32)
    if c["count"]:                                   # the oracle has no count likelihood: float32 torch throughout
        return got
    B, K = c["B"], c["K"]
    obs = vo.obs_log_prob(c["x_obs"], np.arange(K), c["obs_values"], c["variance"], c["obs_matrix"], F32) if K else np.zeros(B, F32)
    prior, post = vo.theta_log_probs(c["theta"], c["post_mean"], c["post_log_std"], c["pos"], c["lognormal"], c["prior_mean"],
                                     c["prior_std"], F32)
    s, g, j = c["sde_lp"], c["gen_lp"], c["jac"]
    got["out"] = np.array([t.sum(dtype=F32) / F32(B) for t in (obs + s - g + j + prior - post, obs, s, g, prior, post)], F32)
    return got


def tail_cpu_ratio():
    return max(R.tail_ratio(R.tail_case(*shape), correct_tail(R.tail_case(*shape))) for shape in R.tail_shapes() + list(R.COUNT_SHAPES))


@pytest.mark.parametrize("shape", [(257, 1, 5, 1, "all"), (700, 2, 1, 0, "last"), (2, 3, 5, 1, "none"), (1, 0, 0, 0, "all"), *R.COUNT_SHAPES],
                         ids=lambda s: "-".join(map(str, s)))
def test_tail_formulas_equal_autograd(shape):
    c = R.tail_case(*shape)
    ref, f = R.tail_reference(c), R.tail_formulas(c)
    for k in ref:
        assert R.ratio(f[k].v, ref[k], f[k].m) * R.C24 <= 1e-12, k


def test_tail_bounds_hold_for_a_correct_float32_evaluation_at_every_gpu_shape():
    worst = tail_cpu_ratio()
    print(f"tail, oracle f32 sums / float32 torch gradients: {worst:.3f}")
    assert worst <= R.C_TAIL / 4, worst


TAIL_DEFECT_CASE = (700, 1, 5, 1, "last")          # B > 256, S 3, O 16, P 16 with a matrix, theta mask = bit 15 only


def test_tail_emulation_passes():
    for shape in (TAIL_DEFECT_CASE, (257, 3, 1, 0, "all"), (1, 2, 0, 1, "none"), *R.COUNT_SHAPES):
        c = R.tail_case(*shape)
        assert R.tail_ratio(c, _vals(R.tail_formulas(c, F32))) <= R.C_TAIL, shape


@pytest.mark.parametrize("defect", R.TAIL_DEFECTS)
def test_tail_defect_is_rejected(defect):
    c = R.tail_case(*TAIL_DEFECT_CASE)
    assert R.tail_ratio(c, _vals(R.tail_formulas(c, F32, defect))) > R.C_TAIL


# ============================================================================================================= simulator
em_ratios = R.em_ratios


def oracle_em(c):
    """The oracle's f32 instantiation; kind 4, which it does not have: the float32 torch step and its float32 Jacobians."""
    if c["name"] in R.CRN:
        return _em_emulated(c)
    kind = R.ORACLE_KIND[c["name"]]
    traj = vo.euler_maruyama(kind, c["x0"], c["theta"], c["noise"], c["dt"], c["pos"], F32)
    return (traj,) + tuple(vo.euler_maruyama_bwd(kind, c["theta"], c["noise"], traj, c["g_traj"], c["dt"], c["pos"], F32))


def em_cpu_ratios():
    """Worst [step, adjoint] ratios over every simulator case of the GPU file, kinds 1..3 and kind 4 apart."""
    worst = {False: [0.0, 0.0], True: [0.0, 0.0]}
    for shape in R.em_shapes():
        c = R.em_case(*shape)
        out = oracle_em(c)
        assert R.em_clamped_at_sites(c, out[0]), shape               # every case does clamp at its sites
        crn = shape[0] in R.CRN
        worst[crn] = [max(w, r) for w, r in zip(worst[crn], em_ratios(c, *out))]
    return worst[False], worst[True]


@pytest.mark.parametrize("name", [n for n in R.EM_KINDS if n not in R.CRN])
def test_em_step_formulas_equal_autograd(name):
    """One step and its vector-Jacobian product against float64 torch autograd of the step written the torch way."""
    c = R.em_case(name, 65, R.em_ts(name)[-1])
    S = c["S"]
    traj = vo.euler_maruyama(R.ORACLE_KIND[name], c["x0"], c["theta"], c["noise"], c["dt"], c["pos"], np.float64)
    t = c["ch"]                                                  # the step from a clamped state (hit paths) and a free one
    x, e, a = traj[:, t], c["noise"][:, t].astype(np.float64), c["g_traj"][:, t + 1].astype(np.float64)
    assert all(x[b, d] == 1e-6 for b, d in c["hit"])
    xt, tt = torch.tensor(x, requires_grad=True), torch.tensor(c["theta"].astype(np.float64), requires_grad=True)
    et, dt = torch.tensor(e), c["dt"]
    if name == "ou":
        y = xt + tt[:, 0:1] * (tt[:, 1:2] - xt) * dt + tt[:, 2:3] * et * dt ** 0.5
    elif name == "lv":
        u, v = xt[:, 0], xt[:, 1]
        cov00, cov01, cov11 = tt[:, 0] * u + tt[:, 1] * u * v, -tt[:, 1] * u * v, tt[:, 2] * v + tt[:, 1] * u * v
        l00 = torch.sqrt(cov00.clamp(min=1e-6))
        l10 = cov01 / l00.clamp(min=1e-6)
        l11 = torch.sqrt((cov11 - l10 ** 2).clamp(min=1e-6))
        f = torch.stack([tt[:, 0] * u - tt[:, 1] * u * v, tt[:, 1] * u * v - tt[:, 2] * v], 1)
        y = xt + f * dt + torch.stack([l00 * et[:, 0], l10 * et[:, 0] + l11 * et[:, 1]], 1) * dt ** 0.5
    else:
        y = xt - tt[:, :S] * xt * dt + (torch.nn.functional.softplus(tt[:, S:]) + 1e-3) * et * dt ** 0.5
    gx, gt = torch.autograd.grad((y * torch.tensor(a)).sum(), [xt, tt])
    step = R.em_step(name, x, c["theta"], e, dt)
    ax, gth = R.em_step_bwd(name, x, c["theta"], e, R.VM(a), dt)
    for got, want in ((step, y.detach().numpy()), (ax, gx.numpy()), (gth, gt.numpy())):
        assert R.ratio(got.v, want, got.m) * R.C24 <= 1e-12


def test_em_bounds_hold_for_a_correct_float32_evaluation_at_every_gpu_shape():
    (step, adj), (step4, adj4) = em_cpu_ratios()
    print(f"simulator, oracle f32: step {step:.3f}, adjoint {adj:.3f}; kind 4, float32 torch: step {step4:.3f}, adjoint {adj4:.3f}")
    assert max(step, step4) <= R.C_EM_STEP / 4 and adj <= R.C_EM_ADJ / 4 and adj4 <= R.C_EM_ADJ_CRN / 4, (step, adj, step4, adj4)


@pytest.mark.parametrize("name", R.CRN)
def test_crn_step_formula_equals_the_torch_spec(name):
    c = R.em_case(name, 65, R.em_ts(name)[-1])
    traj = R.em_simulate(c, np.float64)
    for t in (0, c["ch"], c["ch"] + 1):                               # free states, and states with the last species on the floor
        args = (name, traj[:, t], c["theta"], c["noise"][:, t], c["dt"])
        f = R.crn_step_formula(*args)
        assert R.ratio(f.v, R.em_step(*args).v, f.m) * R.C24 <= 1e-12


def _em_emulated(c, fwd_defect=None, bwd_defect=None):
    traj = R.em_simulate(c, F32, fwd_defect)
    a, gth = R.em_adjoint(c, traj, F32, bwd_defect)
    return traj, a.v, gth.v


def _em_passes(c, out):
    step, adj = em_ratios(c, *out)
    return step <= R.C_EM_STEP and adj <= R.em_adj_c(c["name"])


@pytest.mark.parametrize("name", list(R.EM_KINDS))
def test_em_emulation_passes_and_defects_are_rejected(name):
    c = R.em_case(name, 130, R.em_ts(name)[-1])                    # a partial third workgroup, two chunk boundaries
    assert _em_passes(c, _em_emulated(c))
    for defect in R.EM_DEFECTS_FWD:
        assert not _em_passes(c, _em_emulated(c, fwd_defect=defect)), defect
    for defect in R.EM_DEFECTS_BWD:
        assert not _em_passes(c, _em_emulated(c, bwd_defect=defect)), defect


@pytest.mark.parametrize("defect", R.EM_DEFECTS_FWD + R.EM_DEFECTS_BWD)
def test_em_defect_is_rejected(defect):
    c = R.em_case("lv", 130, R.em_ts("lv")[-1])
    fwd = defect if defect in R.EM_DEFECTS_FWD else None
    bwd = defect if defect in R.EM_DEFECTS_BWD else None
    assert not _em_passes(c, _em_emulated(c, fwd, bwd))
