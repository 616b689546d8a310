"""GPU: the ELBO path-term and tail kernels (csrc/vsde_elbo.hip) and the Euler-Maruyama simulator of kinds 1..4
(csrc/vsde_sde.hip) against the float64 references of tests/sde_reference.py, per element:
|got - ref| <= c 2^-24 magnitude with the magnitudes and the c of that module (no bound is relative to a tensor's maximum).

Every case calls one ``viforsdes_amd._hip`` wrapper directly.  Each input is a contiguous view at offset 64 of a NaN-filled 1-D
buffer and the strict upper triangle of the factors holds NaN, so a read outside an input or above a diagonal turns an output
NaN, which no bound admits; g_chol / g_diffusion have magnitude zero above the diagonal and must be exactly zero there.  Every
kernel runs twice and must give the same bits.

Dispatch coverage (case -> instantiation / edge):

  test_path_terms          S 1..16 at (B 3, T 257)          elbo_path_terms_kernel<S> / _bwd_kernel<S>, every instantiation; forward
                                                            stride wraps once (t = 256); backward second block in x holds tau =
                                                            256, 257: the tau-1 role across the block seam and the tau > T guard
                           S {1, 2, 3, 8, 16} x T {1, 2}    first step = last step; tau = T is the only "next" role
                           ... x T {255, 256}               255: one block, no wrap; 256: tau = T = 256 alone in the second block
                           ... x T 600                      two wraps of the forward stride, three blocks of the backward
                           B {1, 3}                         gridDim.x (forward) / gridDim.y (backward) of 1 and more
                           masks none / all / alt / last    jac = 0 exactly; every bit; bit S - 1 alone (bit 15 at S = 16)
                           path 0, rows 1..5                -100, -20, 0, 20, 100 on a positive dimension: saturated log_sigmoid, __expf overflow in the gradient
  test_path_terms_bwd_refuses_...   B = 65536               the host check before the launch (gridDim.y limit)
  test_tail                B {1, 2}                         most threads idle in the 256-row tree sum
                           B {255, 256, 257}                the last thread idle / every thread one path / thread 0 strides once
                           B 700                            two and three paths per thread
                           (S, O, P, matrix) (2, 2, 3, -)   identity observation; (3, 16, 16, yes) O > S, P = kTailMaxDim, mask bit 15;
                           (16, 1, 5, yes) O < S, S = kTailMaxDim; (16, 16, 16, -) all three at kTailMaxDim
                           K {0, 1, 5}                      no observation term (NULL x_obs) / one row / several
                           prior normal / log-normal, theta mask none / all / bit P - 1
                           count, B 257                     elbo_tail_fwd_kernel<true> / _bwd_kernel<true>: Poisson (identity, S 2) and negative
                                                            binomial (matrix, O 16) through vsde_count_elbo_tail_fwd / _bwd; negative
                                                            predictions bind the rate floor
  test_simulator           ou, lv                           em_fwd_kernel<1>, <2> / em_bwd_kernel<1>, <2>, CH = 32
                           diag5, diag8                     em_diag_fwd_kernel / em_diag_bwd_kernel at S = 5, 8 (B S across a 256-thread block at B 63 .. 130)
                           net3, chain8                     em_fwd_kernel<4, 3, NR> / em_bwd_kernel<4, 3, NR> (CH 16) and <4, 8, NR> (CH 8)
                           B {1, 63, 64, 65, 130}           rows = min(64, B - b0): 1, 63, 64, 64 + 1, 64 + 64 + 2
                           T {1, CH-1, CH, CH+1, 2 CH + 3}  one partial chunk; a full one; a one-step second chunk; three chunks
                           clamp sites CH, CH + 1, T        the clamped entry in the +1 row the backward stages at a chunk boundary,
                                                            the first step of the next chunk, the last step
"""
import numpy as np
import pytest
import torch

import sde_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64


def guarded(a):
    """``a`` on the GPU as a contiguous view at a non-zero offset of a NaN-filled 1-D buffer (None stays None)."""
    if a is None:
        return None
    a = np.ascontiguousarray(a, np.float32)
    buf = torch.full((a.size + 2 * GUARD,), float("nan"), device=DEV, dtype=torch.float32)
    view = buf[GUARD:GUARD + a.size].view(a.shape)
    view.copy_(torch.from_numpy(a))
    assert view.is_contiguous() and view.storage_offset() == GUARD
    return view


def same_bits(first, second):
    return all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(first, second))


def _np(t):
    return t.cpu().numpy()


# ------------------------------------------------------------------------------------------------------------ path terms
@pytest.mark.parametrize("S,B,T,mask", R.path_shapes(), ids=lambda v: str(v))
def test_path_terms(S, B, T, mask):
    from viforsdes_amd import _hip
    c = R.path_case(S, B, T, mask)
    args = [guarded(c[k]) for k in ("z", "x", "means", "chol", "drift", "diffusion")]
    ups = [guarded(c[k]) for k in ("g_sde", "g_gen", "g_jac")]
    fwd = _hip.elbo_path_terms(*args, c["pos"], c["dt"])
    bwd = _hip.elbo_path_terms_bwd(*args, c["pos"], c["dt"], *ups)
    assert same_bits(fwd, _hip.elbo_path_terms(*args, c["pos"], c["dt"]))
    assert same_bits(bwd, _hip.elbo_path_terms_bwd(*args, c["pos"], c["dt"], *ups))
    got = dict(zip(R.PATH_NAMES + R.PATH_GRADS, [_np(t) for t in fwd + bwd]))
    up = np.triu_indices(S, 1)
    for k in ("g_chol", "g_diffusion"):
        assert (got[k][..., up[0], up[1]] == 0).all(), k
    f, b = R.path_ratios(c, got)
    print(f"RATIO path_fwd {f:.4f} path_bwd {b:.4f}")
    assert f <= R.C_PATH_FWD and b <= R.C_PATH_BWD, (f, b)


def test_path_terms_bwd_refuses_more_paths_than_grid_rows():
    """B = 65536 does not fit gridDim.y: an argument error from the host check, before any launch."""
    from viforsdes_amd import _hip
    B = 65536
    z = torch.zeros(B, 2, 1, device=DEV)
    one = torch.ones(B, 1, 1, device=DEV)
    g = torch.ones(B, device=DEV)
    with pytest.raises(ValueError, match="at most 65535 paths"):
        _hip.elbo_path_terms_bwd(z, z, one, one.view(B, 1, 1, 1), one, one.view(B, 1, 1, 1), [], 0.1, g, g, g)


# ------------------------------------------------------------------------------------------------------------------ tail
def _count_terms(c, obs_values):
    """What the count entry points take in place of the variance: the package's own row constants for these observations."""
    from viforsdes_amd import NegativeBinomialObservationLikelihood, PoissonObservationLikelihood
    H = None if c["obs_matrix"] is None else torch.from_numpy(c["obs_matrix"]).to(DEV)
    if c["count"] == "poisson":
        like = PoissonObservationLikelihood(scale=R.COUNT_SCALE, obs_matrix=H)
    else:
        like = NegativeBinomialObservationLikelihood(scale=R.COUNT_SCALE, dispersion=R.COUNT_DISPERSION, obs_matrix=H)
    return tuple(like.kernel_terms(obs_values))


@pytest.mark.parametrize("B,dims,K,lognormal,mask,count", [s + (None,) for s in R.tail_shapes()] + list(R.COUNT_SHAPES),
                         ids=lambda v: str(v))
def test_tail(B, dims, K, lognormal, mask, count):
    from viforsdes_amd import _hip
    c = R.tail_case(B, dims, K, lognormal, mask, count)
    t = {k: guarded(c[k]) for k in ("x_obs", "obs_values", "obs_matrix", "theta", "post_mean", "post_log_std", "sde_lp", "gen_lp",
                                    "jac", "g_out")}
    term = _count_terms(c, t["obs_values"]) if count else c["variance"]
    head = (t["x_obs"], t["obs_values"], t["obs_matrix"], term, t["theta"], c["lognormal"], c["prior_mean"], c["prior_std"],
            t["post_mean"], t["post_log_std"], c["pos"])
    fwd = lambda: (_hip.elbo_tail_fwd(*head, t["sde_lp"], t["gen_lp"], t["jac"]),)
    bwd = lambda: _hip.elbo_tail_bwd(*head, t["g_out"])
    out, grads = fwd(), bwd()
    assert same_bits(out, fwd()) and same_bits(grads, bwd())
    got = dict(zip(R.TAIL_OUT, [_np(v) for v in out + tuple(grads)]))
    r = R.tail_ratio(c, got)
    print(f"RATIO tail {r:.4f}")
    assert r <= R.C_TAIL, r


# ------------------------------------------------------------------------------------------------------------- simulator
@pytest.mark.parametrize("name,B,T", R.em_shapes(), ids=lambda v: str(v))
def test_simulator(name, B, T):
    from viforsdes_amd import _hip
    c = R.em_case(name, B, T)
    x0, theta, noise, g_traj = (guarded(c[k]) for k in ("x0", "theta", "noise", "g_traj"))
    net = R.crn_sde(name).network_descriptor() if name in R.CRN else None
    run = lambda: _hip.euler_maruyama_fwd(c["kind"], x0, theta, noise, c["dt"], c["pos"], network=net)
    traj = run()
    back = lambda: _hip.euler_maruyama_bwd(c["kind"], theta, noise, traj, g_traj, c["dt"], c["pos"], network=net)
    grads = back()
    assert same_bits((traj,), (run(),)) and same_bits(grads, back())
    tr = _np(traj)
    assert R.em_clamped_at_sites(c, tr)                             # the clamp is exercised at every site
    step, adj = R.em_ratios(c, tr, _np(grads[0]), _np(grads[1]))
    print(f"RATIO em_step {step:.4f} {'em_adj_crn' if name in R.CRN else 'em_adj'} {adj:.4f}")
    assert step <= R.C_EM_STEP and adj <= R.em_adj_c(name), (step, adj)
