"""GPU: the log-weight kernel of csrc/vsde_elbo.hip and the coefficient and forecast kernels of csrc/vsde_sde.hip against the float64
references of tests/sde_aux_reference.py, per element: |got - ref| <= c 2^-24 magnitude with the magnitudes and the c of that module (no bound is
relative to a tensor's maximum), and the log-weight accumulator of csrc/vsde_elbo.hip against float64 logsumexp / ESS / sum.

Every case calls one ``viforsdes_amd._hip`` wrapper directly.  Each float input is a contiguous view at offset 64 of a NaN-filled
1-D buffer; row T of x (which no coefficient kernel may read) and the strict upper triangle of g_diffusion hold NaN, so a read
outside an input turns an output NaN, which no bound admits.  The strict upper triangle of the diffusion factor and row T of g_x
have magnitude zero and must be exactly zero.  Every kernel runs twice and must give the same bits.

Dispatch coverage (case -> instantiation / edge).  log_weights_impl reaches log_weight_kernel<0, S> at S 1..16, <3, S> at S 1..8
(its dispatch goes to 16, but kind 3 has P = 2 S and the tail takes P <= 16: test_log_weights_of_kind_3_refuse_...), <1, 1>, <2, 2>
and <4, S, NR, KIN> on S 1..8 x NR {4, 8, 16} x {mass action, rate laws}, each in a Gaussian and a count form;
route_dispatch<0> of coefficients_fwd / coefficients_bwd / forecast reaches kinds 1, 2, kind 3 once (S at run time), and kind 4
on the same S x NR x KIN grid.  Of the kind-4 grid one network per reaction bound and rate-law flag runs (S 2, 3, 8):

  test_log_weights         k0 S 1..16 at (B 2, T 257)       log_weight_kernel<0, S>, every instantiation; the stride wraps once (t = 256)
                           diag S 1..8 at (B 2, T 257)      log_weight_kernel<3, S>, every reachable instantiation
                           ou, lv                           <1, 1>, <2, 2>; lv: every third path with z = -30 on the prey, both radicands floored
                           sir, net3, chain8                <4, 2, 4>, <4, 3, 8>, <4, 8, 16>, mass action
                           autoreg, repress3, chain8k       <4, 2, 4, true>, <4, 3, 8, true>, <4, 8, 16, true> on rates [B, 2R]
                           poisson (S 2, identity),         log_weight_kernel<0, S, ., false, true>, and <2, 2, ..., true>, <4, 3, 8, false, true>:
                           negbin (matrix, O 16)            vsde_count_log_weights / vsde_crn_count_log_weights; negative predictions bind
                                                            the rate floor
                           k0 S {1, 2, 16} x T {1, 2}       one thread busy; first step = last step
                           ... x T {255, 256}               no stride; every thread one step
                           ... x T {257, 600}               step 256 alone in the second round; two wraps
                           B {1, 2, 3}                      gridDim.x
                           K {0, 1, 5}                      no observation term (empty obs_rows is admitted); row T; rows 0, a repeated row,
                                                            T and T + 3 (clamped to T)
                           obs id / wide / narrow           no matrix; O > S; O < S
                           state masks none/all/alt/last    every bit, bit S - 1 alone; theta masks none / all / bit P - 1; prior normal and
                                                            log-normal
                           path 0, rows 1..5 (kinds 0..3)   -100, -20, 0, 20, 100 on a positive dim: saturated softplus / log_sigmoid

  test_coefficients        ou, lv                           coef_fwd_kernel<1>, <2> / coef_bwd_kernel<1>, <2>
                           diag1, diag5, diag8, diag32      coef_diag_fwd_kernel / coef_diag_bwd_kernel: 256, 51, 32, 8 time slots; S = 5 leaves
                                                            thread 255 idle; one b_i = 25 (softplus threshold branch), one b_i = -25
                           sir, net3, chain8                coef_*_kernel<4, 2, 4>, <4, 3, 8>, <4, 8, 16> (R 2, 5, 9), mass action
                           autoreg, repress3, chain8k       coef_*_kernel<4, 2, 4, true>, <4, 3, 8, true>, <4, 8, 16, true>: Hill n 1..4,
                                                            repression and activation, Michaelis-Menten, fixed and shared constants
                           clamp2                           <4, 2, 4, true> with the modifier at 0 (gradient passes), below 0 (none), above
                           B {1, 3}                         gridDim.x of the backward (workgroup = path)
                           T {1, 255, 256, 257, 600}        forward: B T and B T S are no multiples of 256 (last block partly filled) except
                           (S = 8 networks: 1, 257)         at (1, 256); backward: row t = T written by the thread after the last data row in
                                                            the same stride round (T <= 255) or the next one (T = 256: thread 0, second
                                                            round), two rows in the second round (257), three rounds (600); g_theta through
                                                            the 256-row tree with 1, 255, 256 rows in use
                           lv rows t % 3                    u = 0 (v = 1e-9 on every other: both radicands floored), u = 1e-9 (first radicand
                                                            below half the floor, gate closed), both populations >= 1 (gates open)
  test_forecast            ou, lv  B {1, 255, 256, 257}     forecast_kernel<1>, <2>: one thread; the last thread of a workgroup idle; a full
                                                            workgroup; a second one with one thread
                           ou0                              kappa = 0 from x = 0: step 1 has magnitude sigma sqrt(dt) |z| alone, the bound
                                                            pins each normal to a few ulps
                           diag5 B {51, 52}, diag32, diag1  forecast_kernel<3>: B S = 255, 260 (thread = (path, dim) across the block seam), S = 32
                                                            with mask none / all / bit 31 alone, S = 1
                           sir, net3, chain8, autoreg       forecast_kernel<4, 2, 4>, <4, 3, 8>, <4, 8, 16> (rows written inline, no staging),
                                                            <4, 2, 4, true>
                           T {1, 3, 4, 5, 8, 9}             a partial block; a full one; a one-step second block; two full; a third partial
                           out_steps = 1..T                 the whole trajectory, scored teacher-forced per step
                           subsets [T], [1], [1, 4, 5],     bit for bit the same rows: the last row alone; the early exit on k = K; rows across
                           [4, 4, 8], [9, 9]                a block seam; duplicates on a block's last step; the last partial block only
                           [1, T, T + 1]                    an entry above T gives a NaN row and leaves the other rows' bits unchanged
                           x_start U(0, 1e-3) on positive   the floor is reached (asserted); one path started at NaN poisons that path only
                           dims
  test_accumulator         n {1, 255, 256, 257}             one thread busy; the last idle; all busy; thread 0 strides once
                           all -inf chunk first / last      the merge with M = -inf on either side
                           a +inf entry                     counted non-finite, left out of the sums
"""
import math

import numpy as np
import pytest
import torch

import sde_aux_reference as A
from test_sde_ops_gpu import _count_terms, guarded, same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _np(t):
    return t.cpu().numpy()


# ----------------------------------------------------------------------------------------------------------- log weights
@pytest.mark.parametrize("shape", A.lw_shapes(), ids=lambda s: "-".join(map(str, s)))
def test_log_weights(shape):
    from viforsdes_amd import _hip
    c = A.lw_case(*shape)
    t = {k: guarded(c[k]) for k in ("z", "means", "chol", "drift", "diffusion", "theta", "rates", "obs_values", "obs_matrix", "post_mean",
                                    "post_log_std")}
    rows = torch.tensor(c["obs_rows"], dtype=torch.int32, device=DEV)
    term = _count_terms(c, t["obs_values"]) if c["count"] else c["variance"]
    net = A.network(c["model"])
    run = lambda: _hip.log_weights(c["kind"], t["z"], t["means"], t["chol"], t["drift"], t["diffusion"], t["theta"], rows, t["obs_values"],
                                   t["obs_matrix"], term, c["lognormal"], c["prior_mean"], c["prior_std"], t["post_mean"],
                                   t["post_log_std"], c["pos"], c["theta_pos"], c["dt"], network=net, rates=t["rates"])
    out = run()
    assert same_bits((out,), (run(),))
    r = A.lw_ratio(shape, _np(out))
    print(f"RATIO {'lw_count' if c['count'] else 'lw'} {r:.4f}")
    assert r <= A.lw_c(shape), r


def test_log_weights_of_kind_3_refuse_more_than_8_state_dims():
    """Kind 3 has P = 2 S parameters and the per-sample tail takes P <= 16: S = 9 is an argument error from the host check, before
    any launch, so log_weight_kernel<3, 9..16> cannot be reached."""
    from viforsdes_amd import _hip
    S, B, T = 9, 2, 4
    z = torch.zeros(B, T + 1, S, device=DEV)
    eye = torch.eye(S, device=DEV).expand(B, T, S, S).contiguous()
    rows = torch.zeros(0, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="dims <= 16"):
        _hip.log_weights("linear_diagonal", z, z[:, 1:], eye, None, None, torch.ones(B, 2 * S, device=DEV), rows,
                         torch.zeros(0, S, device=DEV), None, 0.3, 0, 0.0, 1.0, torch.zeros(2 * S, device=DEV),
                         torch.zeros(2 * S, device=DEV), [], [], 0.1)


# ---------------------------------------------------------------------------------------------------------- coefficients
@pytest.mark.parametrize("name,B,T", A.coef_shapes(), ids=lambda v: str(v))
def test_coefficients(name, B, T):
    from viforsdes_amd import _hip
    c = A.coef_case(name, B, T)
    x, th, gf, gG = (guarded(c[k]) for k in ("x", "theta", "g_drift", "g_diffusion"))
    net = A.network(name)
    fwd = lambda: _hip.sde_coefficients_fwd(c["kind"], x, th, network=net)
    bwd = lambda: _hip.sde_coefficients_bwd(c["kind"], x, th, gf, gG, network=net)
    out, grads = fwd(), bwd()
    assert same_bits(out, fwd()) and same_bits(grads, bwd())
    got = dict(zip(A.COEF_OUT, [_np(t) for t in tuple(out) + tuple(grads)]))
    up = np.triu_indices(c["S"], 1)
    assert (got["diffusion"][..., up[0], up[1]] == 0).all()
    assert (got["g_x"][:, T] == 0).all()
    f, v = A.coef_ratios(c, got)
    print(f"RATIO coef_fwd {f:.4f} {'coef_vjp_crn' if A.is_crn(name) else 'coef_vjp'} {v:.4f}")
    assert f <= A.C_COEF_FWD and v <= A.coef_vjp_c(name), (f, v)


# -------------------------------------------------------------------------------------------------------------- forecast
def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("name,B,T,mask", A.fc_shapes(), ids=lambda v: str(v))
def test_forecast(name, B, T, mask):
    from viforsdes_amd import _hip
    c = A.fc_case(name, B, T, mask)
    x0, th = guarded(c["x0"]), guarded(c["theta"])
    key = torch.from_numpy(np.array(c["key"], dtype=np.uint32).view(np.int32)).to(DEV)
    net = A.network(c["model"])

    def run(steps):
        steps = torch.tensor(steps, dtype=torch.int32, device=DEV)
        return _hip.forecast(c["kind"], x0, th, T, steps, key, c["dt"], c["pos"], network=net)

    every = list(range(1, T + 1))
    out = run(every)
    assert same_bits((out,), (run(every),))
    o = _np(out)
    assert A.fc_gates_ok(c, o)
    if c["pos"] and B > 1:
        assert (o == np.float32(A.FLOOR32)).any()                     # the floor is reached
    r = A.fc_ratio(c, o)
    print(f"RATIO {'fc_step_crn' if A.is_crn(c['model']) else 'fc_step'} {r:.4f}")
    assert r <= A.fc_c(name), r
    # the row-writing logic: subsets of the steps give the same bits as the same rows of the all-steps run
    for sub in [(T,), (1,)] + [s for s in A.FC_SUBSETS if max(s) <= T]:
        got = run(list(sub))
        assert torch.equal(_bits(got), _bits(out[:, [s - 1 for s in sub]])), sub
    above = run([1, T, T + 1])
    assert bool(above[:, 2].isnan().all())
    assert torch.equal(_bits(above[:, :2]), _bits(out[:, [0, T - 1]]))


# ----------------------------------------------------------------------------------------------------------- accumulator
@pytest.mark.parametrize("edge", A.ACC_EDGES)
@pytest.mark.parametrize("n", A.ACC_NS)
def test_accumulator(n, edge):
    """Tolerances of tests/test_evidence_gpu.py: log-sum-exp 1e-12, ESS 1e-10, the sum 1e-9, relative."""
    from viforsdes_amd import _hip
    chunks = A.acc_case(n, edge)
    bufs = [guarded(ch) for ch in chunks]                             # what lies beyond n is NaN: it must not count

    def run():
        state = _hip.log_weight_state(torch.device(DEV))
        for buf in bufs:
            _hip.log_weight_accumulate(buf, buf.shape[0], state)
        return state

    s1, s2 = run(), run()
    assert torch.equal(s1.view(torch.int64), s2.view(torch.int64))
    M, a, b, total, count, bad = s1.tolist()
    m, lse, ess, ref_total, ref_count, ref_bad = A.acc_reference(chunks)
    assert M == m and count == ref_count and bad == ref_bad
    if math.isinf(lse):
        assert a == 0.0 and b == 0.0
    else:
        assert abs(M + math.log(a) - lse) <= 1e-12 * abs(lse)
        assert abs(a * a / b - ess) <= 1e-10 * ess
    assert total == ref_total if math.isinf(ref_total) else abs(total - ref_total) <= 1e-9 * abs(ref_total)
