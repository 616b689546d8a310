"""CPU: the residual-bridge proposal (``proposal="residual_bridge"``) on the torch route -- the specification -- against the
independent numpy restatement of tests/residual_bridge_reference.py, the n = 1 identity, unbiasedness against the exact Kalman
likelihood, the variance gain on the Lotka-Volterra example, the smoother and particle MCMC with the new proposal, and the guards."""
import ctypes
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import guided_filter_reference as gref
import particle_filter_reference as pref
import residual_bridge_reference as rref
from philox_reference import forecast_noise

CASES = ["ou", "lv", "lv_prey", "sir", "chain4", "autoreg", "chain4_full", "lindiag3"]
PROPOSAL = "residual_bridge"


def _key(k0, k1):
    return torch.from_numpy(np.array([k0, k1], dtype=np.uint32).view(np.int32))


# ------------------------------------------------------------------------------------- 1. torch route against the numpy reference
@pytest.mark.parametrize("name", CASES)
def test_torch_route_matches_the_numpy_reference_in_float64(name):
    """Particles and log_weights, segment by segment, with the tolerances tests/test_guided_filter.py uses for the bridge.  Rows
    [0, 1, 3, 3, 8, 20] for every case: first passes of 1, 2, 5 and 12 steps, a shared row, a segment inside one Philox block and
    segments that cross blocks.  tests/guided_filter_reference.py ends the Lotka-Volterra cases at row 14 because the bridge
    filter's float64 ESS falls to 2 of 64 over the 12 steps 8 -> 20; re-derived here for this proposal on the CPU in float64 (M = 64
    filters, the keys of the GPU test): the residual bridge keeps the 12-step segment.  Smallest float64 ESS over filters and
    observations at N = 64 / at the kernel's largest N: ou 42.1 / 635.7 (of 1024), lv 28.7 / 572.4 (1024), lv_prey 29.7 / 616.0
    (1024), sir 14.2 / 350.2 (1024), chain4 7.1 / 118.0 (512), autoreg 11.4 / 206.0 (1024), chain4_full 8.5 / 100.8 (512), lindiag3
    7.2 / 301.0 (1024): all above N / 20."""
    from viforsdes_amd import particle_filter
    M, N = 8, 16
    rows = rref.rows_of(name)
    sde, obs, like, th, x0, dt, pos = gref.case(name, M, rows=rows)
    key = (0x1234ABCD, 0x0BADF00D + len(name))
    res = particle_filter(sde, obs, like, th.double(), dt, n_particles=N, initial_state=x0.double(), positive_dims=pos,
                          return_particles=True, key=_key(*key), proposal=PROPOSAL)
    K, S = len(rows), sde.state_dim
    assert [b - a for a, b in zip(rows, rows[1:])] == [1, 2, 0, 5, 12]
    assert res.log_weights.shape == (M, K, N) and res.particles.shape == (M, K, N, S) and res.particles.dtype == torch.float64
    parts, anc, lw = res.particles.numpy(), res.ancestors.long().numpy(), res.log_weights.numpy()
    noise = forecast_noise(M * N, rows[-1], S, key)
    theta = np.repeat(th.double().numpy(), N, axis=0)
    H = None if like.obs_matrix is None else like.obs_matrix.double().numpy()
    coef = gref.sde_coefficients(sde)
    for k in range(K):
        if k == 0:
            want_x, want_lr = np.repeat(x0.double().numpy(), N, axis=0), np.zeros(M * N)
        else:
            start = np.take_along_axis(parts[:, k - 1], anc[:, k - 1, :, None], axis=1).reshape(M * N, S)
            z = noise[:, rows[k - 1]:rows[k]]
            want_x, want_lr, _ = rref.residual_segment(coef, start, theta, z, obs.values[k].numpy(), H, like.variance, dt, pos)
        want_lw = want_lr.reshape(M, N) + pref.gaussian_log_weights(obs.values[k].numpy(), want_x.reshape(M, N, S), like.variance, H)
        np.testing.assert_allclose(parts[:, k].reshape(M * N, S), want_x, rtol=1e-9, atol=1e-9 * np.abs(want_x).max())
        np.testing.assert_allclose(lw[:, k], want_lw, rtol=0, atol=1e-8 * max(1.0, np.abs(want_lw).max()))
        for m in range(M):
            inc = pref.observation_stage(lw[m, k], parts[m, k])[0]
            assert abs(float(res.increments[m, k]) - inc) <= 1e-10 * max(1.0, abs(inc))
    assert torch.allclose(res.log_likelihood, res.increments.sum(dim=1))
    again = particle_filter(sde, obs, like, th.double(), dt, n_particles=N, initial_state=x0.double(), positive_dims=pos,
                            key=_key(*key), proposal=PROPOSAL)
    assert torch.equal(again.log_likelihood, res.log_likelihood) and again.log_weights is None      # same key => same result
    if name != "ou":
        # the companion path matters: the bridge's particles are others (the OU drift is linear: there the two agree to rounding)
        bridge = particle_filter(sde, obs, like, th.double(), dt, n_particles=N, initial_state=x0.double(), positive_dims=pos,
                                 return_particles=True, key=_key(*key), proposal="bridge")
        assert not torch.equal(bridge.particles, res.particles)


def test_the_clamp_on_x_binds_in_a_positive_state_case():
    """The Lotka-Volterra case starts every fourth filter with the predators AT the floor, where the data keep them."""
    from viforsdes_amd import particle_filter
    sde, obs, like, th, x0, dt, pos = gref.case("lv", 8, rows=rref.ROWS)
    res = particle_filter(sde, obs, like, th.double(), dt, n_particles=16, initial_state=x0.double(), positive_dims=pos,
                          return_particles=True, key=_key(5, 6), proposal=PROPOSAL)
    parts = res.particles[:, 1:][..., list(pos)]
    assert bool((parts >= 1e-6).all()) and bool((parts == 1e-6).any())


# ------------------------------------------------------------------------------------------------------- 2. the n = 1 identity
@pytest.mark.parametrize("name", ["ou", "lv", "lv_prey", "chain4", "chain4_full", "lindiag3"])
def test_one_step_segments_give_the_fully_adapted_weight(name):
    """n = 1, eta's clamp not binding: the step ratio plus the observation term is log N(y; H (x + f dt), dt H L L^T H^T + v I),
    whatever the normals are."""
    from viforsdes_amd import particle_filter
    M, N, rows = 8, 16, [0, 1, 2, 3, 4]
    sde, obs, like, th, x0, dt, pos = gref.case(name, M, rows=rows, interior=True)
    th, x0 = th.double(), x0.double()
    res = particle_filter(sde, obs, like, th, dt, n_particles=N, initial_state=x0, positive_dims=pos, return_particles=True,
                          key=_key(3, 4), proposal=PROPOSAL)
    S = sde.state_dim
    H = np.eye(S) if like.obs_matrix is None else like.obs_matrix.double().numpy()
    parts, anc = res.particles.numpy(), res.ancestors.long().numpy()
    coef = gref.sde_coefficients(sde)
    theta = np.repeat(th.numpy(), N, axis=0)
    for k in range(1, len(rows)):
        prev = np.take_along_axis(parts[:, k - 1], anc[:, k - 1, :, None], axis=1).reshape(M * N, S)
        _, _, bound = rref.companion_path(coef, prev, theta, 1, dt, pos)
        assert not bound.any()                                                          # eta's clamp did not bind
        f, L = coef(prev, theta)
        HL = np.einsum("ok,bki->boi", H, L)
        cov = dt * np.einsum("boi,bqi->boq", HL, HL) + like.variance * np.eye(H.shape[0])
        want = gref.gaussian_log_density(obs.values[k].numpy(), (prev + f * dt) @ H.T, cov).reshape(M, N)
        np.testing.assert_allclose(res.log_weights[:, k].numpy(), want, rtol=0, atol=1e-9 * max(1.0, np.abs(want).max()))


# --------------------------------------------------------------------------------------------------------------- 3. unbiasedness
def _unbiased(ll, exact, M):
    r = np.exp(ll - exact)
    return abs(r.mean() - 1.0) / (r.std(ddof=1) / math.sqrt(M))


def test_residual_bridge_is_unbiased_on_the_ou_model():
    """exp(log p^) against the float64 Kalman likelihood of the discretised OU model: M = 4096 filters of N = 64, z < 5."""
    from viforsdes_amd import GaussianObservationLikelihood, particle_filter
    from viforsdes_amd.examples.sdes import ou_problem
    M, N, theta, variance = 4096, 64, (0.8, 1.0, 0.5), 0.01
    sde, obs, _, _, _, dt, _, _ = ou_problem()
    rows = np.round(obs.times.numpy() / dt).astype(int)
    exact = gref.ou_kalman(theta, dt, variance, obs.values[0].numpy(), rows, obs.values.numpy())
    th = torch.tensor([theta], dtype=torch.float64).expand(M, 3)
    ll = particle_filter(sde, obs, GaussianObservationLikelihood(variance=variance), th, dt, n_particles=N,
                         initial_state=obs.values[0].double(), key=_key(25, 26), proposal=PROPOSAL).log_likelihood.numpy()
    z = _unbiased(ll, exact, M)
    print(f"OU variance {variance}, N = {N}, residual bridge: std of log p^ {ll.std(ddof=1):.4f}, z {z:.2f}")
    assert z < 5.0


@pytest.mark.parametrize("S,O", [(2, 2), (4, 3)])
def test_residual_bridge_is_unbiased_on_the_linear_diagonal_models(S, O):
    from viforsdes_amd import GaussianObservationLikelihood, Observations, particle_filter
    from viforsdes_amd.examples.sdes import LinearDiagonalSDE
    M, N, dt, rows = 4096, 64, 0.05, [0, 1, 7, 20]
    g = torch.Generator().manual_seed(17 + S)
    H = torch.randn(O, S, generator=g)
    theta = tuple((0.4 + 0.3 * torch.arange(S)).tolist()) + tuple((-1.2 + 0.4 * torch.arange(S)).tolist())
    x0 = 0.5 * torch.randn(S, generator=g)
    obs = Observations(times=torch.tensor(rows) * dt, values=0.3 * torch.randn(len(rows), O, generator=g))
    like = GaussianObservationLikelihood(variance=0.01, obs_matrix=H)
    exact = pref.linear_diagonal_kalman(theta, dt, 0.01, H.numpy(), x0.numpy(), rows, obs.values.numpy())
    ll = particle_filter(LinearDiagonalSDE(S), obs, like, torch.tensor([theta], dtype=torch.float64).expand(M, 2 * S), dt,
                         n_particles=N, initial_state=x0.double(), key=_key(41, S), proposal=PROPOSAL).log_likelihood.numpy()
    z = _unbiased(ll, exact, M)
    print(f"linear-diagonal S={S}, O={O}, residual bridge: exact {exact:.4f}, std of log p^ {ll.std(ddof=1):.4f}, z {z:.2f}")
    assert z < 5.0


# ------------------------------------------------------------------------------------------------------------ 4. variance gain
def test_variance_gain_on_the_lotka_volterra_example():
    """The file's one slow test (three torch-route filters over 400 steps: about 10 s; the suite registers no marker for that).
    The Lotka-Volterra example (400 steps, 5 observations 100 steps apart), theta = (0.5, 0.0025, 0.3), float64, 64 filters of
    128 particles, one key: the standard deviation of log p^ under the residual bridge is at most a quarter of the bootstrap
    filter's and below the bridge's, and its mean log p^ is above the bootstrap filter's."""
    from viforsdes_amd import particle_filter
    from viforsdes_amd.examples.sdes import lv_problem
    M, N = 64, 128
    sde, obs, like, _, _, dt, state_pos, _ = lv_problem()
    th = torch.tensor([[0.5, 0.0025, 0.3]], dtype=torch.float64).expand(M, 3)
    out = {}
    for proposal in ("bootstrap", "bridge", PROPOSAL):
        res = particle_filter(sde, obs, like, th, dt, n_particles=N, initial_state=obs.values[0].double(), positive_dims=state_pos,
                              key=_key(101, 102), proposal=proposal)
        ll = res.log_likelihood.numpy()
        out[proposal] = (ll.mean(), ll.std(ddof=1))
        print(f"LV example, N = {N}, M = {M}, {proposal}: mean log p^ {ll.mean():.2f}, std {ll.std(ddof=1):.2f}, median over filters "
              f"of the smallest ESS {float(res.effective_sample_size.min(dim=1).values.median()):.1f}")
    assert np.isfinite(out[PROPOSAL]).all()
    assert out[PROPOSAL][1] <= 0.25 * out["bootstrap"][1]
    assert out[PROPOSAL][1] < out["bridge"][1]
    assert out[PROPOSAL][0] > out["bootstrap"][0]


# ----------------------------------------------------------------------------------------------------- 5. smoother and PMMH
@pytest.mark.parametrize("name", ["ou", "lv", "sir"])
def test_smoother_paths_pass_through_the_stored_particles(name):
    import particle_smoother_reference as sref
    from viforsdes_amd import Observations, particle_filter, particle_smoother
    M, N, D = 3, 64, 7
    for rows in (sref.BLOCK_ROWS, sref.LATE_ROWS):
        sde, obs, like, th, x0, dt, pos = sref.case(name, M, rows=rows)
        obs = Observations(times=obs.times.double(), values=obs.values.double())
        kw = dict(n_particles=N, initial_state=x0.double(), positive_dims=pos, key=_key(0x51ED270B, 0x2545F491 ^ len(name)),
                  proposal=PROPOSAL)
        sm = particle_smoother(sde, obs, like, th.double(), dt, n_draws=D, **kw)
        pf = particle_filter(sde, obs, like, th.double(), dt, return_particles=True, **kw)
        S, K = x0.shape[1], len(rows)
        assert torch.equal(sm.log_likelihood, pf.log_likelihood) and bool(torch.isfinite(sm.paths).all())
        lin = sm.lineage.long()
        for k in range(K - 1, 0, -1):
            assert torch.equal(lin[:, :, k - 1], torch.gather(pf.ancestors[:, k - 1].long(), 1, lin[:, :, k]))
        assert torch.equal(sm.paths[:, :, 0], x0.double()[:, None, :].expand(M, D, S))
        worst = 0.0
        for k in range(K):
            want = torch.gather(pf.particles[:, k], 1, lin[:, :, k, None].expand(-1, -1, S))
            worst = max(worst, float(((sm.paths[:, :, rows[k]] - want).abs() / want.abs().clamp(min=1e-300)).max()))
        print(f"{name} rows {rows}: replayed state at the observation rows vs stored particle, max relative {worst:.1e}")
        assert worst <= 1e-12                      # the bound tests/test_particle_smoother.py holds the other proposals to


def test_pmmh_theta_chain_is_the_same_with_and_without_paths():
    import particle_mcmc_reference as mref
    from viforsdes_amd import GaussianObservationLikelihood, Observations, Prior, PriorType, particle_mcmc
    from viforsdes_amd.examples.sdes import OrnsteinUhlenbeck
    F64 = torch.float64
    obs = Observations(times=torch.tensor(mref.OU_TIMES, dtype=F64), values=torch.tensor(mref.OU_VALUES, dtype=F64)[:, None])
    prior = Prior(type=PriorType.LOG_NORMAL, mean=mref.OU_PRIOR[1], std=mref.OU_PRIOR[2], dim=3)
    like = GaussianObservationLikelihood(variance=mref.OU_VARIANCE)
    run = lambda proposal, **kw: particle_mcmc(OrnsteinUhlenbeck(), obs, like, prior, mref.OU_DT,
                                               torch.tensor(mref.ou_initial_theta(5), dtype=F64), 6, n_particles=64, filters_per_chain=2,
                                               theta_positive_dims=(0, 1, 2), key=_key(11, 13), proposal=proposal, **kw)
    plain, paths = run(PROPOSAL), run(PROPOSAL, return_paths=True)
    for name in ("samples", "log_likelihood", "log_target", "acceptance_rate"):
        assert torch.equal(getattr(plain, name), getattr(paths, name)), name
    T = mref.OU_ROWS[-1]
    assert plain.paths is None and paths.paths.shape == (6, 5, T + 1, 1) and bool(torch.isfinite(paths.paths).all())
    assert torch.equal(paths.paths[:, :, 0, 0], obs.values[0].expand(6, 5))
    assert bool(torch.isfinite(plain.log_likelihood).all())


# --------------------------------------------------------------------------------------------------------------------- 6. guards
def test_guards():
    from viforsdes_amd import PoissonObservationLikelihood, _hip, particle_filter, particle_mcmc, particle_smoother
    from viforsdes_amd.inference import particle_filter as pf
    assert pf.PROPOSALS == ("bootstrap", "bridge", "residual_bridge")
    sde, obs, like, th, x0, dt, pos = gref.case("ou", 2)
    for fn in (particle_filter, particle_smoother):
        with pytest.raises(ValueError, match="GaussianObservationLikelihood"):
            fn(sde, obs, PoissonObservationLikelihood(), th, dt, n_particles=8, proposal=PROPOSAL)
        with pytest.raises(ValueError, match="proposal"):
            fn(sde, obs, like, th, dt, n_particles=8, proposal="guided")
    from viforsdes_amd import Prior, PriorType
    prior = Prior(type=PriorType.LOG_NORMAL, mean=0.0, std=1.0, dim=3)
    with pytest.raises(ValueError, match="GaussianObservationLikelihood"):
        particle_mcmc(sde, obs, PoissonObservationLikelihood(), prior, dt, th, 2, n_particles=8, proposal=PROPOSAL)
    # the particle limits: the residual rule's own argument, and the other proposals' values as they were
    limit = _hip.particle_filter_max_particles
    for kind, S, want in (("lotka_volterra", 2, 1024), ("ornstein_uhlenbeck", 1, 1024), ("linear_diagonal", 3, 1024),
                          ("linear_diagonal", 4, 512), ("reaction_network", 3, 1024), ("reaction_network", 4, 512)):
        assert limit(kind, S, proposal=PROPOSAL) == want
    assert limit("linear_diagonal", 4, proposal="bridge") == 512 and limit("linear_diagonal", 3, proposal="bridge") == 1024
    assert limit("reaction_network", 4) == 1024 and limit("reaction_network", 5) == 512 and limit("linear_diagonal", 16) == 1024
    with pytest.raises(ValueError, match="proposal"):
        limit("lotka_volterra", 2, proposal="guided")


def test_five_dims_route_to_torch(monkeypatch):
    """S = 5 or O = 5 is not the kernel's: _kernel_route says no even where everything else would qualify (checked on the routing
    function with CUDA-typed stand-ins, no device needed), and the public call returns finite results."""
    from viforsdes_amd import GaussianObservationLikelihood, Observations, particle_filter
    from viforsdes_amd.examples.sdes import LinearDiagonalSDE
    from viforsdes_amd.inference import particle_filter as pf

    class OnDevice:
        """What _kernel_route reads of a tensor, saying it lives on the GPU."""
        def __init__(self, t):
            self.is_cuda, self.dtype, self.shape = True, t.dtype, t.shape

    g = torch.Generator().manual_seed(3)
    for S, O, takes in ((5, 2, False), (2, 5, False), (4, 4, True), (2, 2, True)):
        sde = LinearDiagonalSDE(S)
        H = torch.randn(O, S, generator=g) / 2.0
        like = GaussianObservationLikelihood(variance=0.04, obs_matrix=H)
        obs = Observations(times=torch.tensor([0.0, 0.05, 0.25]), values=0.3 * torch.randn(3, O, generator=g))
        theta = torch.tensor([tuple((0.3 + 0.1 * torch.arange(S)).tolist()) + tuple((-1.0 + 0.2 * torch.arange(S)).tolist())]).expand(4, 2 * S)
        stand_in = SimpleNamespace(times=obs.times, values=OnDevice(obs.values))
        route = pf._kernel_route(sde, stand_in, like, OnDevice(theta), 64, PROPOSAL)
        assert (route is not None) == takes, (S, O)
        if takes:
            assert pf._kernel_route(sde, stand_in, like, OnDevice(theta), 1024 if S < 4 else 512, PROPOSAL) is not None
            assert pf._kernel_route(sde, stand_in, like, OnDevice(theta), 2048 if S < 4 else 1024, PROPOSAL) is None
        res = particle_filter(sde, obs, like, theta, 0.05, n_particles=64, initial_state=0.3 * torch.randn(S, generator=g),
                              key=_key(5, S), proposal=PROPOSAL)
        assert bool(torch.isfinite(res.log_likelihood).all())


BADARG = -1        # include/vsde_hip.h: VSDE_E_BADARG
PTR = ctypes.c_void_p(0x1000)      # "some device pointer": a refused call reads none of them
NULL = ctypes.c_void_p(None)


def _route_args(lib, form, name):
    """(entry point, its leading route arguments, P for S = 2) of one of the three forms of an entry point."""
    from viforsdes_amd import _hip
    if form == "kind":
        return getattr(lib, "vsde_" + name), (ctypes.c_int(3),), 4
    net = _hip.CrnNetwork()
    net.S, net.R = 2, 2
    if form == "crn":
        return getattr(lib, "vsde_crn_" + name), (ctypes.byref(net),), 2
    kin = _hip.CrnKinetics()
    return getattr(lib, "vsde_crn_kinetic_" + name), (ctypes.byref(net), ctypes.byref(kin)), 4


@pytest.mark.parametrize("form", ["kind", "crn", "crn_kinetic"])
def test_residual_entry_points_refuse_bad_arguments_before_any_hip_call(form):
    """The bad arguments tests/test_pmmh_paths.py::_replay tries on the guided anchored replay, on all nine new entry points; the
    pointers are never read, no device needed."""
    from viforsdes_amd import _hip
    lib = _hip.load()
    i, d = ctypes.c_int, ctypes.c_double
    mask = (ctypes.c_uint8 * 32)()

    def anchored(**kw):
        fn, lead, P = _route_args(lib, form, "residual_anchored_replay")
        a = dict(B=4, S=2, P=P, K=3, O=2, T=10, obs_values=PTR, anchors=PTR)
        a.update(kw)
        return fn(*lead, i(a["B"]), i(a["S"]), i(a["P"]), i(a["K"]), i(a["O"]), i(a["T"]), PTR, PTR, PTR, a["obs_values"], NULL, d(0.5),
                  a["anchors"], PTR, PTR, d(0.1), mask, PTR, NULL)

    def replay(**kw):
        fn, lead, P = _route_args(lib, form, "residual_filter_replay")
        a = dict(M=4, N=64, S=2, P=P, K=3, O=2, D=2, T=10, obs_values=PTR, anchors=PTR)
        a.update(kw)
        return fn(*lead, i(a["M"]), i(a["N"]), i(a["S"]), i(a["P"]), i(a["K"]), i(a["O"]), i(a["D"]), i(a["T"]), PTR, PTR, PTR,
                  a["obs_values"], NULL, d(0.5), PTR, d(0.1), mask, a["anchors"], PTR, PTR, PTR, NULL, NULL)

    def filt(**kw):
        fn, lead, P = _route_args(lib, form, "residual_particle_filter")
        a = dict(M=4, N=64, S=2, P=P, K=3, O=2, obs_values=PTR, anchors=PTR)
        a.update(kw)
        return fn(*lead, i(a["M"]), i(a["N"]), i(a["S"]), i(a["P"]), i(a["K"]), i(a["O"]), PTR, PTR, PTR, a["obs_values"], NULL, d(0.5),
                  PTR, d(0.1), mask, PTR, PTR, PTR, a["anchors"], PTR, NULL, NULL, NULL, NULL)

    wide = dict(S=5, P=10, O=5) if form == "kind" else dict(S=5, O=5)
    for fn in (anchored, replay, filt):
        cases = [wide, dict(S=2, O=5), dict(K=0), dict(obs_values=NULL), dict(anchors=NULL)]
        if fn is not filt:
            cases.append(dict(T=-1))
        for kw in cases:
            assert fn(**kw) == BADARG, (fn.__name__, kw)
            assert lib.vsde_last_error()
    assert replay(N=100) == BADARG and b"particles" in lib.vsde_last_error()
    assert filt(N=2048) == BADARG and b"particles" in lib.vsde_last_error()
