"""CPU: the guided (bridge) particle filter's torch route -- the specification -- against the independent numpy restatement of
tests/guided_filter_reference.py, the n = 1 identity, unbiasedness and the variance gain against the exact Kalman likelihood, the
unchanged bootstrap results, the errors, and ``reweight_parameters(proposal="bridge")``."""
import math

import numpy as np
import pytest
import torch

import guided_filter_reference as gref
from philox_reference import forecast_noise

CASES = ["ou", "lv", "lv_prey", "sir", "chain4", "autoreg", "chain4_full", "lindiag3"]


def _key(k0, k1):
    return torch.from_numpy(np.array([k0, k1], dtype=np.uint32).view(np.int32))


def _ou(M, variance, theta=(0.8, 1.0, 0.5)):
    from viforsdes_amd import GaussianObservationLikelihood
    from viforsdes_amd.examples.sdes import ou_problem
    sde, obs, _, _, _, dt, _, _ = ou_problem()
    th = torch.tensor([theta], dtype=torch.float64).expand(M, 3)
    rows = np.round(obs.times.numpy() / dt).astype(int)
    exact = gref.ou_kalman(theta, dt, variance, obs.values[0].numpy(), rows, obs.values.numpy())
    return sde, obs, GaussianObservationLikelihood(variance=variance), th, dt, exact


@pytest.mark.parametrize("name", CASES)
def test_torch_route_matches_the_numpy_reference_in_float64(name):
    from viforsdes_amd import particle_filter
    M, N = 8, 16
    sde, obs, like, th, x0, dt, pos = gref.case(name, M)
    key = (0x1234ABCD, 0x0BADF00D + len(name))
    res = particle_filter(sde, obs, like, th.double(), dt, n_particles=N, initial_state=x0.double(), positive_dims=pos,
                          return_particles=True, key=_key(*key), proposal="bridge")
    rows = gref.rows_of(name)
    K, S = len(rows), sde.state_dim
    assert res.log_weights.shape == (M, K, N) and res.particles.shape == (M, K, N, S) and res.particles.dtype == torch.float64
    parts, anc, lw = res.particles.numpy(), res.ancestors.long().numpy(), res.log_weights.numpy()
    noise = forecast_noise(M * N, rows[-1], S, key)
    theta = np.repeat(th.double().numpy(), N, axis=0)
    H = None if like.obs_matrix is None else like.obs_matrix.double().numpy()
    coef = gref.sde_coefficients(sde)
    from particle_filter_reference import gaussian_log_weights, observation_stage
    for k in range(K):
        if k == 0:
            want_x, want_lr = np.repeat(x0.double().numpy(), N, axis=0), np.zeros(M * N)
        else:
            start = np.take_along_axis(parts[:, k - 1], anc[:, k - 1, :, None], axis=1).reshape(M * N, S)
            z = noise[:, rows[k - 1]:rows[k]]
            want_x, want_lr = gref.guided_segment(coef, start, theta, z, obs.values[k].numpy(), H, like.variance, dt, pos)
        want_lw = want_lr.reshape(M, N) + gaussian_log_weights(obs.values[k].numpy(), want_x.reshape(M, N, S), like.variance, H)
        np.testing.assert_allclose(parts[:, k].reshape(M * N, S), want_x, rtol=1e-9, atol=1e-9 * np.abs(want_x).max())
        np.testing.assert_allclose(lw[:, k], want_lw, rtol=0, atol=1e-8 * max(1.0, np.abs(want_lw).max()))
        for m in range(M):
            inc = observation_stage(lw[m, k], parts[m, k])[0]
            assert abs(float(res.increments[m, k]) - inc) <= 1e-10 * max(1.0, abs(inc))
    assert torch.allclose(res.log_likelihood, res.increments.sum(dim=1))
    again = particle_filter(sde, obs, like, th.double(), dt, n_particles=N, initial_state=x0.double(), positive_dims=pos,
                            key=_key(*key), proposal="bridge")
    assert torch.equal(again.log_likelihood, res.log_likelihood) and again.log_weights is None      # same key => same result


@pytest.mark.parametrize("name", ["ou", "lv", "lv_prey", "chain4", "chain4_full", "lindiag3"])
def test_one_step_segments_give_the_fully_adapted_weight(name):
    """n = 1: the step ratio plus the observation term is log N(y; H (x + f dt), dt H L L^T H^T + v I), whatever the normals are."""
    from viforsdes_amd import particle_filter
    M, N, rows = 8, 16, [0, 1, 2, 3, 4]
    sde, obs, like, th, x0, dt, pos = gref.case(name, M, rows=rows, interior=True)            # no clamp binds
    th, x0 = th.double(), x0.double()
    res = particle_filter(sde, obs, like, th, dt, n_particles=N, initial_state=x0, positive_dims=pos, return_particles=True,
                          key=_key(3, 4), proposal="bridge")
    S = sde.state_dim
    H = np.eye(S) if like.obs_matrix is None else like.obs_matrix.double().numpy()
    parts, anc = res.particles.numpy(), res.ancestors.long().numpy()
    if pos:
        assert (parts[..., list(pos)] > gref.STATE_FLOOR).all()
    coef = gref.sde_coefficients(sde)
    for k in range(1, len(rows)):
        prev = np.take_along_axis(parts[:, k - 1], anc[:, k - 1, :, None], axis=1).reshape(M * N, S)
        f, L = coef(prev, np.repeat(th.numpy(), N, axis=0))
        HL = np.einsum("ok,bki->boi", H, L)
        cov = dt * np.einsum("boi,bqi->boq", HL, HL) + like.variance * np.eye(H.shape[0])
        want = gref.gaussian_log_density(obs.values[k].numpy(), (prev + f * dt) @ H.T, cov).reshape(M, N)
        np.testing.assert_allclose(res.log_weights[:, k].numpy(), want, rtol=0, atol=1e-9 * max(1.0, np.abs(want).max()))


def test_bridge_is_unbiased_and_less_noisy_than_bootstrap_on_the_ou_model():
    """exp(log p^) is unbiased against the float64 Kalman likelihood (M = 4096 filters, z < 5) for both proposals; with the
    observation variance 0.01 the float64 bootstrap route's standard deviation of log p^ is more than 3x the bridge's (the
    condition that makes the comparison meaningful), and the bridge's is the smaller."""
    from viforsdes_amd import particle_filter
    M, N = 4096, 64
    sde, obs, like, th, dt, exact = _ou(M, 0.01)
    x0 = obs.values[0].double()
    out = {}
    for proposal, key in (("bootstrap", (21, 22)), ("bridge", (23, 24))):
        ll = particle_filter(sde, obs, like, th, dt, n_particles=N, initial_state=x0, key=_key(*key),
                             proposal=proposal).log_likelihood.numpy()
        r = np.exp(ll - exact)
        z = abs(r.mean() - 1.0) / (r.std(ddof=1) / math.sqrt(M))
        out[proposal] = (ll.std(ddof=1), z)
        print(f"OU variance 0.01, N = {N}, {proposal}: std of log p^ {ll.std(ddof=1):.4f}, mean exp(log p^ - exact) {r.mean():.4f}, z {z:.2f}")
    assert out["bridge"][1] < 5.0 and out["bootstrap"][1] < 5.0
    print(f"std ratio bootstrap / bridge: {out['bootstrap'][0] / out['bridge'][0]:.1f}")
    assert out["bootstrap"][0] >= 3.0 * out["bridge"][0]                      # the case is one where the proposal matters
    assert out["bridge"][0] < out["bootstrap"][0]


def test_bootstrap_results_are_what_they_were():
    from viforsdes_amd import particle_filter
    from viforsdes_amd.inference import particle_filter as pf
    sde, obs, like, th, x0, dt, pos = gref.case("lv", 4)
    kw = dict(n_particles=32, initial_state=x0, positive_dims=pos, return_particles=True, key=_key(9, 10))
    a = particle_filter(sde, obs, like, th, dt, **kw)
    b = particle_filter(sde, obs, like, th, dt, proposal="bootstrap", **kw)
    c = pf._torch_filter(sde, obs, like, th, float(dt), 32, x0, pos, True, _key(9, 10))
    for name in ("log_likelihood", "increments", "effective_sample_size", "filtered_mean", "filtered_std", "particles", "ancestors"):
        assert torch.equal(getattr(a, name), getattr(b, name)) and torch.equal(getattr(a, name), getattr(c, name)), name
    # the new field: the Gaussian log-weight of the stored particles
    want = like.log_prob(obs.values[None, :, None, :].expand(4, -1, 32, -1).reshape(-1, 2), a.particles.reshape(-1, 2)).reshape(4, -1, 32)
    assert torch.equal(a.log_weights, want)
    assert pf.ParticleFilterResult(*[getattr(a, n) for n in ("log_likelihood", "increments", "effective_sample_size", "filtered_mean",
                                                             "filtered_std", "particles", "ancestors")]).log_weights is None
    bridge = particle_filter(sde, obs, like, th, dt, proposal="bridge", **kw)
    assert not torch.equal(bridge.particles, a.particles)


def test_errors():
    from viforsdes_amd import _hip, particle_filter
    sde, obs, like, th, x0, dt, pos = gref.case("ou", 2)
    with pytest.raises(ValueError, match="proposal"):
        particle_filter(sde, obs, like, th, dt, n_particles=8, proposal="guided")

    class Laplace:
        def log_prob(self, observations, state):
            return -(observations - state).abs().sum(dim=-1)

    assert particle_filter(sde, obs, Laplace(), th, dt, n_particles=8).log_likelihood.shape == (2,)
    with pytest.raises(ValueError, match="GaussianObservationLikelihood"):
        particle_filter(sde, obs, Laplace(), th, dt, n_particles=8, proposal="bridge")
    assert _hip.particle_filter_max_particles("lotka_volterra", 2) == _hip.particle_filter_max_particles("lotka_volterra", 2, proposal="bootstrap")
    assert _hip.particle_filter_max_particles("lotka_volterra", 2, proposal="bridge") == 1024
    assert _hip.particle_filter_max_particles("linear_diagonal", 3, proposal="bridge") == 1024
    assert _hip.particle_filter_max_particles("linear_diagonal", 4, proposal="bridge") == 512
    assert _hip.particle_filter_max_particles("reaction_network", 4, proposal="bridge") == 512
    assert _hip.particle_filter_max_particles("reaction_network", 4) == 1024
    with pytest.raises(ValueError, match="proposal"):
        _hip.particle_filter_max_particles("lotka_volterra", 2, proposal="guided")


def test_reweight_parameters_takes_the_bridge_on_a_cpu_posterior():
    from viforsdes_amd import EncoderConfig, HeadConfig
    from viforsdes_amd.examples.sdes import ou_problem
    from viforsdes_amd.inference.exponential_moving_average import ExponentialMovingAverage
    from viforsdes_amd.inference.state_space import StateSpace
    from viforsdes_amd.models.variational_sde_posterior import VariationalSDEPosterior
    from viforsdes_amd.posterior.variational_posterior import VariationalPosterior
    torch.manual_seed(0)
    sde, obs, like, prior, horizon, dt, _, theta_pos = ou_problem()
    model = VariationalSDEPosterior(obs.values.shape[1], 1, 3, EncoderConfig(hidden_dim=32, cond_dim=32, num_heads=4, depth=1),
                                    HeadConfig(hidden_dim=32, num_layers=1), theta_pos)
    vp = VariationalPosterior(model=model, exponential_moving_average=ExponentialMovingAverage(model), prior=prior,
                              observations=obs, time_horizon=horizon, time_step=dt, state_space=StateSpace(1, []),
                              evidence_lower_bound_history=[], device=torch.device("cpu"))
    torch.manual_seed(3)
    rw = vp.reweight_parameters(sde, like, n_samples=16, n_particles=32, chunk_size=8, proposal="bridge")
    assert rw.n_nonfinite == 0 and bool(torch.isfinite(rw.log_weights).all()) and math.isfinite(rw.log_evidence)
    with pytest.raises(ValueError, match="proposal"):
        vp.reweight_parameters(sde, like, n_samples=4, n_particles=8, proposal="guided")
