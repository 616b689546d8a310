"""CPU: the torch route of ``particle_filter`` (the specification) and ``VariationalPosterior.reweight_parameters``.

* exp(log p^) is unbiased: against the Kalman filter of the discretised Ornstein-Uhlenbeck / linear-diagonal models, z < 5.
* Mechanics: keys, the sum of the increments, systematic resampling's defining properties, NaN and dead filters, edge sizes, and
  the noise stream element by element against tests/philox_reference.py.
* reweight_parameters reproduces the formulae of EvidenceEstimate and float64 numpy moments / quantiles when the filter is replaced
  by the exact likelihood, and agrees with that value when it is not."""
import math

import numpy as np
import pytest
import torch

import particle_filter_reference as ref
from philox_reference import forecast_noise

KEY = (0x1234ABCD, 0xDEADBEEF)


def _key(k0, k1):
    return torch.from_numpy(np.array([k0, k1], dtype=np.uint32).view(np.int32))


def _ou():
    from viforsdes_amd.examples.sdes import ou_problem
    sde, obs, like, _, _, dt, _, _ = ou_problem()
    return sde, obs, like, dt


def _z_of_ratio(log_hat, exact):
    r = np.exp(np.asarray(log_hat, dtype=np.float64) - exact)
    se = r.std(ddof=1) / math.sqrt(r.size)
    return abs(r.mean() - 1.0) / se, r.std(ddof=1) / r.mean()


# ------------------------------------------------------------------------------------------- 1. unbiased against the exact value
@pytest.mark.parametrize("theta", [(0.8, 1.0, 0.5), (1.5, 0.5, 1.0), (0.3, 2.0, 0.3)])
def test_ou_likelihood_is_unbiased(theta):
    from viforsdes_amd import particle_filter
    sde, obs, like, dt = _ou()
    M, N = 512, 1024
    rows = np.round(obs.times.numpy() / dt).astype(int)
    exact = ref.ou_kalman(theta, dt, like.variance, obs.values[0].numpy(), rows, obs.values.numpy())
    res = particle_filter(sde, obs, like, torch.tensor([theta]).expand(M, 3), dt, n_particles=N, key=_key(11, int(theta[0] * 100)))
    z, cv = _z_of_ratio(res.log_likelihood.numpy(), exact)
    print(f"OU theta {theta}: exact {exact:.4f}, mean log p^ {float(res.log_likelihood.mean()):.4f}, cv {cv:.3f}, z {z:.2f}, "
          f"min particle ESS {float(res.effective_sample_size.min()):.0f}")
    assert cv < 0.3          # the z-test's condition
    assert z < 5.0


def test_linear_diagonal_likelihood_with_obs_matrix_is_unbiased():
    from viforsdes_amd import GaussianObservationLikelihood, Observations, particle_filter
    from viforsdes_amd.examples.sdes import LinearDiagonalSDE
    sde, dt, M, N = LinearDiagonalSDE(2), 0.05, 512, 1024
    H = torch.tensor([[1.0, 0.5], [-0.3, 2.0]])
    obs = Observations(times=torch.tensor([0.0, 1.0, 2.0]), values=torch.tensor([[0.5, -0.3], [0.2, 0.1], [-0.4, 0.6]]))
    like = GaussianObservationLikelihood(variance=0.09, obs_matrix=H)
    theta = (0.7, 0.4, -0.5, -1.0)
    x0 = torch.tensor([0.6, -0.1])
    exact = ref.linear_diagonal_kalman(theta, dt, 0.09, H.numpy(), x0.numpy(), [0, 20, 40], obs.values.numpy())
    res = particle_filter(sde, obs, like, torch.tensor([theta]).expand(M, 4), dt, n_particles=N, initial_state=x0, key=_key(5, 6))
    z, cv = _z_of_ratio(res.log_likelihood.numpy(), exact)
    print(f"linear-diagonal: exact {exact:.4f}, mean log p^ {float(res.log_likelihood.mean()):.4f}, cv {cv:.3f}, z {z:.2f}")
    assert cv < 0.3
    assert z < 5.0


# ------------------------------------------------------------------------------------------------------------------ 2. mechanics
def _lv_run(key, M=3, N=256, **kw):
    from viforsdes_amd import GaussianObservationLikelihood, Observations, particle_filter
    from viforsdes_amd.examples.sdes import LotkaVolterra
    obs = Observations(times=torch.tensor([0.0, 1.0, 2.0, 2.0, 3.5]),          # two observations on one grid row
                       values=torch.tensor([[71.0, 79.0], [80.0, 70.0], [95.0, 75.0], [90.0, 78.0], [100.0, 90.0]]))
    like = GaussianObservationLikelihood(variance=400.0)
    theta = torch.tensor([0.5, 0.0025, 0.3]) * (1.0 + 0.05 * torch.arange(M)[:, None])
    return like, obs, particle_filter(LotkaVolterra(), obs, like, theta, 0.1, n_particles=N, positive_dims=(0, 1),
                                      return_particles=True, key=key, **kw)


def test_keys_increments_and_shapes():
    _, obs, a = _lv_run(_key(1, 2))
    _, _, b = _lv_run(_key(1, 2))
    _, _, c = _lv_run(_key(1, 3))
    M, N, K = 3, 256, 5
    assert a.log_likelihood.shape == (M,) and a.increments.shape == (M, K) and a.effective_sample_size.shape == (M, K)
    assert a.filtered_mean.shape == (M, K, 2) and a.filtered_std.shape == (M, K, 2)
    assert a.particles.shape == (M, K, N, 2) and a.ancestors.shape == (M, K, N) and a.ancestors.dtype == torch.int32
    for f in ("log_likelihood", "increments", "effective_sample_size", "filtered_mean", "filtered_std", "particles", "ancestors"):
        assert torch.equal(getattr(a, f), getattr(b, f)), f
    assert not torch.equal(a.log_likelihood, c.log_likelihood) and not torch.equal(a.ancestors, c.ancestors)
    assert torch.allclose(a.increments.sum(dim=1), a.log_likelihood, rtol=1e-6, atol=1e-5)
    assert bool(torch.isfinite(a.log_likelihood).all())
    assert bool((a.effective_sample_size > 0).all()) and bool((a.effective_sample_size <= N * (1 + 1e-5)).all())
    # all particles start at the first observation: full ESS and zero spread at row 0; zero steps between observations 2 and 3
    assert torch.allclose(a.effective_sample_size[:, 0], torch.full((M,), float(N)))
    assert bool((a.filtered_std[:, 0] == 0).all())
    anc2 = a.ancestors[:, 2].long()
    moved = torch.gather(a.particles[:, 2], 1, anc2[..., None].expand(-1, -1, 2))
    assert torch.equal(a.particles[:, 3], moved)
    from viforsdes_amd import particle_filter
    from viforsdes_amd.examples.sdes import LotkaVolterra
    like, obs, _ = _lv_run(_key(1, 2))
    plain = particle_filter(LotkaVolterra(), obs, like, torch.tensor([0.5, 0.0025, 0.3]), 0.1, n_particles=64, positive_dims=(0, 1))
    assert plain.particles is None and plain.ancestors is None and plain.log_likelihood.shape == (1,)


def test_default_key_comes_from_the_torch_generator():
    from viforsdes_amd import particle_filter
    sde, obs, like, dt = _ou()
    th = torch.tensor([[0.8, 1.0, 0.5]])
    torch.manual_seed(3)
    a = particle_filter(sde, obs, like, th, dt, n_particles=64)
    torch.manual_seed(3)
    b = particle_filter(sde, obs, like, th, dt, n_particles=64)
    c = particle_filter(sde, obs, like, th, dt, n_particles=64)
    assert torch.equal(a.log_likelihood, b.log_likelihood) and not torch.equal(b.log_likelihood, c.log_likelihood)


def test_systematic_resampling_properties():
    like, obs, res = _lv_run(_key(7, 8), M=4, N=512)
    N = 512
    anc = res.ancestors.long()
    assert bool((anc >= 0).all()) and bool((anc < N).all())
    assert bool((anc[..., 1:] >= anc[..., :-1]).all())                      # non-decreasing in j
    worst = 0.0
    for m in range(4):
        for k in range(obs.values.shape[0]):
            lw = ref.gaussian_log_weights(obs.values[k].numpy(), res.particles[m, k].numpy(), like.variance)
            w = np.exp(lw - lw.max())
            counts = np.bincount(anc[m, k].numpy(), minlength=N)
            worst = max(worst, float(np.abs(counts - N * w / w.sum()).max()))
    print(f"systematic resampling: largest |count - N w / sum w| = {worst:.4f}")
    assert worst < 1.0 + 1e-3           # each particle gets floor or ceil of its expected count (fp32 weights: 1e-3 of slack)


def test_nan_particles_get_zero_weight():
    from viforsdes_amd import GaussianObservationLikelihood, Observations, make_sde, particle_filter
    drift = lambda x, th: torch.where(x > 2.3, torch.full_like(x, float("nan")), th[..., 0:1] * (th[..., 1:2] - x))
    diffusion = lambda x, th: th[..., 2:3].reshape(x.shape[0], 1, 1)
    sde = make_sde(drift, diffusion, 1, 3)
    obs = Observations(times=torch.tensor([0.0, 0.5, 1.0]), values=torch.tensor([[2.0], [1.8], [1.7]]))
    like = GaussianObservationLikelihood(variance=0.5)
    res = particle_filter(sde, obs, like, torch.tensor([[0.5, 1.0, 0.8]]), 0.05, n_particles=256, return_particles=True, key=_key(2, 9))
    bad = torch.isnan(res.particles[0, :, :, 0])                          # [K, N]
    assert bool(bad[1].any()) and not bool(bad[1].all())                  # some particles crossed into the NaN region
    assert bool(torch.isfinite(res.increments).all()) and bool(torch.isfinite(res.filtered_mean).all())
    assert bool(torch.isfinite(res.filtered_std).all())
    for k in (1, 2):
        chosen = res.ancestors[0, k].long()
        assert not bool(bad[k][chosen].any())                             # a NaN particle is nobody's ancestor
    good = int((~bad[1]).sum())
    assert float(res.effective_sample_size[0, 1]) <= good


def test_dead_filter_and_edge_sizes():
    from viforsdes_amd import Observations, particle_filter
    sde, obs, like, dt = _ou()
    x0 = torch.tensor([[2.0], [float("nan")]])
    res = particle_filter(sde, obs, like, torch.tensor([[0.8, 1.0, 0.5]]).expand(2, 3), dt, n_particles=64, initial_state=x0,
                          return_particles=True, key=_key(4, 4))
    assert bool(torch.isfinite(res.log_likelihood[0])) and float(res.log_likelihood[1]) == float("-inf")
    assert bool(torch.isneginf(res.increments[1]).all()) and bool((res.effective_sample_size[1] == 0).all())
    assert torch.equal(res.ancestors[1], torch.arange(64, dtype=torch.int32).expand(6, 64))
    assert bool(torch.isnan(res.filtered_mean[1]).all())
    # one particle: the increments are the observation densities of the single path; one observation
    one = particle_filter(sde, obs, like, torch.tensor([0.8, 1.0, 0.5]), dt, n_particles=1, return_particles=True, key=_key(4, 4))
    lp = like.log_prob(obs.values, one.particles[0, :, 0])
    assert torch.allclose(one.increments[0], lp, atol=1e-6) and bool((one.ancestors == 0).all())
    assert torch.allclose(one.effective_sample_size, torch.ones(1, 6))
    single = Observations(times=obs.times[3:4], values=obs.values[3:4])
    k1 = particle_filter(sde, single, like, torch.tensor([0.8, 1.0, 0.5]), dt, n_particles=128, initial_state=torch.tensor([2.0]),
                         key=_key(4, 4))
    assert k1.increments.shape == (1, 1) and bool(torch.isfinite(k1.log_likelihood).all())


def test_noise_stream_and_uniforms_are_the_specified_ones():
    from viforsdes_amd import GaussianObservationLikelihood, Observations, particle_filter
    from viforsdes_amd.examples.sdes import OrnsteinUhlenbeck
    from viforsdes_amd.inference import particle_filter as pf
    M, N, T = 3, 64, 9
    obs = Observations(times=torch.arange(T + 1, dtype=torch.float32), values=torch.zeros(T + 1, 1))
    like = GaussianObservationLikelihood(variance=25.0)
    # kappa = 0, sigma = 1, dt = 1: x_{t+1} - x_t = z_t, with an observation (and a resampling) on every grid row
    res = particle_filter(OrnsteinUhlenbeck(), obs, like, torch.tensor([[0.0, 0.0, 1.0]]).expand(M, 3), 1.0, n_particles=N,
                          return_particles=True, key=_key(*KEY))
    x = res.particles[..., 0].double()                                        # [M, K, N], before resampling at k
    start = torch.gather(x[:, :-1], 2, res.ancestors[:, :-1].long())          # after resampling at k - 1
    z = (x[:, 1:] - start).permute(0, 2, 1).reshape(M * N, T).numpy()         # path b = m N + j
    want = forecast_noise(M * N, T, 1, KEY)[:, :, 0]
    err = np.abs(z - want).max()
    print(f"noise stream: max |z - z_ref| = {err:.2e}")
    assert err < 1e-5
    u = np.stack([pf.resampling_uniforms(M, k, _key(*KEY)).numpy() for k in range(T + 1)], axis=1)
    assert np.array_equal(u, ref.resampling_uniforms(M, T + 1, KEY))
    assert u.dtype == np.float32 and (u > 0).all() and (u <= 1).all()
    # the ancestors are those of the specified uniforms (float64 resampling of the float64 weights of the same particles)
    diff = total = 0
    for m in range(M):
        for k in range(T + 1):
            lw = ref.gaussian_log_weights([0.0], res.particles[m, k].numpy(), 25.0)
            want_anc = ref.systematic_ancestors(np.exp(lw - lw.max()), u[m, k])
            d = np.abs(want_anc - res.ancestors[m, k].numpy())
            assert d.max() <= 1
            diff, total = diff + int((d != 0).sum()), total + N
    assert diff <= max(1, total // 1000)


def test_path_normals_of_given_paths_and_per_row_keys_are_rows_of_the_stream():
    from viforsdes_amd.inference import particle_filter as pf
    key, S = _key(*KEY), 3
    paths = torch.tensor([130, 7, 191, 0, 64, 65, 7], dtype=torch.int64)      # a permuted subset, one index twice
    for block in (0, 5):
        want = pf.stream_normals(192, block, S, key)
        assert want.shape == (192, S, 4) and want.dtype == torch.float64 and bool(torch.isfinite(want).all())
        assert torch.equal(pf.path_normals(paths, block, S, key), want[paths])
        assert torch.equal(pf.path_normals(paths, block, S, key.expand(len(paths), 2)), want[paths])


def test_validation():
    from viforsdes_amd import particle_filter
    from viforsdes_amd.examples.sdes import LinearDiagonalSDE
    sde, obs, like, dt = _ou()
    th = torch.tensor([[0.8, 1.0, 0.5]])
    with pytest.raises(ValueError, match="n_particles"):
        particle_filter(sde, obs, like, th, dt, n_particles=0)
    with pytest.raises(ValueError, match="time_step"):
        particle_filter(sde, obs, like, th, 0.0)
    with pytest.raises(ValueError, match="theta"):
        particle_filter(sde, obs, like, torch.ones(2, 4), dt)
    with pytest.raises(ValueError, match="initial_state"):
        particle_filter(sde, obs, like, th, dt, initial_state=torch.ones(3, 1))
    with pytest.raises(ValueError, match="initial_state"):
        particle_filter(LinearDiagonalSDE(2), obs, like, torch.ones(1, 4), dt)     # 1-D observations, 2-D state: no default start
    with pytest.raises(ValueError, match="key"):
        particle_filter(sde, obs, like, th, dt, key=torch.zeros(3, dtype=torch.int32))


# ----------------------------------------------------------------------------------------------------------- 3. posterior check
def _cpu_posterior():
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
    return sde, like, vp


def _exact_filter(sde, observations, observation_likelihood, theta, time_step, n_particles=1024, initial_state=None, **kw):
    from viforsdes_amd import ParticleFilterResult
    rows = np.round(observations.times.numpy() / time_step).astype(int)
    ll = [ref.ou_kalman(t, time_step, observation_likelihood.variance, initial_state.numpy(), rows, observations.values.numpy())
          for t in theta.double().numpy()]
    M, K = theta.shape[0], len(rows)
    return ParticleFilterResult(torch.tensor(ll, dtype=theta.dtype), torch.zeros(M, K), torch.full((M, K), float(n_particles)),
                                torch.zeros(M, K, 1), torch.zeros(M, K, 1))


def test_reweighting_reproduces_the_formulae_with_exact_weights(monkeypatch):
    from viforsdes_amd.inference import particle_filter as pf
    from viforsdes_amd.posterior.variational_posterior import QUANTILE_LEVELS, EvidenceEstimate
    sde, like, vp = _cpu_posterior()
    monkeypatch.setattr(pf, "particle_filter", _exact_filter)
    n = 400
    torch.manual_seed(21)
    r = vp.reweight_parameters(sde, like, n_samples=n, n_particles=64, chunk_size=150)
    assert vp._captured == {} and vp._calls == {}
    torch.manual_seed(21)
    with torch.no_grad(), vp.exponential_moving_average.apply():
        theta = vp.model.sde_parameter_posterior.rsample(n)
        log_q = vp.model.sde_parameter_posterior.log_prob(theta).double().numpy()
    assert torch.equal(theta, r.sde_parameters)
    th = theta.double().numpy()
    log_prior = (-0.5 * th * th - 0.5 * math.log(2.0 * math.pi)).sum(axis=1)                    # Normal(0, 1) on each coordinate
    lw = log_prior + r.log_likelihood.double().numpy() - log_q
    # the package evaluates the prior and q densities in the draws' fp32: a few roundings of 6e-8 on terms of the size of lw itself
    assert np.allclose(r.log_weights.numpy(), lw, rtol=1e-5, atol=1e-5)
    lw = r.log_weights.numpy()
    m = lw.max()
    e = np.exp(lw - m)
    want = EvidenceEstimate.from_state([m, e.sum(), (e * e).sum(), lw.sum(), n, 0])
    assert r.n_samples == n and r.n_nonfinite == 0
    assert abs(r.log_evidence - want.log_evidence) < 1e-6
    assert abs(r.effective_sample_size - want.effective_sample_size) < 1e-6 * n
    assert abs(r.standard_error - want.standard_error) < 1e-6
    wn = e / e.sum()
    mean = (wn[:, None] * th).sum(axis=0)
    std = np.sqrt((wn[:, None] * (th - mean) ** 2).sum(axis=0))
    assert np.allclose(r.mean.numpy(), mean, rtol=1e-5, atol=1e-6) and np.allclose(r.std.numpy(), std, rtol=1e-5, atol=1e-6)
    for level, got in zip(QUANTILE_LEVELS, (r.quantiles.q05, r.quantiles.q25, r.quantiles.q50, r.quantiles.q75, r.quantiles.q95)):
        for d in range(3):
            order = np.argsort(th[:, d], kind="stable")
            cdf = np.cumsum(wn[order])
            q = th[order, d][min(int((cdf < level).sum()), n - 1)]
            assert abs(float(got[d]) - q) < 1e-6, (level, d)
    assert np.allclose(r.variational_mean.numpy(), th.mean(axis=0), atol=1e-5)
    assert np.allclose(r.variational_std.numpy(), th.std(axis=0, ddof=1), atol=1e-5)
    assert r.filter_effective_sample_size.shape == (n,)
    short = vp.reweight_parameters(sde, like, n_samples=10, n_particles=64, return_draws=False)
    assert short.sde_parameters is None and short.log_likelihood is None and short.log_weights is None


def test_reweighting_with_the_real_filter_agrees_with_the_exact_weights(monkeypatch):
    from viforsdes_amd.inference import particle_filter as pf
    sde, like, vp = _cpu_posterior()
    n = 256
    torch.manual_seed(22)
    real = vp.reweight_parameters(sde, like, n_samples=n, n_particles=256, chunk_size=100)
    monkeypatch.setattr(pf, "particle_filter", _exact_filter)
    torch.manual_seed(23)
    exact = vp.reweight_parameters(sde, like, n_samples=n, n_particles=256, chunk_size=100)
    se = math.sqrt(real.standard_error ** 2 + exact.standard_error ** 2)
    print(f"log evidence: particle filter {real.log_evidence:.3f} +- {real.standard_error:.3f} (ESS {real.effective_sample_size:.1f}), "
          f"exact likelihood {exact.log_evidence:.3f} +- {exact.standard_error:.3f} (ESS {exact.effective_sample_size:.1f})")
    assert math.isfinite(real.log_evidence) and math.isfinite(exact.log_evidence)
    assert abs(real.log_evidence - exact.log_evidence) < 5.0 * se
    assert bool((real.filter_effective_sample_size > 0).all()) and bool((real.filter_effective_sample_size <= 256 * (1 + 1e-5)).all())


def test_reweighting_validation():
    from viforsdes_amd.examples.sdes import LinearDiagonalSDE
    sde, like, vp = _cpu_posterior()
    with pytest.raises(ValueError, match="state_dim"):
        vp.reweight_parameters(LinearDiagonalSDE(2), like, n_samples=8)
    with pytest.raises(ValueError, match="n_samples"):
        vp.reweight_parameters(sde, like, n_samples=0)


# ------------------------------------------------------------------------------------------------------------------------ ABI
def test_entry_points_refuse_bad_arguments_before_any_hip_call():
    """No GPU here: the checks return VSDE_E_BADARG (-1) with every pointer NULL, so nothing was launched or dereferenced."""
    import ctypes
    from viforsdes_amd import _hip
    lib = _hip.load()
    null, dbl = ctypes.c_void_p(None), ctypes.c_double

    def plain(kind, M, N, S, P, K, O):
        return lib.vsde_particle_filter(*(ctypes.c_int(v) for v in (kind, M, N, S, P, K, O)), *([null] * 5), dbl(0.1), null, dbl(0.05),
                                        *([null] * 9))

    for args, word in [((1, 4, 100, 1, 3, 6, 1), b"particles"), ((1, 4, 2048, 1, 3, 6, 1), b"particles"),
                       ((3, 4, 64, 17, 34, 6, 17), b"state_dim"), ((3, 4, 64, 2, 4, 6, 17), b"obs_dim"),
                       ((1, 4, 64, 1, 3, 0, 1), b"K=0"), ((7, 4, 64, 1, 3, 6, 1), b"kind"), ((2, 4, 64, 1, 3, 6, 1), b"Lotka"),
                       ((1, 4, 64, 1, 3, 6, 1), b"NULL")]:
        assert plain(*args) == -1 and word in lib.vsde_last_error(), (args, lib.vsde_last_error())
    net = _hip.CrnNetwork()
    net.S, net.R = 2, 17
    tail = [ctypes.c_int(v) for v in (4, 64, 2, 17, 6, 2)] + [null] * 5 + [dbl(0.1), null, dbl(0.05)] + [null] * 9
    assert lib.vsde_crn_particle_filter(ctypes.byref(net), *tail) == -1 and b"reactions" in lib.vsde_last_error()
    kin = _hip.CrnKinetics()
    kin.law[0] = 9
    net.R = 2
    tail[3] = ctypes.c_int(4)
    assert lib.vsde_crn_kinetic_particle_filter(ctypes.byref(net), ctypes.byref(kin), *tail) == -1
    assert b"law code" in lib.vsde_last_error()
