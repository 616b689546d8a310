"""GPU: the particle-filter kernel (csrc/vsde_filter.hip) through ``_hip.particle_filter`` and the public ``particle_filter``, and
``VariationalPosterior.reweight_parameters`` on the device.

The kernel is compared STAGE BY STAGE against float64 on its own previous stage, never the whole filter at once: one flipped
ancestor legitimately changes everything after it.

* propagation: particles before resampling at observation k against a float64 Euler-Maruyama segment (reference noise) started
  from the kernel's particles at k - 1 gathered through the kernel's ancestors: 2e-4 of the largest magnitude (the forecast bound);
* weights and summaries from the kernel's particles in float64: increments within 1e-5 max(1, largest finite |lw|); ESS, mean, std
  to 1e-4 relative -- the mean relative to the weighted mean of |x| (the size of the terms of its sum: a mean near zero has no
  relative accuracy of its own), the std with a floor of 1e-6 of that size (the fp32 rounding of the mean it is taken around);
* ancestors against float64 systematic resampling of those weights with the specified uniform: at most 1e-3 of the entries
  differ, each by exactly 1, and they never decrease in j; the float64 particle ESS is asserted above N / 20 at every observation.
* z-scores below 5 for the unbiasedness of exp(log p^) (M = 4096) and for kernel route against torch route."""
import math

import numpy as np
import pytest
import torch

import particle_filter_reference as ref
from philox_reference import forecast_noise

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FLOOR = float(np.float32(1e-6))
SIR = dict(reactants=[[1, 1], [0, 1]], products=[[0, 2], [0, 0]])
AUTOREG_KW = dict(reactants=[[0, 0], [1, 0], [1, 0], [0, 1]], products=[[1, 0], [1, 1], [0, 0], [0, 0]], species=["M", "P"],
                  reactions=["transcription", "translation", "mRNA decay", "protein decay"],
                  rate_constants=["k_tx", "k_tl", 0.1, "d_P"])


def _key(k0, k1, dev=DEV):
    return torch.from_numpy(np.array([k0, k1], dtype=np.uint32).view(np.int32)).to(dev)


def _autoreg():
    from viforsdes_amd import Hill, ReactionNetworkSDE
    return ReactionNetworkSDE(**AUTOREG_KW, rate_laws={"transcription": Hill("P", K="K", n=2, repression=True)})


def _case(name, M=64):
    """(sde, observations, likelihood, theta [M, P], x0 [M, S], dt, positive dims) on the CPU."""
    from viforsdes_amd import GaussianObservationLikelihood, Observations, ReactionNetworkSDE
    from viforsdes_amd.examples.sdes import LinearDiagonalSDE, LotkaVolterra, ou_problem
    g = torch.Generator().manual_seed(29)
    jitter = lambda base, rel: torch.tensor(base) * (1.0 + rel * (2.0 * torch.rand(M, len(base), generator=g) - 1.0))
    if name == "ou":
        sde, obs, like, _, _, dt, _, _ = ou_problem()
        return sde, obs, like, jitter([0.8, 1.0, 0.5], 0.2), obs.values[0].expand(M, 1).clone(), dt, ()
    if name == "lv":          # observations near the model's own mean at the classical parameters (a variance of 1.0 as in the example
        # starves a bootstrap filter: DESIGN section 7); every 4th filter starts from populations at the 1e-6 floor
        obs = Observations(times=torch.tensor([0.0, 10.0, 20.0, 20.0, 40.0]),
                           values=torch.tensor([[71.0, 79.0], [50.0, 390.0], [115.0, 63.0], [110.0, 66.0], [140.0, 95.0]]))
        x0 = obs.values[0].expand(M, 2).clone()
        x0[::4] = torch.rand(len(x0[::4]), 2, generator=g) * 1e-3
        return LotkaVolterra(), obs, GaussianObservationLikelihood(variance=3600.0), jitter([0.5, 0.0025, 0.3], 0.03), x0, 0.1, (0, 1)
    if name == "lindiag16":
        S, O = 16, 5
        sde = LinearDiagonalSDE(S)
        H = torch.randn(O, S, generator=g) / 4.0
        obs = Observations(times=torch.tensor([0.0, 0.5, 1.0, 2.0]), values=torch.randn(4, O, generator=g) * 0.3)
        th = torch.cat([0.2 + torch.rand(M, S, generator=g), -1.0 + 0.5 * torch.randn(M, S, generator=g)], 1)
        x0 = 0.5 * torch.randn(M, S, generator=g)
        pos = (0, 3, 9, 15)
        x0[:, pos] = x0[:, pos].abs() * 0.02
        return sde, obs, GaussianObservationLikelihood(variance=0.5, obs_matrix=H), th, x0, 0.05, pos
    if name == "sir":
        sde = ReactionNetworkSDE(**SIR, species=["S", "I"], reactions=["infection", "removal"])
        obs = Observations(times=torch.tensor([0.0, 1.0, 2.0, 3.0, 5.0]),
                           values=torch.tensor([[95.0, 5.0], [93.0, 6.0], [90.5, 6.5], [88.0, 7.5], [83.0, 8.5]]))
        x0 = obs.values[0].expand(M, 2).clone()
        x0[::4, 1] = 1e-3        # hardly anyone infected: I sits at the floor
        return sde, obs, GaussianObservationLikelihood(variance=64.0), jitter([0.004, 0.25], 0.1), x0, 0.05, (0, 1)
    assert name == "autoreg"
    obs = Observations(times=torch.tensor([0.0, 5.0, 10.0, 15.0, 20.0]),
                       values=torch.tensor([[5.0, 20.0], [20.0, 44.0], [18.0, 65.0], [14.5, 71.0], [12.5, 70.0]]))
    return (_autoreg(), obs, GaussianObservationLikelihood(variance=100.0), jitter([20.0, 0.5, 0.1, 15.0], 0.1),
            obs.values[0].expand(M, 2).clone(), 0.1, (0, 1))


def _run(name, N, key, M=64):
    from viforsdes_amd import particle_filter
    sde, obs, like, th, x0, dt, pos = _case(name, M)
    res = particle_filter(sde, obs.to(DEV), like, th.to(DEV), dt, n_particles=N, initial_state=x0.to(DEV), positive_dims=pos,
                          return_particles=True, key=_key(*key))
    return sde, obs, like, th, x0, dt, pos, res


_RUNS = {}


def _cached(name, N):
    if (name, N) not in _RUNS:
        from viforsdes_amd import _hip
        from viforsdes_amd.inference import particle_filter as pf
        calls = []
        real = _hip.particle_filter
        _hip.particle_filter = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
        try:
            key = (0x9E3779B9 ^ N, 0x7F4A7C15 + len(name))
            _RUNS[(name, N)] = _run(name, N, key) + (key,)
        finally:
            _hip.particle_filter = real
        assert calls == [1] and pf.HIP_FILTER                    # the public function took the kernel route
    return _RUNS[(name, N)]


CASES = ["ou", "lv", "lindiag16", "sir", "autoreg"]
SIZES = [64, 1024]


# ------------------------------------------------------------------------------------------------------------- 4. propagation
@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("name", CASES)
def test_propagation_matches_float64_euler_maruyama(name, N):
    from viforsdes_amd.core.euler_maruyama import euler_maruyama
    sde, obs, like, th, x0, dt, pos, res, key = _cached(name, N)
    M, K, S = th.shape[0], obs.values.shape[0], sde.state_dim
    rows = np.round(obs.times.numpy() / dt).astype(int)
    parts, anc = res.particles.double().cpu(), res.ancestors.long().cpu()
    assert bool(torch.isfinite(parts).all())
    assert torch.equal(parts[:, 0], x0.double()[:, None, :].expand(M, N, S))
    noise = torch.from_numpy(forecast_noise(M * N, int(rows[-1]), S, key))
    theta = th.double()[:, None, :].expand(M, N, th.shape[1]).reshape(M * N, -1)
    worst = 0.0
    for k in range(1, K):
        start = torch.gather(parts[:, k - 1], 1, anc[:, k - 1, :, None].expand(-1, -1, S)).reshape(M * N, S)
        n = int(rows[k] - rows[k - 1])
        if n == 0:
            assert torch.equal(parts[:, k].reshape(M * N, S), start)
            continue
        assert n <= 400
        want = euler_maruyama(sde, start, theta, n * dt, dt, pos, noise=noise[:, rows[k - 1]:rows[k]])[:, -1]
        worst = max(worst, float((parts[:, k].reshape(M * N, S) - want).abs().max() / want.abs().max()))
    print(f"{name} N={N}: propagation max error {worst:.2e} of the largest magnitude")
    assert worst < 2e-4
    if pos:
        assert bool((parts[..., list(pos)] >= FLOOR).all())
    if name in ("lv", "sir", "lindiag16"):
        assert bool((parts[:, 1:] == FLOOR).any())                 # the clamp was exercised


# --------------------------------------------------------------------------------------------------- 5. weights and summaries
@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("name", CASES)
def test_weights_and_summaries_match_float64_on_the_kernels_particles(name, N):
    sde, obs, like, th, x0, dt, pos, res, key = _cached(name, N)
    M, K = th.shape[0], obs.values.shape[0]
    H = None if like.obs_matrix is None else like.obs_matrix.double().numpy()
    parts = res.particles.double().cpu().numpy()
    got = [t.double().cpu().numpy() for t in (res.increments, res.effective_sample_size, res.filtered_mean, res.filtered_std)]
    e_inc = e_ess = e_mean = e_std = 0.0
    for m in range(M):
        for k in range(K):
            lw = ref.gaussian_log_weights(obs.values[k].numpy(), parts[m, k], like.variance, H)
            inc, ess, mean, std, w = ref.observation_stage(lw, parts[m, k])
            size = (w[:, None] * np.abs(parts[m, k])).sum(axis=0) / w.sum()          # weighted mean of |x|, per dim
            e_inc = max(e_inc, abs(got[0][m, k] - inc) / max(1.0, np.abs(lw[np.isfinite(lw)]).max()))
            e_ess = max(e_ess, abs(got[1][m, k] - ess) / ess)
            e_mean = max(e_mean, float((np.abs(got[2][m, k] - mean) / np.maximum(size, 1e-30)).max()))
            e_std = max(e_std, float((np.abs(got[3][m, k] - std) / (std + 1e-2 * size + 1e-30)).max()))
    print(f"{name} N={N}: increments {e_inc:.2e} (of max(1, |lw|)), ESS {e_ess:.2e}, mean {e_mean:.2e}, std {e_std:.2e} (relative)")
    assert e_inc < 1e-5
    assert e_ess < 1e-4 and e_mean < 1e-4 and e_std < 1e-4       # std: |error| <= 1e-4 std + 1e-6 size
    total = res.increments.double().sum(dim=1)
    assert torch.allclose(res.log_likelihood.double(), total, rtol=1e-6, atol=1e-5 * float(res.increments.abs().max()))


# --------------------------------------------------------------------------------------------------------------- 6. ancestors
@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("name", CASES)
def test_ancestors_match_float64_systematic_resampling(name, N):
    sde, obs, like, th, x0, dt, pos, res, key = _cached(name, N)
    M, K = th.shape[0], obs.values.shape[0]
    H = None if like.obs_matrix is None else like.obs_matrix.double().numpy()
    parts = res.particles.double().cpu().numpy()
    anc = res.ancestors.cpu().numpy().astype(np.int64)
    assert anc.min() >= 0 and anc.max() < N
    assert (np.diff(anc, axis=-1) >= 0).all()                                      # never decrease in j
    u = ref.resampling_uniforms(M, K, key)
    differ, low = 0, float("inf")
    for m in range(M):
        for k in range(K):
            lw = ref.gaussian_log_weights(obs.values[k].numpy(), parts[m, k], like.variance, H)
            w = np.exp(lw - lw.max())
            low = min(low, w.sum() ** 2 / (w * w).sum())
            d = np.abs(anc[m, k] - ref.systematic_ancestors(w, u[m, k]))
            assert d.max() <= 1, (m, k, int(d.max()))
            differ += int((d != 0).sum())
    print(f"{name} N={N}: {differ} of {anc.size} ancestors differ from float64 ({differ / anc.size:.1e}); smallest float64 ESS {low:.1f}")
    assert low > N / 20                                                            # there was something to compare
    assert differ <= 1e-3 * anc.size


# -------------------------------------------------------------------------------------------------------------- 7. statistics
def test_likelihood_is_unbiased_on_the_device():
    from viforsdes_amd import GaussianObservationLikelihood, Observations, particle_filter
    from viforsdes_amd.examples.sdes import LinearDiagonalSDE, ou_problem
    M, N = 4096, 1024
    sde, obs, like, _, _, dt, _, _ = ou_problem()
    rows = np.round(obs.times.numpy() / dt).astype(int)
    for theta in [(0.8, 1.0, 0.5), (1.5, 0.5, 1.0), (0.3, 2.0, 0.3)]:
        exact = ref.ou_kalman(theta, dt, like.variance, obs.values[0].numpy(), rows, obs.values.numpy())
        res = particle_filter(sde, obs.to(DEV), like, torch.tensor([theta], device=DEV).expand(M, 3), dt, n_particles=N,
                              key=_key(11, int(theta[0] * 100)))
        r = np.exp(res.log_likelihood.double().cpu().numpy() - exact)
        z, cv = abs(r.mean() - 1.0) / (r.std(ddof=1) / math.sqrt(M)), r.std(ddof=1) / r.mean()
        print(f"OU theta {theta}: exact {exact:.4f}, cv {cv:.3f}, z {z:.2f}")
        assert cv < 0.3 and z < 5.0
    sde2 = LinearDiagonalSDE(2)
    H = torch.tensor([[1.0, 0.5], [-0.3, 2.0]])
    obs2 = Observations(times=torch.tensor([0.0, 1.0, 2.0]), values=torch.tensor([[0.5, -0.3], [0.2, 0.1], [-0.4, 0.6]]))
    like2 = GaussianObservationLikelihood(variance=0.09, obs_matrix=H)
    theta, x0 = (0.7, 0.4, -0.5, -1.0), torch.tensor([0.6, -0.1])
    exact = ref.linear_diagonal_kalman(theta, 0.05, 0.09, H.numpy(), x0.numpy(), [0, 20, 40], obs2.values.numpy())
    res = particle_filter(sde2, obs2.to(DEV), like2, torch.tensor([theta], device=DEV).expand(M, 4), 0.05, n_particles=N,
                          initial_state=x0.to(DEV), key=_key(5, 6))
    r = np.exp(res.log_likelihood.double().cpu().numpy() - exact)
    z, cv = abs(r.mean() - 1.0) / (r.std(ddof=1) / math.sqrt(M)), r.std(ddof=1) / r.mean()
    print(f"linear-diagonal: exact {exact:.4f}, cv {cv:.3f}, z {z:.2f}")
    assert cv < 0.3 and z < 5.0


def test_kernel_route_and_torch_route_agree_on_the_sir_network(monkeypatch):
    from viforsdes_amd import particle_filter
    from viforsdes_amd.inference import particle_filter as pf
    M, N = 512, 256
    sde, obs, like, th, x0, dt, pos = _case("sir", M)
    th, x0 = th[1:2].expand(M, 2).contiguous(), x0[1:2].expand(M, 2).contiguous()
    run = lambda k: particle_filter(sde, obs.to(DEV), like, th.to(DEV), dt, n_particles=N, initial_state=x0.to(DEV),
                                    positive_dims=pos, key=_key(*k)).log_likelihood.double().cpu().numpy()
    a = run((31, 32))
    monkeypatch.setattr(pf, "HIP_FILTER", False)
    b = run((33, 34))
    z = abs(a.mean() - b.mean()) / math.sqrt(a.var(ddof=1) / M + b.var(ddof=1) / M)
    print(f"SIR: mean log p^ kernel {a.mean():.4f}, torch {b.mean():.4f}, two-sample z {z:.2f}")
    assert z < 5.0


# ------------------------------------------------------------------------------------------------------------------ 8. capture
def test_graph_replays_take_a_fresh_key():
    from viforsdes_amd import _hip
    sde, obs, like, th, x0, dt, pos = _case("lv", 16)
    th, x0, values = th.to(DEV), x0.to(DEV), obs.values.to(DEV)
    rows = torch.round(obs.times / dt).to(torch.int32).to(DEV)

    def launch(key=None):
        if key is None:
            key = torch.randint(-2 ** 31, 2 ** 31, (2,), device=DEV, dtype=torch.int32)
        return key, _hip.particle_filter("lotka_volterra", x0, th, rows, values, None, like.variance, key, dt, 128, pos,
                                         return_particles=True)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        key_s, out_s = launch()
    replays = []
    for _ in range(2):
        graph.replay()
        replays.append((key_s.clone(), [o.clone() for o in out_s]))
    torch.cuda.synchronize()
    (k1, o1), (k2, o2) = replays
    assert not torch.equal(k1, k2) and not torch.equal(o1[0], o2[0])
    for k, o in replays:
        for got, want in zip(launch(k)[1], o):
            assert torch.equal(got, want)


# --------------------------------------------------------------------------------------------------------------- 9. end to end
def test_reweighting_and_log_evidence_agree_after_a_short_fit():
    from viforsdes_amd import (EncoderConfig, GaussianObservationLikelihood, HeadConfig, InferenceConfig, Prior, PriorType,
                               TrainingConfig, infer)
    from viforsdes_amd.console import Console
    from viforsdes_amd.examples.sdes import ou_problem
    sde, obs, _, _, horizon, dt, _, _ = ou_problem()
    like = GaussianObservationLikelihood(variance=0.5)                       # the fit of tests/test_evidence_gpu.py, shorter
    prior = Prior(type=PriorType.LOG_NORMAL, mean=0.0, std=0.5, dim=3)
    cfg = InferenceConfig(training=TrainingConfig(time_step=dt, batch_size=256, n_iterations=2000, learning_rate=2e-3,
                                                  sde_param_lr=2e-2),
                          encoder=EncoderConfig(hidden_dim=32, cond_dim=32, num_heads=4, depth=1),
                          head=HeadConfig(hidden_dim=32, num_layers=1), sde_param_positive_dims=[0, 1, 2],
                          mixed_precision=False, console=Console(enabled=False), seed=1)
    vp = infer(sde, obs, like, prior, horizon, cfg)
    torch.manual_seed(5)
    rw = vp.reweight_parameters(sde, like, n_samples=4096, n_particles=512, chunk_size=1024)
    assert vp._captured == {} and vp._calls == {}
    ev = vp.log_evidence(sde, like, n_samples=8192, chunk_size=2048)
    se = max(math.hypot(rw.standard_error, ev.standard_error), 0.05)
    print(f"log p(y): theta reweighting {rw.log_evidence:.4f} +- {rw.standard_error:.4f} (ESS {rw.effective_sample_size:.0f} / 4096, "
          f"smallest particle ESS {float(rw.filter_effective_sample_size.min()):.0f}), path importance sampling "
          f"{ev.log_evidence:.4f} +- {ev.standard_error:.4f} (ESS {ev.effective_sample_size:.0f} / 8192)")
    assert rw.n_nonfinite == 0 and rw.sde_parameters.shape == (4096, 3) and rw.sde_parameters.is_cuda
    assert abs(rw.log_evidence - ev.log_evidence) < 5.0 * se
    assert bool(torch.isfinite(rw.mean).all()) and bool((rw.std > 0).all())
    assert bool((rw.quantiles.q05 <= rw.quantiles.q50).all()) and bool((rw.quantiles.q50 <= rw.quantiles.q95).all())


def test_autoregulation_filter_never_calls_python_propensities(monkeypatch):
    from viforsdes_amd import particle_filter
    from viforsdes_amd.core import reaction_network
    calls = {"propensities": 0}
    real = reaction_network.propensities

    def counting(*a, **k):
        calls["propensities"] += 1
        return real(*a, **k)

    monkeypatch.setattr(reaction_network, "propensities", counting)
    sde, obs, like, th, x0, dt, pos = _case("autoreg", 32)
    res = particle_filter(sde, obs.to(DEV), like, th.to(DEV), dt, n_particles=256, initial_state=x0.to(DEV), positive_dims=pos)
    assert bool(torch.isfinite(res.log_likelihood).all()) and calls["propensities"] == 0
    # 5..8 species: the kernel takes up to 512 particles, 1024 go the torch route (and call the Python propensities)
    from viforsdes_amd import _hip
    assert _hip.particle_filter_max_particles("reaction_network", 8) == 512 and _hip.particle_filter_max_particles("reaction_network", 4) == 1024


# ----------------------------------------------------------------------------------------------------------------------- 10. ABI
def test_bad_arguments_are_refused():
    from viforsdes_amd import _hip
    sde, obs, like, th, x0, dt, pos = _case("ou", 4)
    th, x0, values = th.to(DEV), x0.to(DEV), obs.values.to(DEV)
    rows = torch.round(obs.times / dt).to(torch.int32).to(DEV)
    key = _key(1, 2)
    call = lambda kind="ornstein_uhlenbeck", N=64, x0=x0, th=th, rows=rows, values=values, H=None, network=None: _hip.particle_filter(
        kind, x0, th, rows, values, H, 0.1, key, dt, N, (), network=network)
    assert call()[0].shape == (4,)
    for N in (0, 32, 100, 1088, 2048):
        with pytest.raises(ValueError, match="particles"):
            call(N=N)
    with pytest.raises(ValueError, match="state_dim"):
        call("linear_diagonal", x0=torch.zeros(4, 17, device=DEV), th=torch.zeros(4, 34, device=DEV), values=torch.zeros(6, 17, device=DEV))
    with pytest.raises(ValueError, match="obs_dim"):
        call("linear_diagonal", x0=torch.zeros(4, 2, device=DEV), th=torch.zeros(4, 4, device=DEV), values=torch.zeros(6, 17, device=DEV),
             H=torch.zeros(17, 2, device=DEV))
    with pytest.raises(ValueError, match="K="):
        call(rows=rows[:0], values=values[:0])
    with pytest.raises(ValueError, match="obs_dim must equal"):
        call("linear_diagonal", x0=torch.zeros(4, 2, device=DEV), th=torch.zeros(4, 4, device=DEV), values=torch.zeros(6, 3, device=DEV))
    net = _hip.CrnNetwork()
    net.S, net.R = 2, 0
    with pytest.raises(ValueError, match="reactions"):
        call("reaction_network", x0=torch.ones(4, 2, device=DEV), th=torch.ones(4, 2, device=DEV), values=torch.zeros(6, 2, device=DEV),
             network=net)
    big = _hip.crn_network([[1] + [0] * 7] * 2, [[-1] + [0] * 7] * 2)            # 8 species: up to 512 particles
    with pytest.raises(ValueError, match="particles"):
        call("reaction_network", N=1024, x0=torch.ones(4, 8, device=DEV), th=torch.ones(4, 2, device=DEV),
             values=torch.zeros(6, 8, device=DEV), network=big)
    torch.cuda.synchronize()
