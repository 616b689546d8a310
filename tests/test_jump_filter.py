"""CPU: the torch specification of the jump-process particle filter (viforsdes_amd/inference/jump_filter.py) against the
independent numpy restatement (tests/jump_filter_reference.py), segment 0 against ``jump_process``, the exact likelihood of an
immigration-death process observed with Poisson noise (forward algorithm), the edge rules, the argument checks, and the wiring of
``particle_mcmc(..., dynamics="jump")``.  Every call runs with ``max_events <= 4096``."""
import math

import numpy as np
import pytest
import torch

import jump_filter_reference as ref
import jump_process_reference as jref
from reaction_networks import BD, SIR
from viforsdes_amd import (GaussianObservationLikelihood, JumpParticleFilterResult, Observations, PoissonObservationLikelihood, Prior,
                           PriorType, ReactionNetworkSDE, jump_particle_filter, jump_process, particle_mcmc)

KEY = (2024, 77)
CASES = jref.cases()
TIMES = [0.0, 0.25, 0.25, 1.0]
F64 = torch.float64


def _obs(times, values):
    return Observations(times=torch.tensor(times, dtype=F64), values=torch.tensor(values, dtype=F64))


def _counts(x0, K, seed):
    """K rows of counts near the start state (what a Poisson likelihood accepts)."""
    rng = np.random.default_rng(seed)
    return (np.asarray(x0)[None, :] + rng.integers(0, 4, size=(K, len(x0)))).astype(np.float64)


def _compare(res, want, N):
    assert isinstance(res, JumpParticleFilterResult)
    assert res.particles.dtype == torch.int32 and res.ancestors.dtype == torch.int32 and res.events.dtype == torch.int32
    assert res.stopped.dtype == torch.int32 and res.log_weights.dtype == F64
    for name in ("particles", "ancestors", "events", "stopped"):
        assert np.array_equal(getattr(res, name).numpy(), want[name]), name
    for name, field in (("log_likelihood", "log_likelihood"), ("increments", "increments"), ("ess", "effective_sample_size"),
                        ("mean", "filtered_mean"), ("std", "filtered_std"), ("mean_events", "mean_events"), ("log_weights", "log_weights")):
        got = getattr(res, field).numpy()
        assert got.shape == want[name].shape, name
        np.testing.assert_allclose(got, want[name], rtol=1e-10, atol=1e-10, equal_nan=True, err_msg=name)
    assert want["events"].sum() > 3 * N                            # something happened


@pytest.mark.parametrize("N", [64, 96])
@pytest.mark.parametrize("name", sorted(CASES))
def test_torch_route_matches_the_numpy_reference(name, N):
    spec, x0, theta = CASES[name]
    net = ReactionNetworkSDE(**spec)
    xs, th = jref.per_path_inputs(x0, theta, 3, seed=len(name))
    ys = _counts(x0, len(TIMES), seed=N)
    res = jump_particle_filter(net, _obs(TIMES, ys), PoissonObservationLikelihood(scale=0.9), torch.from_numpy(th), n_particles=N,
                               initial_state=torch.from_numpy(xs), return_particles=True, key=torch.tensor(KEY), max_events=4096)
    rates = net.kernel_parameters(torch.from_numpy(th)).numpy()
    want = ref.run_filter(jref.tables(net), xs, rates, TIMES, ys, ("poisson", 0.9, None), N, KEY, 4096)
    _compare(res, want, N)
    assert int(res.stopped.sum()) == 0


def test_gaussian_likelihood_with_an_observation_matrix_matches_the_reference():
    spec, x0, theta = CASES["sir"]
    net = ReactionNetworkSDE(**spec)
    xs, th = jref.per_path_inputs(x0, theta, 3, seed=9)
    H = torch.tensor([[1.0, 0.5]], dtype=F64)
    ys = [[97.0], [96.5], [95.0], [93.0]]
    res = jump_particle_filter(net, _obs(TIMES, ys), GaussianObservationLikelihood(variance=4.0, obs_matrix=H), torch.from_numpy(th),
                               n_particles=64, initial_state=torch.from_numpy(xs), return_particles=True, key=torch.tensor(KEY), max_events=4096)
    want = ref.run_filter(jref.tables(net), xs, net.kernel_parameters(torch.from_numpy(th)).numpy(), TIMES, ys,
                          ("gaussian", 4.0, H.numpy()), 64, KEY, 4096)
    _compare(res, want, 64)


@pytest.mark.parametrize("name", ["bd", "autoreg"])
def test_segment_zero_is_the_jump_process(name):
    spec, x0, theta = CASES[name]
    net = ReactionNetworkSDE(**spec)
    M, N = 3, 64
    xs, th = jref.per_path_inputs(x0, theta, M, seed=4)
    obs = _obs([0.7, 1.1], _counts(x0, 2, seed=1))
    res = jump_particle_filter(net, obs, PoissonObservationLikelihood(), torch.from_numpy(th), n_particles=N,
                               initial_state=torch.from_numpy(xs), return_particles=True, key=torch.tensor(KEY), max_events=4096)
    jp = jump_process(net, torch.from_numpy(xs).repeat_interleave(N, 0), torch.from_numpy(th).repeat_interleave(N, 0), obs.times[:1],
                      key=KEY, max_events=4096)
    assert torch.equal(res.particles[:, 0].reshape(M * N, -1), jp.states[:, 0])
    assert torch.equal(res.events[:, 0].reshape(-1), jp.n_events) and bool(jp.complete.all())


@pytest.mark.parametrize("dtype", [F64, torch.float32])
def test_likelihood_of_immigration_death_is_unbiased(dtype):
    net = ReactionNetworkSDE(**BD)
    M, N = 256, 128
    exact = ref.immigration_death_log_likelihood(10.0, 0.5, 30, ref.IMMIGRATION_DEATH_TIMES, ref.IMMIGRATION_DEATH_COUNTS)
    obs = Observations(times=torch.tensor(ref.IMMIGRATION_DEATH_TIMES, dtype=F64),
                       values=torch.tensor(ref.IMMIGRATION_DEATH_COUNTS, dtype=dtype)[:, None])
    res = jump_particle_filter(net, obs, PoissonObservationLikelihood(), torch.tensor([10.0, 0.5, 0.0], dtype=dtype).expand(M, 3),
                               n_particles=N, key=torch.tensor(KEY), max_events=4096)
    r = np.exp(res.log_likelihood.double().numpy() - exact)
    sd = r.std(ddof=1)
    z = (r.mean() - 1.0) / (sd / math.sqrt(M))
    print(f"immigration-death {dtype}: exact {exact:.4f}, std(r) {sd:.3f}, z {z:.2f}, events per segment {float(res.mean_events.mean()):.1f}")
    assert int(res.stopped.sum()) == 0
    assert sd <= 0.5
    assert abs(r.mean() - 1.0) <= 4.5 * sd / math.sqrt(M)


def test_exact_likelihood_reference_against_direct_enumeration():
    """The forward algorithm itself, on a case small enough to check: one observation at t > 0 is sum_n pmf(n) Poisson(y; n)."""
    pmf = jref.immigration_death_pmf(5, 2.0, 0.7, 1.3, 200)[0]
    n = np.arange(200)
    direct = math.log(sum(pmf[i] * math.exp(3 * math.log(max(i, 1e-6)) - max(i, 1e-6) - math.lgamma(4.0)) for i in n))
    assert abs(ref.immigration_death_log_likelihood(2.0, 0.7, 5, [1.3], [3.0]) - direct) <= 1e-12


# ------------------------------------------------------------------------------------------------------------------ edge rules
def _bd_run(theta, times, ys, like=None, x0=(5,), N=64, **kw):
    net = ReactionNetworkSDE(**BD)
    return jump_particle_filter(net, _obs(times, ys), like or PoissonObservationLikelihood(), torch.tensor(theta, dtype=F64), n_particles=N,
                                initial_state=torch.tensor(x0), return_particles=True, key=kw.pop("key", torch.tensor(KEY)),
                                max_events=kw.pop("max_events", 4096), **kw)


def test_a_nan_observation_gives_a_dead_filter_whose_particles_carry_on():
    res = _bd_run([4.0, 0.5, 0.0], [0.5, 1.0, 1.5], [[6.0], [float("nan")], [7.0]], GaussianObservationLikelihood(variance=4.0))
    N = 64
    assert bool(torch.isneginf(res.log_weights[0, 1]).all()) and res.increments[0, 1] == float("-inf") and res.effective_sample_size[0, 1] == 0
    assert bool(torch.isnan(res.filtered_mean[0, 1]).all()) and bool(torch.isnan(res.filtered_std[0, 1]).all())
    assert res.ancestors[0, 1].tolist() == list(range(N)) and res.log_likelihood[0] == float("-inf")
    assert bool(torch.isfinite(res.increments[0, [0, 2]]).all()) and int(res.stopped.sum()) == 0
    assert int(res.events[0, 2].sum()) > 0                         # the particles went on from where they were


def test_the_event_cap_stops_particles_and_a_dead_filter_carries_on():
    res = _bd_run([200.0, 0.1, 0.0], [0.0, 10.0, 20.0], [[5.0], [30.0], [40.0]], max_events=3)
    N = 64
    assert res.stopped.tolist() == [[0, N, N]] and res.events[0, 0].tolist() == [0] * N
    assert res.events[0, 1].tolist() == [3] * N and res.events[0, 2].tolist() == [3] * N
    assert res.increments[0, 1:].tolist() == [float("-inf")] * 2 and res.ancestors[0, 1].tolist() == list(range(N))
    assert bool(torch.isfinite(res.increments[0, 0]))
    moved = (res.particles[0, 2] - res.particles[0, 1]).abs().sum(dim=-1)
    assert bool((moved > 0).all())                                 # from the state they stopped in, three more events
    assert res.mean_events.tolist() == [[0.0, 3.0, 3.0]]


def test_an_invalid_theta_row_is_stopped_throughout():
    theta = [[4.0, 0.5, 0.0], [4.0, -0.5, 0.0], [float("nan"), 0.5, 0.0]]
    res = _bd_run(theta, [0.0, 0.5, 1.0], [[5.0], [6.0], [6.0]])
    N = 64
    assert res.stopped.tolist() == [[0] * 3, [N] * 3, [N] * 3]
    assert bool(torch.isfinite(res.log_likelihood[0])) and res.log_likelihood[1:].tolist() == [float("-inf")] * 2
    assert int(res.events[1:].sum()) == 0 and bool((res.particles[1:] == 5).all())


def test_an_absorbed_particle_stays():
    net = ReactionNetworkSDE(**SIR)
    res = jump_particle_filter(net, _obs([0.0, 1.0, 2.0], [[40.0, 0.0]] * 3), PoissonObservationLikelihood(),
                               torch.tensor([0.01, 0.2], dtype=F64), n_particles=64, return_particles=True, key=torch.tensor(KEY))
    assert bool((res.particles == torch.tensor([40, 0], dtype=torch.int32)).all()) and int(res.events.sum()) == 0
    assert int(res.stopped.sum()) == 0 and bool(torch.isfinite(res.log_likelihood).all())
    assert torch.allclose(res.effective_sample_size, torch.full((1, 3), 64.0, dtype=F64))


def test_the_same_key_gives_the_same_result_and_another_key_another():
    run = lambda key: _bd_run([4.0, 0.5, 0.0], [0.5, 1.0], [[6.0], [7.0]], key=key)
    a, b, c = run(torch.tensor(KEY)), run(torch.tensor(KEY)), run(torch.tensor((KEY[0] + 1, KEY[1])))
    assert torch.equal(a.particles, b.particles) and torch.equal(a.log_likelihood, b.log_likelihood) and torch.equal(a.ancestors, b.ancestors)
    assert not torch.equal(a.particles, c.particles) and not torch.equal(a.log_likelihood, c.log_likelihood)


def test_bad_arguments_are_refused():
    from viforsdes_amd.examples.sdes import ou_problem
    net = ReactionNetworkSDE(**SIR)
    like = PoissonObservationLikelihood()
    obs = _obs([0.5, 1.0], [[95.0, 5.0], [94.0, 6.0]])
    th = torch.tensor([0.02, 0.5], dtype=F64)
    ok = dict(net=net, observations=obs, observation_likelihood=like, theta=th, n_particles=8, max_events=64)
    jump_particle_filter(**ok)
    one_dim = _obs([0.5], [[95.0]])
    H = torch.tensor([[1.0, 1.0]], dtype=F64)
    for kw in (dict(net=ou_problem()[0]), dict(theta=th[:1]), dict(theta=torch.tensor([1, 2])), dict(n_particles=0), dict(max_events=0),
               dict(max_events=2 ** 23 + 1), dict(observations=_obs([0.5, 1.0], [[95.5, 5.0], [94.0, 6.0]])),       # default start not integer
               dict(observations=one_dim, observation_likelihood=PoissonObservationLikelihood(obs_matrix=H)),      # O != S: a start is needed
               dict(initial_state=torch.tensor([95.0, 4.5])), dict(initial_state=torch.tensor([95, -1])),
               dict(initial_state=torch.tensor([2 ** 30 + 1, 0])), dict(initial_state=torch.tensor([95, 5, 1])),
               dict(initial_state=torch.tensor([float("nan"), 1.0])), dict(observations=_obs([-0.5, 1.0], [[95.0, 5.0], [94.0, 6.0]])),
               dict(observations=_obs([0.5, float("inf")], [[95.0, 5.0], [94.0, 6.0]])), dict(key=torch.tensor([1.0, 2.0])),
               dict(theta=th.expand(2 ** 12, 2), n_particles=2 ** 20)):
        with pytest.raises(ValueError):
            jump_particle_filter(**{**ok, **kw})
    with pytest.raises(TypeError):
        jump_particle_filter(**ok, proposal="bridge")              # there is no proposal: it is the bootstrap filter
    jump_particle_filter(**{**ok, "observations": one_dim, "observation_likelihood": PoissonObservationLikelihood(obs_matrix=H),
                            "initial_state": torch.tensor([95, 5])})
    jump_particle_filter(**{**ok, "initial_state": torch.tensor([2 ** 30, 0]), "max_events": 1})


# ----------------------------------------------------------------------------------------------------------------- PMMH wiring
def _pmmh_problem():
    net = ReactionNetworkSDE(**BD)
    obs = _obs([0.0, 0.25, 0.5], [[30.0], [29.0], [27.0]])              # short segments: the torch route pays per event
    prior = Prior(type=PriorType.LOG_NORMAL, mean=0.0, std=2.0, dim=3)
    g = torch.Generator().manual_seed(3)
    theta = torch.tensor([10.0, 0.5, 0.01], dtype=F64) * (0.8 + 0.4 * torch.rand(8, 3, generator=g, dtype=F64))
    return net, obs, PoissonObservationLikelihood(), prior, theta


def test_pmmh_on_the_jump_process_is_pmmh_with_the_jump_filter_as_estimator():
    net, obs, like, prior, theta = _pmmh_problem()
    key = torch.tensor([11, 12])
    kw = dict(n_iterations=30, warmup=10, n_particles=64, theta_positive_dims=(0, 1, 2), key=key)
    a = particle_mcmc(net, obs, like, prior, None, theta, dynamics="jump", max_events=4096, positive_dims=None, **kw)
    seen = []

    def estimator(rows, i, fkey):
        seen.append(i)
        return jump_particle_filter(net, obs, like, rows, n_particles=64, key=fkey, max_events=4096).log_likelihood

    b = particle_mcmc(net, obs, like, prior, 0.1, theta, _estimator=estimator, **kw)
    assert seen == list(range(30))
    assert torch.equal(a.samples, b.samples) and torch.equal(a.log_likelihood, b.log_likelihood)
    assert torch.equal(a.acceptance_rate, b.acceptance_rate) and a.samples.shape == (20, 8, 3)
    assert bool(torch.isfinite(a.log_likelihood).all()) and float(a.acceptance_rate.mean()) > 0
    for bad in (dict(return_paths=True), dict(proposal="bridge"), dict(initial_state=torch.tensor([30.5], dtype=F64)), dict(max_events=0)):
        with pytest.raises(ValueError):
            particle_mcmc(net, obs, like, prior, None, theta, dynamics="jump", **{**kw, **bad})
    with pytest.raises(ValueError):
        particle_mcmc(net, obs, like, prior, 0.1, theta, dynamics="tau_leaping", **kw)


def test_diffusion_dynamics_is_the_call_without_the_keyword():
    net, obs, like, prior, theta = _pmmh_problem()
    kw = dict(n_iterations=8, n_particles=64, theta_positive_dims=(0, 1, 2), positive_dims=(0,), key=torch.tensor([5, 6]))
    a = particle_mcmc(net, obs, like, prior, 0.05, theta, **kw)
    b = particle_mcmc(net, obs, like, prior, 0.05, theta, dynamics="diffusion", max_events=7, **kw)
    assert torch.equal(a.samples, b.samples) and torch.equal(a.log_likelihood, b.log_likelihood) and torch.equal(a.acceptance_rate, b.acceptance_rate)
