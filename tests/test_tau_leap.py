"""CPU: tau-leaping (viforsdes_amd/core/tau_leap.py, viforsdes_amd/inference/tau_leap_filter.py,
``particle_mcmc(dynamics="tau_leap")``) on the torch route against the independent numpy float64 restatement of
tests/tau_leap_reference.py, the sampler's moments, the hand cases of the rule, the Euler recursion of the mean, the exact
likelihood of the tau-leap of pure death, and the conditions on the cases of tests/test_tau_leap_gpu.py that concern the reference
alone."""
import math

import numpy as np
import pytest
import torch

import jump_process_reference as jref
import tau_leap_reference as ref
from reaction_networks import AUTOREG, BD, SIR
from viforsdes_amd import (GaussianObservationLikelihood, Observations, PoissonObservationLikelihood, Prior, PriorType, ReactionNetworkSDE,
                           TauLeapFilterResult, TauLeapResult, particle_mcmc, tau_leap_particle_filter, tau_leap_process)
from viforsdes_amd.core.tau_leap import poisson_draw, tau_leap_segment

KEY = (2025, 41)
F64 = torch.float64
DEATH = dict(reactants=[[1]], products=[[0]])                    # X -> 0
IMMIGRATION_DEATH = dict(reactants=[[0], [1]], products=[[1], [0]])     # 0 -> X, X -> 0


# ---------------------------------------------------------------------------------------------------------------- the sampler
@pytest.mark.parametrize("lam", [0.0, 1e-3, 0.3, 4.0, 9.999, 10.0, 12.0, 150.0, 2000.0, 1e6])
def test_poisson_draw_equals_the_numpy_reference_on_the_same_words(lam):
    B = 4096
    paths = torch.arange(B, dtype=torch.int64) * 3 + 1
    step = torch.arange(B, dtype=torch.int64) % 7
    n, attempts, ok = poisson_draw(torch.full((B,), lam, dtype=F64), step, 5, paths, KEY)
    want_n, want_q, want_ok = ref.poisson_draws(np.full(B, lam), step.numpy(), 5, paths.numpy(), KEY)
    assert np.array_equal(n.numpy(), want_n) and np.array_equal(attempts.numpy(), want_q) and np.array_equal(ok.numpy(), want_ok)
    assert bool(ok.all()) and n.dtype == torch.int64
    if lam == 0.0:
        assert int(n.sum()) == 0 and int(attempts.sum()) == 0
    elif lam < 10.0:
        assert attempts.tolist() == [1] * B and int(n.max()) <= 63
    else:
        print(f"lam = {lam}: mean attempts {float(attempts.double().mean()):.3f}, most {int(attempts.max())}")
        assert int(attempts.min()) >= 1 and float(attempts.double().mean()) < 1.5


def test_poisson_draw_takes_a_tensor_key_and_an_int_step():
    lam = torch.tensor([0.0, 2.5, 40.0], dtype=F64)
    a = poisson_draw(lam, 3, 1, torch.tensor([0, 1, 2]), KEY)
    b = poisson_draw(lam.float(), torch.tensor([3, 3, 3]), 1, torch.tensor([0, 1, 2]), torch.tensor(KEY))
    assert all(torch.equal(u, v) for u, v in zip(a, b))


@pytest.mark.parametrize("lam", [0.3, 9.9, 10.0, 37.0, 2000.0])
def test_sample_mean_and_variance_of_the_draws(lam):
    B = 2 ** 16
    n = poisson_draw(torch.full((B,), lam, dtype=F64), 0, 0, torch.arange(B), (99, 7))[0].double().numpy()
    mean, var = n.mean(), n.var(ddof=1)
    se_mean = math.sqrt(lam / B)
    se_var = math.sqrt((lam + 2.0 * lam * lam * B / (B - 1)) / B)          # Var(s^2) = mu_4 / B - sigma^4 (B - 3) / (B (B - 1)), mu_4 = lam + 3 lam^2
    print(f"lam = {lam}: mean off by {(mean - lam) / se_mean:+.2f} s.e., variance by {(var - lam) / se_var:+.2f} s.e.")
    assert abs(mean - lam) <= 5.0 * se_mean
    assert abs(var - lam) <= 5.0 * se_var


# --------------------------------------------------------------------------------------------------------------- the simulator
PROCESS_CASES = {
    "sir": (SIR, [400, 5], [0.004, 0.5], 0.25),
    "immigration_death": (IMMIGRATION_DEATH, [3], [6.0, 0.8], 0.5),
    "autoreg": (AUTOREG, [2, 10], [50.0, 2.0, 0.3, 8.0], 0.2),
}


@pytest.mark.parametrize("name", sorted(PROCESS_CASES))
def test_torch_route_matches_the_numpy_reference(name):
    spec, x0, theta, tau = PROCESS_CASES[name]
    net = ReactionNetworkSDE(**spec)
    B, E = 48, 12
    xs, th = jref.per_path_inputs(x0, theta, B, seed=len(name))
    times = [0.0, 3 * tau, 3 * tau, 7 * tau, 12 * tau]
    res = tau_leap_process(net, torch.from_numpy(xs), torch.from_numpy(th), times, tau, key=KEY, record_steps=E)
    rates = net.kernel_parameters(torch.from_numpy(th)).numpy()
    states, status, capped, draws = ref.simulate(jref.tables(net), xs, rates, [0, 3, 3, 7, 12], tau, KEY, E)
    assert isinstance(res, TauLeapResult) and all(t.dtype == torch.int32 for t in (res.states, res.status, res.capped, res.draws))
    assert res.states.shape == (B, 5, len(x0)) and res.draws.shape == (B, E, net.num_reactions)
    assert np.array_equal(res.states.numpy(), states) and np.array_equal(res.draws.numpy(), draws)
    assert np.array_equal(res.status.numpy(), status) and np.array_equal(res.capped.numpy(), capped)
    assert bool(res.complete.all()) and np.array_equal(states[:, 0], xs) and (draws >= 0).all() and draws.sum() > 10 * B
    bare = tau_leap_process(net, torch.from_numpy(xs), torch.from_numpy(th), times, tau, key=KEY)
    assert bare.draws is None and torch.equal(bare.states, res.states) and torch.equal(bare.capped, res.capped)


def test_sir_runs_out_of_susceptibles_under_the_cap():
    net = ReactionNetworkSDE(**SIR)
    res = tau_leap_process(net, [30, 20], torch.tensor([0.05, 0.1], dtype=F64), [1.0, 2.0], 1.0, n_paths=64, key=KEY, record_steps=2)
    want = ref.simulate(jref.tables(net), np.tile([30, 20], (64, 1)), np.tile([0.05, 0.1, 1.0, 1.0], (64, 1)), [1, 2], 1.0, KEY, 2)
    assert np.array_equal(res.states.numpy(), want[0]) and np.array_equal(res.capped.numpy(), want[2])
    assert int(res.capped.sum()) > 0 and int(res.states.min()) >= 0 and bool((res.states.sum(dim=-1) <= 50).all())


def test_pure_death_with_a_large_rate_ends_at_zero_with_one_capped_draw():
    net = ReactionNetworkSDE(**DEATH)
    res = tau_leap_process(net, [3], torch.tensor([50.0 / 3.0], dtype=F64), [1.0, 2.0], 1.0, n_paths=32, key=KEY, record_steps=2)
    assert res.states.tolist() == [[[0], [0]]] * 32 and res.capped.tolist() == [1] * 32 and res.status.tolist() == [0] * 32
    assert int(res.draws[:, 0].min()) > 3 and res.draws[:, 1].tolist() == [[0]] * 32       # lam = 50, then lam = 0


def test_a_zero_propensity_reads_no_words_and_leaves_the_state(monkeypatch):
    from viforsdes_amd.core import tau_leap as tl
    net = ReactionNetworkSDE(**DEATH)
    calls = []
    real = tl.philox4x32_10
    monkeypatch.setattr(tl, "philox4x32_10", lambda *a: (calls.append(1), real(*a))[1])
    res = tau_leap_process(net, [0], torch.tensor([2.0], dtype=F64), [0.5, 1.5], 0.5, n_paths=4, key=KEY, record_steps=3)
    assert calls == [] and res.states.tolist() == [[[0], [0]]] * 4 and res.draws.tolist() == [[[0]] * 3] * 4
    assert res.status.tolist() == [0] * 4 and res.capped.tolist() == [0] * 4
    tau_leap_process(net, [1], torch.tensor([2.0], dtype=F64), [0.5], 0.5, key=KEY)
    assert calls == [1]


def test_a_negative_theta_stops_the_path_with_status_2():
    net = ReactionNetworkSDE(**IMMIGRATION_DEATH)
    theta = torch.tensor([[2.0, 0.5], [2.0, -0.5], [float("nan"), 0.5], [float("inf"), 0.5]], dtype=F64)
    res = tau_leap_process(net, [4], theta, [0.0, 1.0, 2.0], 0.5, key=KEY, record_steps=4)
    assert res.status.tolist() == [0, 2, 2, 2]
    assert res.states[1:].tolist() == [[[4], [-1], [-1]]] * 3       # row 0 needs no step
    assert bool((res.draws[1:] == -1).all()) and bool((res.draws[0] >= 0).all()) and res.capped[1:].tolist() == [0] * 3


def test_a_step_past_two_to_the_thirty_stops_the_path_and_keeps_the_state():
    net = ReactionNetworkSDE(**IMMIGRATION_DEATH)
    top = 2 ** 30
    theta = torch.tensor([[1000.0, 0.0], [2.0 ** 31, 0.0], [1000.0, 0.0]], dtype=F64)
    x0 = torch.tensor([[top - 100], [5], [top - 100000]])
    res = tau_leap_process(net, x0, theta, [0.0, 1.0, 2.0], 1.0, key=KEY, record_steps=2)
    assert res.status.tolist() == [2, 2, 0]                         # a copy number above 2^30; a rate above 2^30; neither
    assert res.states[0].tolist() == [[top - 100], [-1], [-1]] and res.states[1].tolist() == [[5], [-1], [-1]]
    assert bool((res.draws[:2] == -1).all()) and int(res.states[2, 2]) > top - 100000 + 1500
    x, status, _ = tau_leap_segment(net, x0.to(torch.int64), theta, 1.0, 0, 2, torch.arange(3), KEY)
    assert x[:2].tolist() == [[top - 100], [5]] and status.tolist() == [2, 2, 0]      # the state from before the step


def test_the_mean_follows_the_explicit_euler_recursion():
    """Without a capped draw E[x_{t+1} | x_t] = x_t + tau (k - d x_t), so the mean obeys m <- m + tau (k - d m) exactly."""
    net = ReactionNetworkSDE(**IMMIGRATION_DEATH)
    B, k, d, tau, m, v = 2 ** 16, 40.0, 0.3, 0.25, 200.0, 0.0
    res = tau_leap_process(net, [200], torch.tensor([k, d], dtype=F64), [2 * tau, 5 * tau, 9 * tau], tau, n_paths=B, key=(5, 6))
    assert int(res.capped.sum()) == 0 and bool(res.complete.all())
    x = res.states.double().numpy()[:, :, 0]
    row = 0
    for t in range(9):
        # Var x_{t+1} = Var(E[. | x_t]) + E[Var(. | x_t)] = (1 - tau d)^2 v + tau (k + d m)
        m, v = m + tau * (k - d * m), (1.0 - tau * d) ** 2 * v + tau * (k + d * m)
        if t + 1 in (2, 5, 9):
            z = (x[:, row].mean() - m) / math.sqrt(v / B)
            print(f"row {t + 1}: mean {x[:, row].mean():.3f} against {m:.3f} ({z:+.2f} s.e.)")
            assert abs(z) <= 5.0
            row += 1


def test_process_arguments_are_validated():
    net = ReactionNetworkSDE(**SIR)
    th = torch.tensor([0.02, 0.5], dtype=F64)
    ok = dict(net=net, x0=[95, 5], theta=th, times=[0.5, 1.0], time_step=0.25, key=KEY)
    tau_leap_process(**ok)
    from viforsdes_amd.examples.sdes import ou_problem
    for kw in (dict(net=ou_problem()[0]), dict(time_step=0.0), dict(time_step=-0.1), dict(time_step=float("inf")), dict(x0=[95.5, 5]),
               dict(x0=[95, -1]), dict(x0=[2 ** 30 + 1, 0]), dict(theta=torch.tensor([1, 2])), dict(theta=th[:1]), dict(times=[]),
               dict(times=[1.0, 0.5]), dict(times=[-1.0]), dict(times=[float("nan")]), dict(record_steps=-1), dict(n_paths=0),
               dict(x0=[[95, 5]] * 3, theta=th.expand(2, 2)), dict(key=torch.tensor([1.0, 2.0])), dict(times=[1e12], time_step=1e-3)):
        with pytest.raises(ValueError):
            tau_leap_process(**{**ok, **kw})


# ------------------------------------------------------------------------------------------------------------------ the filter
def _obs(times, values, dtype=F64):
    return Observations(times=torch.tensor(times, dtype=F64), values=torch.tensor(values, dtype=dtype))


FILTER_TIMES, FILTER_ROWS, FILTER_TAU = [0.75, 0.75, 1.75, 2.0], [3, 3, 7, 8], 0.25


def _compare(res, want):
    assert isinstance(res, TauLeapFilterResult)
    assert all(getattr(res, n).dtype == torch.int32 for n in ("particles", "ancestors", "stopped", "capped")) and res.log_weights.dtype == F64
    for name in ("particles", "ancestors", "stopped", "capped"):
        assert np.array_equal(getattr(res, name).numpy(), want[name]), name
    for name, field in (("log_likelihood", "log_likelihood"), ("increments", "increments"), ("ess", "effective_sample_size"),
                        ("mean", "filtered_mean"), ("std", "filtered_std"), ("log_weights", "log_weights")):
        got = getattr(res, field).numpy()
        assert got.shape == want[name].shape, name
        np.testing.assert_allclose(got, want[name], rtol=1e-10, atol=1e-10, equal_nan=True, err_msg=name)


@pytest.mark.parametrize("N", [64, 96])
@pytest.mark.parametrize("name", sorted(PROCESS_CASES))
def test_filter_torch_route_matches_the_numpy_reference(name, N):
    spec, x0, theta, _ = PROCESS_CASES[name]
    net = ReactionNetworkSDE(**spec)
    xs, th = jref.per_path_inputs(x0, theta, 3, seed=len(name))
    rng = np.random.default_rng(N)
    ys = (np.asarray(x0)[None, :] + rng.integers(0, 4, size=(4, len(x0)))).astype(np.float64)
    res = tau_leap_particle_filter(net, _obs(FILTER_TIMES, ys), PoissonObservationLikelihood(scale=0.9), torch.from_numpy(th), FILTER_TAU,
                                   n_particles=N, initial_state=torch.from_numpy(xs), return_particles=True, key=torch.tensor(KEY))
    rates = net.kernel_parameters(torch.from_numpy(th)).numpy()
    want = ref.run_filter(jref.tables(net), xs, rates, FILTER_ROWS, FILTER_TAU, ys, ("poisson", 0.9, None), N, KEY)
    _compare(res, want)
    assert int(res.stopped.sum()) == 0 and np.isfinite(want["log_likelihood"]).all()
    assert np.array_equal(want["particles"][:, 1], want["particles"][:, 0][np.arange(3)[:, None], want["ancestors"][:, 0]])   # the empty segment


def test_filter_with_a_gaussian_likelihood_and_an_observation_matrix_matches_the_reference():
    spec, x0, theta, _ = PROCESS_CASES["sir"]
    net = ReactionNetworkSDE(**spec)
    xs, th = jref.per_path_inputs(x0, theta, 3, seed=9)
    H = torch.tensor([[1.0, 0.5]], dtype=F64)
    ys = [[400.0], [398.0], [390.0], [385.0]]
    res = tau_leap_particle_filter(net, _obs(FILTER_TIMES, ys), GaussianObservationLikelihood(variance=100.0, obs_matrix=H),
                                   torch.from_numpy(th), FILTER_TAU, n_particles=64, initial_state=torch.from_numpy(xs), return_particles=True,
                                   key=torch.tensor(KEY))
    want = ref.run_filter(jref.tables(net), xs, net.kernel_parameters(torch.from_numpy(th)).numpy(), FILTER_ROWS, FILTER_TAU, ys,
                          ("gaussian", 100.0, H.numpy()), 64, KEY)
    _compare(res, want)


@pytest.mark.parametrize("name", ["immigration_death", "autoreg"])
def test_segment_zero_is_the_process_bit_for_bit(name):
    spec, x0, theta, tau = PROCESS_CASES[name]
    net = ReactionNetworkSDE(**spec)
    M, N = 3, 64
    xs, th = jref.per_path_inputs(x0, theta, M, seed=4)
    obs = _obs([5 * tau, 7 * tau], np.tile(np.asarray(x0, dtype=np.float64), (2, 1)))
    res = tau_leap_particle_filter(net, obs, PoissonObservationLikelihood(), torch.from_numpy(th), tau, n_particles=N,
                                   initial_state=torch.from_numpy(xs), return_particles=True, key=torch.tensor(KEY))
    tp = tau_leap_process(net, torch.from_numpy(xs).repeat_interleave(N, 0), torch.from_numpy(th).repeat_interleave(N, 0), obs.times[:1],
                          tau, key=KEY)
    assert torch.equal(res.particles[:, 0].reshape(M * N, -1), tp.states[:, 0]) and bool(tp.complete.all())
    assert torch.equal(res.capped[:, 0], tp.capped.reshape(M, N).sum(dim=1).to(torch.int32))
    assert not torch.equal(res.particles[:, 0], torch.from_numpy(xs)[:, None, :].expand(M, N, -1).to(torch.int32))


def _id_run(theta, times, ys, like=None, x0=(5,), N=64, key=KEY, tau=0.25):
    net = ReactionNetworkSDE(**IMMIGRATION_DEATH)
    return tau_leap_particle_filter(net, _obs(times, ys), like or PoissonObservationLikelihood(), torch.tensor(theta, dtype=F64), tau,
                                    n_particles=N, initial_state=torch.tensor(x0), return_particles=True, key=torch.tensor(key))


def test_a_nan_observation_gives_a_dead_filter_whose_particles_carry_on():
    res = _id_run([4.0, 0.5], [0.5, 1.0, 1.5], [[6.0], [float("nan")], [7.0]], GaussianObservationLikelihood(variance=4.0))
    N = 64
    assert bool(torch.isneginf(res.log_weights[0, 1]).all()) and res.increments[0, 1] == float("-inf") and res.effective_sample_size[0, 1] == 0
    assert bool(torch.isnan(res.filtered_mean[0, 1]).all()) and bool(torch.isnan(res.filtered_std[0, 1]).all())
    assert res.ancestors[0, 1].tolist() == list(range(N)) and res.log_likelihood[0] == float("-inf")
    assert bool(torch.isfinite(res.increments[0, [0, 2]]).all()) and int(res.stopped.sum()) == 0
    assert not torch.equal(res.particles[0, 2], res.particles[0, 1])        # the particles went on from where they were


def test_an_invalid_theta_row_is_stopped_throughout_and_carries_on_in_its_dead_filter():
    res = _id_run([[4.0, 0.5], [4.0, -0.5]], [0.0, 0.5, 1.0], [[5.0], [6.0], [6.0]])
    N = 64
    assert res.stopped.tolist() == [[0] * 3, [0, N, N]]             # row 0 needs no step
    assert bool(torch.isfinite(res.log_likelihood[0])) and res.log_likelihood[1] == float("-inf")
    assert bool((res.particles[1] == 5).all()) and res.ancestors[1, 1].tolist() == list(range(N))


def test_the_same_key_gives_the_same_result_and_another_key_another():
    run = lambda key: _id_run([4.0, 0.5], [0.5, 1.0], [[6.0], [7.0]], key=key)
    a, b, c = run(KEY), run(KEY), run((KEY[0] + 1, KEY[1]))
    assert torch.equal(a.particles, b.particles) and torch.equal(a.log_likelihood, b.log_likelihood) and torch.equal(a.ancestors, b.ancestors)
    assert not torch.equal(a.particles, c.particles) and not torch.equal(a.log_likelihood, c.log_likelihood)


def test_exact_likelihood_reference_against_direct_enumeration():
    """The forward recursion itself on a case small enough to write out: one step from x0 = 2, one observation."""
    lam = 0.7 * 2 * 0.5
    p = [math.exp(-lam), lam * math.exp(-lam)]
    states = [(2, p[0]), (1, p[1]), (0, 1.0 - p[0] - p[1])]
    pois = lambda y, r: math.exp(y * math.log(r) - r - math.lgamma(y + 1.0))
    direct = math.log(sum(w * pois(1.0, max(float(x), 1e-6)) for x, w in states))
    assert abs(ref.pure_death_log_likelihood(0.7, 0.5, 2, [1], [1.0]) - direct) <= 1e-12


def test_likelihood_of_the_pure_death_tau_leap_is_unbiased():
    net = ReactionNetworkSDE(**DEATH)
    M, N, d, tau = 256, 64, 0.4, 0.5
    rows, ys = [3, 6], [6.0, 2.0]
    exact = ref.pure_death_log_likelihood(d, tau, 10, rows, ys)
    res = tau_leap_particle_filter(net, _obs([1.5, 3.0], [[v] for v in ys]), PoissonObservationLikelihood(),
                                   torch.full((M, 1), d, dtype=F64), tau, n_particles=N, initial_state=torch.tensor([10]), key=torch.tensor(KEY))
    r = np.exp(res.log_likelihood.numpy() - exact)
    se = r.std(ddof=1) / math.sqrt(M)
    print(f"pure death: exact {exact:.4f}, mean ratio {r.mean():.4f}, s.e. {se:.4f}, capped {int(res.capped.sum())}")
    assert int(res.stopped.sum()) == 0 and int(res.capped.sum()) > 0        # the cap is part of the model being checked
    assert abs(r.mean() - 1.0) <= 4.0 * se


def test_filter_arguments_are_validated():
    from viforsdes_amd.examples.sdes import ou_problem
    net = ReactionNetworkSDE(**SIR)
    obs = _obs([0.5, 1.0], [[95.0, 5.0], [94.0, 6.0]])
    th = torch.tensor([0.02, 0.5], dtype=F64)
    ok = dict(net=net, observations=obs, observation_likelihood=PoissonObservationLikelihood(), theta=th, time_step=0.25, n_particles=8)
    tau_leap_particle_filter(**ok)
    for kw in (dict(net=ou_problem()[0]), dict(theta=th[:1]), dict(theta=torch.tensor([1, 2])), dict(n_particles=0), dict(time_step=0.0),
               dict(time_step=None), dict(observations=_obs([0.5, 1.0], [[95.5, 5.0], [94.0, 6.0]])),
               dict(initial_state=torch.tensor([95.0, 4.5])), dict(initial_state=torch.tensor([95, -1])),
               dict(initial_state=torch.tensor([2 ** 30 + 1, 0])), dict(observations=_obs([-0.5, 1.0], [[95.0, 5.0], [94.0, 6.0]])),
               dict(key=torch.tensor([1.0, 2.0])), dict(theta=th.expand(2 ** 12, 2), n_particles=2 ** 20)):
        with pytest.raises(ValueError):
            tau_leap_particle_filter(**{**ok, **kw})
    with pytest.raises(TypeError):
        tau_leap_particle_filter(**ok, proposal="bridge")          # there is no proposal: it is the bootstrap filter


# ------------------------------------------------------------------------------------------------------------------------ PMMH
def _pmmh_problem():
    net = ReactionNetworkSDE(**BD)
    obs = _obs([0.0, 0.5, 1.0], [[30.0], [29.0], [27.0]])
    prior = Prior(type=PriorType.LOG_NORMAL, mean=0.0, std=2.0, dim=3)
    g = torch.Generator().manual_seed(3)
    theta = torch.tensor([10.0, 0.5, 0.01], dtype=F64) * (0.8 + 0.4 * torch.rand(8, 3, generator=g, dtype=F64))
    return net, obs, PoissonObservationLikelihood(), prior, theta


def test_pmmh_on_the_tau_leap_is_pmmh_with_the_tau_leap_filter_as_estimator():
    net, obs, like, prior, theta = _pmmh_problem()
    kw = dict(n_iterations=30, warmup=10, n_particles=64, theta_positive_dims=(0, 1, 2), key=torch.tensor([11, 12]))
    a = particle_mcmc(net, obs, like, prior, 0.1, theta, dynamics="tau_leap", positive_dims=None, **kw)
    seen = []

    def estimator(rows, i, fkey):
        seen.append(i)
        return tau_leap_particle_filter(net, obs, like, rows, 0.1, n_particles=64, key=fkey).log_likelihood

    b = particle_mcmc(net, obs, like, prior, 0.1, theta, _estimator=estimator, **kw)
    assert seen == list(range(30))
    assert torch.equal(a.samples, b.samples) and torch.equal(a.log_likelihood, b.log_likelihood)
    assert torch.equal(a.acceptance_rate, b.acceptance_rate) and a.samples.shape == (20, 8, 3)
    assert bool(torch.isfinite(a.log_likelihood).all()) and float(a.acceptance_rate.mean()) > 0
    c = particle_mcmc(net, obs, like, prior, 0.05, theta, dynamics="tau_leap", **kw)
    assert not torch.equal(a.log_likelihood, c.log_likelihood)     # time_step is in use


def test_pmmh_refusals():
    from viforsdes_amd.examples.sdes import ou_problem
    net, obs, like, prior, theta = _pmmh_problem()
    kw = dict(n_iterations=4, n_particles=8, theta_positive_dims=(0, 1, 2), key=torch.tensor([11, 12]))
    for bad in (dict(return_paths=True), dict(path_times=[0.25]), dict(return_paths=True, path_times=[0.25]), dict(proposal="bridge"),
                dict(initial_state=torch.tensor([30.5], dtype=F64))):
        with pytest.raises(ValueError):
            particle_mcmc(net, obs, like, prior, 0.1, theta, dynamics="tau_leap", **{**kw, **bad})
    for step in (None, 0.0):
        with pytest.raises(ValueError):
            particle_mcmc(net, obs, like, prior, step, theta, dynamics="tau_leap", **kw)
    sde = ou_problem()[0]
    with pytest.raises(ValueError):
        particle_mcmc(sde, obs, like, prior, 0.1, theta, dynamics="tau_leap", **kw)


# ------------------------------------------------------- the conditions on the GPU cases that concern the reference alone
def test_the_gpu_simulator_cases_meet_their_conditions_in_float64():
    """tests/test_tau_leap_gpu.py asserts these on the kernel's own log; here the same counts on the float64 run of the same
    inputs: every rate at most 2000, at least 100 draws in each sampler branch, a draw with lam = 0, a capped draw, and a flagged
    share of at most 1e-2."""
    total = dict(zero=0, inversion=0, ptrs=0, capped=0, flagged=0, draws=0)
    for name in sorted(ref.sim_cases()):
        net, xs, th32, time_step, key = ref.sim_case(name)
        tab = jref.tables(net)
        rates = net.kernel_parameters(torch.as_tensor(th32)).double().numpy()
        tau = float(np.float32(time_step))
        states, status, capped, draws = ref.simulate(tab, xs, rates, ref.SIM_ROWS, tau, key, ref.SIM_STEPS)
        x, lam_max = xs.copy(), 0.0
        for t in range(ref.SIM_STEPS):
            live = np.nonzero(draws[:, t, 0] >= 0)[0]
            lam = ref.step_rates(tab, x[live], rates[live], tau)[0]
            _, flagged = ref.flagged_draws(lam, t, np.arange(lam.shape[1])[None, :], live[:, None], key)
            total["zero"] += int((lam == 0).sum())
            total["inversion"] += int(((lam > 0) & (lam < 10)).sum())
            total["ptrs"] += int((lam >= 10).sum())
            total["flagged"] += int(flagged.sum())
            total["draws"] += lam.size
            lam_max = max(lam_max, float(lam.max()))
            x[live] = ref.apply_draws(tab, x[live], draws[live, t])[0]
        total["capped"] += int(capped.sum())
        print(f"{name}: largest rate {lam_max:.1f}, capped {int(capped.sum())}, stopped {int((status != 0).sum())}")
        assert lam_max <= 2000.0
        assert int((status != 0).sum()) == (1 if name == "sir" else 0)
    print(total)
    assert total["zero"] >= 1 and total["inversion"] >= 100 and total["ptrs"] >= 100 and total["capped"] >= 1
    assert total["flagged"] <= 1e-2 * total["draws"]


def test_the_gpu_filter_cases_stay_alive_with_rates_of_at_most_200_in_float64():
    for name, N in ref.FILTER_RUNS:
        net, th, xs, ys, like, time_step, key = ref.filter_case(name, N)
        tab, tau = jref.tables(net), float(np.float32(time_step))
        rates = net.kernel_parameters(th.double()).numpy()
        out = ref.run_filter(tab, xs, rates, ref.FILTER_ROWS, tau, ys, like, N, key)
        lam_max = max(float(ref.step_rates(tab, out["particles"][m, k], np.repeat(rates[m][None], N, axis=0), tau)[0].max())
                      for m in range(ref.FILTER_M) for k in range(len(ref.FILTER_ROWS)))
        print(f"{name} N={N}: smallest ESS {out['ess'].min():.1f}, largest rate {lam_max:.1f}, capped {int(out['capped'].sum())}")
        assert out["ess"].min() > N / 20 and int(out["stopped"].sum()) == 0 and lam_max <= 200.0
