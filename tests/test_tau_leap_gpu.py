"""GPU: the tau-leap kernels (csrc/vsde_tau_leap.hip: tl_kernel, tlf_kernel; the sampler of csrc/vsde_poisson.h) through the public
``tau_leap_process``, ``tau_leap_particle_filter`` and ``particle_mcmc(..., dynamics="tau_leap")``.

The method is that of tests/test_jump_process_gpu.py and tests/test_jump_filter_gpu.py: no whole trajectory is compared.  The state
before every step is rebuilt from x0 and the kernel's own logged draws, or from the kernel's particles gathered through the kernel's
ancestors, and each step is then judged against float64 on that state (tests/tau_leap_reference.py).

A draw is flagged (undecidable) when, in the float64 reference, the result or the attempt count differs between ``lam64 (1 -
2^-20)`` and ``lam64 (1 + 2^-20)``, or those two rates straddle 10.  2^-20 is 16 fp32 roundings; the longest propensity chain of
the specification (Hill n = 4, gate, tau) has 11.

* simulator: B = 256, 16 steps, all logged; SIR, immigration-death, the repressilator (Hill n = 2, 3, 4) and the 8-species /
  16-reaction network.  Asserted: every rate at most 2000; across the cases at least 100 draws in each sampler branch, a draw with
  lam = 0, a capped draw; the reference's flagged share at most 1e-2 (first: a cap, not a tolerance); every unflagged draw equals
  the kernel's; ``states``, ``capped`` and ``status`` follow exactly, in integers, from the kernel's own draws;
* filter: M = 4, N in {64, 256}, K = 3 with segments of 3, 0 and 4 steps; Poisson, negative binomial with an ``obs_matrix``,
  Gaussian with an ``obs_matrix``; rates of at most 200.  Segments replayed in float64 from the kernel's particles through its
  ancestors: at most 2e-2 of the (particle, segment) pairs flagged (first), every other pair equal; log-weights, increments, ESS
  and moments against float64 of the kernel's own particles, and ancestors against float64 systematic resampling, with the checks
  and tolerances of tests/jump_filter_reference.py;
* one small case per ``(S, NR, KIN)`` instantiation of both kernels (the cells of tests/sde_sweep_reference.py);
* PMMH on the kernel loop through ``_trace``; the routes."""
import numpy as np
import pytest
import torch

import jump_filter_reference as jfref
import sde_sweep_reference as W
import tau_leap_reference as ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _times(rows, tau):
    return torch.tensor(rows, dtype=torch.float64) * tau


# --------------------------------------------------------------------------------------------------------------- the simulator
_SIM = {}


def _sim(name):
    if name not in _SIM:
        from viforsdes_amd import tau_leap_process
        net, xs, th32, tau, key = ref.sim_case(name)
        assert net.kernel_compatible()
        calls, real, wrapped = ref.counted("tau_leap_process")
        from viforsdes_amd import _hip
        _hip.tau_leap_process = wrapped
        try:
            res = tau_leap_process(net, torch.from_numpy(xs), torch.from_numpy(th32).to(DEV), _times(ref.SIM_ROWS, tau), tau, key=key,
                                   record_steps=ref.SIM_STEPS)
        finally:
            _hip.tau_leap_process = real
        assert calls == [1]                                         # the public function took the kernel route
        _SIM[name] = (net, xs, th32, tau, key, res, ref.check_process(net, xs, th32, ref.SIM_ROWS, tau, res, key, name))
    return _SIM[name]


@pytest.mark.parametrize("name", sorted(ref.sim_cases()))
def test_simulator_draws_match_float64_on_the_state_the_kernels_log_implies(name):
    net, xs, th32, tau, key, res, counts = _sim(name)
    assert counts["max_rate"] <= 2000.0
    assert counts["stopped"] == (1 if name == "sir" else 0)
    assert res.states.shape == (ref.SIM_B, len(ref.SIM_ROWS), xs.shape[1]) and np.array_equal(res.states[:, 0].cpu().numpy(), xs)


def test_simulator_cases_cover_every_branch_of_the_sampler():
    total = {k: sum(_sim(name)[6][k] for name in ref.sim_cases()) for k in ("zero", "inversion", "ptrs", "capped", "flagged", "draws")}
    print(total)
    assert total["inversion"] >= 100 and total["ptrs"] >= 100 and total["zero"] >= 1 and total["capped"] >= 1
    assert total["flagged"] <= 1e-2 * total["draws"]


def test_simulator_without_a_log_gives_the_same_rows():
    from viforsdes_amd import tau_leap_process
    net, xs, th32, tau, key, res, _ = _sim("repress3")
    bare = tau_leap_process(net, torch.from_numpy(xs), torch.from_numpy(th32).to(DEV), _times(ref.SIM_ROWS, tau), tau, key=key)
    assert bare.draws is None and torch.equal(bare.states, res.states) and torch.equal(bare.capped, res.capped)
    short = tau_leap_process(net, torch.from_numpy(xs), torch.from_numpy(th32).to(DEV), _times(ref.SIM_ROWS, tau), tau, key=key,
                             record_steps=20)
    assert torch.equal(short.draws[:, :ref.SIM_STEPS], res.draws) and bool((short.draws[:, ref.SIM_STEPS:] == -1).all())


def test_simulator_stops_at_a_copy_number_or_a_rate_above_two_to_the_thirty():
    from viforsdes_amd import ReactionNetworkSDE, tau_leap_process
    net = ReactionNetworkSDE(reactants=[[0], [1]], products=[[1], [0]])
    top = 2 ** 30
    theta = torch.tensor([[1000.0, 0.0], [2.0 ** 31, 0.0], [1000.0, 0.0]], device=DEV)
    x0 = torch.tensor([[top - 100], [5], [top - 100000]])
    res = tau_leap_process(net, x0, theta, [0.0, 1.0, 2.0], 1.0, key=(3, 4), record_steps=2)
    assert res.status.tolist() == [2, 2, 0]
    assert res.states[0].tolist() == [[top - 100], [-1], [-1]] and res.states[1].tolist() == [[5], [-1], [-1]]
    assert bool((res.draws[:2] == -1).all()) and int(res.states[2, 2]) > top - 100000 + 1500 and res.capped.tolist() == [0, 0, 0]


# ------------------------------------------------------------------------------------------------------------------ the filter
_RUNS = {}


def _filter_run(net, th, xs, ys, like, tau, key, N, rows):
    from viforsdes_amd import Observations, _hip, tau_leap_particle_filter
    obs = Observations(times=_times(rows, tau), values=torch.tensor(ys, dtype=torch.float32))
    calls, real, wrapped = ref.counted("tau_leap_particle_filter")
    _hip.tau_leap_particle_filter = wrapped
    try:
        res = tau_leap_particle_filter(net, obs.to(DEV), jfref.likelihood(like), th.to(DEV), tau, n_particles=N,
                                       initial_state=torch.from_numpy(xs).to(DEV), return_particles=True, key=jfref.key_tensor(*key, DEV))
    finally:
        _hip.tau_leap_particle_filter = real
    assert calls == [1]                                             # the public function took the kernel route
    assert all(t.dtype == torch.int32 for t in (res.particles, res.ancestors, res.stopped, res.capped))
    return res


def _cached(name, N):
    if (name, N) not in _RUNS:
        net, th, xs, ys, like, tau, key = ref.filter_case(name, N)
        _RUNS[(name, N)] = (net, th, xs, ys, like, tau, key, _filter_run(net, th, xs, ys, like, tau, key, N, ref.FILTER_ROWS))
    return _RUNS[(name, N)]


@pytest.mark.parametrize("name,N", ref.FILTER_RUNS)
def test_filter_segments_match_float64_on_the_kernels_previous_stage(name, N):
    net, th, xs, ys, like, tau, key, res = _cached(name, N)
    ref.check_filter_propagation(net, th, xs, ref.FILTER_ROWS, tau, res, key, f"{name} N={N}")
    assert int(res.stopped.sum()) == 0 and res.particles.shape == (ref.FILTER_M, len(ref.FILTER_ROWS), N, xs.shape[1])
    assert torch.equal(res.particles[:, 1], torch.gather(res.particles[:, 0], 1, res.ancestors[:, 0].long()[..., None].expand(-1, -1, xs.shape[1])))


@pytest.mark.parametrize("name,N", ref.FILTER_RUNS)
def test_filter_weights_and_summaries_match_float64_on_the_kernels_particles(name, N):
    net, th, xs, ys, like, tau, key, res = _cached(name, N)
    jfref.check_weights_and_summaries(like, ys, res, f"{name} N={N}")


@pytest.mark.parametrize("name,N", ref.FILTER_RUNS)
def test_filter_ancestors_match_float64_systematic_resampling(name, N):
    net, th, xs, ys, like, tau, key, res = _cached(name, N)
    jfref.check_ancestors(like, ys, res, key, f"{name} N={N}")


def test_segment_zero_is_the_simulator_kernel_bit_for_bit():
    from viforsdes_amd import tau_leap_process
    net, th, xs, ys, like, tau, key, res = _cached("sir_poisson", 64)
    M, N = ref.FILTER_M, 64
    tp = tau_leap_process(net, torch.from_numpy(xs).repeat_interleave(N, 0), th.to(DEV).repeat_interleave(N, 0),
                          _times(ref.FILTER_ROWS[:1], tau), tau, key=jfref.key_tensor(*key, DEV))
    assert torch.equal(res.particles[:, 0].reshape(M * N, -1), tp.states[:, 0]) and bool(tp.complete.all())
    assert torch.equal(res.capped[:, 0], tp.capped.reshape(M, N).sum(dim=1).to(torch.int32))


def test_a_dead_filter_carries_on_and_an_invalid_row_is_stopped():
    from viforsdes_amd import GaussianObservationLikelihood, Observations, ReactionNetworkSDE, tau_leap_particle_filter
    net = ReactionNetworkSDE(reactants=[[0], [1]], products=[[1], [0]])
    obs = Observations(times=torch.tensor([0.5, 1.0, 1.5], dtype=torch.float64), values=torch.tensor([[6.0], [float("nan")], [7.0]])).to(DEV)
    theta = torch.tensor([[4.0, 0.5], [4.0, -0.5]], device=DEV)
    N = 64
    res = tau_leap_particle_filter(net, obs, GaussianObservationLikelihood(variance=4.0), theta, 0.25, n_particles=N,
                                   initial_state=torch.tensor([5]), return_particles=True, key=jfref.key_tensor(1, 2, DEV))
    assert res.stopped.tolist() == [[0] * 3, [N] * 3] and res.log_likelihood.tolist() == [float("-inf")] * 2
    assert bool(torch.isneginf(res.log_weights[0, 1]).all()) and res.ancestors[0, 1].tolist() == list(range(N))
    assert bool(torch.isfinite(res.increments[0, [0, 2]]).all()) and bool(torch.isnan(res.filtered_mean[0, 1]).all())
    assert not torch.equal(res.particles[0, 2], res.particles[0, 1]) and bool((res.particles[1] == 5).all())


# ---------------------------------------------------------------------------------- every instantiation of the two kernels
SWEEP_ROWS, SWEEP_TAU = [0, 1, 1, 4], 0.25


@pytest.mark.parametrize("name", W.NAMES)
def test_simulator_cell(name):
    from viforsdes_amd import tau_leap_process
    net, xs, th32, _, key = W.jump_case(name)
    assert net.kernel_compatible()
    res = tau_leap_process(net, torch.from_numpy(xs), torch.from_numpy(th32).to(DEV), _times(SWEEP_ROWS, SWEEP_TAU), SWEEP_TAU, key=key,
                           record_steps=SWEEP_ROWS[-1])
    counts = ref.check_process(net, xs, th32, SWEEP_ROWS, SWEEP_TAU, res, key, name)
    assert counts["stopped"] == 0 and counts["draws"] == W.JUMP_B * SWEEP_ROWS[-1] * net.num_reactions
    assert counts["draws"] - counts["zero"] >= 200                  # something was drawn


@pytest.mark.parametrize("name", W.NAMES)
def test_filter_cell(name):
    net, th, xs, ys, like, key, N = W.filter_case(name)
    res = _filter_run(net, th, xs, ys, like, SWEEP_TAU, key, N, SWEEP_ROWS)
    label = f"{name} N={N} {like[0]}"
    ref.check_filter_propagation(net, th, xs, SWEEP_ROWS, SWEEP_TAU, res, key, label)
    jfref.check_weights_and_summaries(like, ys, res, label)
    jfref.check_ancestors(like, ys, res, key, label)


def test_too_many_particles_are_refused_before_any_launch():
    from viforsdes_amd import _hip
    for S in (1, 8):
        name = W.NAMES[W.CELLS.index((S, 16, S % 2 == 0))]
        net, th, xs, ys, like, key, N = W.filter_case(name)
        too_many = _hip.tau_leap_filter_max_particles(S, net.num_reactions, not net.plain) + 64
        rates = (th if net.plain else net.kernel_parameters(th)).to(DEV)
        with pytest.raises(ValueError, match="particles"):
            _hip.tau_leap_particle_filter(torch.from_numpy(xs).to(torch.int32).to(DEV), rates, torch.tensor(SWEEP_ROWS, dtype=torch.int32, device=DEV),
                                          torch.tensor(ys, dtype=torch.float32, device=DEV), None, 25.0, jfref.key_tensor(*key, DEV), SWEEP_TAU,
                                          too_many, network=net.kernel_descriptor(), return_particles=True)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- PMMH, routes
def _pmmh_problem():
    from viforsdes_amd import Observations, PoissonObservationLikelihood, Prior, PriorType, ReactionNetworkSDE
    from reaction_networks import BD
    net = ReactionNetworkSDE(**BD)
    obs = Observations(times=torch.tensor([0.0, 0.5, 1.0], dtype=torch.float64), values=torch.tensor([[30.0], [29.0], [27.0]])).to(DEV)
    prior = Prior(type=PriorType.LOG_NORMAL, mean=0.0, std=2.0, dim=3)
    g = torch.Generator().manual_seed(3)
    theta = (torch.tensor([10.0, 0.5, 0.01]) * (0.8 + 0.4 * torch.rand(8, 3, generator=g))).to(DEV)
    return net, obs, PoissonObservationLikelihood(), prior, theta


def test_pmmh_on_the_kernel_loop_runs_the_tau_leap_filter_kernel_under_the_iterations_key(monkeypatch):
    from viforsdes_amd import particle_mcmc, tau_leap_particle_filter
    from viforsdes_amd.inference.particle_mcmc import filter_key
    net, obs, like, prior, theta = _pmmh_problem()
    key = jfref.key_tensor(11, 12, DEV)
    calls = ref.counted("tau_leap_particle_filter", monkeypatch)[0]
    steps = ref.counted("pmmh_step", monkeypatch)[0]
    trace = []
    res = particle_mcmc(net, obs, like, prior, 0.1, theta, 6, n_particles=64, theta_positive_dims=(0, 1, 2), key=key, dynamics="tau_leap",
                        _trace=trace)
    assert len(calls) == 6 and len(steps) >= 7 and len(trace) == 6  # the kernel loop: a filter launch per iteration
    assert res.samples.shape == (6, 8, 3) and bool(torch.isfinite(res.log_likelihood).all())
    for i, row in enumerate(trace):
        assert torch.equal(row["filter_key"].cpu(), filter_key(i, key).cpu())
        direct = tau_leap_particle_filter(net, obs, like, row["theta_prop"], 0.1, n_particles=64, key=row["filter_key"])
        assert torch.equal(direct.log_likelihood.reshape(row["loglik"].shape), row["loglik"])


def test_fp64_theta_and_too_many_particles_take_the_torch_route(monkeypatch):
    from viforsdes_amd import _hip, tau_leap_particle_filter, tau_leap_process
    net, obs, like, prior, theta = _pmmh_problem()
    calls = ref.counted("tau_leap_particle_filter", monkeypatch)[0]
    sims = ref.counted("tau_leap_process", monkeypatch)[0]
    cap = _hip.tau_leap_filter_max_particles(1, 3)
    assert cap == 512
    a = tau_leap_particle_filter(net, obs, like, theta[:2].double(), 0.1, n_particles=64, key=jfref.key_tensor(1, 2, DEV))
    b = tau_leap_particle_filter(net, obs, like, theta[:1], 0.1, n_particles=cap + 64, key=jfref.key_tensor(1, 2, DEV))
    c = tau_leap_particle_filter(net, obs, like, theta[:1], 0.1, n_particles=72, key=jfref.key_tensor(1, 2, DEV))
    tau_leap_process(net, [30], theta[:2].double(), [0.5], 0.1, key=(1, 2))
    assert calls == [] and sims == []
    assert a.log_likelihood.dtype == torch.float64 and all(bool(torch.isfinite(r.log_likelihood).all()) for r in (a, b, c))
    tau_leap_particle_filter(net, obs, like, theta[:1], 0.1, n_particles=cap, key=jfref.key_tensor(1, 2, DEV))
    tau_leap_process(net, [30], theta[:2], [0.5], 0.1, key=(1, 2))
    assert calls == [1] and sims == [1]
