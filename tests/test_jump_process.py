"""CPU: the torch specification of the jump process (viforsdes_amd/core/jump_process.py, float64) against the independent numpy
restatement (tests/jump_process_reference.py), its edge rules, the exact law of an immigration-death process, the fields of
``diffusion_approximation_check``, and the argument checks of the two C entry points (made before any HIP call, so they run
without a device)."""
import ctypes
import math

import numpy as np
import pytest
import torch

import jump_process_reference as ref
from reaction_networks import BD, ISOMER, SIR
from viforsdes_amd import (DiffusionApproximationCheck, JumpProcessResult, ReactionNetworkSDE, diffusion_approximation_check,
                           jump_process)

KEY = (123, 456)
CASES = ref.cases()
IMMIGRATION_DEATH = dict(reactants=[[0], [1]], products=[[1], [0]])


def rates_of(net, theta):
    return net.kernel_parameters(torch.as_tensor(theta, dtype=torch.float64)).numpy()


@pytest.mark.parametrize("name", sorted(CASES))
def test_torch_route_matches_the_numpy_reference(name):
    spec, x0, theta = CASES[name]
    net = ReactionNetworkSDE(**spec)
    B, E, times = 37, 64, [0.0, 0.5, 0.5, 2.0]
    xs, th = ref.per_path_inputs(x0, theta, B, seed=len(name))
    res = jump_process(net, torch.from_numpy(xs), torch.from_numpy(th), times, key=KEY, max_events=4096, record_events=E)
    assert isinstance(res, JumpProcessResult)
    states, n_events, status, ev_t, ev_r = ref.simulate(ref.tables(net), xs, rates_of(net, th), times, KEY, 4096, E)
    assert res.states.dtype == torch.int32 and res.n_events.dtype == torch.int32 and res.status.dtype == torch.int32
    assert res.event_times.dtype == torch.float64 and res.event_reactions.dtype == torch.int32
    assert np.array_equal(res.event_reactions.numpy(), ev_r)
    assert np.array_equal(res.states.numpy(), states)
    assert np.array_equal(res.n_events.numpy(), n_events)
    assert np.array_equal(res.status.numpy(), status) and bool(res.complete.all())
    got = res.event_times.numpy()
    assert np.array_equal(np.isnan(got), np.isnan(ev_t))
    live = ~np.isnan(ev_t)
    assert live.sum() > 10 * B
    assert np.max(np.abs(got[live] - ev_t[live]) / ev_t[live]) <= 1e-12


def test_second_order_reaction_needs_two_molecules():
    net = ReactionNetworkSDE(reactants=[[2]], products=[[1]])          # 2X -> X alone
    res = jump_process(net, [1], torch.tensor([3.0], dtype=torch.float64), [1.0, 5.0], n_paths=5, key=KEY)
    assert res.states.tolist() == [[[1], [1]]] * 5 and res.n_events.tolist() == [0] * 5 and res.status.tolist() == [0] * 5
    res = jump_process(net, [2], torch.tensor([3.0], dtype=torch.float64), [50.0], n_paths=5, key=KEY)
    assert res.states.tolist() == [[[1]]] * 5 and res.n_events.tolist() == [1] * 5


def test_a_zero_constant_is_never_chosen():
    net = ReactionNetworkSDE(**BD)
    res = jump_process(net, [6], torch.tensor([4.0, 0.5, 0.0], dtype=torch.float64), [3.0], n_paths=64, key=KEY, record_events=64)
    assert int(res.n_events.min()) > 0 and not bool((res.event_reactions == 2).any())


def test_isomerisation_conserves_the_total():
    net = ReactionNetworkSDE(**ISOMER)
    res = jump_process(net, [7, 3], torch.tensor([1.0, 2.0], dtype=torch.float64), [0.0, 0.3, 1.0, 4.0], n_paths=64, key=KEY)
    assert bool((res.states.sum(dim=-1) == 10).all()) and bool((res.states >= 0).all())
    assert len(torch.unique(res.states[:, -1, 0])) > 1


def test_absorbed_state_fills_the_outputs():
    net = ReactionNetworkSDE(**SIR)
    res = jump_process(net, [40, 0], torch.tensor([0.01, 0.2], dtype=torch.float64), [0.0, 1.0, 2.0], n_paths=3, key=KEY,
                       record_events=4)
    assert res.states.tolist() == [[[40, 0]] * 3] * 3 and res.status.tolist() == [0] * 3 and res.n_events.tolist() == [0] * 3
    assert bool(torch.isnan(res.event_times).all()) and bool((res.event_reactions == -1).all())


def test_event_cap_stops_with_status_1():
    net = ReactionNetworkSDE(**BD)
    res = jump_process(net, [5], torch.tensor([200.0, 0.1, 0.0], dtype=torch.float64), [0.0, 10.0, 20.0], n_paths=8, key=KEY,
                       max_events=3, record_events=8)
    assert res.status.tolist() == [1] * 8 and res.n_events.tolist() == [3] * 8 and not bool(res.complete.any())
    assert res.states[:, 0].tolist() == [[5]] * 8 and bool((res.states[:, 1:] == -1).all())
    assert bool(torch.isfinite(res.event_times[:, :3]).all()) and bool(torch.isnan(res.event_times[:, 3:]).all())


def test_negative_constant_stops_with_status_2():
    net = ReactionNetworkSDE(**BD)
    theta = torch.tensor([[1.0, 0.5, 0.0], [1.0, -0.5, 0.0], [float("nan"), 0.5, 0.0]], dtype=torch.float64)
    res = jump_process(net, [5], theta, [1.0], key=KEY)
    assert res.status.tolist() == [0, 2, 2] and res.states[1:].tolist() == [[[-1]], [[-1]]] and res.complete.tolist() == [True, False, False]


def test_same_key_same_result_other_key_other_result():
    net = ReactionNetworkSDE(**SIR)
    theta = torch.tensor([0.02, 0.5], dtype=torch.float64)
    a = jump_process(net, [95, 5], theta, [1.0, 2.0], n_paths=32, key=KEY)
    b = jump_process(net, [95, 5], theta, [1.0, 2.0], n_paths=32, key=torch.tensor(KEY))
    c = jump_process(net, [95, 5], theta, [1.0, 2.0], n_paths=32, key=(123, 457))
    assert torch.equal(a.states, b.states) and torch.equal(a.n_events, b.n_events)
    assert not torch.equal(a.states, c.states)
    torch.manual_seed(3)
    d = jump_process(net, [95, 5], theta, [1.0, 2.0], n_paths=32)
    torch.manual_seed(3)
    e = jump_process(net, [95, 5], theta, [1.0, 2.0], n_paths=32)
    assert torch.equal(d.states, e.states)


def test_argument_errors():
    net = ReactionNetworkSDE(**SIR)
    theta = torch.tensor([0.02, 0.5], dtype=torch.float64)
    ok = dict(net=net, x0=[95, 5], theta=theta, times=[1.0, 2.0], key=KEY)
    jump_process(**ok)
    bad = [dict(x0=[95.5, 5]), dict(x0=[-1, 5]), dict(x0=[2 ** 30 + 1, 5]), dict(x0=[float("nan"), 5.0]), dict(times=[2.0, 1.0]),
           dict(times=[-1.0, 1.0]), dict(times=[]), dict(times=[[1.0, 2.0]]), dict(max_events=0), dict(max_events=2 ** 23 + 1),
           dict(record_events=-1), dict(x0=[95, 5, 1]), dict(theta=torch.ones(3, dtype=torch.float64)),
           dict(x0=torch.ones(4, 2), theta=torch.ones(3, 2, dtype=torch.float64)), dict(x0=torch.ones(4, 2), n_paths=5),
           dict(theta=torch.ones(2, dtype=torch.int64)), dict(key=(1, 2, 3)), dict(n_paths=0), dict(net="sir")]
    for change in bad:
        with pytest.raises(ValueError):
            jump_process(**{**ok, **change})
    jump_process(**{**ok, "x0": torch.tensor([2.0 ** 30, 0.0]), "theta": torch.zeros(2, dtype=torch.float64)})


# --- exact law: immigration-death from x0 = 30, x(t) ~ Binomial(30, e^{-0.5 t}) + Poisson(20 (1 - e^{-0.5 t}))
def test_exact_law_of_immigration_death():
    net = ReactionNetworkSDE(**BD)
    res = jump_process(net, [30], torch.tensor([10.0, 0.5, 0.0], dtype=torch.float64), [1.0, 2.0], n_paths=65536, key=KEY)
    assert bool(res.complete.all()) and int(res.n_events.max()) < 200
    for k, t in enumerate((1.0, 2.0)):
        ref.check_exact_law(res.states[:, k, 0].numpy(), 30, 10.0, 0.5, t)


def test_first_event_time_of_sir_is_exponential():
    net = ReactionNetworkSDE(**SIR)
    B = 16384
    res = jump_process(net, [95, 5], torch.tensor([0.004, 0.15], dtype=torch.float64), [100.0], n_paths=B, key=KEY, max_events=1,
                       record_events=1)
    a0 = 0.004 * 95 * 5 + 0.15 * 5
    first = res.event_times[:, 0].numpy()
    z = (first.mean() - 1 / a0) / (1 / a0 / math.sqrt(B))
    print(f"first event: mean {first.mean():.5f} against {1 / a0:.5f}, z = {z:.3f}")
    assert res.n_events.tolist() == [1] * B and abs(z) <= 4.5


# --- diffusion_approximation_check
def test_diffusion_approximation_check_high_and_low_copy_numbers():
    net = ReactionNetworkSDE(**IMMIGRATION_DEATH)
    torch.manual_seed(0)
    times, dt = [0.1, 0.25, 0.5], 0.01
    high = diffusion_approximation_check(net, [1000], torch.tensor([500.0, 0.5], dtype=torch.float64), times, dt, n_paths=1024, key=KEY)
    low = diffusion_approximation_check(net, [1], torch.tensor([0.5, 1.0], dtype=torch.float64), times, dt, n_paths=1024, key=KEY)
    for chk in (high, low):
        assert isinstance(chk, DiffusionApproximationCheck) and chk.n_incomplete == 0
        assert chk.times.tolist() == pytest.approx(times) and chk.jump_states.shape == (1024, 3, 1)
        ref.check_fields(chk)
    print(f"KS distance: high copy {float(high.ks_distance.max()):.4f}, low copy {float(low.ks_distance.max()):.4f}")
    assert float(low.ks_distance.max()) > float(high.ks_distance.max())
    assert float(high.zero_fraction.max()) == 0.0 and float(low.zero_fraction.min()) > 0.0
    with pytest.raises(ValueError):
        diffusion_approximation_check(net, [1], torch.tensor([0.5, 1.0], dtype=torch.float64), [0.004, 0.5], dt, n_paths=8)


def test_diffusion_approximation_check_takes_theta_rows_and_leaves_incomplete_paths_out():
    net = ReactionNetworkSDE(**SIR)
    theta = torch.tensor([0.004, 0.15], dtype=torch.float64) * torch.linspace(0.9, 1.1, 48, dtype=torch.float64)[:, None]
    theta[5, 1] = -1.0                                   # an invalid row: status 2, left out of both sides
    chk = diffusion_approximation_check(net, [95, 5], theta, [1.0, 2.0], 0.05, key=KEY)
    assert chk.n_incomplete == 1 and chk.jump_states.shape == (47, 2, 2) and chk.diffusion_states.shape == (47, 2, 2)
    ref.check_fields(chk)


# --- the C entry points' own checks: VSDE_E_BADARG before any HIP call
def _entry(kinetic):
    from viforsdes_amd import _hip
    lib = _hip.load()
    net = _hip.crn_network(SIR["reactants"], [[-1, 1], [0, -1]])
    head = [ctypes.byref(net)]
    if kinetic:
        head.append(ctypes.byref(_hip.crn_kinetics([None, (1, 0, 2)])))
    return lib, getattr(lib, "vsde_crn_kinetic_jump_process" if kinetic else "vsde_crn_jump_process"), net, head


def _arguments(**over):
    """The arguments after the descriptors, every pointer a non-NULL dummy (never read: each case fails a check first)."""
    a = dict(B=4, S=2, P=2, K=3, E=0, x0=8, theta=8, out_times=8, key=8, max_events=16, states=8, n_events=8, status=8,
             event_times=0, event_reactions=0)
    a.update(over)
    ints = ("B", "S", "P", "K", "E")
    return ([ctypes.c_int(a[n]) for n in ints] + [ctypes.c_void_p(a[n] or None) for n in ("x0", "theta", "out_times", "key")]
            + [ctypes.c_int(a["max_events"])]
            + [ctypes.c_void_p(a[n] or None) for n in ("states", "n_events", "status", "event_times", "event_reactions")]
            + [ctypes.c_void_p(None)])


BAD_ARGUMENTS = [dict(S=3), dict(P=5), dict(K=0), dict(E=-1), dict(B=0), dict(max_events=0), dict(max_events=2 ** 23 + 1),
                 dict(x0=0), dict(theta=0), dict(out_times=0), dict(key=0), dict(states=0), dict(n_events=0), dict(status=0),
                 dict(E=4, event_times=0, event_reactions=8), dict(E=4, event_times=8, event_reactions=0)]


@pytest.mark.parametrize("kinetic", [False, True])
def test_entry_points_refuse_bad_arguments_before_any_hip_call(kinetic):
    lib, fn, net, head = _entry(kinetic)
    fn.restype = ctypes.c_int
    width = 4 if kinetic else 2
    for over in BAD_ARGUMENTS:
        over = {"P": width, **over}
        assert fn(*head, *_arguments(**over)) == -1, over
        assert lib.vsde_last_error()
    # descriptor limits: S, R outside 1..8 / 1..16, an order above 3; a NULL descriptor
    for field, value in (("S", 9), ("S", 0), ("R", 17), ("R", 0)):
        old = getattr(net, field)
        setattr(net, field, value)
        assert fn(*head, *_arguments(P=width)) == -1, (field, value)
        setattr(net, field, old)
    net.order[0][0] = 4
    assert fn(*head, *_arguments(P=width)) == -1
    net.order[0][0] = 1
    assert fn(ctypes.c_void_p(None), *head[1:], *_arguments(P=width)) == -1
    if kinetic:
        assert fn(head[0], ctypes.c_void_p(None), *_arguments(P=width)) == -1
