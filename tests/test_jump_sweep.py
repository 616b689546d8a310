"""CPU: the conditions of the jump sweep (tests/test_jump_sweep_gpu.py) on the float64 references alone; no
kernel output enters.

* every case's network is served by the kernels, and the key salts of tests/sde_sweep_reference.py are the first that meet the
  conditions below (``find_salts`` reproduces the tables);
* ``jump_kernel`` cases: at least 200 events in total, no path at the cap of 64, undecidable reaction choices at most 1e-3 of the
  events;
* ``jf_kernel`` cases: ESS > N / 20 at every observation, no particle stopped, flagged (particle, segment) pairs at most 2e-2 (the
  kernel check's cap), and at N = 64 no resampling threshold within 1e-5 of a cumulative sum: none per case, which is within the
  particle-filter sweep's caps of 2 per case and 1e-3 overall;
* the vectorised segment runner the sweep uses equals ``run_segment`` particle by particle."""
import numpy as np
import pytest

import jump_filter_reference as jf
import jump_process_reference as jref
import sde_sweep_reference as W


def test_networks_are_kernel_compatible_with_integer_start_states():
    for name in W.NAMES:
        net, theta, start = W.jump_net(name)
        assert net.kernel_compatible() and len(theta) == net.sde_param_dim and all(isinstance(v, int) and v > 0 for v in start)


def test_jump_cases_meet_the_reference_conditions():
    assert len(W.JUMP_SALTS) == len(W.NAMES)
    events = undecidable = 0
    for name in W.NAMES:
        c = W.jump_conditions(name)
        assert c["events"] >= 200 and c["capped"] == 0 and c["undecidable"] <= 1e-3 * c["events"], (name, c)
        events, undecidable = events + c["events"], undecidable + c["undecidable"]
    print(f"jump sweep: {events} events over {len(W.NAMES)} cases, {undecidable} undecidable")


def test_jump_salts_are_the_first_that_meet_the_conditions():
    salted = [n for n, s in zip(W.NAMES, W.JUMP_SALTS) if s]
    assert W.find_salts(W.jump_conditions, salted) == tuple(s for s in W.JUMP_SALTS if s)


def test_filter_cases_meet_the_reference_conditions():
    assert len(W.JF_SALTS) == len(W.NAMES)
    total = entries = 0
    for name in W.NAMES:
        c = W.filter_conditions(name)
        assert c["ess"] > W.JF_N / 20 and c["stopped"] == 0 and c["flagged"] <= 2e-2 * c["pairs"], (name, c)
        assert c["undecidable"] <= 2 and c["events"] > c["pairs"], (name, c)
        total, entries = total + c["undecidable"], entries + c["pairs"]
    assert total <= 1e-3 * entries
    assert W.find_salts(W.filter_conditions, W.NAMES) == W.JF_SALTS


@pytest.mark.parametrize("name", W.JF_BIG)
def test_large_filter_cells_meet_the_reference_conditions(name):
    c = W.filter_conditions(name, big=True)
    print(name, c)
    assert c["ess"] > W.JF_BIG_N / 20 and c["stopped"] == 0 and c["flagged"] <= 2e-2 * c["pairs"], c


@pytest.mark.parametrize("name", ["sw-S1-NR4", "sw-S4-NR8-k", "sw-S8-NR16-k", "sw-S6-NR8-R5"])
def test_vectorised_segments_equal_the_scalar_reference(name):
    net, th, xs, ys, like, key, N = W.filter_case(name)
    tab = jref.tables(net)
    rates = net.kernel_parameters(th.double()).numpy()
    start = np.repeat(xs[1][None], N, axis=0) + np.arange(N)[:, None] % 3
    for cap in (4096, 2):
        x, fired, status, near = jf.run_segments(tab, start, rates[1], 0.25, 1.0, 3, N + np.arange(N), key, cap)
        for j in range(N):
            want = jf.run_segment(tab, start[j], rates[1], 0.25, 1.0, 3, N + j, key, cap)
            assert np.array_equal(x[j], want[0]) and (fired[j], status[j], bool(near[j])) == want[1:], (cap, j)
        assert (status == (1 if cap == 2 else 0)).any()
