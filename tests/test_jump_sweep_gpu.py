"""GPU: every instantiation ``<S, NR, KIN>`` of the jump-process kernel (csrc/vsde_jump.hip: jump_kernel) and of the jump-process
particle-filter kernel (csrc/vsde_jump_filter.hip: jf_kernel) on the cases of tests/sde_sweep_reference.py (the 48 cells of
``crn_dispatch`` and the lower-edge points R = 5, 9), through the public ``jump_process`` and ``jump_particle_filter``
(DESIGN section 3.31).  The Gillespie event loops with their ``crn_pick<S>`` select and the 2-bit packed ``orders`` word are
compiled per cell; the named networks of the other jump tests reach seven of them.

* ``jump_kernel``: B = 65 paths (a full wave and a wave of one lane) with per-path theta and x0, times [0, 0.25, 0.25, 1] (a zero and
  a duplicate), max_events = 64 so that the log holds every event; scored with ``jump_process_reference.check_stages`` as
  tests/test_jump_process_gpu.py scores the named networks: waiting time 1e-5 relative, reaction equal to float64's unless
  undecidable (at most 1e-3 of the events), outputs bit-exact against the kernel's own log.
* ``jf_kernel``: M = 3 filters of N = 64 particles on the same times, Gaussian, Poisson and negative-binomial terms alternating
  over the cases; scored stage by stage on the kernel's own previous stage with the three checks of
  tests/test_jump_filter_gpu.py (``jump_filter_reference.check_propagation`` / ``check_weights_and_summaries`` /
  ``check_ancestors``).  S = 1 and S = 8 at NR = 16, both forms, run again at N = 1024.
* N = 1088 is refused by the entry point before any launch, for every species count.

The conditions on the float64 references alone (events, caps, ESS, undecidable shares, the key salts) are asserted by
tests/test_jump_sweep.py on the CPU."""
import pytest
import torch

import jump_filter_reference as jf
import jump_process_reference as jref
import sde_sweep_reference as W

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.mark.parametrize("name", W.NAMES)
def test_jump_kernel_cell(name):
    from viforsdes_amd import jump_process
    net, xs, th32, times, key = W.jump_case(name)
    assert net.kernel_compatible()
    res = jump_process(net, torch.as_tensor(xs), torch.as_tensor(th32, device=DEV), times, n_paths=W.JUMP_B, key=key,
                       max_events=W.JUMP_E, record_events=W.JUMP_E)
    events, _ = jref.check_stages(net, xs, th32, times, res, W.JUMP_E, key)
    assert events >= 200 and int(res.status.sum()) == 0
    bare = jump_process(net, torch.as_tensor(xs), torch.as_tensor(th32, device=DEV), times, n_paths=W.JUMP_B, key=key,
                        max_events=W.JUMP_E)
    assert bare.event_times is None and torch.equal(res.states, bare.states) and torch.equal(res.n_events, bare.n_events)


def _filter_cell(name, big):
    from viforsdes_amd import Observations, _hip, jump_particle_filter
    net, th, xs, ys, like, key, N = W.filter_case(name, big)
    obs = Observations(times=torch.tensor(W.JUMP_TIMES, dtype=torch.float64), values=torch.tensor(ys, dtype=torch.float32))
    calls, real, wrapped = jf.counted()
    _hip.jump_particle_filter = wrapped
    try:
        res = jump_particle_filter(net, obs.to(DEV), jf.likelihood(like), th.to(DEV), n_particles=N, initial_state=torch.from_numpy(xs).to(DEV),
                                   return_particles=True, key=jf.key_tensor(*key, DEV), max_events=W.JF_MAX_EVENTS)
    finally:
        _hip.jump_particle_filter = real
    assert calls == [1]                                             # the public function took the kernel route
    label = f"{name} N={N} {like[0]}"
    jf.check_propagation(net, th, xs, W.JUMP_TIMES, res, key, label, vectorized=True)
    jf.check_weights_and_summaries(like, ys, res, label)
    jf.check_ancestors(like, ys, res, key, label)


@pytest.mark.parametrize("name", W.NAMES)
def test_jump_filter_cell(name):
    _filter_cell(name, False)


@pytest.mark.parametrize("name", W.JF_BIG)
def test_jump_filter_cell_at_1024_particles(name):
    _filter_cell(name, True)


def test_too_many_particles_are_refused_before_any_launch():
    from viforsdes_amd import _hip
    for S in range(1, W.CRN_MAX_S + 1):
        name = W.NAMES[W.CELLS.index((S, 16, S % 2 == 0))]
        net, th, xs, ys, like, key, N = W.filter_case(name)
        too_many = _hip.jump_filter_max_particles(S, net.num_reactions, not net.plain) + 64
        assert too_many == W.JF_BIG_N + 64
        rates = (th if net.plain else net.kernel_parameters(th)).to(DEV)
        with pytest.raises(ValueError, match="particles"):
            _hip.jump_particle_filter(torch.from_numpy(xs).to(torch.int32).to(DEV), rates, torch.tensor(W.JUMP_TIMES, dtype=torch.float64, device=DEV),
                                      torch.tensor(ys, dtype=torch.float32, device=DEV), None, 25.0, jf.key_tensor(*key, DEV), W.JF_MAX_EVENTS, too_many,
                                      network=net.kernel_descriptor(), return_particles=True)
    torch.cuda.synchronize()
