"""GPU: every instantiation ``<S, NR, KIN, ANCHORED>`` of the jump-segment replay kernel (csrc/vsde_jump_replay.hip: jr_kernel) on
the cases of tests/sde_sweep_reference.py (the 48 cells of ``crn_dispatch`` and the lower-edge points R = 5, 9; DESIGN section
3.33), every launch through ``_hip``.  Per case, M = 3 filters of N = 64 particles, D = 22 draws per filter whose final slots come
from a seeded generator (slot 0, slot N - 1, a repeated slot and a dead draw in every row): B K = 264 threads, a full block and a
block of 8.

a. the filter on the kernel route, as tests/test_jump_sweep_gpu.py runs it;
b. the filter-form replay of its store: lineage equal to ``particle_smoother._trace`` of the kernel's ancestors, paths at
   ``q(T_k)`` and event counts equal to the store bit for bit, status 0, dead draws -1; every (record, segment) pair against float64
   from the kernel's own particles (``jump_smoother_reference.score_records``);
c. the anchored replay of the same records, built in torch from (b): the same bits as (b);
d. the anchored replay at the cap ``JR_SMALL_CAP`` with one more record whose first rate constant is negative: against float64
   at the same cap; the bad record has status 2, no event and -1 throughout;
e. (b) and (c) twice for the same bits;
f. ``max_events`` 0 and 2^23 + 1 are refused before any launch, in both forms, for one cell of each S.

Everything is exact outside undecidable pairs, whose share (at most 2e-2 of the pairs of a launch) is asserted first.  The
conditions on the float64 reference alone are asserted by tests/test_jump_replay_sweep.py on the CPU."""
import numpy as np
import pytest
import torch

import jump_filter_reference as jf
import jump_process_reference as jref
import jump_smoother_reference as ref
import sde_sweep_reference as W

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F64 = torch.float64
TIMES, PATH_TIMES = W.JUMP_TIMES, ref.REPLAY_PATH_TIMES
AT_OBS = [0, 3, 3, 6]                                             # q(T_k)


def _kernel_rows(net, th):
    """(theta as the kernels take it, on the device; the float64 effective constants of the reference) of theta fp32 [M, P]."""
    return (th if net.plain else net.kernel_parameters(th)).to(DEV).contiguous(), net.kernel_parameters(th.double()).numpy()


def _grid():
    return (torch.tensor(TIMES, dtype=F64, device=DEV), torch.tensor(PATH_TIMES, dtype=F64, device=DEV),
            torch.from_numpy(ref.ownership(PATH_TIMES, TIMES).astype(np.int32)))


@pytest.mark.parametrize("name", W.NAMES)
def test_jump_replay_cell(name):
    from viforsdes_amd import Observations, _hip, jump_particle_filter
    from viforsdes_amd.inference.particle_smoother import _trace
    net, th, xs, ys, like, key, N, last = W.replay_case(name)
    M, D, K, Q, S = W.JF_M, W.JR_D, len(TIMES), len(PATH_TIMES), xs.shape[1]
    B = M * D
    # a. the filter
    obs = Observations(times=torch.tensor(TIMES, dtype=F64), values=torch.tensor(ys, dtype=torch.float32))
    calls, real, wrapped = jf.counted()
    _hip.jump_particle_filter = wrapped
    try:
        res = jump_particle_filter(net, obs.to(DEV), jf.likelihood(like), th.to(DEV), n_particles=N, initial_state=torch.from_numpy(xs).to(DEV),
                                   return_particles=True, key=jf.key_tensor(*key, DEV), max_events=W.JF_MAX_EVENTS)
    finally:
        _hip.jump_particle_filter = real
    assert calls == [1] and int(res.stopped.sum()) == 0             # the kernel route; no particle stopped
    assert res.particles.dtype == torch.int32 and res.ancestors.dtype == torch.int32 and tuple(res.particles.shape) == (M, K, N, S)
    # b. the filter form
    network, keyt = net.kernel_descriptor(), jf.key_tensor(*key, DEV)
    x0, (kth, rates) = torch.from_numpy(xs).to(torch.int32).to(DEV), _kernel_rows(net, th)
    times, pt, q_begin = _grid()
    last_dev = torch.from_numpy(last).to(DEV)
    form_b = lambda: _hip.jump_filter_replay(x0, kth, times, pt, q_begin, keyt, W.JR_CAP, res.particles, res.ancestors, last_dev, network=network)
    paths, lineage, n_events, status = form_b()
    assert tuple(paths.shape) == (M, D, Q, S) and all(tuple(t.shape) == (M, D, K) for t in (lineage, n_events, status))
    assert torch.equal(lineage, _trace(res.ancestors, last_dev))
    live = last_dev >= 0
    assert int((~live).sum()) == M and bool((lineage[~live] == -1).all()) and bool((lineage[live] >= 0).all())
    assert bool((paths[~live] == -1).all()) and int(n_events[~live].abs().sum()) == 0 and int(status.abs().sum()) == 0
    slot = lineage.long().clamp(min=0)
    for k, q in enumerate(AT_OBS):
        stored = torch.stack([res.particles[m, k][slot[m, :, k]] for m in range(M)])
        fired = torch.stack([res.events[m, k][slot[m, :, k]] for m in range(M)])
        assert torch.equal(paths[:, :, q][live], stored[live]) and torch.equal(n_events[:, :, k][live], fired[live]), k
    tab = jref.tables(net)
    records = ref.records_of_lineage(res.particles.cpu().numpy(), lineage.cpu().numpy(), xs, rates, key)
    want = ref.replay_records(tab, *records, TIMES, PATH_TIMES, W.JR_CAP)
    ref.score_records(want, paths.reshape(B, Q, S).cpu().numpy(), n_events.reshape(B, K).cpu().numpy(), status.reshape(B, K).cpu().numpy(),
                      records[2], TIMES, PATH_TIMES, f"{name} filter form")
    assert int(n_events.sum()) > B * K                              # something happened
    # c. the anchored form of the same records
    xb, thb, anchors, noise, keys = ref.anchored_inputs(res.particles, lineage, x0, kth, keyt)
    assert np.array_equal(anchors.cpu().numpy(), records[2]) and np.array_equal(noise.cpu().numpy().view(np.uint32), records[3])
    assert int((noise[:, -1] == -1).sum()) == M                     # all ones: the dead draws
    form_c = lambda: _hip.jump_anchored_replay(xb, thb, times, pt, q_begin, anchors, noise, keys, W.JR_CAP, network=network)
    a_paths, a_events, a_status = form_c()
    assert torch.equal(a_paths, paths.reshape(B, Q, S)) and torch.equal(a_events, n_events.reshape(B, K)) and torch.equal(a_status, status.reshape(B, K))
    # d. the anchored form, stopped: the small cap, and one more record with a negative rate constant on the feed (no reactants:
    # they are always present), which is an invalid propensity from the first event of every segment
    assert not tab["reactants"][0].any() and bool((thb[:, 0] > 0).all())
    r0 = int(torch.nonzero(noise[:, -1] != -1)[0])                  # the first live record lends the bad one its anchors
    bad_th, bad_rates = thb[r0].clone(), records[1][r0].copy()
    bad_th[0], bad_rates[0] = -bad_th[0].abs(), -abs(bad_rates[0])
    plus = lambda t, row: torch.cat([t, row[None]]).contiguous()
    s_paths, s_events, s_status = _hip.jump_anchored_replay(plus(xb, xb[r0]), plus(thb, bad_th), times, pt, q_begin, plus(anchors, anchors[r0]),
                                                            plus(noise, noise[r0]), plus(keys, keys[r0]), W.JR_SMALL_CAP, network=network)
    more = [np.concatenate([v, row[None]]) for v, row in zip(records, (records[0][r0], bad_rates, records[2][r0], records[3][r0], records[4][r0]))]
    want = ref.replay_records(tab, *more, TIMES, PATH_TIMES, W.JR_SMALL_CAP)
    ref.score_records(want, s_paths.cpu().numpy(), s_events.cpu().numpy(), s_status.cpu().numpy(), more[2], TIMES, PATH_TIMES,
                      f"{name} anchored form, cap {W.JR_SMALL_CAP}")
    assert (want["status"][B] == 2).all() and bool((s_status[B] == 2).all()) and int(s_events[B].abs().sum()) == 0 and bool((s_paths[B] == -1).all())
    assert bool((s_status[:B] == 1).any()) and bool((s_status[:B] == 0).any()) and int(s_events.max()) == W.JR_SMALL_CAP
    # e. the same bits twice
    for first, again in (((paths, lineage, n_events, status), form_b()), ((a_paths, a_events, a_status), form_c())):
        assert all(torch.equal(u, v) for u, v in zip(first, again))


def test_bad_event_caps_are_refused_before_any_launch():
    from viforsdes_amd import _hip
    times, pt, q_begin = _grid()
    K, D, N = len(TIMES), 2, W.JF_N
    i32 = dict(dtype=torch.int32, device=DEV)
    for S in range(1, W.CRN_MAX_S + 1):
        name = W.NAMES[W.CELLS.index((S, 16, S % 2 == 0))]
        net, th, xs, ys, like, key, _ = W.filter_case(name)
        M = len(xs)
        x0, kth, keyt = torch.from_numpy(xs).to(torch.int32).to(DEV), _kernel_rows(net, th)[0], jf.key_tensor(*key, DEV)
        parts, anc, last = x0[:, None, None, :].expand(M, K, N, S).contiguous(), torch.arange(N, **i32).expand(M, K, N).contiguous(), torch.zeros(M, D, **i32)
        lineage = torch.zeros(M, D, K, **i32)
        xb, thb, anchors, noise, keys = ref.anchored_inputs(parts, lineage, x0, kth, keyt)
        for cap in (0, 2 ** 23 + 1):
            with pytest.raises(ValueError, match="max_events"):
                _hip.jump_filter_replay(x0, kth, times, pt, q_begin, keyt, cap, parts, anc, last, network=net.kernel_descriptor())
            with pytest.raises(ValueError, match="max_events"):
                _hip.jump_anchored_replay(xb, thb, times, pt, q_begin, anchors, noise, keys, cap, network=net.kernel_descriptor())
    torch.cuda.synchronize()
