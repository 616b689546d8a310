"""CPU: the conditions of the replay sweep (tests/test_jump_replay_sweep_gpu.py) on the float64 references alone;
no kernel output enters.  The float64 filter (``jump_filter_reference.run_filter``) with the seeded final slots of
``sde_sweep_reference.last_slots`` gives the lineages, ``jump_smoother_reference.replay_records`` replays along them.

* per case, at the cap 4096: flagged (record, segment) pairs at most 2e-2 of the 264, no segment stopped, the replay passes through
  the filter's store, and some interior output differs from the outputs at both neighbouring observation times in some record
  (outputs copied from an endpoint would otherwise pass);
* per case, at the small cap ``JR_SMALL_CAP``: flagged pairs at most 2e-2, a segment with status 0 and one with status 1, and (a
  condition of this file's own) a complete segment that fired three events, so that complete and stopped segments alike draw
  both halves of the first Philox block and from the second; over the sweep a status-1 segment that wrote some of its outputs and
  left others at -1, and one that left all of them at -1.  ``JR_SMALL_CAP`` is the smallest cap that shows all of this;
* the scorer binds: it accepts the reference's own outputs and rejects them with each of four defects injected in Python;
* the records the GPU file builds for the anchored form are the records ``particle_mcmc`` keeps (``draw_path_records``), on bd."""
import numpy as np
import pytest
import torch

import jump_filter_reference as jf
import jump_process_reference as jref
import jump_smoother_reference as ref
import sde_sweep_reference as W

TIMES, PATH_TIMES = W.JUMP_TIMES, ref.REPLAY_PATH_TIMES
PAIRS = W.JF_M * W.JR_D * len(TIMES)


def test_the_shapes_and_the_final_slots_are_what_the_sweep_says():
    assert len(W.NAMES) == 52 and PAIRS == 264 and PAIRS > 256 and (W.JF_M * W.JR_D) & (W.JF_M * W.JR_D - 1) != 0
    assert ref.ownership(PATH_TIMES, TIMES).tolist() == [0, 1, 4, 4, 7]           # segment 2 has no length and owns nothing
    for name in W.NAMES:
        last = W.last_slots(name)
        assert last.shape == (W.JF_M, W.JR_D) and last.dtype == np.int32 and np.array_equal(last, W.last_slots(name))
        for row in last:
            live = row[row >= 0]
            assert 0 in row and W.JF_N - 1 in row and (row == -1).sum() == 1 and live.max() < W.JF_N and len(np.unique(live)) < len(live)


def test_replay_cases_meet_the_reference_conditions():
    """Conditions (i)-(iii) per case and the two over the sweep; the totals are printed for DESIGN."""
    tot = {cap: dict(flagged=0, events=0, status=np.zeros(3, dtype=np.int64), partial=0, empty=0) for cap in (W.JR_CAP, W.JR_SMALL_CAP)}
    for name in W.NAMES:
        full, small = W.replay_conditions(name, W.JR_CAP), W.replay_conditions(name, W.JR_SMALL_CAP)
        assert full["pairs"] == small["pairs"] == PAIRS
        assert full["flagged"] <= ref.CAP * PAIRS and small["flagged"] <= ref.CAP * PAIRS, (name, full, small)          # (i)
        assert full["by_status"][1:] == [0, 0] and full["moved"], (name, full)                                           # (ii)
        assert small["by_status"][0] > 0 and small["by_status"][1] > 0 and small["by_status"][2] == 0, (name, small)     # (iii)
        assert small["three"], (name, small)
        assert full["ok"] and small["ok"]
        # the float64 replay passes through the float64 filter's own store: the same computation twice
        records, out = W.replay_lineages(name)[3], W.replay_reference(name, W.JR_CAP)
        live = records[3][:, -1] != ref.DEAD_PATH
        assert live.sum() == W.JF_M * (W.JR_D - 1) and np.array_equal(out["ends"][live], records[2][live])
        assert (out["paths"][~live] == -1).all() and not out["n_events"][~live].any() and out["n_events"].sum() > PAIRS
        for cap, c in ((W.JR_CAP, full), (W.JR_SMALL_CAP, small)):
            t = tot[cap]
            t["flagged"], t["events"], t["status"] = t["flagged"] + c["flagged"], t["events"] + c["events"], t["status"] + np.array(c["by_status"])
            t["partial"], t["empty"] = t["partial"] + c["partial"], t["empty"] + c["empty"]
    for cap, t in tot.items():
        print(f"replay sweep, float64 alone, cap {cap}: {t['flagged']} of {PAIRS * len(W.NAMES)} pairs flagged, {t['events']} events, live "
              f"segments by status {t['status'].tolist()}, status-1 segments with some / none of their outputs written {t['partial']} / {t['empty']}")
    assert tot[W.JR_SMALL_CAP]["partial"] > 0 and tot[W.JR_SMALL_CAP]["empty"] > 0


def test_the_small_cap_is_the_smallest_that_meets_the_conditions():
    assert W.find_small_cap() == W.JR_SMALL_CAP
    # without the three-event condition the stopped segments would never leave the even half of the first Philox block
    assert W.find_small_cap(second_block=False) == 1


# ------------------------------------------------------------------------------------------------------- the scorer binds
def _shifted_ownership():
    """The injected table: a ``t_q == T_k`` goes to segment k + 1 (``T_{k-1} <= t_q < T_k``), and the last output to nobody."""
    pt = np.asarray(PATH_TIMES)
    return np.concatenate([[0], [(pt < t).sum() for t in TIMES]]).astype(np.int64)


def _hi_dropped(tab):
    change = tab["change"].copy()
    change[:, 4:] = 0
    return dict(tab, change=change)


def _rejected(want, got, anchors):
    try:
        ref.score_records(want, got["paths"], got["n_events"], got["status"], anchors, TIMES, PATH_TIMES, quiet=True)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("name", W.NAMES)
def test_the_scorer_rejects_injected_defects(name):
    """Each defect in the reference's own outputs at the cap 4096, scored as a launch is (the anchors are the launch's inputs).
    ``late``, ``shifted`` and ``counter`` can show in every case: every case fires an event after an owned output of the same
    segment, has an output at the last observation time (which the shifted table gives to nobody), and has a segment with a second
    event.  ``hi`` can show where species 4..7 exist and change: every case with S > 4; at S <= 4 it is no defect and must pass."""
    tab, times, path_times, records = W.replay_lineages(name)
    want = W.replay_reference(name, W.JR_CAP)
    anchors = records[2]
    assert want["undecidable"].sum() <= ref.CAP * PAIRS               # so that a rejection below is a differing pair, not the cap
    assert not _rejected(want, want, anchors)
    run = lambda tab=tab, **kw: ref.replay_records(tab, *records, times, path_times, W.JR_CAP, **kw)
    assert _rejected(want, run(_late=True), anchors)
    assert _rejected(want, run(begin=_shifted_ownership()), anchors)
    assert _rejected(want, run(_counter=lambda e: e), anchors)
    S = len(records[0][0])
    assert _rejected(want, run(tab=_hi_dropped(tab)), anchors) == (S > 4)
    # the small cap: the scorer takes the stopped segments of the reference itself and rejects one that ran on past the cap
    small = W.replay_reference(name, W.JR_SMALL_CAP)
    assert not _rejected(small, small, anchors) and _rejected(small, want, anchors)


# ------------------------------------------------------------------------------ the anchored inputs are particle MCMC's records
def test_anchored_inputs_are_the_records_particle_mcmc_keeps():
    """bd through the torch route: the records ``draw_path_records`` forms from a filter's store are what ``anchored_inputs`` forms
    from the same store along the same lineage, and ``replay_records`` (the torch route of ``particle_mcmc``'s paths) gives on them
    the paths the float64 reference gives."""
    from viforsdes_amd import Observations, ReactionNetworkSDE, jump_particle_filter
    from viforsdes_amd.inference import jump_smoother as js
    from viforsdes_amd.inference import particle_mcmc as mc
    from viforsdes_amd.inference.particle_smoother import _trace
    N = 64
    spec, xs, th, ys, key = ref.replay_case("bd", N)
    net = ReactionNetworkSDE(**spec)
    th = torch.from_numpy(th).float().double()
    obs = Observations(times=torch.tensor(TIMES, dtype=torch.float64), values=torch.tensor(ys, dtype=torch.float64))
    flt = jump_particle_filter(net, obs, jf.likelihood(("poisson", 0.9, None)), th, n_particles=N, initial_state=torch.from_numpy(xs),
                               return_particles=True, key=torch.tensor(key), max_events=4096)
    M, K = len(xs), len(TIMES)
    loglik = flt.log_likelihood.clone()[:, None]                    # C = 3 chains of one filter each; the middle chain is dead
    loglik[1] = float("-inf")
    anchors, noise = mc.draw_path_records(loglik, flt.particles.double(), flt.ancestors, 5, torch.tensor([11, 12]))
    dead = noise[:, -1] == mc.DEAD_PATH
    assert dead.tolist() == [False, True, False] and mc.DEAD_PATH == ref.DEAD_PATH
    last = torch.where(dead, torch.full_like(noise[:, -1], -1), noise[:, -1] - torch.arange(M) * N)[:, None]
    lineage = _trace(flt.ancestors, last)
    x0, theta, mine, my_noise, keys = ref.anchored_inputs(flt.particles.to(torch.int32), lineage, torch.from_numpy(xs).to(torch.int32), th,
                                                          jf.key_tensor(*key, "cpu"))
    my_noise, keys = my_noise.long() & 0xFFFFFFFF, keys.long() & 0xFFFFFFFF
    assert torch.equal(my_noise[:, -1], noise[:, -1]) and torch.equal(my_noise[~dead], noise[~dead])
    assert torch.equal(mine[~dead].double(), anchors[~dead]) and keys.tolist() == [[int(v) & 0xFFFFFFFF for v in key]] * M
    assert torch.equal(x0.long(), torch.from_numpy(xs)) and torch.equal(theta, th)
    # numpy and torch form the same records
    n_x0, n_rates, n_anchors, n_noise, n_keys = ref.records_of_lineage(flt.particles.numpy(), lineage.numpy(), xs, net.kernel_parameters(th).numpy(), key)
    assert np.array_equal(n_anchors, mine.numpy()) and np.array_equal(n_noise, my_noise.numpy()) and np.array_equal(n_keys, keys.numpy())
    t_out = torch.tensor(PATH_TIMES, dtype=torch.float64)
    q_begin = js.ownership_ranges(t_out, obs.times)
    assert q_begin.tolist() == ref.ownership(PATH_TIMES, TIMES).tolist()
    rates = net.kernel_parameters(th)
    for cap in (4096, W.JR_SMALL_CAP):
        got = js.replay_records(net, rates, x0.long(), obs.times, t_out, q_begin, mine, torch.where(dead[:, None], 0, my_noise), keys, cap, dead)
        theirs = js.replay_records(net, rates, x0.long(), obs.times, t_out, q_begin, torch.nan_to_num(anchors, nan=0.0).to(torch.int32),
                                   torch.where(dead[:, None], 0, noise), keys, cap, dead)
        assert all(torch.equal(a, b) for a, b in zip(got, theirs))
        want = ref.replay_records(jref.tables(net), n_x0, n_rates, n_anchors, n_noise, n_keys, TIMES, PATH_TIMES, cap)
        ref.score_records(want, got[0].numpy(), got[1].numpy(), got[2].numpy(), n_anchors, TIMES, PATH_TIMES, f"bd records, torch route, cap {cap}")
        assert bool((got[0][1] == -1).all()) and int(got[1][1].sum()) == 0
