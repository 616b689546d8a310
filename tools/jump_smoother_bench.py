#!/usr/bin/env python3
"""Measures the jump-segment replay kernel (csrc/vsde_jump_replay.hip) against the filter launch it follows, in the same process:

* the smoother: SIR from (95, 5) with theta (0.004, 0.15), K = 5 observations (t = 0, 5, 10, 15, 20: the states of one exact
  trajectory under a Poisson likelihood, as tools/jump_filter_bench.py), M filters of N particles, D draws per filter read at Q
  output times spread evenly over [0, 20]: ``_hip.jump_particle_filter(..., return_particles=True)`` and then
  ``_hip.jump_filter_replay`` on its store;
* PMMH with paths on the same problem: ``particle_mcmc(..., dynamics="jump", return_paths=True)`` with C chains for ``--iterations``
  iterations; the arguments of its filter launches and of its one replay launch are captured and timed again on their own, next to
  the whole call with and without paths.

Time per call: one pair of device events around each of ``--reps`` calls after ``--warmup``, twice (the pair of runs shows the
spread); the figure is the median over the calls of the faster run.  The whole PMMH calls are host clocks around a call that ends
in a device synchronise.  Prints one JSON line.

    python tools/jump_smoother_bench.py [--m 256] [--n 512] [--draws 64] [--q 64] [--reps 20] [--chains 256] [--iterations 50]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from viforsdes_amd import (Observations, PoissonObservationLikelihood, Prior, PriorType, ReactionNetworkSDE, _hip, jump_process,  # noqa: E402
                           particle_mcmc)
from viforsdes_amd.inference import jump_smoother as js  # noqa: E402
from viforsdes_amd.inference import particle_smoother as ps  # noqa: E402

DEV = torch.device("cuda:0")
KEY = (12345, 678)
TIMES = [0.0, 5.0, 10.0, 15.0, 20.0]
MAX_EVENTS = 4096


def timed(fn, warmup, reps):
    """Median milliseconds per call over ``reps`` calls, one pair of device events per call."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for e0, e1 in pairs:
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    return statistics.median(e0.elapsed_time(e1) for e0, e1 in pairs)


def twice(fn, warmup, reps):
    a, b = timed(fn, warmup, reps), timed(fn, 0, reps)
    return min(a, b), [round(a, 4), round(b, 4)]


def captured(name):
    """Replace ``_hip.<name>`` by a wrapper that keeps the arguments of every call; returns (calls, undo)."""
    calls, real = [], getattr(_hip, name)
    setattr(_hip, name, lambda *a, **k: (calls.append((a, k)), real(*a, **k))[1])
    return calls, lambda: setattr(_hip, name, real)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=256)
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--draws", type=int, default=64)
    ap.add_argument("--q", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--chains", type=int, default=256)
    ap.add_argument("--iterations", type=int, default=50)
    a = ap.parse_args()
    M, N, D, Q = a.m, a.n, a.draws, a.q
    net = ReactionNetworkSDE(reactants=[[1, 1], [0, 1]], products=[[0, 2], [0, 0]], species=["S", "I"])
    theta1 = torch.tensor([0.004, 0.15], device=DEV)
    truth = jump_process(net, (95, 5), theta1, TIMES, n_paths=1, key=KEY, max_events=MAX_EVENTS).states[0].float()
    times = torch.tensor(TIMES, dtype=torch.float64)
    obs = Observations(times=times.to(DEV), values=truth)
    like = PoissonObservationLikelihood()
    key = torch.tensor(KEY, dtype=torch.int32, device=DEV)
    network = net.kernel_descriptor()
    x0 = torch.tensor([[95, 5]], dtype=torch.int32, device=DEV).expand(M, 2).contiguous()
    th = theta1.expand(M, 2).contiguous()
    t_out = torch.linspace(0.0, TIMES[-1], Q, dtype=torch.float64)
    q_begin = js.ownership_ranges(t_out, times)
    term = like.kernel_terms(obs.values)
    run_filter = lambda: _hip.jump_particle_filter(x0, th, obs.times, obs.values, None, term, key, MAX_EVENTS, N, network=network,
                                                   return_particles=True)
    f_ms, f_runs = twice(run_filter, a.warmup, a.reps)
    out = run_filter()
    particles, ancestors, lw, events = out[7], out[8], out[9][:, -1], out[10]
    w = torch.exp(lw - lw.max(dim=1, keepdim=True).values)
    last = ps.systematic_draws(w, ps.smoothing_uniforms(M, key), D).to(torch.int32)
    t_dev = t_out.to(DEV)
    run_replay = lambda: _hip.jump_filter_replay(x0, th, obs.times, t_dev, q_begin, key, MAX_EVENTS, particles, ancestors, last, network=network)
    r_ms, r_runs = twice(run_replay, a.warmup, a.reps)
    paths, lineage, n_events, status = run_replay()
    rec = {"tool": "jump_smoother_bench", "device": torch.cuda.get_device_name(DEV), "max_events": MAX_EVENTS, "times": TIMES,
           "observations": truth.long().tolist(),
           "smoother": {"M": M, "N": N, "D": D, "Q": Q, "filter_launch_ms": round(f_ms, 4), "filter_launch_ms_runs": f_runs,
                        "replay_launch_ms": round(r_ms, 4), "replay_launch_ms_runs": r_runs, "replay_over_filter": round(r_ms / f_ms, 3),
                        "filter_events": int(events.sum()), "replay_events": int(n_events.sum()),
                        "replay_events_per_s": round(float(n_events.sum()) / (r_ms * 1e-3), 0),
                        "filter_events_per_s": round(float(events.sum()) / (f_ms * 1e-3), 0), "bytes_written": 4 * M * D * (Q * 2 + 3 * len(TIMES)),
                        "status_nonzero": int((status != 0).sum()), "paths_negative": int((paths < 0).sum()),
                        "distinct_lineages_at_first_observation_mean": round(float(
                            (1 + (lineage[:, :, 0].sort(dim=1).values.diff(dim=1) != 0).sum(dim=1)).float().mean()), 1)}}
    # PMMH with paths: the loop's own launches, captured and timed again
    C, n_it = a.chains, a.iterations
    g = torch.Generator().manual_seed(0)
    theta0 = (theta1.cpu() * (0.9 + 0.2 * torch.rand(C, 2, generator=g))).to(DEV)
    prior = Prior(type=PriorType.LOG_NORMAL, mean=-3.0, std=2.0, dim=2)
    kw = dict(n_particles=N, theta_positive_dims=(0, 1), initial_state=torch.tensor([95, 5]), key=key, dynamics="jump", max_events=MAX_EVENTS)

    def whole(**extra):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = particle_mcmc(net, obs, like, prior, None, theta0, n_it, **kw, **extra)
        torch.cuda.synchronize()
        return res, (time.perf_counter() - t0) * 1e3

    whole(), whole(return_paths=True, path_times=t_out)                 # warm-up of every shape
    _, plain_ms = whole()
    filters, undo_f = captured("jump_particle_filter")
    replays, undo_r = captured("jump_anchored_replay")
    try:
        res, paths_ms = whole(return_paths=True, path_times=t_out)
    finally:
        undo_f(), undo_r()
    fa, fk = filters[-1]
    pf_ms, pf_runs = twice(lambda: _hip.jump_particle_filter(*fa, **fk), a.warmup, a.reps)
    ra, rk = replays[0]
    pr_ms, pr_runs = twice(lambda: _hip.jump_anchored_replay(*ra, **rk), a.warmup, a.reps)
    rec["pmmh"] = {"C": C, "N": N, "iterations": n_it, "records": int(res.paths.shape[0] * res.paths.shape[1]), "Q": Q,
                   "filter_launches": len(filters), "replay_launches": len(replays), "filter_launch_ms": round(pf_ms, 4),
                   "filter_launch_ms_runs": pf_runs, "replay_launch_ms": round(pr_ms, 4), "replay_launch_ms_runs": pr_runs,
                   "replay_in_filter_launches": round(pr_ms / pf_ms, 2), "whole_call_ms_without_paths": round(plain_ms, 1),
                   "whole_call_ms_with_paths": round(paths_ms, 1), "dead_records": int((res.path_iteration < 0).sum()),
                   "acceptance": round(float(res.acceptance_rate.mean()), 3)}
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
