#!/usr/bin/env python3
"""Measures the jump-process particle-filter kernel (csrc/vsde_jump_filter.hip through ``jump_particle_filter``) at M filters of N
particles and K = 5 observations (t = 0, 5, 10, 15, 20) of two networks: SIR from (95, 5) with theta (0.004, 0.15), and the
negative-autoregulation model of the README (Hill repression, n = 2, a fixed mRNA decay) from (2, 10).  The observations are the
states of one exact trajectory (``jump_process``, a fixed key) under a Poisson likelihood.  Next to it, in the same process and on
the same device: the torch route of the same call (``HIP_JUMP_FILTER = False``: one Python iteration per event), and
``particle_filter``, the filter on the Euler-Maruyama SDE (``--dt``), at the same M, N, K and the same observations.  Prints one
JSON line.

Time per call: one pair of device events around each of ``--reps`` calls after ``--warmup``, twice (the pair of runs shows the
spread); the figure is the median over the calls of the faster run.  ``mean_events``: events per particle and segment.
Lane efficiency: per segment and wave of 64 particle slots, mean events over the wave's maximum (the lanes of a wave wait for their
slowest particle at every observation; 1.0 would be no idle lanes), averaged over waves and segments with events.  The feature has
no earlier version: the baselines are the torch route and the SDE filter.

    python tools/jump_filter_bench.py [--m 256] [--n 512] [--reps 20] [--torch-reps 1] [--dt 0.05]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from viforsdes_amd import (Hill, Observations, PoissonObservationLikelihood, ReactionNetworkSDE, jump_particle_filter,  # noqa: E402
                           jump_process, particle_filter)
from viforsdes_amd.inference import jump_filter as jf  # noqa: E402

DEV = torch.device("cuda:0")
KEY = (12345, 678)
TIMES = [0.0, 5.0, 10.0, 15.0, 20.0]
MAX_EVENTS = 4096


def timed(fn, warmup, reps):
    """(mean, median) milliseconds per call over ``reps`` calls, one pair of device events per call."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for e0, e1 in pairs:
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    ms = [e0.elapsed_time(e1) for e0, e1 in pairs]
    return sum(ms) / len(ms), statistics.median(ms)


def case(net, x0, theta, a):
    M, N = a.m, a.n
    theta1 = torch.tensor(theta, dtype=torch.float32, device=DEV)
    truth = jump_process(net, x0, theta1, TIMES, n_paths=1, key=KEY, max_events=MAX_EVENTS).states[0].float()
    obs = Observations(times=torch.tensor(TIMES, dtype=torch.float64, device=DEV), values=truth)
    like = PoissonObservationLikelihood()
    th = theta1.expand(M, -1).contiguous()
    start = torch.tensor(x0, device=DEV)
    key = torch.tensor(KEY, dtype=torch.int32, device=DEV)
    call = lambda **kw: jump_particle_filter(net, obs, like, th, n_particles=N, initial_state=start, key=key, max_events=MAX_EVENTS, **kw)
    res = call(return_particles=True)
    k1, k2 = timed(call, a.warmup, a.reps), timed(call, 0, a.reps)
    jf.HIP_JUMP_FILTER = False
    try:
        tt = timed(call, 1, a.torch_reps)
        want = call()
    finally:
        jf.HIP_JUMP_FILTER = True
    sde = lambda: particle_filter(net, obs, like, th, a.dt, n_particles=N, initial_state=start.float(), positive_dims=tuple(range(len(x0))),
                                  key=key)
    s1 = timed(sde, a.warmup, a.reps)
    sde_res = sde()
    ev = res.events.double().reshape(M, len(TIMES), N // 64, 64)
    busy = ev.amax(dim=-1) > 0
    eff = (ev.mean(dim=-1)[busy] / ev.amax(dim=-1)[busy]).mean()
    km = min(k1, k2, key=lambda p: p[1])
    ll, ll_t, ll_s = res.log_likelihood.double(), want.log_likelihood.double(), sde_res.log_likelihood.double()
    return {"M": M, "N": N, "K": len(TIMES), "x0": list(x0), "theta": [round(float(v), 6) for v in theta], "times": TIMES,
            "observations": truth.long().tolist(), "kernel_ms_median": round(km[1], 4), "kernel_ms_mean": round(km[0], 4),
            "kernel_ms_median_runs": [round(k1[1], 4), round(k2[1], 4)], "torch_route_ms": round(tt[1], 1),
            "torch_over_kernel": round(tt[1] / km[1], 1), "sde_filter_ms_median": round(s1[1], 4), "sde_time_step": a.dt,
            "sde_steps": int(round(TIMES[-1] / a.dt)), "kernel_over_sde_filter": round(km[1] / s1[1], 2),
            "mean_events": [round(float(v), 2) for v in res.mean_events.double().mean(dim=0).tolist()],
            "events_per_particle_total": round(float(res.events.double().sum(dim=1).mean()), 2),
            "events_per_s": round(float(res.events.double().sum()) / (km[1] * 1e-3), 0), "lane_efficiency": round(float(eff), 3),
            "stopped": int(res.stopped.sum()), "log_likelihood_mean": round(float(ll.mean()), 4), "log_likelihood_std": round(float(ll.std()), 4),
            "torch_route_log_likelihood_mean": round(float(ll_t.mean()), 4), "sde_filter_log_likelihood_mean": round(float(ll_s.mean()), 4),
            "min_ess": round(float(res.effective_sample_size.min()), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=256)
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--torch-reps", type=int, default=1)
    ap.add_argument("--dt", type=float, default=0.05)
    a = ap.parse_args()
    sir = ReactionNetworkSDE(reactants=[[1, 1], [0, 1]], products=[[0, 2], [0, 0]], species=["S", "I"])
    autoreg = ReactionNetworkSDE(reactants=[[0, 0], [1, 0], [1, 0], [0, 1]], products=[[1, 0], [1, 1], [0, 0], [0, 0]],
                                 species=["M", "P"], reactions=["transcription", "translation", "mRNA decay", "protein decay"],
                                 rate_laws={"transcription": Hill("P", K="K", n=2, repression=True)},
                                 rate_constants=["k_tx", "k_tl", 0.1, "d_P"])
    rec = {"tool": "jump_filter_bench", "device": torch.cuda.get_device_name(DEV), "max_events": MAX_EVENTS,
           "sir": case(sir, (95, 5), (0.004, 0.15), a),
           "autoregulation": case(autoreg, (2, 10), (5.0, 2.0, 0.3, 8.0), a)}
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
