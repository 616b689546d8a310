#!/usr/bin/env python3
"""Measures an iteration of particle MCMC (``particle_mcmc``) at the Lotka-Volterra example (400 Euler steps, 5 observations, its
classical parameters jittered, observation variance 3600 so that the bootstrap filter is not starved): C chains x N particles, R = 1.
Three figures, in ms per iteration, in the same process:

(a) the filter launch alone on the same [C, P] batch (``_hip.particle_filter``): what an iteration cannot go below;
(b) the kernel route: the step kernel (csrc/vsde_mcmc.hip) and the filter launch;
(c) ``particle_mcmc.HIP_MCMC = False``: the torch step around the same kernel filter, on the same device;
(d) the kernel route with ``return_paths=True`` (the filter stores particles and ancestors, the step kernel draws the records of
    the chains it accepts), and the one replay launch after the loop over its ``(reps + 1) C`` records, by events of its own.

Time: device events around ``--reps`` iterations after ``--warmup`` warm-up iterations of the same call (the events are recorded
from ``particle_mcmc._ITERATION_HOOK``), twice (the pair shows the spread).  Prints one JSON line.

    python tools/particle_mcmc_bench.py [--c 256] [--n 512] [--reps 200] [--warmup 50]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from viforsdes_amd import GaussianObservationLikelihood, Observations, Prior, PriorType, _hip, particle_mcmc  # noqa: E402
from viforsdes_amd.examples.sdes import LotkaVolterra  # noqa: E402
from viforsdes_amd.inference import particle_mcmc as mc  # noqa: E402

DEV = torch.device("cuda:0")


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--c", type=int, default=256)
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    a = ap.parse_args()
    C, N, dt, pos = a.c, a.n, 0.1, (0, 1)
    g = torch.Generator().manual_seed(0)
    sde = LotkaVolterra()
    obs = Observations(times=torch.tensor([0.0, 10.0, 20.0, 30.0, 40.0]),
                       values=torch.tensor([[71.0, 79.0], [50.0, 390.0], [115.0, 63.0], [60.0, 250.0], [140.0, 95.0]])).to(DEV)
    like = GaussianObservationLikelihood(variance=3600.0)
    prior = Prior(type=PriorType.LOG_NORMAL, mean=0.0, std=1.5, dim=3)
    theta = (torch.tensor([0.5, 0.0025, 0.3]) * (1.0 + 0.03 * torch.rand(C, 3, generator=g))).to(DEV)
    x0 = obs.values[0].expand(C, 2).contiguous()
    rows = torch.round(obs.times / dt).to(torch.int32)
    key = torch.tensor([12345, 678], dtype=torch.int32, device=DEV)
    run_filter = lambda: _hip.particle_filter("lotka_volterra", x0, theta, rows, obs.values, None, like.variance, key, dt, N, pos)
    f1, f2 = timed(run_filter, 3, a.reps), timed(run_filter, 0, a.reps)

    replay_ms = []
    real_replay = _hip.anchored_replay

    def timed_replay(*args, **kw):
        r0, r1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        r0.record()
        out = real_replay(*args, **kw)
        r1.record()
        torch.cuda.synchronize()
        replay_ms.append(r0.elapsed_time(r1))
        return out

    _hip.anchored_replay = timed_replay

    def chain_ms(hip, paths=False):
        mc.HIP_MCMC = hip
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

        def hook(i):
            if i == a.warmup:
                e0.record()
            elif i == a.warmup + a.reps:
                e1.record()

        mc._ITERATION_HOOK = hook
        try:
            res = particle_mcmc(sde, obs, like, prior, dt, theta, a.warmup + a.reps + 1, warmup=a.warmup, n_particles=N,
                                theta_positive_dims=(0, 1, 2), positive_dims=pos, key=key, return_paths=paths)
        finally:
            mc._ITERATION_HOOK, mc.HIP_MCMC = None, True
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.reps, res

    k1, res = chain_ms(True)
    k2, _ = chain_ms(True)
    t1, res_t = chain_ms(False)
    t2, _ = chain_ms(False)
    p1, res_p = chain_ms(True, paths=True)
    p2, _ = chain_ms(True, paths=True)
    k3, _ = chain_ms(True)                                # once more without paths, after them: drift of the box shows here
    fa, kb, tc, pd = min(f1, f2), min(k1, k2, k3), min(t1, t2), min(p1, p2)
    rec = {"tool": "particle_mcmc_bench", "device": torch.cuda.get_device_name(DEV), "C": C, "N": N, "R": 1, "steps": int(rows[-1]),
           "observations": int(rows.shape[0]), "reps": a.reps, "warmup": a.warmup,
           "filter_alone_ms": round(fa, 4), "filter_alone_ms_runs": [round(f1, 4), round(f2, 4)],
           "kernel_route_ms_per_iteration": round(kb, 4), "kernel_route_ms_runs": [round(k1, 4), round(k2, 4), round(k3, 4)],
           "paths_ms_per_iteration": round(pd, 4), "paths_ms_runs": [round(p1, 4), round(p2, 4)], "paths_over_kernel_route": round(pd / kb, 3),
           "replay_ms": round(min(replay_ms), 4), "replay_ms_runs": [round(v, 4) for v in replay_ms], "replay_records": (a.reps + 1) * C,
           "paths_equal_theta_chain": bool(torch.equal(res.samples, res_p.samples)),
           "torch_step_ms_per_iteration": round(tc, 4), "torch_step_ms_runs": [round(t1, 4), round(t2, 4)],
           "step_overhead_over_filter": round((kb - fa) / fa, 3), "torch_over_kernel_route": round(tc / kb, 2),
           "acceptance_rate": round(float(res.acceptance_rate.mean()), 3), "acceptance_rate_torch_step": round(float(res_t.acceptance_rate.mean()), 3),
           "step_size": round(res.step_size, 4), "n_filters_dead": res.n_filters_dead}
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
