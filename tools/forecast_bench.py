#!/usr/bin/env python3
"""Measures the forecast kernel (csrc/vsde_sde.hip: vsde_forecast) against the route it replaces, and VariationalPosterior.predict.
Prints one JSON line.

  (a) vsde_forecast: Philox noise made in the kernel, only the K requested states written;
  (b) torch.randn [n, T, S] noise -> the simulator kernel vsde_euler_maruyama_fwd -> [n, T+1, S] trajectory -> gather of K rows.

Kernel time: device events around `--reps` launches (after `--warmup`), per call.  Peak memory: torch's peak allocation during
one call, above what was allocated before it (the inputs).  predict(): host wall clock around a synchronised call at the Lotka-
Volterra example posterior (example model sizes, untrained weights), n = 16 384, 10 times up to 100 steps after the horizon,
with the fp32 encoder and with ``mixed_precision=True`` (bf16 encoder).

    python tools/forecast_bench.py [--n 65536] [--steps 1000] [--reps 10]"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from viforsdes_amd import _hip  # noqa: E402

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


def peak_mb(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated(DEV)
    torch.cuda.reset_peak_memory_stats(DEV)
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(DEV) - base
    del out
    return peak / 2 ** 20


def compare(kind, x, th, T, steps_list, dt, pos, warmup, reps):
    steps = torch.tensor(steps_list, dtype=torch.int32, device=DEV)
    rows = steps.long()
    n, S = x.shape
    key = torch.tensor([12345, 678], dtype=torch.int32, device=DEV)

    def a():
        return _hip.forecast(kind, x, th, T, steps, key, dt, pos)

    def b():
        noise = torch.randn(n, T, S, device=DEV)
        return _hip.euler_maruyama_fwd(kind, x, th, noise, dt, pos)[:, rows]

    ta, tb = timed(a, warmup, reps), timed(b, warmup, reps)
    ta2, tb2 = timed(a, 0, reps), timed(b, 0, reps)          # second alternation: the spread of the pair
    out_a = a()
    return {"forecast_ms": round(min(ta, ta2), 4), "randn_em_gather_ms": round(min(tb, tb2), 4),
            "forecast_ms_runs": [round(ta, 4), round(ta2, 4)], "randn_em_gather_ms_runs": [round(tb, 4), round(tb2, 4)],
            "forecast_peak_mb": round(peak_mb(a), 2), "randn_em_gather_peak_mb": round(peak_mb(b), 2),
            "forecast_finite": bool(torch.isfinite(out_a).all())}


def predict_wall(n, reps, mixed_precision):
    from bench import build_trainer
    from viforsdes_amd.examples.sdes import lv_problem
    from viforsdes_amd.inference.state_space import StateSpace
    from viforsdes_amd.posterior.variational_posterior import VariationalPosterior
    problem = lv_problem()
    sde, obs, like, prior, horizon, dt, state_pos, _ = problem
    tr = build_trainer(problem, 16, DEV, False, seed=0)
    vp = VariationalPosterior(model=tr.ctx.model, exponential_moving_average=tr.ctx.ema, prior=prior, observations=obs,
                              time_horizon=horizon, time_step=dt, state_space=StateSpace(sde.state_dim, state_pos),
                              evidence_lower_bound_history=[], device=DEV)
    times = horizon + dt * torch.arange(10, 101, 10, dtype=torch.float64)
    vp.predict(sde, times, n_samples=n, observation_likelihood=like, mixed_precision=mixed_precision)   # warm-up: capture, caches
    walls = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pred = vp.predict(sde, times, n_samples=n, observation_likelihood=like, mixed_precision=mixed_precision)
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t0) * 1e3)
    return {"n": n, "times": times.numel(), "steps_ahead_max": 100, "wall_ms": round(min(walls), 2),
            "wall_ms_runs": [round(w, 2) for w in walls], "states_finite_fraction": float(torch.isfinite(pred.states).float().mean())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--predict-n", type=int, default=16384)
    a = ap.parse_args()
    n, T = a.n, a.steps
    steps = [T * (k + 1) // 10 for k in range(10)]
    g = torch.Generator().manual_seed(0)
    lv_th = (torch.tensor([0.5, 0.0025, 0.3]) * (1.0 + 0.1 * torch.rand(n, 3, generator=g))).to(DEV)
    lv_x = torch.tensor([[71.0, 79.0]]).repeat(n, 1).to(DEV)
    ou_th = torch.stack([0.5 + torch.rand(n, generator=g), torch.randn(n, generator=g), 0.3 + torch.rand(n, generator=g)], 1).to(DEV)
    ou_x = torch.randn(n, 1, generator=g).to(DEV)
    rec = {"tool": "forecast_bench", "device": torch.cuda.get_device_name(DEV), "n": n, "T": T, "K": len(steps),
           "lv": compare("lotka_volterra", lv_x, lv_th, T, steps, 0.1, [0, 1], a.warmup, a.reps),
           "ou": compare("ornstein_uhlenbeck", ou_x, ou_th, T, steps, 0.05, [], a.warmup, a.reps),
           "predict_lv": predict_wall(a.predict_n, 3, False), "predict_lv_bf16_encoder": predict_wall(a.predict_n, 3, True)}
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
