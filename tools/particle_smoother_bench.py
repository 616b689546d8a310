#!/usr/bin/env python3
"""Measures the replay kernel of the particle smoother (csrc/vsde_filter.hip: rp_kernel through ``_hip.filter_replay``) at the
Lotka-Volterra example (400 Euler steps, 5 observations, its classical parameters jittered, observation variance 3600 so that the
bootstrap filter is not starved): M filters x N particles, D draws per filter.  Next to it, in the same process: the filter kernel
that stores the particles and ancestors the replay reads (``_hip.particle_filter(..., return_particles=True)``), and the torch-route
replay (``particle_smoother._torch_replay``) on the same device from the same stored particles.  Prints one JSON line.

Time per call: device events around ``--reps`` calls after ``--warmup``, twice (the pair shows the spread); the torch route is
thousands of small launches: ``--torch-reps`` calls.  Bytes of the replay: the M D (T + 1) S floats of the paths it writes, and its
reads (K ancestors and one particle per segment).

    python tools/particle_smoother_bench.py [--m 256] [--n 512] [--draws 1 512] [--reps 200] [--torch-reps 2]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from viforsdes_amd import GaussianObservationLikelihood, Observations, _hip  # noqa: E402
from viforsdes_amd.examples.sdes import LotkaVolterra  # noqa: E402
from viforsdes_amd.inference import particle_smoother as ps  # noqa: E402

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
    ap.add_argument("--m", type=int, default=256)
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--draws", type=int, nargs="+", default=[1, 512])
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--torch-reps", type=int, default=2)
    a = ap.parse_args()
    M, N, dt, pos = a.m, a.n, 0.1, (0, 1)
    g = torch.Generator().manual_seed(0)
    sde = LotkaVolterra()
    obs = Observations(times=torch.tensor([0.0, 10.0, 20.0, 30.0, 40.0]),
                       values=torch.tensor([[71.0, 79.0], [50.0, 390.0], [115.0, 63.0], [60.0, 250.0], [140.0, 95.0]])).to(DEV)
    like = GaussianObservationLikelihood(variance=3600.0)
    theta = (torch.tensor([0.5, 0.0025, 0.3]) * (1.0 + 0.03 * torch.rand(M, 3, generator=g))).to(DEV)
    x0 = obs.values[0].expand(M, 2).contiguous()
    rows = torch.round(obs.times / dt).to(torch.int32)
    T, K, S = int(rows[-1]), rows.shape[0], 2
    key = torch.tensor([12345, 678], dtype=torch.int32, device=DEV)
    run_filter = lambda: _hip.particle_filter("lotka_volterra", x0, theta, rows, obs.values, None, like.variance, key, dt, N, pos,
                                              return_particles=True)
    f1, f2 = timed(run_filter, a.warmup, a.reps), timed(run_filter, 0, a.reps)
    out = run_filter()
    particles, ancestors = out[5], out[6]
    rec = {"tool": "particle_smoother_bench", "device": torch.cuda.get_device_name(DEV), "M": M, "N": N, "steps": T, "observations": K,
           "filter_kernel_ms": round(min(f1, f2), 4), "filter_kernel_ms_runs": [round(f1, 4), round(f2, 4)],
           "finite_fraction": float(torch.isfinite(out[0]).float().mean()), "min_particle_ess": round(float(out[2].min()), 1), "draws": {}}
    lw = like.log_prob(obs.values[-1].expand(M * N, -1), particles[:, -1].reshape(M * N, S)).reshape(M, N)
    w = torch.exp(lw - lw.max(dim=1, keepdim=True).values)
    for D in a.draws:
        last = ps.systematic_draws(w, ps.smoothing_uniforms(M, key), D).to(torch.int32)
        run = lambda: _hip.filter_replay("lotka_volterra", x0, theta, rows, key, dt, particles, ancestors, last, pos, n_steps=T)
        r1, r2 = timed(run, a.warmup, a.reps), timed(run, 0, a.reps)
        paths, lineage = run()
        torch_run = lambda: ps._torch_replay(sde, obs, like, theta, dt, x0, pos, key, False, particles, lineage, rows.tolist())
        tt = timed(torch_run, 1, a.torch_reps)
        want = torch_run()
        rk = min(r1, r2)
        rec["draws"][str(D)] = {
            "replay_kernel_ms": round(rk, 4), "replay_kernel_ms_runs": [round(r1, 4), round(r2, 4)], "torch_replay_ms": round(tt, 2),
            "torch_over_kernel": round(tt / rk, 1), "replay_over_filter": round(rk / min(f1, f2), 3),
            "path_steps_per_s": round(M * D * T / (rk * 1e-3), 0), "bytes_written": 4 * M * D * (T + 1) * S,
            "write_gb_per_s": round(4 * M * D * (T + 1) * S / (rk * 1e-3) / 1e9, 2),
            "max_rel_diff_torch_vs_kernel": float((paths - want).abs().max() / want.abs().max()),
            "distinct_lineages_at_first_observation_mean": round(float(
                (1 + (lineage[:, :, 0].sort(dim=1).values.diff(dim=1) != 0).sum(dim=1)).float().mean()), 1)}
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
