#!/usr/bin/env python3
"""Measures the jump-process kernel (csrc/vsde_jump.hip through ``jump_process``) at B trajectories of two networks: SIR from
(95, 5) with theta (0.004, 0.15) read at t = 5, 10, 15, 20, and the negative-autoregulation model of the README (Hill repression,
n = 2, a fixed mRNA decay) from (2, 10) at the same times.  Next to it, in the same process and on the same device from the same
key: the torch route (``core.jump_process._jump_process_torch``, fp32, one Python iteration per event).  Prints one JSON line.

Kernel time: device events around ``--reps`` launches (``_hip.jump_process`` on prepared tensors) after ``--warmup``, twice (the
pair shows the spread); ``call_ms`` is the public ``jump_process`` with its argument checks and allocations.  The torch route is
hundreds of small launches per event: ``--torch-reps`` calls.  Events per second: all events of the B paths over the kernel time.
Lane efficiency: mean events per path over the mean of the per-wave maximum (a wave of 64 paths runs until its longest path
ends; 1.0 would be no idle lanes).  The feature has no earlier version: the baseline is the torch route.

    python tools/jump_process_bench.py [--b 65536] [--reps 20] [--torch-reps 1]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from viforsdes_amd import Hill, ReactionNetworkSDE, _hip, jump_process  # noqa: E402
from viforsdes_amd.core import jump_process as jp  # noqa: E402

DEV = torch.device("cuda:0")
KEY = (12345, 678)
TIMES = [5.0, 10.0, 15.0, 20.0]
MAX_EVENTS = 4096


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


def case(net, x0, theta, B, a):
    theta = torch.tensor(theta, dtype=torch.float32, device=DEV)
    call = lambda: jump_process(net, x0, theta, TIMES, n_paths=B, key=KEY, max_events=MAX_EVENTS)
    res = call()
    times = torch.tensor(TIMES, dtype=torch.float64, device=DEV)
    xs = torch.tensor(x0, dtype=torch.int64, device=DEV).expand(B, -1)
    rates = (theta if net.plain else net.kernel_parameters(theta)).expand(B, -1)
    key = torch.tensor(KEY, dtype=torch.int64, device=DEV)
    x32, r32, k32, network = xs.to(torch.int32).contiguous(), rates.contiguous(), key.to(torch.int32), net.kernel_descriptor()
    run = lambda: _hip.jump_process(x32, r32, times, k32, MAX_EVENTS, 0, network=network)       # the launch alone
    k1, k2 = timed(run, a.warmup, a.reps), timed(run, 0, a.reps)
    c1 = timed(call, a.warmup, a.reps)
    assert torch.equal(run()[0], res.states)
    torch_run = lambda: jp._jump_process_torch(net, xs, rates, times, key, MAX_EVENTS, 0)
    tt = timed(torch_run, 1, a.torch_reps)
    want = torch_run()
    n = res.n_events.double()
    waves = n[:B // 64 * 64].reshape(-1, 64)
    km = min(k1, k2)
    return {"B": B, "x0": list(x0), "theta": [round(float(v), 6) for v in theta.tolist()], "times": TIMES,
            "kernel_ms": round(km, 4), "kernel_ms_runs": [round(k1, 4), round(k2, 4)], "call_ms": round(c1, 4), "torch_route_ms": round(tt, 1),
            "torch_over_kernel": round(tt / km, 1), "events_per_path_mean": round(float(n.mean()), 2),
            "events_per_path_max": int(n.max()), "events_per_s": round(float(n.sum()) / (km * 1e-3), 0),
            "lane_efficiency": round(float(n.mean() / waves.max(dim=1).values.mean()), 3),
            "complete_fraction": float(res.complete.double().mean()),
            "paths_equal_to_torch_route": round(float((res.states == want[0]).all(-1).all(-1).double().mean()), 5),
            "mean_at_last_time": [round(float(v), 3) for v in res.states[:, -1].double().mean(0).tolist()],
            "torch_route_mean_at_last_time": [round(float(v), 3) for v in want[0][:, -1].double().mean(0).tolist()]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--b", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--torch-reps", type=int, default=1)
    a = ap.parse_args()
    sir = ReactionNetworkSDE(reactants=[[1, 1], [0, 1]], products=[[0, 2], [0, 0]], species=["S", "I"])
    autoreg = ReactionNetworkSDE(reactants=[[0, 0], [1, 0], [1, 0], [0, 1]], products=[[1, 0], [1, 1], [0, 0], [0, 0]],
                                 species=["M", "P"], reactions=["transcription", "translation", "mRNA decay", "protein decay"],
                                 rate_laws={"transcription": Hill("P", K="K", n=2, repression=True)},
                                 rate_constants=["k_tx", "k_tl", 0.1, "d_P"])
    rec = {"tool": "jump_process_bench", "device": torch.cuda.get_device_name(DEV), "max_events": MAX_EVENTS,
           "sir": case(sir, (95, 5), (0.004, 0.15), a.b, a),
           "autoregulation": case(autoreg, (2, 10), (5.0, 2.0, 0.3, 8.0), a.b, a)}
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
