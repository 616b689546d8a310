#!/usr/bin/env python3
"""Measures the reaction-network kernels (kind 4: ReactionNetworkSDE) against Lotka-Volterra's closed form (kind 2) and the
Python callables, on Lotka-Volterra written as a network (``network-LV``: the same model, theta in the same order).  Prints one
JSON line.

  (a) coefficients forward + backward (vsde_crn_sde_coefficients_fwd/_bwd) at B = 512, T = 400: network-LV, kind 2, and the
      Python drift / diffusion + autograd (the route of any other SDE);
  (b) pre-training, 100 iterations x 4096 paths x 400 steps (trainer.pretrain_sde_parameters, graph-replayed): network-LV on
      the simulator kernels against ``make_sde`` with LotkaVolterra's callables (the torch time loop);
  (c) forecast, n = 65 536, T = 1000, K = 10: network-LV, kind 2, and the torch route (torch.randn noise, euler_maruyama
      through the Python callables, gather);
  (d) ms per ELBO training step at the LV bench shape (B = 512, T = 400, bench.py's model), LotkaVolterra against network-LV,
      alternated in one process.

Kernel times: device events around `--reps` calls after warm-up, per call, two alternations (spread in the *_runs lists).

    python tools/crn_bench.py [--reps 20] [--pretrain-iters 100]"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from viforsdes_amd import ReactionNetworkSDE, _hip  # noqa: E402
from viforsdes_amd.examples.sdes import LotkaVolterra, lv_problem  # noqa: E402

DEV = torch.device("cuda:0")
LV_NET = dict(reactants=[[1, 0], [1, 1], [0, 1]], products=[[2, 0], [0, 2], [0, 0]], species=["prey", "predator"])


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


def alternate(fns, warmup, reps):
    """{name: (best ms, [run ms, run ms])}, the candidates timed in turn twice."""
    runs = {k: [] for k in fns}
    for r in range(2):
        for k, fn in fns.items():
            runs[k].append(round(timed(fn, warmup if r == 0 else 1, reps), 4))
    return {k: {"ms": min(v), "ms_runs": v} for k, v in runs.items()}


def coefficients(reps):
    from viforsdes_amd.inference.evidence_lower_bound import sde_coefficients
    from viforsdes_amd.inference import evidence_lower_bound as elbo_mod
    B, T = 512, 400
    g = torch.Generator().manual_seed(0)
    x = (5.0 + 300.0 * torch.rand(B, T + 1, 2, generator=g)).to(DEV)
    th = (torch.tensor([0.5, 0.0025, 0.3]) * (1.0 + 0.1 * torch.rand(B, 3, generator=g))).to(DEV)
    gf, gG = torch.randn(B, T, 2, generator=g).to(DEV), torch.randn(B, T, 2, 2, generator=g).to(DEV)
    net_sde = ReactionNetworkSDE(**LV_NET)
    net = net_sde.network_descriptor()

    def kernels(kind, network):
        def run():
            f, G = _hip.sde_coefficients_fwd(kind, x, th, network=network)
            return _hip.sde_coefficients_bwd(kind, x, th, gf, gG, network=network)
        return run

    xr, thr = x.clone().requires_grad_(True), th.clone().requires_grad_(True)

    def python_callables():
        elbo_mod.HIP_COEFFICIENTS = False
        try:
            f, G = sde_coefficients(LotkaVolterra(), xr, thr)
            return torch.autograd.grad((f * gf).sum() + (G * gG).sum(), [xr, thr])
        finally:
            elbo_mod.HIP_COEFFICIENTS = True

    out = alternate({"network_lv": kernels("reaction_network", net), "kind2_lv": kernels("lotka_volterra", None),
                     "python_callables_lv": python_callables}, 3, reps)
    out["network_over_kind2"] = round(out["network_lv"]["ms"] / out["kind2_lv"]["ms"], 3)
    return out


def pretrain(iters):
    from bench import build_trainer
    from viforsdes_amd import PretrainConfig, make_sde
    lv = LotkaVolterra()
    cases = {"network_lv_kernels": ReactionNetworkSDE(**LV_NET),
             "make_sde_lv_torch_loop": make_sde(lv.drift, lv.diffusion, 2, 3)}
    out = {}
    for name, sde in cases.items():
        problem = (sde,) + tuple(lv_problem()[1:])
        tr = build_trainer(problem, 16, DEV, True, seed=1, enc_hidden=64, enc_depth=1)
        tr.pretrain_sde_parameters(PretrainConfig(n_iterations=3))          # warm-up: capture, caches
        torch.manual_seed(0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        best = tr.pretrain_sde_parameters(PretrainConfig(n_iterations=iters))
        torch.cuda.synchronize()
        out[name] = {"s": round(time.perf_counter() - t0, 3), "best_mean": [round(v, 4) for v in best.tolist()]}
    out["iterations"], out["paths"], out["steps"] = iters, 4096, 400
    return out


def forecast(reps):
    from viforsdes_amd.core.euler_maruyama import euler_maruyama
    n, T, dt = 65536, 1000, 0.1
    steps_list = [T * (k + 1) // 10 for k in range(10)]
    steps = torch.tensor(steps_list, dtype=torch.int32, device=DEV)
    g = torch.Generator().manual_seed(0)
    th = (torch.tensor([0.5, 0.0025, 0.3]) * (1.0 + 0.1 * torch.rand(n, 3, generator=g))).to(DEV)
    x = torch.tensor([[71.0, 79.0]]).repeat(n, 1).to(DEV)
    key = torch.tensor([12345, 678], dtype=torch.int32, device=DEV)
    net = ReactionNetworkSDE(**LV_NET).network_descriptor()
    lv = LotkaVolterra()
    from viforsdes_amd import make_sde
    user = make_sde(lv.drift, lv.diffusion, 2, 3)

    def torch_route():
        with torch.no_grad():
            return euler_maruyama(user, x, th, T * dt, dt, [0, 1])[:, steps.long()]

    out = alternate({"network_lv": lambda: _hip.forecast("reaction_network", x, th, T, steps, key, dt, (0, 1), network=net),
                     "kind2_lv": lambda: _hip.forecast("lotka_volterra", x, th, T, steps, key, dt, (0, 1))}, 2, reps)
    out["torch_route_lv"] = {"ms": round(timed(torch_route, 1, 1), 2)}
    a = _hip.forecast("reaction_network", x, th, T, steps, key, dt, (0, 1), network=net)
    b = _hip.forecast("lotka_volterra", x, th, T, steps, key, dt, (0, 1))
    out["network_over_kind2"] = round(out["network_lv"]["ms"] / out["kind2_lv"]["ms"], 3)
    out["max_rel_diff_vs_kind2"] = float((a - b).abs().max() / b.abs().max())
    out.update(n=n, T=T, K=len(steps_list))
    return out


def elbo_step(steps):
    from bench import build_trainer
    problems = {"lotka_volterra": lv_problem(), "network_lv": (ReactionNetworkSDE(**LV_NET),) + tuple(lv_problem()[1:])}
    trainers = {k: build_trainer(p, 512, DEV, True, seed=0) for k, p in problems.items()}
    for tr in trainers.values():
        for _ in range(3):
            tr._train_step(tr.ctx.model)
    runs = {k: [] for k in trainers}
    for r in range(4):                                     # alternated: LV, network, LV, network, ...
        for k, tr in trainers.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                tr._train_step(tr.ctx.model)
            torch.cuda.synchronize()
            runs[k].append(round((time.perf_counter() - t0) * 1e3 / steps, 3))
    out = {k: {"ms_per_step": min(v), "ms_runs": v} for k, v in runs.items()}
    out["network_over_lv"] = round(out["network_lv"]["ms_per_step"] / out["lotka_volterra"]["ms_per_step"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--pretrain-iters", type=int, default=100)
    ap.add_argument("--elbo-steps", type=int, default=10)
    ap.add_argument("--parts", default="abcd", help="which of (a) .. (d) to run")
    a = ap.parse_args()
    rec = {"tool": "crn_bench", "device": torch.cuda.get_device_name(DEV)}
    if "a" in a.parts:
        rec["a_coefficients_B512_T400"] = coefficients(a.reps)
    if "b" in a.parts:
        rec["b_pretrain"] = pretrain(a.pretrain_iters)
    if "c" in a.parts:
        rec["c_forecast"] = forecast(a.reps)
    if "d" in a.parts:
        rec["d_elbo_step_lv_bench_shape"] = elbo_step(a.elbo_steps)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
