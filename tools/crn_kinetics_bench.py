#!/usr/bin/env python3
"""Measures the rate-law kernels (the KIN instantiations of kind 4: ReactionNetworkSDE with rate_laws / rate_constants) on the
negative-autoregulation network of the README (M, P; transcription repressed by P through a Hill law, n = 2; a fixed mRNA decay
rate), against the Python callables of the same model.  Prints one JSON line.

  (a) coefficients forward + backward at B = 512, T = 400: the kinetic entry points (with the theta map and its backward), the
      mass-action network of the same shape (Hill law dropped) on the mass-action entry points, and the Python drift /
      diffusion + autograd;
  (b) pre-training, 100 iterations x 4096 paths x 400 steps (trainer.pretrain_sde_parameters, graph-replayed): the network on
      the simulator kernels against ``make_sde`` with its own drift / diffusion (the torch time loop);
  (c) forecast, n = 65 536, T = 1000, K = 10: the network, the mass-action network of the same shape, and the torch route.

Kernel times: device events around `--reps` calls after warm-up, per call, two alternations (spread in the *_runs lists).

    python tools/crn_kinetics_bench.py [--reps 20] [--pretrain-iters 100] [--parts abc]"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from viforsdes_amd import GaussianObservationLikelihood, Hill, Observations, Prior, PriorType, ReactionNetworkSDE, _hip  # noqa: E402

DEV = torch.device("cuda:0")
AUTOREG = dict(reactants=[[0, 0], [1, 0], [1, 0], [0, 1]], products=[[1, 0], [1, 1], [0, 0], [0, 0]],
               species=["M", "P"], reactions=["transcription", "translation", "mRNA decay", "protein decay"])
KINETICS = dict(rate_laws={"transcription": Hill("P", K="K", n=2, repression=True)},
                rate_constants=["k_tx", "k_tl", 0.1, "d_P"])
THETA = [20.0, 0.5, 0.1, 15.0]           # k_tx, k_tl, d_P, K
THETA_MA = [2.0, 0.5, 0.1, 0.1]          # the mass-action network: one constant per reaction
X_LEVEL = [12.0, 60.0]


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


def _theta(base, n, g):
    return (torch.tensor(base) * (0.8 + 0.4 * torch.rand(n, len(base), generator=g))).to(DEV)


def coefficients(reps):
    from viforsdes_amd.inference import evidence_lower_bound as elbo_mod
    B, T = 512, 400
    g = torch.Generator().manual_seed(0)
    x = (torch.tensor(X_LEVEL) * (0.5 + torch.rand(B, T + 1, 2, generator=g))).to(DEV)
    gf, gG = torch.randn(B, T, 2, generator=g).to(DEV), torch.randn(B, T, 2, 2, generator=g).to(DEV)
    kin, ma = ReactionNetworkSDE(**AUTOREG, **KINETICS), ReactionNetworkSDE(**AUTOREG)
    th = _theta(THETA, B, g).requires_grad_(True)
    th_ma = _theta(THETA_MA, B, g).requires_grad_(True)

    def route(sde, theta):
        def run():
            f, G = elbo_mod.sde_coefficients(sde, x, theta)
            return torch.autograd.grad((f * gf).sum() + (G * gG).sum(), [theta])
        return run

    def python_callables():
        elbo_mod.HIP_COEFFICIENTS = False
        try:
            return route(kin, th)()
        finally:
            elbo_mod.HIP_COEFFICIENTS = True

    out = alternate({"autoreg_kernels": route(kin, th), "mass_action_kernels": route(ma, th_ma),
                     "python_callables": python_callables}, 3, reps)
    out["kernels_over_mass_action"] = round(out["autoreg_kernels"]["ms"] / out["mass_action_kernels"]["ms"], 3)
    out["python_over_kernels"] = round(out["python_callables"]["ms"] / out["autoreg_kernels"]["ms"], 1)
    return out


def pretrain(iters):
    from bench import build_trainer
    from viforsdes_amd import PretrainConfig, make_sde
    from viforsdes_amd.core.euler_maruyama import euler_maruyama
    kin = ReactionNetworkSDE(**AUTOREG, **KINETICS)
    horizon, dt = 40.0, 0.1
    g = torch.Generator().manual_seed(3)
    truth = euler_maruyama(kin, torch.tensor([[5.0, 20.0]], dtype=torch.float64), torch.tensor([THETA], dtype=torch.float64),
                           horizon, dt, [0, 1], noise=torch.randn(1, round(horizon / dt), 2, generator=g, dtype=torch.float64))[0]
    times = torch.linspace(0.0, horizon, 11)
    obs = Observations(times=times, values=(truth[(times / dt).round().long()] + torch.randn(11, 2, generator=g,
                                                                                           dtype=torch.float64)).float())
    rest = (obs, GaussianObservationLikelihood(variance=1.0), Prior(type=PriorType.LOG_NORMAL, mean=0.0, std=2.0, dim=4),
            horizon, dt, [0, 1], [0, 1, 2, 3])
    cases = {"autoreg_kernels": kin, "make_sde_torch_loop": make_sde(kin.drift, kin.diffusion, 2, 4)}
    out = {}
    for name, sde in cases.items():
        tr = build_trainer((sde,) + rest, 16, DEV, True, seed=1, enc_hidden=64, enc_depth=1)
        tr.pretrain_sde_parameters(PretrainConfig(n_iterations=3))          # warm-up: capture, caches
        torch.manual_seed(0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        best = tr.pretrain_sde_parameters(PretrainConfig(n_iterations=iters))
        torch.cuda.synchronize()
        out[name] = {"s": round(time.perf_counter() - t0, 3), "best_mean": [round(v, 4) for v in best.tolist()]}
    out["iterations"], out["paths"], out["steps"] = iters, 4096, round(horizon / dt)
    out["torch_over_kernels"] = round(out["make_sde_torch_loop"]["s"] / out["autoreg_kernels"]["s"], 1)
    return out


def forecast(reps):
    from viforsdes_amd import make_sde
    from viforsdes_amd.core.euler_maruyama import euler_maruyama
    n, T, dt = 65536, 1000, 0.1
    steps_list = [T * (k + 1) // 10 for k in range(10)]
    steps = torch.tensor(steps_list, dtype=torch.int32, device=DEV)
    g = torch.Generator().manual_seed(0)
    kin, ma = ReactionNetworkSDE(**AUTOREG, **KINETICS), ReactionNetworkSDE(**AUTOREG)
    th, th_ma = _theta(THETA, n, g), _theta(THETA_MA, n, g)
    x = torch.tensor([X_LEVEL]).repeat(n, 1).to(DEV)
    key = torch.tensor([12345, 678], dtype=torch.int32, device=DEV)
    route, net = kin.kernel_descriptor(), ma.kernel_descriptor()
    user = make_sde(kin.drift, kin.diffusion, 2, 4)

    def torch_route():
        with torch.no_grad():
            return euler_maruyama(user, x, th, T * dt, dt, [0, 1])[:, steps.long()]

    out = alternate({
        "autoreg_kernel": lambda: _hip.forecast("reaction_network", x, kin.kernel_parameters(th), T, steps, key, dt, (0, 1),
                                                network=route),
        "mass_action_kernel": lambda: _hip.forecast("reaction_network", x, th_ma, T, steps, key, dt, (0, 1), network=net)},
        2, reps)
    out["torch_route"] = {"ms": round(timed(torch_route, 1, 1), 2)}
    out["kernel_over_mass_action"] = round(out["autoreg_kernel"]["ms"] / out["mass_action_kernel"]["ms"], 3)
    out.update(n=n, T=T, K=len(steps_list))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--pretrain-iters", type=int, default=100)
    ap.add_argument("--parts", default="abc", help="which of (a) .. (c) to run")
    a = ap.parse_args()
    rec = {"tool": "crn_kinetics_bench", "device": torch.cuda.get_device_name(DEV)}
    if "a" in a.parts:
        rec["a_coefficients_B512_T400"] = coefficients(a.reps)
    if "b" in a.parts:
        rec["b_pretrain"] = pretrain(a.pretrain_iters)
    if "c" in a.parts:
        rec["c_forecast"] = forecast(a.reps)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
