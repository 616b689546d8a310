"""Measure the tau-leap particle filter against the jump-process particle filter on SIR (profiles/tau_leap.txt, DESIGN section
3.34): time per launch at a population of 10^5 from 3 cases (M = 256 filters of N = 512 particles, 200 steps, 5 observations) and at
a population of 100, ``stopped`` of the jump filter at its default ``max_events`` and the ``max_events`` at which it reaches 0,
and the two-sample Kolmogorov distance between ``tau_leap_process`` and ``jump_process`` at the observation times where both are
usable.  ``python tools/tau_leap_bench.py [--reps 5] [--skip-jump]``; VSDE_HIP_LIB selects another build of the library."""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from viforsdes_amd import (Observations, PoissonObservationLikelihood, ReactionNetworkSDE, jump_particle_filter, jump_process,   # noqa: E402
                           tau_leap_particle_filter, tau_leap_process)
from viforsdes_amd.core.jump_process import ks_two_sample   # noqa: E402

SIR = dict(reactants=[[1, 1], [0, 1]], products=[[0, 2], [0, 0]])
DEV = torch.device("cuda:0")


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(reps):
        start.record()
        out = fn()
        stop.record()
        torch.cuda.synchronize()
        times.append(start.elapsed_time(stop))
    times.sort()
    return out, times[len(times) // 2], times[0], times[-1]


def problem(population, cases, M, steps, n_obs, tau):
    """SIR with R0 = 3 and a recovery time of 4: (net, x0, theta [M, 2], observations of the infectives at n_obs instants)."""
    net = ReactionNetworkSDE(**SIR)
    theta = torch.tensor([0.75 / population, 0.25], device=DEV).expand(M, 2).contiguous()
    x0 = torch.tensor([population - cases, cases])
    times = torch.arange(1, n_obs + 1, dtype=torch.float64) * (steps // n_obs) * tau
    data = tau_leap_process(net, x0, theta[:1], times, tau, key=(1, 2)).states[0].float()
    H = torch.tensor([[0.0, 1.0]])
    like = PoissonObservationLikelihood(scale=0.1, obs_matrix=H)
    values = torch.poisson(0.1 * data[:, 1:].cpu().clamp(min=1.0), generator=torch.Generator().manual_seed(0))
    return net, x0, theta, Observations(times=times, values=values).to(DEV), like


def run(population, cases, args, tau, label):
    M, N, steps, n_obs = args.filters, args.particles, 200, 5
    net, x0, theta, obs, like = problem(population, cases, M, steps, n_obs, tau)
    key = torch.tensor([7, 8], dtype=torch.int32, device=DEV)
    print(f"--- {label}: SIR, population {population} from {cases} cases, M = {M}, N = {N}, {steps} steps of {tau}, {n_obs} observations "
          f"(infectives, Poisson at 0.1): y = {obs.values[:, 0].tolist()}")
    res, med, lo, hi = timed(lambda: tau_leap_particle_filter(net, obs, like, theta, tau, n_particles=N, initial_state=x0, key=key), args.reps)
    print(f"tau_leap_particle_filter: {med:.3f} ms per launch (min {lo:.3f}, max {hi:.3f}, {args.reps} launches); "
          f"{M * N * steps * 2 / med / 1e6:.2f} G draws/s; stopped {int(res.stopped.sum())}, capped {int(res.capped.sum())}, "
          f"log p^ {float(res.log_likelihood.mean()):.2f} +- {float(res.log_likelihood.std()):.2f}, smallest ESS "
          f"{float(res.effective_sample_size.min()):.1f}")
    if args.skip_jump:
        return
    for max_events in (2 ** 16, 2 ** 18, 2 ** 20, 2 ** 22):
        t0 = time.time()
        res, med, lo, hi = timed(lambda: jump_particle_filter(net, obs, like, theta, n_particles=N, initial_state=x0, key=key,
                                                              max_events=max_events), 1 if max_events > 2 ** 16 else args.reps)
        stopped = int(res.stopped.sum())
        print(f"jump_particle_filter max_events = 2^{max_events.bit_length() - 1}{' (default)' if max_events == 2 ** 16 else ''}: {med:.3f} ms per launch; "
              f"stopped {stopped} of {M * N * n_obs}; mean events per particle and segment {float(res.mean_events.mean()):.0f}; log p^ "
              f"{float(res.log_likelihood.mean()):.2f} +- {float(res.log_likelihood.std()):.2f}  [{time.time() - t0:.1f} s wall]")
        if stopped == 0:
            break
    if population <= 1000:
        B = 8192
        th = theta[:1].expand(B, 2)
        a = tau_leap_process(net, x0, th, obs.times, tau, key=(3, 4))
        b = jump_process(net, x0, th, obs.times, key=(5, 6))
        ok = a.complete & b.complete
        ks = ks_two_sample(a.states[ok].double(), b.states[ok].double())
        print(f"ks_two_sample(tau_leap_process, jump_process) at the observation times, {int(ok.sum())} paths each, tau = {tau}: "
              f"S {[round(float(v), 4) for v in ks[:, 0]]}, I {[round(float(v), 4) for v in ks[:, 1]]} "
              f"(1.36 sqrt(2 / n) = {1.36 * (2 / int(ok.sum())) ** 0.5:.4f}); capped {int(a.capped.sum())}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--filters", type=int, default=256)
    ap.add_argument("--particles", type=int, default=512)
    ap.add_argument("--skip-jump", action="store_true")
    args = ap.parse_args()
    from viforsdes_amd import _hip
    print(f"library {_hip.library_path()}; {torch.cuda.get_device_name(0)}")
    run(100000, 3, args, 0.25, "large")
    run(100, 3, args, 0.25, "small")


if __name__ == "__main__":
    main()
