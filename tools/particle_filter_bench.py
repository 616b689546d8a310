#!/usr/bin/env python3
"""Measures the particle-filter kernel (csrc/vsde_filter.hip: vsde_particle_filter) against the torch route of
``particle_filter`` on the same GPU, at sizes a user would run: M thetas x N particles, the Lotka-Volterra example grid (400 Euler
steps, 5 observations) and the SIR network (200 steps, 5 observations).  Prints one JSON line.

Time per call: device events around ``--reps`` calls after ``--warmup``, twice (the pair shows the spread; 200 calls make a window
of a few tenths of a second); the torch route is tens of thousands of small launches and seconds per call: ``--torch-reps`` of
them.  Bytes: what the kernel route has to move (theta, start states, observations in; log-likelihood, increments, ESS and moments
out: O(M K S)) against the [M N, S]-sized tensors the torch route reads and writes per Euler step.
There is no earlier version of the feature to compare with: the torch route on the same device is the baseline.

``--proposal bridge`` runs the guided filter instead; ``--proposal both`` adds, per case, what the proposal is for: ONE theta (the
Lotka-Volterra example at the classical values 0.5, 0.0025, 0.3 with its own observation variance 1.0; the SIR case at 0.004, 0.15)
repeated over ``--m`` filters with one key, so the spread of ``log p^`` over the filters is the estimator's own noise -- its
standard deviation and the time per kernel launch, for both proposals, and the ratio of the times.  ``--proposal residual_bridge``
runs the residual bridge; ``--proposal all`` is ``both`` with the residual bridge as the third proposal of the noise record.

``--likelihood poisson`` / ``negbin`` (dispersion ``--dispersion``, default 10) puts a count likelihood on both cases (the
Lotka-Volterra observations rounded to integers) and runs the count instantiations of the kernel (vsde_count_particle_filter); the
bridge proposal needs the Gaussian one.  ``--noise`` adds the one-theta record for the bootstrap proposal alone.

    python tools/particle_filter_bench.py [--m 1024] [--n 1024] [--reps 200] [--torch-reps 2] [--proposal bootstrap|bridge|residual_bridge|both|all]
                                          [--likelihood gaussian|poisson|negbin] [--dispersion 10] [--noise]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from viforsdes_amd import (GaussianObservationLikelihood, NegativeBinomialObservationLikelihood, Observations,  # noqa: E402
                           PoissonObservationLikelihood, ReactionNetworkSDE, particle_filter)
from viforsdes_amd.inference import particle_filter as pf  # noqa: E402

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


def noise(sde, obs, like, theta, dt, N, pos, a, proposals=("bootstrap", "bridge")):
    """Time per kernel launch and the standard deviation of log p^ over ``--m`` filters of ONE theta, for ``proposals``."""
    obs, theta = obs.to(DEV), theta.to(DEV).expand(a.m, -1).contiguous()
    key = torch.tensor([2468, 1357], dtype=torch.int32, device=DEV)
    out = {"M": a.m, "N": N, "theta": [round(float(v), 6) for v in theta[0]], "likelihood": type(like).__name__}
    if hasattr(like, "variance"):
        out["variance"] = float(like.variance)
    for proposal in proposals:
        run = lambda: particle_filter(sde, obs, like, theta, dt, n_particles=N, positive_dims=pos, key=key, proposal=proposal)
        t1 = timed(run, a.warmup, a.reps)
        t2 = timed(run, 0, a.reps)
        res = run()
        ll = res.log_likelihood.double()
        ok = torch.isfinite(ll)
        out[proposal] = {"kernel_ms": round(min(t1, t2), 4), "kernel_ms_runs": [round(t1, 4), round(t2, 4)],
                         "log_likelihood_mean": round(float(ll[ok].mean()), 4), "log_likelihood_std": round(float(ll[ok].std()), 4),
                         "finite_fraction": float(ok.double().mean()),
                         "min_particle_ess": round(float(res.effective_sample_size.min()), 1),
                         "median_min_particle_ess": round(float(res.effective_sample_size.min(dim=1).values.median()), 1)}
    if "bridge" in out and "bootstrap" in out:
        out["time_ratio_bridge_over_bootstrap"] = round(out["bridge"]["kernel_ms"] / out["bootstrap"]["kernel_ms"], 2)
    if "residual_bridge" in out and "bootstrap" in out:
        out["time_ratio_residual_bridge_over_bootstrap"] = round(out["residual_bridge"]["kernel_ms"] / out["bootstrap"]["kernel_ms"], 2)
    return out


def compare(sde, obs, like, theta, dt, N, pos, a):
    obs, theta = obs.to(DEV), theta.to(DEV)
    key = torch.tensor([12345, 678], dtype=torch.int32, device=DEV)
    run = lambda: particle_filter(sde, obs, like, theta, dt, n_particles=N, positive_dims=pos, key=key, proposal=a.proposal)
    M, P = theta.shape
    S, (K, O) = sde.state_dim, obs.values.shape
    T = int(torch.round(obs.times[-1] / dt))
    pf.HIP_FILTER = True
    tk = timed(run, a.warmup, a.reps)
    tk2 = timed(run, 0, a.reps)
    res_k = run()
    pf.HIP_FILTER = False
    try:
        tt = timed(run, 1, a.torch_reps)
        res_t = run()
    finally:
        pf.HIP_FILTER = True
    lk, lt = res_k.log_likelihood.double(), res_t.log_likelihood.double()
    ok = torch.isfinite(lk) & torch.isfinite(lt)
    kernel_bytes = 4 * (M * (P + S) + K * (O + 1) + M * (1 + 2 * K + 2 * K * S))
    torch_bytes = 4 * M * N * S * 3 * T          # at the very least: state read, noise read, state written, per step
    return {"M": M, "N": N, "steps": T, "observations": K, "kernel_ms": round(min(tk, tk2), 4), "kernel_ms_runs": [round(tk, 4), round(tk2, 4)],
            "torch_ms": round(tt, 2), "ratio": round(tt / min(tk, tk2), 1),
            "particle_steps_per_s": round(M * N * T / (min(tk, tk2) * 1e-3), 0),
            "kernel_bytes": kernel_bytes, "torch_bytes_at_least": torch_bytes,
            "mean_log_likelihood": [round(float(lk[ok].mean()), 4), round(float(lt[ok].mean()), 4)],
            "finite_fraction": [float(torch.isfinite(lk).float().mean()), float(torch.isfinite(lt).float().mean())],
            "min_particle_ess": round(float(res_k.effective_sample_size.min()), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=1024)
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--torch-reps", type=int, default=2)
    ap.add_argument("--proposal", choices=["bootstrap", "bridge", "residual_bridge", "both", "all"], default="bootstrap")
    ap.add_argument("--likelihood", choices=["gaussian", "poisson", "negbin"], default="gaussian")
    ap.add_argument("--dispersion", type=float, default=10.0)
    ap.add_argument("--noise", action="store_true", help="add the one-theta record for the bootstrap proposal alone")
    a = ap.parse_args()
    if a.likelihood != "gaussian" and a.proposal != "bootstrap":
        ap.error("the bridge proposal needs --likelihood gaussian")
    from viforsdes_amd.examples.sdes import lv_problem
    g = torch.Generator().manual_seed(0)
    lv, lv_obs, lv_like, _, _, lv_dt, lv_pos, _ = lv_problem()
    lv_th = torch.tensor([0.5, 0.0025, 0.3]) * (1.0 + 0.1 * torch.rand(a.m, 3, generator=g))
    sir = ReactionNetworkSDE(reactants=[[1, 1], [0, 1]], products=[[0, 2], [0, 0]], species=["S", "I"],
                             reactions=["infection", "removal"])
    sir_obs = Observations(times=torch.tensor([0.0, 5.0, 10.0, 15.0, 20.0]),
                           values=torch.tensor([[95.0, 5.0], [85.0, 8.0], [72.0, 11.0], [60.0, 12.0], [50.0, 11.0]]))
    sir_th = torch.tensor([0.004, 0.15]) * (1.0 + 0.1 * torch.rand(a.m, 2, generator=g))
    sir_like = GaussianObservationLikelihood(variance=1.0)
    if a.likelihood != "gaussian":
        lv_obs = Observations(times=lv_obs.times, values=torch.round(lv_obs.values))
        lv_like = sir_like = (PoissonObservationLikelihood() if a.likelihood == "poisson"
                              else NegativeBinomialObservationLikelihood(dispersion=a.dispersion))
    rec = {"tool": "particle_filter_bench", "device": torch.cuda.get_device_name(DEV), "proposal": a.proposal,
           "likelihood": a.likelihood}
    if a.proposal in ("both", "all"):
        proposals = ("bootstrap", "bridge") + (("residual_bridge",) if a.proposal == "all" else ())
        rec["lv_noise"] = noise(lv, lv_obs, lv_like, torch.tensor([[0.5, 0.0025, 0.3]]), lv_dt, a.n, lv_pos, a, proposals)
        rec["sir_noise"] = noise(sir, sir_obs, sir_like, torch.tensor([[0.004, 0.15]]), 0.1, a.n, [0, 1], a, proposals)
    else:
        rec["lv"] = compare(lv, lv_obs, lv_like, lv_th, lv_dt, a.n, lv_pos, a)
        rec["sir"] = compare(sir, sir_obs, sir_like, sir_th, 0.1, a.n, [0, 1], a)
        if a.noise:
            rec["lv_noise"] = noise(lv, lv_obs, lv_like, torch.tensor([[0.5, 0.0025, 0.3]]), lv_dt, a.n, lv_pos, a, (a.proposal,))
            rec["sir_noise"] = noise(sir, sir_obs, sir_like, torch.tensor([[0.004, 0.15]]), 0.1, a.n, [0, 1], a, (a.proposal,))
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
