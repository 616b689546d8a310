"""CPU: ``bench.py --dump-outputs`` -- what the last timed step hands its caller, written as .npy files under a size budget with a
fixed sample of any array that does not fit."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from viforsdes_amd.inference.exponential_moving_average import ExponentialMovingAverage  # noqa: E402
from viforsdes_amd.inference.trainer import TrainStepResult  # noqa: E402
from viforsdes_amd.inference.types import EvidenceLowerBoundComponents, EvidenceLowerBoundResult  # noqa: E402


def test_small_arrays_are_written_whole_with_their_precision(tmp_path):
    a = torch.arange(12, dtype=torch.float32).reshape(3, 4)
    b = torch.tensor(2.5, dtype=torch.float64)
    c = torch.ones(5, dtype=torch.bfloat16)
    names = bench.write_outputs(str(tmp_path), {"a": a, "b": b, "c": c})
    assert names == ["a", "b", "c"]
    ra, rb, rc = (np.load(tmp_path / f"{n}.npy") for n in names)
    assert ra.dtype == np.float32 and ra.shape == (3, 4) and np.array_equal(ra, a.numpy())
    assert rb.dtype == np.float64 and rb.shape == () and float(rb) == 2.5
    assert rc.dtype == np.float32 and np.array_equal(rc, np.ones(5, np.float32))


def test_large_arrays_are_sampled_into_the_budget_the_same_way_every_time(tmp_path):
    budget = 6 << 20
    big = torch.arange(2 << 20, dtype=torch.float32)           # 8 MiB: over the budget on its own
    fits = torch.arange(1 << 19, dtype=torch.float32) * -1.0    # 2 MiB: fits its share whole
    arrays = {"big": big, "fits": fits, "scalar": torch.tensor(1.0)}
    d1, d2 = tmp_path / "one", tmp_path / "two"
    bench.write_outputs(str(d1), arrays, budget=budget)
    bench.write_outputs(str(d2), arrays, budget=budget)
    assert sum(os.path.getsize(d1 / f) for f in os.listdir(d1)) <= budget
    s1, s2 = np.load(d1 / "big.npy"), np.load(d2 / "big.npy")
    assert np.array_equal(s1, s2) and 0 < s1.size < big.numel()
    assert np.all(np.diff(s1) > 0) and np.all(np.isin(s1, big.numpy()))   # sorted distinct elements of the original
    assert np.array_equal(np.load(d1 / "fits.npy"), fits.numpy())


def test_step_outputs_carry_the_elbo_gradient_norm_parameters_and_ema():
    model = torch.nn.Sequential(torch.nn.Linear(3, 2), torch.nn.Linear(2, 1))
    ema = ExponentialMovingAverage(model)
    with torch.no_grad():
        for p in model.parameters():
            p.add_(1.0)
    comps = EvidenceLowerBoundComponents(*[torch.tensor(float(k)) for k in range(5)])
    result = TrainStepResult(elbo_result=EvidenceLowerBoundResult(torch.tensor(-3.0), comps), grad_norm=torch.tensor(0.5))
    out = bench.step_outputs(result, model, ema)
    assert float(out["elbo"]) == -3.0 and float(out["grad_norm"]) == 0.5
    assert float(out["elbo_posterior_log_prob"]) == 4.0 and float(out["elbo_observation_log_prob"]) == 0.0
    flat = torch.cat([p.detach().reshape(-1) for p in model.parameters()])
    shadow = torch.cat([ema.shadow[n].reshape(-1) for n, _ in model.named_parameters()])
    assert torch.equal(out["parameters"], flat) and torch.equal(out["ema_parameters"], shadow)
    assert not torch.equal(flat, shadow)
