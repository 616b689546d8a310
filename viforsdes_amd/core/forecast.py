"""Forecast of the *model* SDE from given start states: the Euler-Maruyama recursion of ``euler_maruyama`` run ``n_steps`` steps
on, keeping only the states after the grid steps ``out_steps``.  Used by ``VariationalPosterior.predict`` to continue each
posterior path past the time horizon with its own theta.

Built-in SDEs on the GPU in fp32 run as ONE kernel (csrc/vsde_sde.hip: vsde_forecast) that makes its Gaussian increments from a
Philox stream: neither the ``[B, n_steps, S]`` noise nor the ``[B, n_steps + 1, S]`` trajectory is ever stored.  Every other
case (a user SDE, CPU tensors, another dtype) runs ``euler_maruyama`` -- which is also the specification -- and gathers."""
from __future__ import annotations

from collections.abc import Sequence

import torch
from torch import Tensor

from .euler_maruyama import euler_maruyama
from .sde import SDE, builtin_sde_route, kernel_theta


def forecast_states(sde: SDE, x_start: Tensor, theta: Tensor, n_steps: int, out_steps, time_step: float,
                    positive_dims: Sequence[int] = ()) -> Tensor:
    """States ``[B, K, S]`` after the steps ``out_steps`` ``[K]`` (non-decreasing, in ``1..n_steps``; a sequence, or an integer
    tensor -- on the device for the kernel route, where it is not checked) of an ``n_steps``-step Euler-Maruyama run from
    ``x_start [B, S]`` with ``theta [B, P]``, time step ``time_step``; positive dims are clamped at 1e-6 after every step.

    The kernel route (built-in SDE, CUDA, fp32) draws its Philox key from torch's generator on the device
    (``torch.randint``), so ``torch.manual_seed`` makes the call repeatable and it can be captured in a HIP graph (fresh draws
    per replay).  The torch route draws ``torch.randn`` noise as ``euler_maruyama`` does.  The two routes give the same
    distribution, not the same draws."""
    if n_steps < 1:
        raise ValueError(f"n_steps must be >= 1, got {n_steps}")
    if time_step <= 0:
        raise ValueError(f"time_step must be positive, got {time_step}")
    if x_start.ndim != 2 or theta.ndim != 2 or theta.shape[0] != x_start.shape[0]:
        raise ValueError(f"x_start [B, S] and theta [B, P] expected, got {tuple(x_start.shape)} and {tuple(theta.shape)}")
    dev = x_start.device
    if isinstance(out_steps, Tensor) and out_steps.is_cuda:
        steps = out_steps.to(device=dev, dtype=torch.int32)
    else:
        host = torch.as_tensor(out_steps, dtype=torch.int64).reshape(-1)
        if host.numel() < 1:
            raise ValueError("out_steps must not be empty")
        if bool((host < 1).any()) or bool((host > n_steps).any()) or bool((host[1:] < host[:-1]).any()):
            raise ValueError(f"out_steps must be non-decreasing and in 1..{n_steps}")
        steps = host.to(torch.int32).to(dev)
    kind, network = builtin_sde_route(sde)
    if kind is not None and x_start.is_cuda and x_start.dtype == torch.float32:
        from .. import _hip
        key = torch.randint(-2 ** 31, 2 ** 31, (2,), device=dev, dtype=torch.int32)
        return _hip.forecast(kind, x_start, kernel_theta(network, theta), n_steps, steps, key, float(time_step),
                             tuple(positive_dims), network=network)
    traj = euler_maruyama(sde, x_start, theta, n_steps * time_step, time_step, positive_dims)
    return traj[:, steps.long()]
