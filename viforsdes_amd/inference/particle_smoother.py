"""Particle smoother: draws of the latent path ``x_{0:T} | y, theta`` of the Euler-Maruyama-discretised model from the genealogy
of a particle filter (``particle_filter`` of this package), for a batch of parameter vectors at once.  It is the yardstick for the
path half of a variational posterior that no network enters (``VariationalPosterior.smooth_paths``), as the filter's
``log_likelihood`` is for the theta half.

Why genealogy tracing is enough here: the filter resamples only at the K observations, so a lineage traced back through the stored
``ancestors`` coalesces at most K times, and with the handful of observations of this package's problems a draw keeps a usable
share of distinct pasts (``distinct_lineages`` says how many) without backward simulation.  Why no trajectory store: every normal
comes from the counter-based Philox stream indexed by (path slot, GLOBAL grid step), so the states between two observations are
recomputed exactly from the stored particle at the previous observation, the slot whose noise the segment used and the step
function.  The filter is not changed at all.

The rule, for filter ``m`` (``D = n_draws``, ``N = n_particles``, ``rows`` the grid rows of the K observations, ``T = rows[K-1]``):

* filter: ``particle_filter(..., return_particles=True, key=key)`` gives the particles ``X[m, k, j]`` (before resampling at k), the
  ancestors ``a[m, k, j]`` and the log-weights ``lw[m, k, j]``;
* final slots: ``W_j = exp(lw[m, K-1, j] - max_j)``, ``C`` its inclusive cumulative sums made non-decreasing by a running maximum,
  one uniform per filter ``u = ((w0 >> 8) + 0.5) 2^-24`` with ``w0`` the first word of ``philox4x32_10({0, 0, m, 2}, key)`` (counter
  word 3: 0 is the normals, 1 the resampling uniforms), ``tau_d = (d + u) / D * C_{N-1}`` and
  ``lineage[m, d, K-1] = min(#{i : C_i <= tau_d}, N - 1)``: systematic sampling with D thresholds over N weights, for any D;
* trace: ``lineage[m, d, k-1] = a[m, k-1, lineage[m, d, k]]`` for k = K-1 .. 1;
* replay: segment k covers the global grid steps ``rows[k-1] .. rows[k] - 1`` (segment 0: ``0 .. rows[0] - 1``, from ``x0[m]``).  For
  k >= 1 it starts at ``X[m, k-1, lineage[m, d, k-1]]``; its noise is that of path ``b = m N + lineage[m, d, k]`` (a slot keeps its
  own stream across resampling); its steps are the filter's towards observation k, for every proposal: the rule is the module
  docstring of ``particle_filter`` and the code is the filter's own (``particle_filter._segment_propagator``), started from the
  segment's stored start state.  The state after step t goes to ``paths[m, d, t+1]``, ``paths[m, d, 0] = x0[m]``; a zero-length
  segment (observations sharing a row) writes nothing;
* a filter with ``log_likelihood[m] = -inf`` (some observation left no positive weight) has no smoothing sample: lineage -1, paths
  NaN, ``distinct_lineages`` 0.

Under ``proposal="bridge"`` or ``"residual_bridge"`` the draws are still draws of the model's smoothing distribution: the filter's weights carry the ratio
model / proposal.

The torch code below is the specification and runs anywhere.  Where ``particle_filter`` takes its kernel route (built-in SDEs and
reaction networks, Gaussian likelihood or a count likelihood with the bootstrap proposal, fp32 on the GPU, ``n_particles`` within the
filter's limits) trace and replay run as ONE kernel (csrc/vsde_filter.hip: rp_kernel, a thread per (k, m, d) segment); every other
case runs the torch route silently, and ``particle_filter.HIP_FILTER = False`` forces it for both stages.  The final slots are drawn
in torch on both routes."""
from __future__ import annotations

from collections.abc import Sequence
from dataclasses import dataclass
from typing import Optional

import torch
from torch import Tensor

from ..core.observations import ObservationLikelihood, Observations
from ..core.sde import SDE, kernel_theta
from . import particle_filter as _pf


@dataclass(frozen=True)
class SmoothedPaths:
    """``paths [M, D, T+1, S]``: D draws of ``x_{0:T} | y, theta_m`` per filter on the grid (``T = rows[K-1]``); ``lineage [M, D, K]``
    (int32): the particle slot the draw occupied before resampling at observation k; ``distinct_lineages [M, K]``: the number of
    different slots among the D draws at observation k, the degeneracy diagnostic (1 at an early k: all draws share their past);
    the rest are the filter's fields of the same name.  A dead filter (``log_likelihood = -inf``): paths NaN, lineage -1,
    distinct_lineages 0."""
    paths: Tensor
    lineage: Tensor
    distinct_lineages: Tensor
    log_likelihood: Tensor
    increments: Tensor
    effective_sample_size: Tensor
    filtered_mean: Tensor
    filtered_std: Tensor


def smoothing_uniforms(n_filters: int, key: Tensor) -> Tensor:
    """The uniform of filter m's final draw for m = 0 .. n_filters - 1: fp32 ``[n_filters]``."""
    dev = key.device
    k0, k1 = _pf._key_words(key)
    m = torch.arange(n_filters, device=dev, dtype=torch.int64)
    zero = torch.zeros(1, device=dev, dtype=torch.int64)
    return _pf._uniform(_pf.philox4x32_10(zero, zero, m, torch.full_like(zero, 2), k0, k1)[0])


def systematic_draws(weights: Tensor, u: Tensor, n_draws: int) -> Tensor:
    """Slots ``[M, D]`` (int64) of systematic sampling with D thresholds over the weights ``[M, N]`` (>= 0, not all zero in a row)
    and one uniform ``u [M]`` per row: ``min(#{i : C_i <= (d + u) / D * C_{N-1}}, N - 1)``."""
    N = weights.shape[1]
    cum = torch.cummax(torch.cumsum(weights, dim=1), dim=1).values
    d = torch.arange(n_draws, device=weights.device, dtype=weights.dtype)
    tau = (d[None, :] + u.to(weights.dtype)[:, None]) / n_draws * cum[:, -1:]
    return torch.searchsorted(cum.contiguous(), tau.contiguous(), right=True).clamp(max=N - 1)


def particle_smoother(sde: SDE, observations: Observations, observation_likelihood: ObservationLikelihood, theta: Tensor,
                      time_step: float, n_particles: int = 1024, n_draws: int = 1, initial_state: Optional[Tensor] = None,
                      positive_dims: Sequence[int] = (), key: Optional[Tensor] = None, proposal: str = "bootstrap") -> SmoothedPaths:
    """``n_draws`` smoothed paths per row of ``theta`` from the genealogy of ``particle_filter`` (the module docstring has the
    rule).  Arguments, validation, ``key`` and ``proposal`` are those of ``particle_filter``; ``n_draws >= 1``.  Draws of one filter
    share ancestors (see ``SmoothedPaths.distinct_lineages``); draws of different filters are independent.  No gradients."""
    bridge, residual = _pf._proposal_flags(proposal, observation_likelihood)
    if n_draws < 1:
        raise ValueError(f"n_draws must be >= 1, got {n_draws}")
    theta, x0 = _pf._validate(sde, observations, theta, time_step, n_particles, initial_state)
    dev = theta.device
    obs = observations if observations.values.device == dev else observations.to(dev)
    key = _pf._call_key(key, dev)
    pos = tuple(positive_dims)
    M, N, D = theta.shape[0], int(n_particles), int(n_draws)
    with torch.no_grad():
        res = _pf.particle_filter(sde, obs, observation_likelihood, theta, time_step, n_particles=N, initial_state=x0,
                                  positive_dims=pos, return_particles=True, key=key, proposal=proposal)
        lw = res.log_weights[:, -1]
        dead = torch.isneginf(res.log_likelihood) | torch.isnan(res.log_likelihood)
        mx = lw.max(dim=1, keepdim=True).values
        live = ~(dead[:, None] | torch.isneginf(mx))
        w = torch.where(live, torch.exp(lw - torch.where(live, mx, torch.zeros_like(mx))), torch.ones_like(lw))
        last = systematic_draws(w, smoothing_uniforms(M, key), D)
        last = torch.where(dead[:, None], torch.full_like(last, -1), last).to(torch.int32)
        route = _pf._kernel_route(sde, obs, observation_likelihood, theta, N, proposal)
        if route is not None:
            kind, network = route
            rows, model = _pf._launch_model(obs, observation_likelihood, theta, time_step)
            paths, lineage = _pf._kernel_call("filter_replay", proposal, (kind, x0, kernel_theta(network, theta), rows), model,
                                              key.to(torch.int32) if key.dtype != torch.int32 else key, float(time_step),
                                              res.particles, res.ancestors, last, pos, network=network)
        else:
            lineage = _trace(res.ancestors, last)
            paths = _torch_replay(sde, obs, observation_likelihood, theta, float(time_step), x0, pos, key, bridge, res.particles,
                                  lineage, torch.round(obs.times / time_step).long().tolist(), residual)
        srt = torch.sort(lineage, dim=1).values
        distinct = 1 + (srt[:, 1:] != srt[:, :-1]).sum(dim=1)
        distinct = torch.where(dead[:, None], torch.zeros_like(distinct), distinct)
    return SmoothedPaths(paths=paths, lineage=lineage, distinct_lineages=distinct, log_likelihood=res.log_likelihood,
                         increments=res.increments, effective_sample_size=res.effective_sample_size,
                         filtered_mean=res.filtered_mean, filtered_std=res.filtered_std)


def _trace(ancestors: Tensor, last: Tensor) -> Tensor:
    """``lineage [M, D, K]`` (int32) from the ancestors [M, K, N] and the final slots [M, D] (-1: dead, kept)."""
    K = ancestors.shape[1]
    cols = [last.long()]
    for k in range(K - 1, 0, -1):
        cur = cols[-1]
        prev = torch.gather(ancestors[:, k - 1].long(), 1, cur.clamp(min=0))
        cols.append(torch.where(cur < 0, cur, prev))
    return torch.stack(cols[::-1], dim=2).to(torch.int32)


def _torch_replay(sde, obs, like, theta, dt, x0, pos, key, bridge, particles, lineage, rows, residual=False) -> Tensor:
    dev, dtype = theta.device, theta.dtype
    M, P = theta.shape
    _, D, K = lineage.shape
    N, S = particles.shape[2], particles.shape[3]
    T = rows[-1]
    lin = lineage.long()
    dead = lin[:, :, -1] < 0                                                   # [M, D]
    slot = lin.clamp(min=0)
    th = theta[:, None, :].expand(M, D, P).reshape(M * D, P)
    advance = _pf._segment_propagator(sde, obs, like, theta, dt, pos, bridge, residual)
    base = torch.arange(M, device=dev, dtype=torch.int64)[:, None] * N
    x_first = x0[:, None, :].expand(M, D, S).reshape(M * D, S)
    paths = torch.empty(M * D, T + 1, S, device=dev, dtype=dtype)
    paths[:, 0] = x_first
    row_prev = 0
    for k in range(K):
        if rows[k] == row_prev:
            continue
        if k == 0:
            x = x_first
        else:
            x = torch.gather(particles[:, k - 1], 1, slot[:, :, k - 1, None].expand(-1, -1, S)).reshape(M * D, S)
        advance(x, th, row_prev, k, rows[k], (base + slot[:, :, k]).reshape(M * D), key, out=paths[:, row_prev + 1:rows[k] + 1])
        row_prev = rows[k]
    paths = paths.reshape(M, D, T + 1, S)
    return torch.where(dead[:, :, None, None], torch.full_like(paths, float("nan")), paths)
