"""Particle smoother on the exact jump process of a ``ReactionNetworkSDE``: draws of the latent path ``x | y, theta`` of the Markov
jump process itself (``core/jump_process.py``), on the integers, read at any instants ``path_times``, from the genealogy of
``jump_particle_filter``.  It is the jump-process sibling of ``particle_smoother``: where ``diffusion_approximation_check`` sends a
user to the jump process (extinctions, copy numbers of a few units) the SDE paths are exactly what goes wrong, and these are the
paths to look at instead.

Why genealogy tracing is enough and why there is no trajectory store: as in ``particle_smoother``.  The filter resamples only at the
K observations, and its noise is counter-based: the uniforms of segment k of path slot b are those of ``philox4x32_10({e >> 1, k, b,
7}, key)``, so a segment is recomputed exactly, event by event, from the stored particle at the previous observation, the slot whose
noise the segment used and theta.  The filter is not changed at all.

The rule, for filter ``m`` (``D = n_draws``, ``N = n_particles``, observation times ``T_0 <= .. <= T_{K-1}``, ``T_{-1} = 0``, output
times ``t_0 <= .. <= t_{Q-1}`` in ``[0, T_{K-1}]``):

* filter: ``jump_particle_filter(..., return_particles=True, key=key)`` gives the particles ``X[m, k, j]`` (before resampling at k),
  the ancestors ``a[m, k, j]``, the log-weights and the event counts;
* final slots: ``particle_smoother``'s rule unchanged (``systematic_draws`` on the last log-weights with ``smoothing_uniforms``:
  counter word 2 in the fourth slot), in torch on both routes;
* trace: ``lineage[m, d, k-1] = a[m, k-1, lineage[m, d, k]]`` for k = K-1 .. 1;
* replay: segment k starts at ``X[m, k-1, lineage[m, d, k-1]]`` (``x0[m]`` for k = 0) with the clock at exactly ``T_{k-1}`` and the
  event counter at 0, and repeats the filter's events of path ``b = m N + lineage[m, d, k]`` (a slot keeps its own stream across
  resampling) word for word until ``T_k < t + tau`` (``core.jump_process.jump_segment_states``).  Segment k owns the output times
  with ``T_{k-1} < t_q <= T_k`` (segment 0: ``0 <= t_q <= T_0``; a zero-length segment owns nothing).  Before the event at ``t + tau``
  is applied every owned ``t_q < t + tau`` not yet written receives the current state: an output time receives the state after every
  event with time ``<= t_q``, the rule of ``jump_process``.  So ``paths`` at ``t_q = T_k`` is ``X[m, k, lineage[m, d, k]]`` and
  ``n_events[m, d, k]`` is the filter's event count of that particle, bit for bit;
* ``status[m, d, k]`` is the segment's status as the replay met it (0 complete, 1 event cap, 2 invalid propensity; the outputs a
  stopped segment did not reach are -1).  A traced lineage has positive weight at every observation, a stopped particle weighs
  -inf, and the replay runs with the filter's own ``max_events``: a traced lineage cannot be a stopped particle, so ``status`` is
  all 0 for a live filter;
* a filter with ``log_likelihood[m] = -inf`` (some observation left no positive weight) has no smoothing sample: lineage -1, paths
  -1, ``n_events`` and ``status`` 0, ``distinct_lineages`` 0.

The torch code below is the specification and runs anywhere.  Exactly where ``jump_particle_filter`` takes its kernel route
(``jump_filter._kernel_route``) trace and replay run as ONE kernel (csrc/vsde_jump_replay.hip: jr_kernel, a thread per (segment,
draw)); every other case runs the torch route silently, and ``jump_filter.HIP_JUMP_FILTER = False`` forces it for both stages."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import torch
from torch import Tensor

from ..core.jump_process import jump_segment_states
from ..core.observations import ObservationLikelihood, Observations
from ..core.reaction_network import ReactionNetworkSDE
from ..core.sde import kernel_theta
from . import jump_filter as _jf
from . import particle_filter as _pf
from .particle_smoother import _trace, smoothing_uniforms, systematic_draws


@dataclass(frozen=True)
class SmoothedJumpPaths:
    """``paths [M, D, Q, S]`` (int32): D draws of the jump process given the data per filter, read at ``path_times [Q]`` (float64);
    ``lineage [M, D, K]`` (int32): the particle slot the draw occupied before resampling at observation k; ``distinct_lineages
    [M, K]``: the number of different slots among the D draws at observation k; ``n_events`` / ``status [M, D, K]`` (int32): the
    events the draw fired in segment k and the segment's status (all 0 for a live filter); the rest are the filter's fields of the
    same name.  A dead filter (``log_likelihood = -inf``): paths -1, lineage -1, distinct_lineages 0."""
    paths: Tensor
    path_times: Tensor
    lineage: Tensor
    distinct_lineages: Tensor
    n_events: Tensor
    status: Tensor
    log_likelihood: Tensor
    increments: Tensor
    effective_sample_size: Tensor
    filtered_mean: Tensor
    filtered_std: Tensor
    stopped: Tensor


def validated_path_times(path_times, obs_times: Tensor) -> Tensor:
    """``path_times`` as a float64 CPU tensor ``[Q]``, ``Q >= 1``: finite, non-decreasing and inside ``[0, T_{K-1}]`` of the
    observation times ``obs_times`` (float64, CPU)."""
    if isinstance(path_times, Tensor) and path_times.dtype != torch.float64:
        raise ValueError(f"path_times must be float64, got {path_times.dtype}")
    t = torch.as_tensor(path_times, dtype=torch.float64).detach().cpu()
    if t.ndim != 1 or t.numel() < 1:
        raise ValueError(f"path_times must be a non-empty 1-D tensor, got shape {tuple(t.shape)}")
    if not bool(torch.isfinite(t).all()) or bool((t[1:] < t[:-1]).any()):
        raise ValueError("path_times must be finite and non-decreasing")
    if bool((t < 0).any()) or bool((t > obs_times[-1]).any()):
        raise ValueError(f"path_times must lie in [0, {float(obs_times[-1])}], the span of the observations, got "
                         f"{float(t.min())} .. {float(t.max())}")
    return t


def ownership_ranges(path_times: Tensor, obs_times: Tensor) -> Tensor:
    """``q_begin`` (int32 CPU ``[K + 1]``): segment k owns the outputs ``q_begin[k] .. q_begin[k+1] - 1``, the ``t_q`` with
    ``T_{k-1} < t_q <= T_k`` (segment 0: from 0), by a float64 search on the host."""
    upto = torch.searchsorted(path_times.contiguous(), obs_times.contiguous(), right=True)
    return torch.cat([torch.zeros(1, dtype=torch.int64), upto]).to(torch.int32)


def jump_particle_smoother(net: ReactionNetworkSDE, observations: Observations, observation_likelihood: ObservationLikelihood,
                           theta: Tensor, path_times, n_particles: int = 1024, n_draws: int = 1, initial_state: Optional[Tensor] = None,
                           key: Optional[Tensor] = None, max_events: int = 2 ** 16) -> SmoothedJumpPaths:
    """``n_draws`` smoothed paths of the jump process per row of ``theta``, read at ``path_times`` (float64 ``[Q]``, ``Q >= 1``,
    finite, non-decreasing, inside ``[0, T_{K-1}]``), from the genealogy of ``jump_particle_filter`` (the module docstring has the
    rule).  The other arguments, their validation and ``key`` are those of ``jump_particle_filter``; ``n_draws >= 1``.  Draws of one
    filter share ancestors (see ``SmoothedJumpPaths.distinct_lineages``); draws of different filters are independent.  No gradients."""
    if n_draws < 1:
        raise ValueError(f"n_draws must be >= 1, got {n_draws}")
    theta, x0, times = _jf._validate(net, observations, theta, n_particles, initial_state, max_events)
    t_out = validated_path_times(path_times, times)
    q_begin = ownership_ranges(t_out, times)
    dev = theta.device
    obs = observations if observations.values.device == dev else observations.to(dev)
    key = _pf._call_key(key, dev)
    M, N, D, max_events = theta.shape[0], int(n_particles), int(n_draws), int(max_events)
    with torch.no_grad():
        res = _jf.jump_particle_filter(net, obs, observation_likelihood, theta, n_particles=N, initial_state=x0, return_particles=True,
                                       key=key, max_events=max_events)
        lw = res.log_weights[:, -1]
        dead = torch.isneginf(res.log_likelihood) | torch.isnan(res.log_likelihood)
        mx = lw.max(dim=1, keepdim=True).values
        live = ~(dead[:, None] | torch.isneginf(mx))
        w = torch.where(live, torch.exp(lw - torch.where(live, mx, torch.zeros_like(mx))), torch.ones_like(lw))
        last = systematic_draws(w, smoothing_uniforms(M, key), D)
        last = torch.where(dead[:, None], torch.full_like(last, -1), last).to(torch.int32)
        if _jf._kernel_route(net, obs, observation_likelihood, theta, N):
            from .. import _hip
            network = net.kernel_descriptor()
            paths, lineage, n_events, status = _hip.jump_filter_replay(
                x0.to(torch.int32).contiguous(), kernel_theta(network, theta).contiguous(), times.to(dev), t_out.to(dev), q_begin,
                key.to(torch.int32) if key.dtype != torch.int32 else key, max_events, res.particles, res.ancestors, last,
                network=network)
        else:
            lineage = _trace(res.ancestors, last)
            paths, n_events, status = _torch_replay(net, theta, x0, times, t_out, q_begin, key, max_events, res.particles, lineage)
        srt = torch.sort(lineage, dim=1).values
        distinct = 1 + (srt[:, 1:] != srt[:, :-1]).sum(dim=1)
        distinct = torch.where(dead[:, None], torch.zeros_like(distinct), distinct)
    return SmoothedJumpPaths(paths=paths, path_times=t_out.to(dev), lineage=lineage, distinct_lineages=distinct, n_events=n_events,
                             status=status, log_likelihood=res.log_likelihood, increments=res.increments,
                             effective_sample_size=res.effective_sample_size, filtered_mean=res.filtered_mean,
                             filtered_std=res.filtered_std, stopped=res.stopped)


def replay_records(net, rates: Tensor, x0: Tensor, times: Tensor, t_out: Tensor, q_begin: Tensor, anchors: Tensor, noise_path: Tensor,
                   keys: Tensor, max_events: int, dead: Tensor) -> tuple[Tensor, Tensor, Tensor]:
    """The replay in torch, segment by segment on ``jump_segment_states``: B records with the effective constants ``rates [B, .]``,
    start states ``x0 [B, S]`` (int64), ``anchors [B, K, S]`` (integers: the state at every observation), ``noise_path [B, K]``
    (int64) and ``keys``: one key ``[2]`` for all records, or one each ``[B, 2]``.  ``times`` /
    ``t_out`` / ``q_begin``: the observation times, the output times and their ownership ranges on the host.  Returns ``(paths
    [B, Q, S], n_events [B, K], status [B, K])``, int32; a ``dead [B]`` record has paths -1, events and status 0."""
    dev = rates.device
    B, K, S = anchors.shape
    Q = t_out.shape[0]
    paths = torch.full((B, Q, S), -1, dtype=torch.int32, device=dev)
    n_events = torch.zeros(B, K, dtype=torch.int32, device=dev)
    status = torch.zeros(B, K, dtype=torch.int32, device=dev)
    idx = torch.nonzero(~dead)[:, 0]
    if idx.numel() == 0:
        return paths, n_events, status
    instants = [0.0] + times.tolist()
    begin = q_begin.tolist()
    live_keys = keys if keys.ndim == 1 else keys[idx]
    for k in range(K):
        start = x0[idx] if k == 0 else anchors[idx, k - 1].to(torch.int64)
        _, ne, st, states = jump_segment_states(net, start, rates[idx], instants[k], instants[k + 1], k, noise_path[idx, k], live_keys,
                                                max_events, t_out[begin[k]:begin[k + 1]])
        n_events[idx, k], status[idx, k] = ne, st
        paths[idx, begin[k]:begin[k + 1]] = states
    return paths, n_events, status


def _torch_replay(net, theta, x0, times, t_out, q_begin, key, max_events, particles, lineage):
    M, D, K = lineage.shape
    N, S = particles.shape[2], particles.shape[3]
    dev = theta.device
    lin = lineage.long()
    dead = (lin[:, :, -1] < 0).reshape(M * D)
    slot = lin.clamp(min=0)
    rates = theta if net.plain else net.kernel_parameters(theta)
    rates = rates[:, None, :].expand(M, D, rates.shape[1]).reshape(M * D, -1)
    anchors = torch.gather(particles, 2, slot.permute(0, 2, 1)[..., None].expand(M, K, D, S)).permute(0, 2, 1, 3).reshape(M * D, K, S)
    noise = (torch.arange(M, device=dev, dtype=torch.int64)[:, None, None] * N + slot).reshape(M * D, K)
    paths, n_events, status = replay_records(net, rates, x0[:, None, :].expand(M, D, S).reshape(M * D, S), times, t_out, q_begin, anchors,
                                             noise, key, max_events, dead)
    return paths.reshape(M, D, -1, S), n_events.reshape(M, D, K), status.reshape(M, D, K)
