"""Bootstrap particle filter whose particles are tau-leap trajectories of the jump process of a ``ReactionNetworkSDE``
(``core/tau_leap.py``): an unbiased estimate of ``p(y | theta)`` of the tau-leap model, on a state that never leaves the integers,
at a cost of ``steps x reactions`` per particle whatever the population.  It fills the gap between ``particle_filter`` (the
chemical Langevin SDE, wrong while a species counts a handful of individuals) and ``jump_particle_filter`` (exact, but as
expensive as there are events: an epidemic in a population of 10^5 is out of its reach).  ``particle_mcmc(..., dynamics="tau_leap")``
runs PMMH on it.

The torch code below is the specification and runs anywhere: any ``ReactionNetworkSDE``, any likelihood, CPU or GPU, fp32 or fp64
theta.  A ``kernel_compatible()`` network with CUDA fp32 theta and observations, a Gaussian or count likelihood of the built-in types
and ``n_particles`` a multiple of 64 up to ``_hip.tau_leap_filter_max_particles`` runs as ONE kernel (csrc/vsde_tau_leap.hip: a
workgroup per theta, a thread per particle) that follows the same rules on the same words with fp32 propensities; every other case
takes the torch route silently, as ``particle_filter`` does.  There are no gradients and there is no ``proposal``: it is the
bootstrap filter.

The rule, for filter ``m`` (``theta_m``, ``N`` particles, all started at the integer ``initial_state``) and the grid rows ``rows =
round(times / time_step)`` of the observation times (float64; ``rows[-1] = 0``):

* segment ``k`` runs the steps ``rows[k-1] .. rows[k] - 1`` of ``core/tau_leap.py`` (``tau_leap_segment``) for particle slot ``j``
  as path ``b = m N + j``: the steps are global and a slot keeps its stream across resampling, as in ``particle_filter``, so the
  particles at observation 0 are ``tau_leap_process(net, x0, theta rows repeated N times, [T_0], time_step, key=key)`` bit for bit.
  An empty segment is not a special case;
* a particle that stops (an invalid propensity, a rate or a copy number above 2^30, a failed draw) keeps the state it stopped in,
  its log-weight at observation ``k`` is -inf, and it only carries on (from that state, at step ``rows[k]``) if the whole filter is
  dead: the jump filter's rule;
* observation ``k`` is ``particle_filter.observation_stage`` unchanged, on the state converted to theta's dtype; NaN counts as
  -inf."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import torch
from torch import Tensor

from ..core.observations import COUNT_LIKELIHOODS, GaussianObservationLikelihood, ObservationLikelihood, Observations
from ..core.reaction_network import ReactionNetworkSDE
from ..core.sde import kernel_theta
from ..core.tau_leap import grid_rows, tau_leap_segment
from . import particle_filter as _pf
from .jump_filter import _launch_model, integer_initial_state

HIP_TAU_LEAP_FILTER = True   # set False to force the torch route (A/B tests)


@dataclass(frozen=True)
class TauLeapFilterResult:
    """``log_likelihood [M]``: log p^(y | theta_m) of the tau-leap model given the start state; ``increments [M, K]``: log p^(y_k |
    y_<k, theta_m); ``effective_sample_size [M, K]``; ``filtered_mean`` / ``filtered_std [M, K, S]``: weighted moments of the
    particles before resampling; ``stopped [M, K]`` (int32): the particles that stopped in segment k (``log_likelihood`` is biased
    downward while any is positive); ``capped [M, K]`` (int32): the draws of segment k reduced because a reactant would have run out
    (0 or rare when ``time_step`` suits the model); and with ``return_particles`` (else None): ``particles [M, K, N, S]`` int32
    (before resampling), ``ancestors [M, K, N]`` int32 and ``log_weights [M, K, N]``."""
    log_likelihood: Tensor
    increments: Tensor
    effective_sample_size: Tensor
    filtered_mean: Tensor
    filtered_std: Tensor
    stopped: Tensor
    capped: Tensor
    particles: Optional[Tensor] = None
    ancestors: Optional[Tensor] = None
    log_weights: Optional[Tensor] = None


def _validate(net, observations, theta, time_step, n_particles, initial_state):
    if not isinstance(net, ReactionNetworkSDE):
        raise ValueError("tau_leap_particle_filter needs a ReactionNetworkSDE: the jump process is defined by its reactions")
    if n_particles < 1:
        raise ValueError(f"n_particles must be >= 1, got {n_particles}")
    if not isinstance(theta, Tensor) or not theta.is_floating_point():
        raise ValueError("theta must be a floating-point tensor")
    theta = theta.detach()
    if theta.ndim == 1:
        theta = theta.unsqueeze(0)
    P = int(net.sde_param_dim)
    if theta.ndim != 2 or theta.shape[0] < 1 or theta.shape[1] != P:
        raise ValueError(f"theta [M, {P}] or [{P}] expected (sde_param_dim {P}), got {tuple(theta.shape)}")
    M = theta.shape[0]
    if M * n_particles >= 2 ** 32:
        raise ValueError(f"M * n_particles = {M * n_particles} paths: the stream indexes fewer than 2^32")
    if observations.values.shape[0] < 1:
        raise ValueError("observations must not be empty")
    if time_step is None:
        raise ValueError("time_step is required: tau-leaping steps on its grid")
    rows = grid_rows(observations.times, time_step, "observation times")
    return theta, integer_initial_state(net, observations, initial_state, M, theta.device), rows


def tau_leap_particle_filter(net: ReactionNetworkSDE, observations: Observations, observation_likelihood: ObservationLikelihood,
                             theta: Tensor, time_step: float, n_particles: int = 1024, initial_state: Optional[Tensor] = None,
                             return_particles: bool = False, key: Optional[Tensor] = None) -> TauLeapFilterResult:
    """Bootstrap particle filters on the tau-leap of ``net`` with the step ``time_step`` and ``n_particles`` particles, one per row of
    ``theta`` (``[M, P]``, or ``[P]`` for M = 1), all started at ``initial_state`` (``[S]`` or ``[M, S]``, integers in ``0 .. 2^30``;
    default: the first observation, which must then have the state's dim and hold integers).  ``observations.times`` are taken as
    float64 (finite, >= 0, non-decreasing) and map to the grid rows ``round(times / time_step)``.  ``key``: two int32 words;
    default: drawn from torch's generator on theta's device.  The same key gives the same result on a route.  The module docstring
    has the rule.  No gradients."""
    theta, x0, rows = _validate(net, observations, theta, time_step, n_particles, initial_state)
    dev = theta.device
    obs = observations if observations.values.device == dev else observations.to(dev)
    key = _pf._call_key(key, dev)
    N = int(n_particles)
    with torch.no_grad():
        if _kernel_route(net, obs, observation_likelihood, theta, N):
            from .. import _hip
            network = net.kernel_descriptor()
            return TauLeapFilterResult(*_hip.tau_leap_particle_filter(
                x0.to(torch.int32).contiguous(), kernel_theta(network, theta).contiguous(), rows.to(device=dev, dtype=torch.int32),
                *_launch_model(obs, observation_likelihood, theta), key.to(torch.int32) if key.dtype != torch.int32 else key,
                float(time_step), N, network=network, return_particles=return_particles))
        return _torch_filter(net, obs, observation_likelihood, theta, rows, float(time_step), N, x0, return_particles, key)


def _kernel_route(net, obs, like, theta, n_particles) -> bool:
    """Whether the kernel takes the call (the module docstring has the conditions)."""
    if not (HIP_TAU_LEAP_FILTER and theta.is_cuda and theta.dtype == torch.float32 and obs.values.dtype == torch.float32):
        return False
    if type(like) not in COUNT_LIKELIHOODS and type(like) is not GaussianObservationLikelihood:
        return False
    if not net.kernel_compatible():
        return False
    from .. import _hip
    S, O, H = int(net.state_dim), obs.values.shape[1], like.obs_matrix
    if O > _hip.PF_MAX_OBS or (H is None and O != S) or (H is not None and tuple(H.shape) != (O, S)):
        return False
    return n_particles % 64 == 0 and n_particles <= _hip.tau_leap_filter_max_particles(S, int(net.num_reactions), not net.plain)


def _torch_filter(net, obs, like, theta, rows, time_step, N, x0, return_particles, key) -> TauLeapFilterResult:
    dev, dtype = theta.device, theta.dtype
    M = theta.shape[0]
    S = x0.shape[1]
    K = rows.shape[0]
    rates = theta if net.plain else net.kernel_parameters(theta)
    x = x0[:, None, :].expand(M, N, S).reshape(M * N, S).clone()
    rt = rates[:, None, :].expand(M, N, rates.shape[1]).reshape(M * N, -1)
    b = torch.arange(M * N, device=dev, dtype=torch.int64)          # slot j of filter m is path m N + j
    neg_inf = torch.tensor(float("-inf"), device=dev, dtype=dtype)
    steps = [0] + rows.tolist()
    incr, ess, means, stds, stop, caps, parts, ancs, lws = [], [], [], [], [], [], [], [], []
    for k in range(K):
        x, status, capped = tau_leap_segment(net, x, rt, time_step, steps[k], steps[k + 1], b, key)
        xm = x.to(dtype).reshape(M, N, S)
        lw = like.log_prob(obs.values[k].to(dtype).unsqueeze(0).expand(M * N, -1), xm.reshape(M * N, S)).reshape(M, N)
        lw = torch.where(torch.isnan(lw) | (status != 0).reshape(M, N), neg_inf, lw)
        inc_k, ess_k, mean, std, anc = _pf.observation_stage(lw, xm, k, key)
        incr.append(inc_k)
        ess.append(ess_k)
        means.append(mean)
        stds.append(std)
        stop.append((status != 0).reshape(M, N).sum(dim=1).to(torch.int32))
        caps.append(capped.reshape(M, N).sum(dim=1).to(torch.int32))
        if return_particles:
            parts.append(x.reshape(M, N, S).to(torch.int32))
            ancs.append(anc.to(torch.int32))
            lws.append(lw)
        x = torch.gather(x.reshape(M, N, S), 1, anc[..., None].expand(-1, -1, S)).reshape(M * N, S)
    increments = torch.stack(incr, dim=1)
    opt = lambda seq: torch.stack(seq, dim=1) if return_particles else None
    return TauLeapFilterResult(
        log_likelihood=increments.sum(dim=1), increments=increments, effective_sample_size=torch.stack(ess, dim=1),
        filtered_mean=torch.stack(means, dim=1), filtered_std=torch.stack(stds, dim=1), stopped=torch.stack(stop, dim=1),
        capped=torch.stack(caps, dim=1), particles=opt(parts), ancestors=opt(ancs), log_weights=opt(lws))
