"""Bootstrap particle filter whose particles are exact trajectories of the Markov jump process of a ``ReactionNetworkSDE``
(``core/jump_process.py``): an unbiased estimate of ``p(y | theta)`` of the jump process itself, with no time discretisation and no
diffusion approximation, on a state that never leaves the integers.  It is what to fit with when ``diffusion_approximation_check``
says the SDE is not adequate (extinctions, copy numbers of a few units): ``particle_mcmc(..., dynamics="jump")`` runs PMMH on it
for the exact theta posterior of the jump process (Golightly and Wilkinson 2011).

The torch code below is the specification and runs anywhere: any ``ReactionNetworkSDE``, any likelihood, CPU or GPU, fp32 or fp64
theta.  A ``kernel_compatible()`` network with CUDA fp32 theta and observations, a Gaussian or count likelihood of the built-in types
and ``n_particles`` a multiple of 64 up to ``_hip.jump_filter_max_particles`` runs as ONE kernel (csrc/vsde_jump_filter.hip: a
workgroup per theta, a thread per particle) that follows the same rules on the same uniforms with fp32 propensities; every other
case takes the torch route silently, as ``particle_filter`` does.  There are no gradients and there is no ``proposal``: it is the
bootstrap filter.

The rule, for filter ``m`` (``theta_m``, ``N`` particles, all started at the integer ``initial_state``), observation times ``T_0 <=
.. <= T_{K-1}`` (float64; a zero and duplicates are allowed) and ``T_{-1} = 0``:

* segment ``k``, from ``T_{k-1}`` to ``T_k``: particle slot ``j`` is path ``b = m N + j``.  Its float64 clock restarts at exactly
  ``T_{k-1}`` (valid because the waiting times are memoryless) and its events ``e = 0, 1, ..`` follow the event rule of
  ``jump_process`` word for word (``core.jump_process.jump_segment``): propensities and cumulative sums in theta's dtype; a NaN,
  infinite or negative propensity stops the particle (status 2); ``a0 == 0``: absorbed; ``tau = -log(u1) / a0``; the segment ends as
  soon as ``T_k < t + tau``; reaction = the smallest ``j`` with ``u2 a0 < c_j``, else the last with ``a_j > 0``.  The uniforms are
  those of ``philox4x32_10({e >> 1, k, b, 7}, key)``: the jump process's stream with the second counter word carrying the segment,
  so with ``T_0 > 0`` the particles at observation 0 are ``jump_process(net, x0, theta rows repeated N times, [T_0], key=key)``
  bit for bit.  An empty segment is not a special case;
* a particle that has fired ``max_events`` events (counted per particle and per segment) without reaching ``T_k`` stops with
  status 1.  A stopped particle keeps the state it stopped in, its log-weight at observation ``k`` is -inf, and it only carries on
  (from that state, at ``T_k``) if the whole filter is dead.  ``stopped > 0`` therefore biases ``p^`` DOWNWARD by the weight the
  stopped particles would have had: raise ``max_events`` until it is 0;
* observation ``k``: ``lw = log p(y_k | x)`` on the state converted to theta's dtype, NaN counts as -inf; increment, ESS and
  weighted moments before resampling, systematic resampling with ``resampling_uniforms(M, k, key)`` and the dead-filter rule
  (ancestors = identity, increment -inf, ESS 0, moments NaN) are ``particle_filter``'s bootstrap rule unchanged
  (``particle_filter.observation_stage``)."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import torch
from torch import Tensor

from ..core.jump_process import MAX_COPY_NUMBER, MAX_EVENTS_LIMIT, jump_segment
from ..core.observations import COUNT_LIKELIHOODS, GaussianObservationLikelihood, ObservationLikelihood, Observations
from ..core.reaction_network import ReactionNetworkSDE
from ..core.sde import kernel_theta
from . import particle_filter as _pf

HIP_JUMP_FILTER = True   # set False to force the torch route (A/B tests)


@dataclass(frozen=True)
class JumpParticleFilterResult:
    """``log_likelihood [M]``: log p^(y | theta_m) of the jump process given the start state; ``increments [M, K]``: log p^(y_k |
    y_<k, theta_m); ``effective_sample_size [M, K]``; ``filtered_mean`` / ``filtered_std [M, K, S]``: weighted moments of the
    particles before resampling; ``stopped [M, K]`` (int32): the particles of segment k that hit the event cap or an invalid
    propensity (``log_likelihood`` is biased downward while any is positive); ``mean_events [M, K]``: events per particle in segment
    k; and with ``return_particles`` (else None): ``particles [M, K, N, S]`` int32 (before resampling), ``ancestors [M, K, N]``
    int32, ``log_weights [M, K, N]`` and ``events [M, K, N]`` int32."""
    log_likelihood: Tensor
    increments: Tensor
    effective_sample_size: Tensor
    filtered_mean: Tensor
    filtered_std: Tensor
    stopped: Tensor
    mean_events: Tensor
    particles: Optional[Tensor] = None
    ancestors: Optional[Tensor] = None
    log_weights: Optional[Tensor] = None
    events: Optional[Tensor] = None


def integer_initial_state(net, observations, initial_state, n_rows: int, dev) -> Tensor:
    """The start states ``[n_rows, S]`` (int64, on ``dev``) of a jump-process filter: ``initial_state`` (``[S]`` or ``[n_rows,
    S]``, holding integers in ``0 .. 2^30``), by default the first observation if it has the state's dim and is integer-valued."""
    S = int(net.state_dim)
    if initial_state is None:
        if observations.values.shape[1] != S:
            raise ValueError(f"initial_state is required: the observations have dim {observations.values.shape[1]}, the state {S}")
        initial_state = observations.values[0]
        what = "initial_state is required: the first observation does not hold integers"
    else:
        initial_state = torch.as_tensor(initial_state)
        what = "initial_state must hold integers (copy numbers)"
    x0 = initial_state.detach()
    if x0.is_floating_point() and not bool((torch.isfinite(x0) & (x0 == x0.round())).all()):
        raise ValueError(what)
    x0 = x0.to(torch.int64)
    if x0.ndim == 1:
        x0 = x0.unsqueeze(0).expand(n_rows, -1)
    if tuple(x0.shape) != (n_rows, S):
        raise ValueError(f"initial_state [{S}] or [{n_rows}, {S}] expected (state_dim {S}), got {tuple(initial_state.shape)}")
    if bool((x0 < 0).any()) or bool((x0 > MAX_COPY_NUMBER).any()):
        raise ValueError(f"initial_state must lie in 0 .. 2^30, got {int(x0.min())} .. {int(x0.max())}")
    return x0.to(dev)


def _validate(net, observations, theta, n_particles, initial_state, max_events):
    if not isinstance(net, ReactionNetworkSDE):
        raise ValueError("jump_particle_filter needs a ReactionNetworkSDE: the jump process is defined by its reactions")
    if n_particles < 1:
        raise ValueError(f"n_particles must be >= 1, got {n_particles}")
    if not 1 <= int(max_events) <= MAX_EVENTS_LIMIT:
        raise ValueError(f"max_events must be in 1 .. 2^23, got {max_events}")
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
    times = observations.times.detach().to(torch.float64)
    host = times.cpu()
    if not bool(torch.isfinite(host).all()) or bool((host < 0).any()) or bool((host[1:] < host[:-1]).any()):
        raise ValueError("observation times must be finite, >= 0 and non-decreasing")
    return theta, integer_initial_state(net, observations, initial_state, M, theta.device), host


def jump_particle_filter(net: ReactionNetworkSDE, observations: Observations, observation_likelihood: ObservationLikelihood,
                         theta: Tensor, n_particles: int = 1024, initial_state: Optional[Tensor] = None,
                         return_particles: bool = False, key: Optional[Tensor] = None,
                         max_events: int = 2 ** 16) -> JumpParticleFilterResult:
    """Bootstrap particle filters on the exact jump process of ``net`` with ``n_particles`` particles, one per row of ``theta``
    (``[M, P]``, or ``[P]`` for M = 1), all started at ``initial_state`` (``[S]`` or ``[M, S]``, integers in ``0 .. 2^30``; default:
    the first observation, which must then have the state's dim and hold integers).  ``observations.times`` are taken as float64
    (finite, >= 0, non-decreasing).  ``max_events`` (``1 .. 2^23``) is counted per particle and per segment.  ``key``: two int32
    words; default: drawn from torch's generator on theta's device.  The same key gives the same result on a route.  The module
    docstring has the rule.  No gradients."""
    theta, x0, times = _validate(net, observations, theta, n_particles, initial_state, max_events)
    dev = theta.device
    obs = observations if observations.values.device == dev else observations.to(dev)
    key = _pf._call_key(key, dev)
    N, max_events = int(n_particles), int(max_events)
    with torch.no_grad():
        if _kernel_route(net, obs, observation_likelihood, theta, N):
            from .. import _hip
            network = net.kernel_descriptor()
            return JumpParticleFilterResult(*_hip.jump_particle_filter(
                x0.to(torch.int32).contiguous(), kernel_theta(network, theta).contiguous(), times.to(dev),
                *_launch_model(obs, observation_likelihood, theta), key.to(torch.int32) if key.dtype != torch.int32 else key,
                max_events, N, network=network, return_particles=return_particles))
        return _torch_filter(net, obs, observation_likelihood, theta, times, N, x0, return_particles, key, max_events)


def _launch_model(obs, like, theta):
    """``(observed values, obs_matrix in theta's dtype or None, the Gaussian variance or the count likelihood's kernel terms)``."""
    H = like.obs_matrix
    term = like.kernel_terms(obs.values) if type(like) in COUNT_LIKELIHOODS else float(like.variance)
    return obs.values, None if H is None else H.to(theta), term


def _kernel_route(net, obs, like, theta, n_particles) -> bool:
    """Whether the kernel takes the call (the module docstring has the conditions)."""
    if not (HIP_JUMP_FILTER and theta.is_cuda and theta.dtype == torch.float32 and obs.values.dtype == torch.float32):
        return False
    if type(like) not in COUNT_LIKELIHOODS and type(like) is not GaussianObservationLikelihood:
        return False
    if not net.kernel_compatible():
        return False
    from .. import _hip
    S, O, H = int(net.state_dim), obs.values.shape[1], like.obs_matrix
    if O > _hip.PF_MAX_OBS or (H is None and O != S) or (H is not None and tuple(H.shape) != (O, S)):
        return False
    return n_particles % 64 == 0 and n_particles <= _hip.jump_filter_max_particles(S, int(net.num_reactions), not net.plain)


def _torch_filter(net, obs, like, theta, times, N, x0, return_particles, key, max_events) -> JumpParticleFilterResult:
    dev, dtype = theta.device, theta.dtype
    M = theta.shape[0]
    S = x0.shape[1]
    K = times.shape[0]
    rates = theta if net.plain else net.kernel_parameters(theta)
    x = x0[:, None, :].expand(M, N, S).reshape(M * N, S).clone()
    rt = rates[:, None, :].expand(M, N, rates.shape[1]).reshape(M * N, -1)
    b = torch.arange(M * N, device=dev, dtype=torch.int64)          # slot j of filter m is path m N + j
    neg_inf = torch.tensor(float("-inf"), device=dev, dtype=dtype)
    instants = [0.0] + times.tolist()
    incr, ess, means, stds, stop, mean_ev, parts, ancs, lws, evs = [], [], [], [], [], [], [], [], [], []
    for k in range(K):
        x, n_events, status = jump_segment(net, x, rt, instants[k], instants[k + 1], k, b, key, max_events)
        xm = x.to(dtype).reshape(M, N, S)
        lw = like.log_prob(obs.values[k].to(dtype).unsqueeze(0).expand(M * N, -1), xm.reshape(M * N, S)).reshape(M, N)
        lw = torch.where(torch.isnan(lw) | (status != 0).reshape(M, N), neg_inf, lw)
        inc_k, ess_k, mean, std, anc = _pf.observation_stage(lw, xm, k, key)
        incr.append(inc_k)
        ess.append(ess_k)
        means.append(mean)
        stds.append(std)
        stop.append((status != 0).reshape(M, N).sum(dim=1).to(torch.int32))
        mean_ev.append(n_events.reshape(M, N).to(dtype).mean(dim=1))
        if return_particles:
            parts.append(x.reshape(M, N, S).to(torch.int32))
            ancs.append(anc.to(torch.int32))
            lws.append(lw)
            evs.append(n_events.reshape(M, N))
        x = torch.gather(x.reshape(M, N, S), 1, anc[..., None].expand(-1, -1, S)).reshape(M * N, S)
    increments = torch.stack(incr, dim=1)
    opt = lambda rows: torch.stack(rows, dim=1) if return_particles else None
    return JumpParticleFilterResult(
        log_likelihood=increments.sum(dim=1), increments=increments, effective_sample_size=torch.stack(ess, dim=1),
        filtered_mean=torch.stack(means, dim=1), filtered_std=torch.stack(stds, dim=1), stopped=torch.stack(stop, dim=1),
        mean_events=torch.stack(mean_ev, dim=1), particles=opt(parts), ancestors=opt(ancs), log_weights=opt(lws), events=opt(evs))
