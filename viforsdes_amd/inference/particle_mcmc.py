"""Particle MCMC: particle marginal Metropolis-Hastings (PMMH; Andrieu, Doucet and Holenstein 2010) for the exact posterior of the
SDE parameters ``p(theta | y)`` of the Euler-Maruyama-discretised model, whatever its shape.  ``particle_filter`` of this package
returns an unbiased estimate ``p^(y | theta)`` for a batch of theta in one launch; a Metropolis-Hastings chain that uses the
estimate in place of the likelihood, and CARRIES the estimate of its current point instead of refreshing it, still has the exact
posterior as its invariant distribution (the pseudo-marginal argument).  Many independent chains run in lock-step, so one filter
launch per iteration serves all of them, and because the chains are independent the Monte-Carlo error of a posterior mean is simply
the spread of the chain means (``ParticleMCMCResult.mean_standard_error``).  Started from draws of a variational q(theta)
(``VariationalPosterior.refine_parameters``) the chains repair what a mean-field q cannot represent.

The rule.  ``u`` is theta with a log taken on ``theta_positive_dims``; the random walk is symmetric in ``u``.  The log-target of a
chain is ``log p(theta) + sum_{positive dims} u_i + ll`` with ``ll = log mean_r exp(log p^_r)`` over the ``R = filters_per_chain``
independent filters of the same theta (a mean of unbiased estimates is unbiased: the way past the kernel's 1024 particles per
filter).  Iteration ``i = 0, 1, ...`` of chain ``c`` (``C`` chains, ``P`` parameters, ``key``: the call's two words):

1. adaptation (warm-up only, below), then the proposal ``u' = u + step_size L z``: ``L = proposal_scale_tril`` (lower triangular
   ``[P, P]``, shared by the chains), ``z_j`` the Box-Muller normal ``j & 3`` of ``philox4x32_10({i, j >> 2, c, 3}, key)`` by the rule
   of ``particle_filter.stream_normals`` (word pairs (w0, w1), (w2, w3), fp32 uniforms ``((w >> 8) + 0.5) 2^-24``).  Iteration 0
   proposes ``initial_theta`` itself;
2. ``theta'`` from ``u'``, and ONE ``particle_filter`` call on the ``[C R, P]`` rows (filter ``m = c R + r`` has ``theta'_c``; every
   other argument is the caller's) with the key of iteration i: the first two words of ``philox4x32_10({i, 0, 0, 5}, key)``.  The
   current point's estimate is never refreshed: that is what keeps the chain exact;
3. acceptance: ``log alpha = target' - target``; ``log_u = log(((w0 >> 8) + 0.5) 2^-24)`` with ``w0`` the first word of
   ``philox4x32_10({i, 0, c, 4}, key)``.  A proposal whose target is NaN or -inf is rejected; otherwise it is accepted iff
   ``log_u < log alpha`` (a current target of -inf gives ``log alpha = +inf``).  Iteration 0 is accepted unless its target is NaN
   (a chain whose start is refused has target -inf and takes the first proposal with a finite one).  On acceptance ``u``,
   ``target`` and ``ll`` become the proposal's.

Counter words 3, 4 and 5 in the fourth slot: 0, 1 and 2 are the path normals, the resampling uniforms and the smoother's final
draw.  The step uses the call's key, the filters the per-iteration keys; the same key gives the same chains.

Warm-up is the first ``warmup`` iterations, is never returned, and is the only time anything adapts, so the kept chain is a plain
Metropolis-Hastings chain.  Before the proposal of iteration i:

* if ``0 < i <= warmup`` and ``i % adapt_interval == 0``: ``a`` = the pooled acceptance rate of iterations ``[i - adapt_interval,
  i)`` (the only host read in the loop) and ``step_size *= exp(a - target_accept)``;
* once, at ``i = warmup // 2``, with ``adapt=True``, ``C > P`` and ``warmup // 4 < warmup // 2``: ``L`` becomes the lower Cholesky
  factor of the sample covariance of all chains' ``u`` over iterations ``[warmup // 4, warmup // 2)`` plus ``1e-8 I`` (kept as it
  was if that matrix is not positive definite) and ``step_size`` is reset to ``2.38 / sqrt(P)``.

Defaults: ``L = diag(std over chains of the initial u)`` floored at 1e-3 (the identity for C = 1), ``step_size = 2.38 / sqrt(P)``,
and ``target_accept = 0.15`` rather than the 0.234 of a random walk with an exact likelihood: the noise of ``log p^`` makes every
chain reject more at any step size and moves the optimum down (Sherlock, Thiery, Roberts and Rosenthal 2015: about 7 % at the
optimal noise level in high dimension, 15..25 % in the few dimensions of this package's models).  After warm-up every ``thin``-th
state is kept and nothing is read back from the device.

Paths (``return_paths=True``).  PMMH as published (section 2.4.2 of the paper) samples the JOINT posterior ``p(theta, x_{0:T} | y)``:
every proposal also draws one trajectory from its filter's genealogy, accepted or rejected together with theta.  The chain carries
the trajectory as a record of a few numbers per observation (the noise is counter-based, so the states between observations are
recomputed at the end).  With ``N`` particles, ``K`` observations at the grid rows ``rows``, ``fkey_i`` the filter key of iteration i:

4. the filter of step 2 runs with ``return_particles=True``: particles ``X[m, k, j]`` (before resampling at k), ancestors ``a[m, k, j]``;
5. the filter: ``w_r = exp(loglik[c, r] - max_r)``, ``C_r`` its inclusive cumulative sums made non-decreasing by a running maximum,
   ``v0`` and ``v1`` the uniforms ``((w >> 8) + 0.5) 2^-24`` of the first and second word of ``philox4x32_10({i, 0, c, 6}, key)``,
   ``r* = min(#{r : C_r <= v0 C_{R-1}}, R - 1)``, ``m* = c R + r*``: a filter chosen in proportion to its estimate is what keeps the
   average of R estimators exact for the path as well;
6. the final slot: ``J = min(floor(v1 N), N - 1)`` (the product in fp32) and ``lineage[K-1] = a[m*, K-1, J]``: the filter's own
   systematic resampling at the last observation gave offspring slot J the threshold ``(J + u) / N``, uniform on (0, 1] for a
   uniform J, so its ancestor is a draw from the final weights, whatever the weights are made of (no weights, no scan, the same
   for Gaussian, count and bridge weights).  Trace: ``lineage[k-1] = a[m*, k-1, lineage[k]]``, every entry clamped into [0, N - 1];
7. the proposal's record: ``anchors[k] = X[m*, k, lineage[k]]`` (``[K, S]``), ``noise_path[k] = m* N + lineage[k]`` (uint32 ``[K]``),
   ``path_iteration = i``.  A proposal whose ``ll`` is -inf or NaN has a dead record: noise paths 0xFFFFFFFF, anchors NaN;
8. on acceptance the record becomes the chain's with ``u``, ``target`` and ``ll`` (the decision of step 3 is untouched; counter word
   6 in the fourth slot is new); at a kept state whose index is a multiple of ``path_thin`` the record is kept with it;
9. after the loop every kept record is replayed as in ``particle_smoother``: segment k, the grid steps ``rows[k-1] .. rows[k] - 1``
   (segment 0 from step 0 and ``x0[c]``), starts at ``anchors[k-1]``, takes the normals of path ``noise_path[k]`` under the key
   ``fkey_{path_iteration}`` and the theta of the kept state, and runs the filter's steps towards observation k from the anchor (the
   rule: the module docstring of ``particle_filter``; the code: ``particle_filter._segment_propagator``, for every proposal).  The
   state after step t goes to ``paths[.., t + 1]``, ``paths[.., 0] = x0[c]``; a dead record (a chain that never reached a finite
   target) gives NaN paths and ``path_iteration`` -1.

With ``return_paths=False`` nothing of this happens: no store, no launch, no random number.

The torch code below is the specification; it takes any SDE, any likelihood and any prior object with ``log_prob``, runs on CPU or
GPU and follows the dtype of ``initial_theta``.  Where ``particle_filter`` takes its kernel route, ``initial_theta`` is CUDA fp32,
``P <= 16`` and ``prior`` is the package's ``Prior``, everything but the filter runs as ONE kernel per iteration
(csrc/vsde_mcmc.hip, a thread per chain: it closes iteration i - 1 and opens iteration i), and an iteration is that launch, the
rate-law map of a kinetic network, and the filter launch with the device key the step kernel wrote.  With paths the same kernel
draws the record of every chain it accepts from the particles and ancestors the filter launch stored (buffers allocated once), and
ONE replay launch after the loop (csrc/vsde_anchored.hip: ar_kernel, a thread per (observation, record)) turns the kept records
into paths.  ``HIP_MCMC = False`` forces the torch step (around whatever route the filter takes) for A/B.

``dynamics="jump"`` (a ``ReactionNetworkSDE``).  Everything above holds with ONE thing replaced: the estimator of step 2 is
``jump_particle_filter`` (inference/jump_filter.py), the bootstrap filter whose particles are exact trajectories of the network's
jump process, under the same per-iteration key.  The chains then sample the exact theta posterior of the jump process itself
(Golightly and Wilkinson 2011): there is no grid, so ``time_step`` and ``positive_dims`` are not used, ``proposal`` must be
``"bootstrap"`` and the start state must hold integers.  Both loops take it: the torch loop through its estimator slot, the kernel
loop by launching the jump filter's kernel where it launches the SDE filter's, so an iteration is still the step kernel and one
filter launch.

Paths of the jump process (``return_paths=True`` with ``path_times``, float64 ``[Q]`` inside ``[0, T_{K-1}]``; without ``path_times``
it raises: there is no grid to put a path on).  Steps 4-8 hold as they stand on the int32 particles of ``jump_particle_filter``:
the anchors are integers, a dead record is known by its noise paths alone.  Step 9 becomes the replay of
``jump_particle_smoother`` (inference/jump_smoother.py has the rule): segment k starts at ``anchors[k-1]`` (``x0[c]`` for k = 0)
with the clock at exactly ``T_{k-1}``, repeats the events of path ``noise_path[k]`` under ``fkey_{path_iteration}`` with the theta
of the kept state until ``T_k < t + tau``, and every ``t_q`` in ``(T_{k-1}, T_k]`` receives the state after every event with time
``<= t_q``.  ``paths`` is int32 ``[n_path, C, Q, S]``, -1 for a dead record; the ``path_*`` summaries are formed in the chain's dtype.
The torch loop calls ``jump_particle_filter(..., return_particles=True)`` and replays through
``core.jump_process.jump_segment_states``.  The kernel loop hands the step kernel the int32 store and the anchor buffers as raw
32-bit words under an fp32 view: its record half only copies words (the NaN it writes into a dead record's anchors is never read),
so csrc/vsde_mcmc.hip serves unchanged, and ONE launch after the loop (csrc/vsde_jump_replay.hip) makes the paths.  The theta chain
is the same bit for bit with and without paths.

``dynamics="tau_leap"`` (a ``ReactionNetworkSDE``).  Again ONE thing is replaced: the estimator of step 2 is
``tau_leap_particle_filter`` (inference/tau_leap_filter.py) with the step ``time_step``, under the same per-iteration key: the chains
sample the theta posterior of the tau-leap model, at a cost per iteration that does not grow with the population.  ``proposal`` must
be ``"bootstrap"`` and the start state must hold integers; ``positive_dims`` is not used.  There is no tau-leap replay:
``return_paths=True`` and ``path_times`` raise.  Both loops take it: the torch loop through its estimator slot, the kernel loop by
launching the tau-leap filter's kernel (csrc/vsde_tau_leap.hip) where it launches the SDE filter's; the step kernel is untouched."""
from __future__ import annotations

import math
from collections.abc import Sequence
from dataclasses import dataclass
from typing import Any, Optional

import torch
from torch import Tensor

from ..core.observations import ObservationLikelihood, Observations
from ..core.priors import Prior, PriorType
from ..core.sde import SDE, kernel_theta
from . import particle_filter as _pf

HIP_MCMC = True   # set False to force the torch step (A/B tests); the filter keeps its own switch
DEFAULT_TARGET_ACCEPT = 0.15
COVARIANCE_JITTER = 1e-8
DEFAULT_SCALE_FLOOR = 1e-3
# what the filter propagates: the Euler-Maruyama SDE, the exact jump process of a reaction network, or its tau-leap
DYNAMICS = ("diffusion", "jump", "tau_leap")
DEAD_PATH = 0xFFFFFFFF   # noise_path of a record without a path
_ITERATION_HOOK = None   # measurement aid (tools/particle_mcmc_bench.py): called with i at the top of every iteration of either loop


@dataclass(frozen=True)
class ParticleMCMCResult:
    """Draws of the exact parameter posterior of the discretised model by particle MCMC (``particle_mcmc``,
    ``VariationalPosterior.refine_parameters``): ``C`` independent chains, ``n_keep`` kept states each.

    * ``samples [n_keep, C, P]``: theta (constrained); ``log_likelihood [n_keep, C]``: the filter estimate ``ll`` each state
      carried (NOT a fresh estimate); ``log_target [n_keep, C]``: log prior + log Jacobian + ``ll``;
    * ``acceptance_rate [C]``: accepted share of the iterations after warm-up;
    * ``mean``, ``std`` ``[P]`` and ``quantiles`` of theta over all kept draws of all chains;
    * ``mean_standard_error [P]``: the std over chains of the per-chain means divided by sqrt(C) -- the chains are independent, so
      this is the Monte-Carlo error of ``mean`` with no autocorrelation estimate in it (NaN for C = 1);
    * ``r_hat [P]``, ``effective_sample_size [P]``: split-R^ and the multi-chain ESS with Geyer's initial-positive-sequence
      truncation (Gelman et al., BDA3, sections 11.4-11.5), computed in float64 on ``u`` (theta with a log on the positive dims);
      NaN when fewer than 4 states were kept;
    * ``step_size``, ``proposal_scale_tril [P, P]``: the final values (what the kept chain ran with);
    * ``n_filters_dead``: proposals (over the whole run, warm-up included) whose every filter returned -inf -- many of them
      means the filter, not the chain, is the problem: more particles, or ``proposal="bridge"`` / ``"residual_bridge"``;
    * ``variational_mean`` / ``variational_std [P]``: plain moments of the q draws the chains started from
      (``refine_parameters`` only, else None);
    * with ``return_paths=True`` (else None): ``paths [n_path, C, T+1, S]``: the latent path of every ``path_thin``-th kept state
      on the grid, a draw of ``x_{0:T} | y`` JOINTLY with that state's theta; ``path_iteration [n_path, C]`` (int32): the iteration
      whose filter the path came from, -1 for a dead record (its path is NaN); ``path_mean``, ``path_std [T+1, S]`` and
      ``path_quantiles`` over all live draws of all chains; ``path_mean_standard_error [T+1, S]``: the std over chains of the
      per-chain path means divided by sqrt(C) (NaN for C = 1).  With ``dynamics="jump"`` the paths are int32 ``[n_path, C, Q, S]``,
      read at ``path_times [Q]`` (float64; None for diffusion dynamics), -1 for a dead record, and the ``path_*`` fields are
      ``[Q, S]`` in the chain's dtype."""
    samples: Tensor
    log_likelihood: Tensor
    log_target: Tensor
    acceptance_rate: Tensor
    mean: Tensor
    std: Tensor
    quantiles: Any
    mean_standard_error: Tensor
    r_hat: Tensor
    effective_sample_size: Tensor
    step_size: float
    proposal_scale_tril: Tensor
    n_filters_dead: int
    variational_mean: Optional[Tensor] = None
    variational_std: Optional[Tensor] = None
    paths: Optional[Tensor] = None
    path_iteration: Optional[Tensor] = None
    path_mean: Optional[Tensor] = None
    path_std: Optional[Tensor] = None
    path_quantiles: Any = None
    path_mean_standard_error: Optional[Tensor] = None
    path_times: Optional[Tensor] = None


def _words(key: Tensor, c0, c1, c2, c3) -> list[Tensor]:
    k0, k1 = _pf._key_words(key)
    as_t = lambda v: v if isinstance(v, Tensor) else torch.full((1,), int(v), device=key.device, dtype=torch.int64)
    return _pf.philox4x32_10(as_t(c0), as_t(c1), as_t(c2), as_t(c3), k0, k1)


def proposal_normals(n_chains: int, n_params: int, iteration: int, key: Tensor) -> Tensor:
    """The normals ``z [C, P]`` (float64) of iteration ``iteration``: u in fp32, log / sqrt / cos / sin in float64."""
    dev = key.device
    c = torch.arange(n_chains, device=dev, dtype=torch.int64)[:, None]
    blk = torch.arange((n_params + 3) // 4, device=dev, dtype=torch.int64)[None, :]
    return _pf._box_muller(_words(key, iteration, blk, c, 3)).reshape(n_chains, -1)[:, :n_params]


def acceptance_log_uniforms(n_chains: int, iteration: int, key: Tensor) -> Tensor:
    """``log_u [C]`` (float64) of iteration ``iteration``."""
    c = torch.arange(n_chains, device=key.device, dtype=torch.int64)
    return torch.log(_pf._uniform(_words(key, iteration, 0, c, 4)[0]).double())


def filter_key(iteration: int, key: Tensor) -> Tensor:
    """The filter key of iteration ``iteration``: two int32 words."""
    w = _words(key, iteration, 0, 0, 5)
    k = torch.cat([w[0].reshape(1), w[1].reshape(1)])
    return torch.where(k >= 2 ** 31, k - 2 ** 32, k).to(torch.int32)


def filter_keys(iterations: Tensor, key: Tensor) -> Tensor:
    """``filter_key`` for a tensor of iterations ``[...]``: int32 ``[..., 2]`` (a negative iteration, a dead record's, counts as 0)."""
    w = _words(key, iterations.to(device=key.device, dtype=torch.int64).clamp(min=0), 0, 0, 5)
    k = torch.stack([w[0], w[1]], dim=-1)
    return torch.where(k >= 2 ** 31, k - 2 ** 32, k).to(torch.int32)


def path_uniforms(n_chains: int, iteration: int, key: Tensor) -> tuple[Tensor, Tensor]:
    """``(v0, v1)``, fp32 ``[C]`` each: the uniforms of the filter choice and of the final slot of iteration ``iteration``."""
    c = torch.arange(n_chains, device=key.device, dtype=torch.int64)
    w = _words(key, iteration, 0, c, 6)
    return _pf._uniform(w[0]), _pf._uniform(w[1])


def draw_path_records(loglik: Tensor, particles: Tensor, ancestors: Tensor, iteration: int, key: Tensor) -> tuple[Tensor, Tensor]:
    """The path records of the proposals of iteration ``iteration`` (steps 5-7 of the module docstring) from the estimates
    ``loglik [C, R]`` and the store ``particles [C R, K, N, S]``, ``ancestors [C R, K, N]`` of their filters: ``(anchors [C, K, S],
    noise_path [C, K])``, the latter int64 holding uint32 values.  A chain whose estimates are all -inf, or hold a NaN, gets a dead
    record."""
    C, R = loglik.shape
    _, K, N, S = particles.shape
    dev = loglik.device
    v0, v1 = path_uniforms(C, iteration, key)
    mx = loglik.max(dim=1, keepdim=True).values
    dead = ~(mx > float("-inf"))                                         # -inf, or NaN
    w = torch.exp(loglik - torch.where(dead, torch.zeros_like(mx), mx))
    w = torch.where(dead | torch.isnan(w), torch.ones_like(w), w)
    cum = torch.cummax(torch.cumsum(w, dim=1), dim=1).values
    tau = v0.to(w.dtype)[:, None] * cum[:, -1:]
    r = torch.searchsorted(cum.contiguous(), tau.contiguous(), right=True).clamp(max=R - 1)[:, 0]
    m = torch.arange(C, device=dev, dtype=torch.int64) * R + r
    slot = torch.floor(v1 * N).long().clamp(max=N - 1)                  # the product in fp32, as the kernel forms it
    anc = ancestors[m].long().clamp(min=0, max=N - 1)                    # [C, K, N]
    cols = [torch.gather(anc[:, K - 1], 1, slot[:, None])[:, 0]]
    for k in range(K - 1, 0, -1):
        cols.append(torch.gather(anc[:, k - 1], 1, cols[-1][:, None])[:, 0])
    lineage = torch.stack(cols[::-1], dim=1)                             # [C, K]
    anchors = torch.gather(particles[m], 2, lineage[:, :, None, None].expand(C, K, 1, S))[:, :, 0]
    noise = m[:, None] * N + lineage
    return (torch.where(dead[:, :, None], torch.full_like(anchors, float("nan")), anchors),
            torch.where(dead, torch.full_like(noise, DEAD_PATH), noise))


def replay_path_records(sde, obs, like, theta: Tensor, x0: Tensor, anchors: Tensor, noise_path: Tensor, keys: Tensor, dt: float,
                        pos: Sequence[int], bridge: bool, residual: bool = False) -> Tensor:
    """Step 9 of the module docstring in torch: ``paths [B, T+1, S]`` of the records ``(theta [B, P], x0 [B, S], anchors [B, K, S],
    noise_path [B, K] int64, keys [B, 2])``, segment by segment on ``particle_filter._segment_propagator`` like ``particle_smoother``'s torch replay."""
    dev, dtype = theta.device, theta.dtype
    B, K, S = anchors.shape
    rows = torch.round(obs.times / dt).long().tolist()
    T = rows[-1]
    dead = noise_path[:, -1] == DEAD_PATH
    noise = torch.where(dead[:, None], torch.zeros_like(noise_path), noise_path)
    start = torch.where(dead[:, None, None], torch.zeros_like(anchors), anchors)
    advance = _pf._segment_propagator(sde, obs, like, theta, dt, pos, bridge, residual)
    paths = torch.empty(B, T + 1, S, device=dev, dtype=dtype)
    paths[:, 0] = x0
    row_prev = 0
    for k in range(K):
        if rows[k] == row_prev:
            continue
        advance(x0 if k == 0 else start[:, k - 1], theta, row_prev, k, rows[k], noise[:, k], keys, out=paths[:, row_prev + 1:rows[k] + 1])
        row_prev = rows[k]
    return torch.where(dead[:, None, None], torch.full_like(paths, float("nan")), paths)


def log_mean_exp(loglik: Tensor) -> Tensor:
    """``log mean_r exp(loglik[c, r])``: NaN if a row holds a NaN, -inf if all of it is -inf."""
    mx = loglik.max(dim=1, keepdim=True).values          # NaN if any entry is
    safe = torch.where(torch.isneginf(mx), torch.zeros_like(mx), mx)
    return (safe + torch.log(torch.exp(loglik - safe).sum(dim=1, keepdim=True)) - math.log(loglik.shape[1]))[:, 0]


def constrain(u: Tensor, positive_mask: Tensor) -> Tensor:
    return torch.where(positive_mask, u.exp(), u)


def unconstrain(theta: Tensor, positive_mask: Tensor) -> Tensor:
    return torch.where(positive_mask, torch.where(positive_mask, theta, torch.ones_like(theta)).log(), theta)


def _log_prior_jacobian(prior, theta: Tensor, u: Tensor, positive_mask: Tensor) -> Tensor:
    lp = prior.log_prob(theta)
    if lp.ndim > 1:
        lp = lp.sum(dim=-1)
    return lp + torch.where(positive_mask, u, torch.zeros_like(u)).sum(dim=-1)


def _accept(iteration: int, log_u: Tensor, prop_target: Tensor, cur_target: Tensor) -> Tensor:
    ok = ~torch.isnan(prop_target)
    if iteration == 0:
        return ok
    return ok & ~torch.isneginf(prop_target) & (log_u.to(prop_target.dtype) < prop_target - cur_target)


def _close(iteration: int, key: Tensor, loglik: Tensor, prop_u: Tensor, prop_log_prior: Tensor, cur_u: Tensor, cur_target: Tensor,
           cur_loglik: Tensor) -> tuple[Tensor, Tensor, Tensor, Tensor]:
    """The end of iteration ``iteration`` on the torch route: (cur_u, cur_target, cur_loglik, accepted) from the filter estimates
    ``loglik [C, R]`` of the pending proposal."""
    ll = log_mean_exp(loglik)
    target = prop_log_prior + ll
    acc = _accept(iteration, acceptance_log_uniforms(cur_u.shape[0], iteration, key), target, cur_target)
    return (torch.where(acc[:, None], prop_u, cur_u), torch.where(acc, target, cur_target), torch.where(acc, ll, cur_loglik), acc)


def adapted_scale_tril(u_history: Tensor, current: Tensor) -> Tensor:
    """Lower Cholesky factor of the sample covariance of ``u_history [n, P]`` plus ``1e-8 I`` (float64 arithmetic), or ``current``
    when that matrix is not finite and positive definite."""
    P = u_history.shape[1]
    x = u_history.double().cpu()                                         # a [P, P] factorisation, once per run: on the host
    cov = torch.cov(x.T).reshape(P, P) + COVARIANCE_JITTER * torch.eye(P, dtype=torch.float64)
    if not bool(torch.isfinite(cov).all()):
        return current
    factor, info = torch.linalg.cholesky_ex(cov)
    if int(info) != 0 or not bool(torch.isfinite(factor).all()):
        return current
    return torch.tril(factor).to(device=current.device, dtype=current.dtype)


def _validate(sde, observations, observation_likelihood, initial_theta, time_step, n_iterations, warmup, n_particles,
              filters_per_chain, thin, theta_positive_dims, initial_state, proposal, proposal_scale_tril, step_size, target_accept,
              adapt_interval, return_paths=False, path_thin=1, estimator=None, dynamics="diffusion", max_events=2 ** 16,
              path_times=None):
    if dynamics not in DYNAMICS:
        raise ValueError(f"dynamics must be one of {DYNAMICS}, got {dynamics!r}")
    if dynamics == "jump" and proposal != "bootstrap":
        raise ValueError(f"dynamics='jump' runs the bootstrap filter on the jump process: proposal must be 'bootstrap', got {proposal!r}")
    if dynamics == "tau_leap" and proposal != "bootstrap":
        raise ValueError(f"dynamics='tau_leap' runs the bootstrap filter on the tau-leap: proposal must be 'bootstrap', got {proposal!r}")
    if dynamics == "tau_leap" and return_paths:
        raise ValueError("return_paths=True with dynamics='tau_leap': there is no tau-leap replay to make the paths with")
    if dynamics == "jump" and return_paths and path_times is None:
        raise ValueError("return_paths=True with dynamics='jump': a jump process has no grid, path_times (the instants to read the "
                         "paths at) is required")
    if path_times is not None and dynamics != "jump":
        raise ValueError("path_times is for dynamics='jump': the paths of dynamics='diffusion' live on the grid of time_step, and "
                         "dynamics='tau_leap' returns no paths")
    if path_thin < 1:
        raise ValueError(f"path_thin must be >= 1, got {path_thin}")
    if return_paths and estimator is not None:
        raise ValueError("return_paths=True needs the particle filter's store: it cannot be combined with _estimator")
    _pf._proposal_flags(proposal, observation_likelihood)
    if thin < 1 or adapt_interval < 1 or filters_per_chain < 1:
        raise ValueError(f"thin, adapt_interval and filters_per_chain must be >= 1 (got {thin}, {adapt_interval}, {filters_per_chain})")
    if warmup < 0 or n_iterations <= warmup:
        raise ValueError(f"0 <= warmup < n_iterations expected, got warmup {warmup}, n_iterations {n_iterations}")
    if not 0.0 < target_accept < 1.0:
        raise ValueError(f"target_accept must lie in (0, 1), got {target_accept}")
    if step_size is not None and not (step_size > 0 and math.isfinite(step_size)):
        raise ValueError(f"step_size must be positive and finite, got {step_size}")
    if not isinstance(initial_theta, Tensor) or not initial_theta.is_floating_point():
        raise ValueError("initial_theta must be a floating-point tensor [C, P]")
    if initial_theta.ndim == 1:
        initial_theta = initial_theta.unsqueeze(0)
    R = int(filters_per_chain)
    rows = initial_theta.repeat_interleave(R, dim=0) if initial_theta.ndim == 2 else initial_theta
    x0 = initial_state
    if x0 is not None and x0.ndim == 2 and initial_theta.ndim == 2 and x0.shape[0] == initial_theta.shape[0]:
        x0 = x0.repeat_interleave(R, dim=0)
    if dynamics == "jump":
        from . import jump_filter as _jf
        rows, x0, _ = _jf._validate(sde, observations, rows, n_particles, x0, max_events)
    elif dynamics == "tau_leap":
        from . import tau_leap_filter as _tlf
        rows, x0, _ = _tlf._validate(sde, observations, rows, time_step, n_particles, x0)
    else:
        rows, x0 = _pf._validate(sde, observations, rows, time_step, n_particles, x0)
    C, P = initial_theta.shape
    pos = sorted({int(d) for d in theta_positive_dims})
    if any(d < 0 or d >= P for d in pos):
        raise ValueError(f"theta_positive_dims must be in [0, {P}), got {tuple(theta_positive_dims)}")
    mask = torch.zeros(P, dtype=torch.bool)
    mask[pos] = True
    mask = mask.to(initial_theta.device)
    if pos and bool((initial_theta[:, pos] <= 0).any()):
        raise ValueError("initial_theta must be positive on theta_positive_dims")
    if proposal_scale_tril is not None:
        L = torch.as_tensor(proposal_scale_tril)
        if tuple(L.shape) != (P, P):
            raise ValueError(f"proposal_scale_tril [{P}, {P}] expected, got {tuple(L.shape)}")
        Lc = L.detach().double().cpu()
        if not bool(torch.isfinite(Lc).all()) or bool((torch.triu(Lc, 1) != 0).any()) or bool((torch.diagonal(Lc) <= 0).any()):
            raise ValueError("proposal_scale_tril must be finite and lower triangular with a positive diagonal")
    return initial_theta, x0, mask, tuple(pos)


def particle_mcmc(sde: SDE, observations: Observations, observation_likelihood: ObservationLikelihood, prior, time_step: float,
                  initial_theta: Tensor, n_iterations: int, warmup: int = 0, n_particles: int = 512, filters_per_chain: int = 1,
                  thin: int = 1, theta_positive_dims: Sequence[int] = (), positive_dims: Sequence[int] = (),
                  initial_state: Optional[Tensor] = None, proposal: str = "bootstrap", proposal_scale_tril: Optional[Tensor] = None,
                  step_size: Optional[float] = None, adapt: bool = True, target_accept: float = DEFAULT_TARGET_ACCEPT,
                  adapt_interval: int = 25, key: Optional[Tensor] = None, return_paths: bool = False, path_thin: int = 1,
                  _estimator=None, _trace: Optional[list] = None, dynamics: str = "diffusion",
                  max_events: int = 2 ** 16, path_times=None) -> ParticleMCMCResult:
    """``C`` independent PMMH chains, one per row of ``initial_theta [C, P]``, run in lock-step for ``n_iterations`` iterations of
    which the first ``warmup`` adapt and are dropped; every ``thin``-th state after them is kept (the module docstring has the
    rule).  ``prior``: the package's ``Prior`` or any object with ``log_prob(theta [C, P])``; ``theta_positive_dims``: the dims of
    theta that walk in log space (``initial_theta`` must be positive there); ``n_particles``, ``initial_state`` (``[S]`` or
    ``[C, S]``; default: the first observation), ``positive_dims`` (of the state) and ``proposal`` go to ``particle_filter``;
    ``filters_per_chain``: independent filters averaged per proposal; ``proposal_scale_tril``, ``step_size``: the random walk
    ``u' = u + step_size L z`` (defaults in the module docstring); ``adapt``: whether L is re-estimated once in warm-up (the step size
    adapts in warm-up either way); ``key``: two int32 words (default: drawn from torch's generator on theta's device).  The same key
    gives the same chains.  ``return_paths``: every ``path_thin``-th kept state also gets the latent path accepted with it (the
    ``paths`` fields of the result; ``path_thin >= 1``); the theta chain is the same with and without.  No gradients.

    ``dynamics="jump"`` (``sde`` must be a ``ReactionNetworkSDE``): the estimator of every iteration is ``jump_particle_filter``
    under ``filter_key(i, key)``, the bootstrap filter on the exact jump process with ``max_events`` events per particle and
    segment, so the chains target the theta posterior of the jump process itself, with no time step and no diffusion approximation.
    ``time_step`` and ``positive_dims`` are ignored (``None`` is accepted), ``proposal`` must be ``"bootstrap"``, ``initial_state``
    must hold integers in ``0 .. 2^30`` (default: the first observation, if it does).  A jump process has no grid, so
    ``return_paths=True`` needs ``path_times`` (float64 ``[Q]``, ``Q >= 1``, finite, non-decreasing, inside ``[0, T_{K-1}]``; without
    it ``ValueError``): ``paths`` is then int32 ``[n_path, C, Q, S]``, the state after every event with time ``<= t_q``, -1 for a
    dead record, and the result's ``path_times`` holds the instants.  ``path_times`` with ``dynamics="diffusion"`` raises.

    ``dynamics="tau_leap"`` (``sde`` must be a ``ReactionNetworkSDE``): the estimator of every iteration is
    ``tau_leap_particle_filter`` under ``filter_key(i, key)`` with the step ``time_step``: the chains target the theta posterior of
    the tau-leap model (``core/tau_leap.py``), which keeps the integers and the extinctions of the jump process at a cost that does
    not grow with the population.  ``proposal`` must be ``"bootstrap"``, ``initial_state`` must hold integers in ``0 .. 2^30``
    (default: the first observation, if it does), ``positive_dims`` is ignored; ``return_paths=True`` and ``path_times`` raise."""
    theta0, x0, mask, pos_theta = _validate(sde, observations, observation_likelihood, initial_theta, time_step, n_iterations, warmup,
                                            n_particles, filters_per_chain, thin, theta_positive_dims, initial_state, proposal,
                                            proposal_scale_tril, step_size, target_accept, adapt_interval, return_paths, path_thin,
                                            _estimator, dynamics, max_events, path_times)
    jump, tau_leap, estimator_given = dynamics == "jump", dynamics == "tau_leap", _estimator is not None
    jump_paths = None
    if jump and return_paths:
        from . import jump_smoother as _js
        host_times = observations.times.detach().to(torch.float64).cpu()
        t_out = _js.validated_path_times(path_times, host_times)
        jump_paths = (t_out, _js.ownership_ranges(t_out, host_times), host_times)
    dev, dtype = theta0.device, theta0.dtype
    C, P = theta0.shape
    R = int(filters_per_chain)
    obs = observations if observations.values.device == dev else observations.to(dev)
    key = _pf._call_key(key, dev)
    with torch.no_grad():
        u0 = unconstrain(theta0, mask)
        if proposal_scale_tril is not None:
            L = torch.tril(torch.as_tensor(proposal_scale_tril).detach().to(device=dev, dtype=dtype))
        elif C > 1:
            L = torch.diag(u0.std(dim=0).clamp(min=DEFAULT_SCALE_FLOOR))
        else:
            L = torch.eye(P, device=dev, dtype=dtype)
        if jump and not estimator_given and jump_paths is None:
            from .jump_filter import jump_particle_filter
            _estimator = lambda rows, i, fkey: jump_particle_filter(sde, obs, observation_likelihood, rows, n_particles=int(n_particles),
                                                                    initial_state=x0, key=fkey, max_events=int(max_events)).log_likelihood
        if tau_leap and not estimator_given:
            from .tau_leap_filter import tau_leap_particle_filter
            _estimator = lambda rows, i, fkey: tau_leap_particle_filter(sde, obs, observation_likelihood, rows, float(time_step),
                                                                        n_particles=int(n_particles), initial_state=x0, key=fkey).log_likelihood
        run = dict(sde=sde, obs=obs, like=observation_likelihood, prior=prior, dt=0.0 if jump else float(time_step), u0=u0, x0=x0, mask=mask,
                   pos_theta=pos_theta, pos_state=() if jump or tau_leap else tuple(positive_dims), n_iterations=int(n_iterations), warmup=int(warmup),
                   N=int(n_particles), R=R, thin=int(thin), proposal=proposal, L=L,
                   step=float(step_size) if step_size is not None else 2.38 / math.sqrt(P), adapt=bool(adapt) and C > P,
                   target_accept=float(target_accept), interval=int(adapt_interval), key=key, estimator=_estimator, trace=_trace,
                   path_thin=int(path_thin) if return_paths else 0, jump_paths=jump_paths, max_events=int(max_events) if jump else 0, tau_leap=tau_leap)
        route = None
        if HIP_MCMC and not estimator_given and theta0.is_cuda and dtype == torch.float32 and type(prior) is Prior and prior.dim == P:
            from .. import _hip
            if P <= _hip.PMMH_MAX_PARAMS and tau_leap:
                from . import tau_leap_filter as _tlf
                if _tlf._kernel_route(sde, obs, observation_likelihood, theta0.repeat_interleave(R, dim=0), int(n_particles)):
                    route = ("reaction_network", sde.kernel_descriptor())
            elif P <= _hip.PMMH_MAX_PARAMS and not jump:
                route = _pf._kernel_route(sde, obs, observation_likelihood, theta0.repeat_interleave(R, dim=0), int(n_particles), proposal)
            elif P <= _hip.PMMH_MAX_PARAMS:
                from . import jump_filter as _jf
                if _jf._kernel_route(sde, obs, observation_likelihood, theta0.repeat_interleave(R, dim=0), int(n_particles)):
                    route = ("reaction_network", sde.kernel_descriptor())
        out = _torch_loop(**run) if route is None else _kernel_loop(route, **run)
        return _result(*out[:7], mask, *out[7:], path_times=None if jump_paths is None else jump_paths[0].to(dev))


def _adaptation(i, warmup, interval, adapt):
    """(whether the step size adapts, whether L is re-estimated) before the proposal of iteration i."""
    return 0 < i <= warmup and i % interval == 0, adapt and i == warmup // 2 and warmup // 4 < warmup // 2


def _torch_loop(sde, obs, like, prior, dt, u0, x0, mask, pos_theta, pos_state, n_iterations, warmup, N, R, thin, proposal, L, step,
                adapt, target_accept, interval, key, estimator, trace, path_thin=0, jump_paths=None, max_events=0, tau_leap=False):
    dev, dtype = u0.device, u0.dtype
    C, P = u0.shape
    cur_u = u0.clone()
    cur_t = torch.full((C,), float("-inf"), device=dev, dtype=dtype)
    cur_ll = cur_t.clone()
    n_keep = (n_iterations - warmup + thin - 1) // thin
    samples = torch.empty(n_keep, C, P, device=dev, dtype=dtype)
    lls, tgts = torch.empty(n_keep, C, device=dev, dtype=dtype), torch.empty(n_keep, C, device=dev, dtype=dtype)
    window = torch.zeros((), device=dev, dtype=torch.int64)
    kept_acc = torch.zeros(C, device=dev, dtype=torch.int64)
    n_dead = torch.zeros((), device=dev, dtype=torch.int64)
    w4, w2 = warmup // 4, warmup // 2
    history = torch.empty(max(w2 - w4, 0), C, P, device=dev, dtype=dtype) if adapt else None
    if path_thin:
        K, S = obs.values.shape[0], x0.shape[1]
        n_path = (n_keep + path_thin - 1) // path_thin
        # the jump process carries its anchors as integers (a dead record: noise_path = DEAD_PATH, the anchor's contents are irrelevant)
        anchor_dtype = torch.int32 if jump_paths is not None else dtype
        cur_anchor = torch.full((C, K, S), -1 if jump_paths is not None else float("nan"), device=dev, dtype=anchor_dtype)
        cur_noise = torch.full((C, K), DEAD_PATH, device=dev, dtype=torch.int64)
        cur_iter = torch.full((C,), -1, device=dev, dtype=torch.int32)
        anchor_rows, noise_rows = torch.empty(n_path, C, K, S, device=dev, dtype=anchor_dtype), torch.empty(n_path, C, K, device=dev, dtype=torch.int64)
        iter_rows = torch.empty(n_path, C, device=dev, dtype=torch.int32)
    for i in range(n_iterations):
        if _ITERATION_HOOK is not None:
            _ITERATION_HOOK(i)
        adapt_step, adapt_L = _adaptation(i, warmup, interval, adapt)
        if adapt_step:
            step *= math.exp(float(window) / (C * interval) - target_accept)
            window.zero_()
        if adapt_L:
            L = adapted_scale_tril(history.reshape(-1, P), L)
            step = 2.38 / math.sqrt(P)
        prop_u = cur_u + step * (proposal_normals(C, P, i, key).to(dtype) @ L.T) if i > 0 else u0.clone()
        theta = constrain(prop_u, mask)
        prop_lp = _log_prior_jacobian(prior, theta, prop_u, mask)
        rows = theta.repeat_interleave(R, dim=0)
        fkey = filter_key(i, key)
        if estimator is not None:
            loglik = estimator(rows, i, fkey)
        elif jump_paths is not None:
            from .jump_filter import jump_particle_filter
            filtered = jump_particle_filter(sde, obs, like, rows, n_particles=N, initial_state=x0, return_particles=True, key=fkey,
                                            max_events=max_events)
            loglik = filtered.log_likelihood
        else:
            filtered = _pf.particle_filter(sde, obs, like, rows, dt, n_particles=N, initial_state=x0, positive_dims=pos_state, key=fkey,
                                           proposal=proposal, return_particles=bool(path_thin))
            loglik = filtered.log_likelihood
        loglik = loglik.to(dtype).reshape(C, R)
        n_dead += torch.isneginf(loglik).all(dim=1).sum()
        cur_u, cur_t, cur_ll, acc = _close(i, key, loglik, prop_u, prop_lp, cur_u, cur_t, cur_ll)
        if path_thin:
            if jump_paths is not None:
                # the int32 particles as float64 (exact), the anchors back to integers: a dead record's NaN becomes 0
                prop_anchor, prop_noise = draw_path_records(loglik, filtered.particles.double(), filtered.ancestors, i, key)
                prop_anchor = torch.nan_to_num(prop_anchor, nan=0.0).to(torch.int32)
            else:
                prop_anchor, prop_noise = draw_path_records(loglik, filtered.particles, filtered.ancestors, i, key)
            cur_anchor = torch.where(acc[:, None, None], prop_anchor.to(anchor_dtype), cur_anchor)
            cur_noise = torch.where(acc[:, None], prop_noise, cur_noise)
            cur_iter = torch.where(acc, torch.full_like(cur_iter, i), cur_iter)
        window += acc.sum()
        if i >= warmup:
            kept_acc += acc
            if (i - warmup) % thin == 0:
                k = (i - warmup) // thin
                samples[k], lls[k], tgts[k] = constrain(cur_u, mask), cur_ll, cur_t
                if path_thin and k % path_thin == 0:
                    anchor_rows[k // path_thin], noise_rows[k // path_thin], iter_rows[k // path_thin] = cur_anchor, cur_noise, cur_iter
        elif history is not None and w4 <= i < w2:
            history[i - w4] = cur_u
        if trace is not None:
            trace.append(dict(prop_u=prop_u, theta_prop=rows, prop_log_prior=prop_lp, loglik=loglik, accept=acc, cur_u=cur_u,
                              cur_log_target=cur_t, cur_loglik=cur_ll, step_size=step, scale_tril=L, filter_key=fkey))
            if path_thin:
                trace[-1].update(cur_anchor=cur_anchor, cur_noise_path=cur_noise, cur_path_iteration=cur_iter)
    rate = kept_acc.to(dtype) / (n_iterations - warmup)
    out = samples, lls, tgts, rate, step, L, n_dead
    if not path_thin:
        return out
    B = n_path * C
    dead_rows = torch.where(noise_rows[:, :, -1] == DEAD_PATH, torch.full_like(iter_rows, -1), iter_rows)
    if jump_paths is not None:
        from . import jump_smoother as _js
        t_out, q_begin, host_times = jump_paths
        th = samples[::path_thin].reshape(B, P)
        dead = noise_rows.reshape(B, K)[:, -1] == DEAD_PATH
        paths, _, _ = _js.replay_records(sde, th if sde.plain else sde.kernel_parameters(th), x0[::R].repeat(n_path, 1), host_times, t_out,
                                         q_begin, anchor_rows.reshape(B, K, S), torch.where(dead[:, None], 0, noise_rows.reshape(B, K)),
                                         filter_keys(iter_rows.reshape(B), key), max_events, dead)
        return out + (paths.reshape(n_path, C, -1, S), dead_rows)
    paths = replay_path_records(sde, obs, like, samples[::path_thin].reshape(B, P), x0[::R].repeat(n_path, 1), anchor_rows.reshape(B, K, S),
                                noise_rows.reshape(B, K), filter_keys(iter_rows.reshape(B), key), dt, pos_state, proposal != "bootstrap",
                                proposal == "residual_bridge")
    return out + (paths.reshape(n_path, C, -1, S), dead_rows)


def _kernel_loop(route, sde, obs, like, prior, dt, u0, x0, mask, pos_theta, pos_state, n_iterations, warmup, N, R, thin, proposal, L,
                 step, adapt, target_accept, interval, key, estimator, trace, path_thin=0, jump_paths=None, max_events=0,
                 tau_leap=False):
    """The loop with the step kernel: launch i closes iteration i - 1 and opens iteration i, the filter launch follows.  When the
    step size or L changes before iteration i (warm-up only) the proposal is opened again with the new values: the open half is a
    pure function of (state, i, key, step size, L).  With paths the filter stores particles and ancestors into two buffers
    allocated here, launch i draws the records of the chains it accepts from them (the filter launch of iteration i overwrites
    them only afterwards), and one replay launch after the loop turns the kept records into paths.  ``max_events > 0`` (``dynamics="jump"``): the filter
    launch is the jump-process filter's (csrc/vsde_jump_filter.hip); ``tau_leap`` (``dynamics="tau_leap"``): it is the tau-leap filter's
    (csrc/vsde_tau_leap.hip) on the grid of ``dt``; everything else is the same loop."""
    from .. import _hip
    kind, network = route
    dev = u0.device
    C, P = u0.shape
    f32 = dict(device=dev, dtype=torch.float32)
    cur_u, prop_u = u0.clone().contiguous(), u0.clone().contiguous()
    cur_t, cur_ll = torch.full((C,), float("-inf"), **f32), torch.full((C,), float("-inf"), **f32)
    prop_lp, theta_prop = torch.empty(C, **f32), torch.empty(C * R, P, **f32)
    fkey, n_acc = torch.empty(2, device=dev, dtype=torch.int32), torch.zeros(C, device=dev, dtype=torch.int32)
    key = key.to(torch.int32).contiguous()
    n_keep = (n_iterations - warmup + thin - 1) // thin
    samples, lls, tgts = torch.empty(n_keep, C, P, **f32), torch.empty(n_keep, C, **f32), torch.empty(n_keep, C, **f32)
    w4, w2 = warmup // 4, warmup // 2
    history = torch.empty(max(w2 - w4, 0), C, P, **f32) if adapt else None
    L_host = L.detach().float().cpu().contiguous()
    prior_args = (1 if prior.type == PriorType.LOG_NORMAL else 0, float(prior.mean), float(prior.std), pos_theta)
    if tau_leap:
        from ..core.tau_leap import grid_rows
        from . import jump_filter as _jf
        model = _jf._launch_model(obs, like, u0)                           # formed once for every launch of the loop
        leap_rows = grid_rows(obs.times, dt, "observation times").to(device=dev, dtype=torch.int32)
        x0 = x0.to(torch.int32).contiguous()
        filter_launch = lambda: _hip.tau_leap_particle_filter(x0, kernel_theta(network, theta_prop), leap_rows, *model, fkey, dt, N,
                                                              network=network)
    elif max_events:
        from . import jump_filter as _jf
        times, model = obs.times.to(torch.float64), _jf._launch_model(obs, like, u0)   # formed once for every launch of the loop
        x0 = x0.to(torch.int32).contiguous()
        filter_launch = lambda: _hip.jump_particle_filter(x0, kernel_theta(network, theta_prop), times, *model, fkey, max_events, N,
                                                          network=network, store=jump_store)
    else:
        rows, model = _pf._launch_model(obs, like, u0, dt)                 # formed once for every launch of the loop
        x0 = x0.contiguous()
        filter_launch = lambda: _pf._kernel_call("particle_filter", proposal, (kind, x0, kernel_theta(network, theta_prop), rows), model,
                                                 fkey, dt, N, pos_state, network=network, store=store)
    logliks, loglik, window_base, pending = [], None, 0, None
    store = jump_store = None
    if path_thin:
        K, S = obs.values.shape[0], x0.shape[1]
        i32 = dict(device=dev, dtype=torch.int32)
        n_path = (n_keep + path_thin - 1) // path_thin
        if jump_paths is None:
            n_steps = int(round(float(obs.times[-1]) / dt))            # read here: nothing is read back once the loop runs
            store = (torch.empty(C * R, K, N, S, **f32), torch.empty(C * R, K, N, **i32))
        else:
            # the jump filter stores int32 particles; the step kernel's record half only copies 32-bit words, so it gets the same
            # memory as fp32 words, and so do the anchors it writes: integers under an fp32 view.  The NaN it writes into a dead
            # record's anchors is never read: deadness is noise_path
            jump_store = (torch.empty(C * R, K, N, S, **i32), torch.empty(C * R, K, N, **i32))
            store = (jump_store[0].view(torch.float32), jump_store[1])
        cur_anchor, cur_noise = torch.full((C, K, S), float("nan"), **f32), torch.full((C, K), -1, **i32)   # all ones: dead
        cur_iter = torch.full((C,), -1, **i32)
        anchor_rows, noise_rows, iter_rows = torch.empty(n_path, C, K, S, **f32), torch.empty(n_path, C, K, **i32), torch.empty(n_path, C, **i32)

    def step_launch(i, closing, keep=None):
        rows_out = (None, None, None) if keep is None else (samples[keep], lls[keep], tgts[keep])
        if path_thin:
            n = keep // path_thin if keep is not None and keep % path_thin == 0 else None
            record_rows = (None, None, None) if n is None else (anchor_rows[n], noise_rows[n], iter_rows[n])
            _hip.pmmh_step_paths(i, L_host, step, *prior_args, key, closing, cur_u, cur_t, cur_ll, prop_u, prop_lp, theta_prop, fkey, n_acc,
                                 *store, cur_anchor, cur_noise, cur_iter, *rows_out, *record_rows)
            return
        _hip.pmmh_step(i, L_host, step, *prior_args, key, closing, cur_u, cur_t, cur_ll, prop_u, prop_lp, theta_prop, fkey, n_acc,
                       *rows_out)

    for i in range(n_iterations + 1):
        if _ITERATION_HOOK is not None and i < n_iterations:
            _ITERATION_HOOK(i)
        closed = i - 1
        keep = (closed - warmup) // thin if closed >= warmup and (closed - warmup) % thin == 0 else None
        before = n_acc.clone() if trace is not None else None
        step_launch(i, loglik, keep)
        if trace is not None and pending is not None:
            pending.update(accept=(n_acc - before) > 0, cur_u=cur_u.clone(), cur_log_target=cur_t.clone(), cur_loglik=cur_ll.clone())
            if path_thin:
                pending.update(cur_anchor=(cur_anchor.view(torch.int32) if jump_paths is not None else cur_anchor).clone(),
                               cur_noise_path=cur_noise.long() & DEAD_PATH, cur_path_iteration=cur_iter.clone())
            trace.append(pending)
        if i == n_iterations:
            break
        if history is not None and w4 <= closed < w2:
            history[closed - w4].copy_(cur_u)
        adapt_step, adapt_L = _adaptation(i, warmup, interval, adapt)
        if adapt_step:
            total = int(n_acc.sum())                       # the only host read of the loop, in warm-up only
            step *= math.exp((total - window_base) / (C * interval) - target_accept)
            window_base = total
        if adapt_L:
            L = adapted_scale_tril(history.reshape(-1, P), L)
            L_host = L.detach().float().cpu().contiguous()
            step = 2.38 / math.sqrt(P)
        if adapt_step or adapt_L:
            step_launch(i, None)                           # open iteration i again with the new step size / L
        if i == warmup:
            n_acc.zero_()
        loglik = filter_launch()[0].view(C, R)
        logliks.append(loglik)
        if trace is not None:
            pending = dict(prop_u=prop_u.clone(), theta_prop=theta_prop.clone(), prop_log_prior=prop_lp.clone(), loglik=loglik,
                           step_size=step, scale_tril=L, filter_key=fkey.clone())
    n_dead = torch.isneginf(torch.stack(logliks)).all(dim=2).sum()
    rate = n_acc.to(torch.float32) / (n_iterations - warmup)
    out = samples, lls, tgts, rate, step, L, n_dead
    if not path_thin:
        return out
    B = n_path * C
    dead_rows = torch.where(noise_rows[:, :, -1] == -1, torch.full_like(iter_rows, -1), iter_rows)
    if jump_paths is not None:
        t_out, q_begin, _ = jump_paths
        paths, _, _ = _hip.jump_anchored_replay(x0[::R].repeat(n_path, 1), kernel_theta(network, samples[::path_thin].reshape(B, P)), times,
                                                t_out.to(dev), q_begin, anchor_rows.view(torch.int32).view(B, K, S), noise_rows.view(B, K),
                                                filter_keys(iter_rows.view(B), key), max_events, network=network)
        return out + (paths.view(n_path, C, -1, S), dead_rows)
    record = (kind, x0[::R].repeat(n_path, 1), kernel_theta(network, samples[::path_thin].reshape(B, P)), rows)
    paths = _pf._kernel_call("anchored_replay", proposal, record, model, anchor_rows.view(B, K, S), noise_rows.view(B, K),
                             filter_keys(iter_rows.view(B), key), dt, pos_state, network=network, n_steps=n_steps)
    return out + (paths.view(n_path, C, -1, S), dead_rows)


def split_r_hat_and_ess(draws: Tensor) -> tuple[Tensor, Tensor]:
    """Split-R^ and the multi-chain effective sample size of ``draws [n, C, P]`` (n states of C chains), per coordinate, float64
    (Gelman et al., BDA3 sections 11.4-11.5): every chain is split into halves (m = 2 C sequences of length h = n // 2, a middle
    state of an odd n dropped), ``W`` the mean within-sequence variance, ``B / h`` the variance of the sequence means,
    ``var+ = (h - 1) / h W + B / h``, ``R^ = sqrt(var+ / W)``; with the variogram ``V_t`` (mean squared difference at lag t over all
    sequences), ``rho_t = 1 - V_t / (2 var+)`` and ``T`` the first odd lag at which ``rho_{T+1} + rho_{T+2} < 0``,
    ``ESS = m h / (1 + 2 sum_{t=1..T} rho_t)``.  NaN for n < 4 or a coordinate that does not move."""
    n, C, P = draws.shape
    nan = torch.full((P,), float("nan"), dtype=torch.float64, device=draws.device)
    if n < 4:
        return nan, nan.clone()
    h = n // 2
    x = torch.cat([draws[:h], draws[n - h:]], dim=1).double()           # [h, m, P]
    m = x.shape[1]
    means = x.mean(dim=0)                                                # [m, P]
    W = x.var(dim=0, unbiased=True).mean(dim=0)                          # [P]
    B_over_h = means.var(dim=0, unbiased=True) if m > 1 else torch.zeros_like(W)
    var_plus = (h - 1) / h * W + B_over_h
    r_hat = torch.sqrt(var_plus / W)
    xc = x - means[None]
    sq = (xc * xc).cumsum(dim=0)                                         # [h, m, P]
    total = sq[-1]
    f = torch.fft.rfft(xc, n=2 * h, dim=0)
    acov = torch.fft.irfft(f * f.conj(), n=2 * h, dim=0)[:h]            # sum_i xc_i xc_{i-t}
    rho = torch.ones(h, P, dtype=torch.float64, device=draws.device)
    for t in range(1, h):
        # sum_i (x_i - x_{i-t})^2 = sum_{i >= t} x_i^2 + sum_{i < h - t} x_i^2 - 2 sum_i x_i x_{i-t}
        s = (total - sq[t - 1]) + sq[h - t - 1] - 2.0 * acov[t]
        rho[t] = 1.0 - (s.sum(dim=0) / (m * (h - t))) / (2.0 * var_plus)
    n_pairs = (h - 2) // 2                                               # pairs (rho_{2k}, rho_{2k+1}), k = 1 .. n_pairs
    tau = 1.0 + 2.0 * rho[1] if h > 1 else torch.ones_like(W)
    if n_pairs > 0:
        pairs = rho[2:2 + 2 * n_pairs].reshape(n_pairs, 2, P).sum(dim=1)
        alive = torch.cumprod((pairs >= 0).to(torch.float64), dim=0)
        tau = tau + 2.0 * (pairs * alive).sum(dim=0)
    ess = m * h / tau
    return r_hat, torch.where(torch.isfinite(r_hat), ess, nan)


def _path_fields(paths: Tensor, path_iteration: Tensor, dtype=None) -> dict:
    """The ``path_*`` fields of the result from ``paths [n_path, C, T+1, S]``: moments and quantiles over the live draws, in
    ``dtype`` (the chain's; the integer paths of the jump process are converted for them, ``paths`` itself stays as it is)."""
    from ..posterior.variational_posterior import _QUANTILE_MAX_ELEMENTS, QUANTILE_LEVELS, Quantiles
    kept = paths
    if dtype is not None and paths.dtype != dtype:
        paths = paths.to(dtype)
    n_path, C, T1, S = paths.shape
    live = path_iteration >= 0                                           # [n_path, C]
    flat = paths.reshape(n_path * C, T1 * S)[live.reshape(-1)]
    nan = torch.full((T1, S), float("nan"), device=paths.device, dtype=paths.dtype)
    fields = dict(paths=kept, path_iteration=path_iteration, path_mean=nan, path_std=nan, path_mean_standard_error=nan,
                  path_quantiles=Quantiles(*([nan] * len(QUANTILE_LEVELS))))
    if flat.shape[0] == 0:
        return fields
    levels = torch.tensor(QUANTILE_LEVELS, device=paths.device, dtype=paths.dtype)
    cols = max(1, _QUANTILE_MAX_ELEMENTS // flat.shape[0])
    q = torch.cat([torch.quantile(flat[:, c:c + cols], levels, dim=0) for c in range(0, flat.shape[1], cols)], dim=1)
    fields.update(path_mean=flat.mean(dim=0).reshape(T1, S), path_quantiles=Quantiles(*q.reshape(len(QUANTILE_LEVELS), T1, S).unbind(0)),
                  path_std=flat.std(dim=0).reshape(T1, S) if flat.shape[0] > 1 else torch.zeros_like(nan))
    if C > 1:
        w = live[:, :, None, None].to(paths.dtype)
        chain_means = torch.where(live[:, :, None, None], paths, torch.zeros_like(paths)).sum(dim=0) / w.sum(dim=0)   # NaN: no live draw
        fields.update(path_mean_standard_error=chain_means.std(dim=0) / math.sqrt(C))
    return fields


def _result(samples, lls, tgts, rate, step, L, n_dead, mask, paths=None, path_iteration=None, path_times=None) -> ParticleMCMCResult:
    from ..posterior.variational_posterior import QUANTILE_LEVELS, Quantiles
    n_keep, C, P = samples.shape
    flat = samples.reshape(n_keep * C, P)
    levels = torch.tensor(QUANTILE_LEVELS, device=samples.device, dtype=samples.dtype)
    nan = torch.full((P,), float("nan"), device=samples.device, dtype=samples.dtype)
    chain_means = samples.mean(dim=0)
    r_hat, ess = (t.to(samples.device) for t in split_r_hat_and_ess(unconstrain(samples, mask).double().cpu()))
    return ParticleMCMCResult(
        samples=samples, log_likelihood=lls, log_target=tgts, acceptance_rate=rate, mean=flat.mean(dim=0),
        std=flat.std(dim=0) if flat.shape[0] > 1 else torch.zeros_like(nan), quantiles=Quantiles(*torch.quantile(flat, levels, dim=0).unbind(0)),
        mean_standard_error=chain_means.std(dim=0) / math.sqrt(C) if C > 1 else nan, r_hat=r_hat, effective_sample_size=ess,
        step_size=float(step), proposal_scale_tril=L, n_filters_dead=int(n_dead),
        **({} if paths is None else _path_fields(paths, path_iteration, samples.dtype)), path_times=path_times)
