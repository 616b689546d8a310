"""Result object of ``infer`` (reference: posterior/variational_posterior.py:23-192): sampling with
the EMA weights, summaries, diagnostics and the on-disk checkpoint

    {model_state, ema_state, time_horizon, time_step, state_positive_dims, evidence_lower_bound_history}

which is byte-compatible with the reference's ``torch.save`` layout (same keys, same tensors)."""
from __future__ import annotations

import math
import os

from dataclasses import dataclass
from pathlib import Path
from typing import Optional

import torch
from pydantic import BaseModel, ConfigDict
from torch import Tensor

from ..core.observations import ObservationLikelihood, Observations
from ..core.priors import Prior
from ..core.sde import SDE
from ..inference import diffusion_path_sampler as _sampler
from ..inference.diffusion_path_sampler import CapturedPathSampler, sample_diffusion_paths
from ..inference.exponential_moving_average import ExponentialMovingAverage
from ..inference.state_space import StateSpace
from ..models.variational_sde_posterior import VariationalSDEPosterior

QUANTILE_LEVELS = (0.05, 0.25, 0.5, 0.75, 0.95)


@dataclass(frozen=True)
class VariationalPosteriorSamples:
    sde_parameters: Tensor
    diffusion_paths: Tensor


@dataclass(frozen=True)
class Quantiles:
    q05: Tensor
    q25: Tensor
    q50: Tensor
    q75: Tensor
    q95: Tensor


@dataclass
class VariationalPosteriorSummary:
    sde_parameter_mean: Tensor
    sde_parameter_std: Tensor
    sde_parameter_quantiles: Quantiles
    diffusion_path_mean: Tensor
    diffusion_path_std: Tensor


@dataclass
class InferenceDiagnostics:
    evidence_lower_bound_history: list[float]
    final_evidence_lower_bound: float
    n_iterations: int


@dataclass(frozen=True)
class EvidenceEstimate:
    """Importance-sampled estimate of the log evidence ``log p(y)`` of the Euler-Maruyama-discretised model (start state = first
    observation), from ``n_samples`` posterior draws with log-weights ``log w`` (``VariationalPosterior.log_evidence``):

    * ``log_evidence = logsumexp(log w) - log n``;
    * ``effective_sample_size = (sum w)^2 / sum w^2`` in ``[0, n]``;
    * ``standard_error = sqrt(1 / ESS - 1 / n)``: delta-method standard error of ``log_evidence``;
    * ``evidence_lower_bound = mean(log w)`` on the same draws (``<= log_evidence``);
    * ``n_nonfinite``: NaN (or +inf) log-weights; if any, every estimate above is NaN.  ``-inf`` weights are zero weights.
    ``log_weights``: the ``[n]`` log-weights when asked for, else None."""
    log_evidence: float
    standard_error: float
    effective_sample_size: float
    evidence_lower_bound: float
    n_samples: int
    n_nonfinite: int
    log_weights: Optional[Tensor] = None

    @classmethod
    def from_state(cls, state, log_weights: Optional[Tensor] = None) -> "EvidenceEstimate":
        """Finalise the accumulator state ``[M, sum exp(lw - M), sum exp(2 (lw - M)), sum lw, n, n_nonfinite]`` (float64,
        ``_hip.log_weight_accumulate``)."""
        m, s1, s2, sum_lw, n, bad = (float(v) for v in state)
        n_i, bad_i = int(round(n)), int(round(bad))
        if bad_i > 0:
            nan = float("nan")
            return cls(nan, nan, nan, nan, n_i, bad_i, log_weights)
        if s1 == 0.0:    # every weight is zero
            return cls(float("-inf"), float("inf"), 0.0, sum_lw / n, n_i, 0, log_weights)
        ess = s1 * s1 / s2
        return cls(m + math.log(s1) - math.log(n), math.sqrt(max(1.0 / ess - 1.0 / n, 0.0)), ess, sum_lw / n, n_i, 0,
                   log_weights)


_QUANTILE_MAX_ELEMENTS = 1 << 24   # torch.quantile refuses larger inputs: wider tensors are taken in column blocks


@dataclass(frozen=True)
class PosteriorPredictive:
    """Posterior predictive draws (``VariationalPosterior.predict``): ``n`` joint draws of theta and the model state at
    ``times`` -- read from the posterior path inside the time horizon, and the model SDE continued from that path's end state
    with the same theta after it -- and, when an observation likelihood was given, one fresh observation of every state.

    ``times [K]``, ``sde_parameters [n, P]``, ``states [n, K, S]``, ``observations [n, K, O]`` or None."""
    times: Tensor
    sde_parameters: Tensor
    states: Tensor
    observations: Optional[Tensor] = None

    def _draws(self, observations: bool) -> Tensor:
        if not observations:
            return self.states
        if self.observations is None:
            raise ValueError("no observation draws: predict() was called without an observation_likelihood")
        return self.observations

    def quantiles(self, observations: bool = False) -> Quantiles:
        """Per-time, per-dimension quantiles ``[K, S]`` (``[K, O]`` for the observations) at the levels ``summary()`` uses."""
        v = self._draws(observations)
        levels = torch.tensor(QUANTILE_LEVELS, device=v.device, dtype=v.dtype)
        flat = v.reshape(v.shape[0], -1)
        cols = max(1, _QUANTILE_MAX_ELEMENTS // flat.shape[0])
        q = torch.cat([torch.quantile(flat[:, c:c + cols], levels, dim=0) for c in range(0, flat.shape[1], cols)], dim=1)
        return Quantiles(*q.reshape(len(QUANTILE_LEVELS), *v.shape[1:]).unbind(0))

    def mean(self, observations: bool = False) -> Tensor:
        return self._draws(observations).mean(dim=0)

    def std(self, observations: bool = False) -> Tensor:
        return self._draws(observations).std(dim=0)


@dataclass(frozen=True)
class ParameterReweighting:
    """Check of q(theta) alone (``VariationalPosterior.reweight_parameters``): ``n_samples`` draws theta ~ q with importance weights
    ``log w = log p(theta) + log p^(y | theta) - log q(theta)``, the marginal likelihood estimated by a bootstrap particle filter
    (unbiased, so the weights are proper although noisy).  Neither the encoder nor the head enters.

    * ``log_evidence``, ``standard_error``, ``effective_sample_size``, ``n_nonfinite``: as in ``EvidenceEstimate``; a second,
      independent estimate of the ``log p(y)`` that ``log_evidence()`` estimates.  The ESS says how far q(theta) is from the exact
      theta posterior (the filter's own noise lowers it further);
    * ``mean``, ``std`` ``[P]`` and ``quantiles`` of theta under the normalised weights (the quantile at level a is the smallest
      draw whose cumulative normalised weight, in sorted order, reaches a), next to ``variational_mean`` / ``variational_std``, the
      plain moments of the same draws;
    * ``filter_effective_sample_size [n]``: the smallest particle ESS seen in each draw's filter -- near 1 the bootstrap filter
      itself is starved (sharply informative observations) and ``log p^`` is noisy: rerun with ``proposal="bridge"``;
    * ``sde_parameters [n, P]``, ``log_likelihood [n]``, ``log_weights [n]`` (float64) when asked for, else None."""
    log_evidence: float
    standard_error: float
    effective_sample_size: float
    n_samples: int
    n_nonfinite: int
    mean: Tensor
    std: Tensor
    quantiles: Quantiles
    variational_mean: Tensor
    variational_std: Tensor
    filter_effective_sample_size: Tensor
    sde_parameters: Optional[Tensor] = None
    log_likelihood: Optional[Tensor] = None
    log_weights: Optional[Tensor] = None


@dataclass(frozen=True)
class PathReweighting:
    """Importance sample of the exact joint posterior ``p(theta, x_{0:T} | y)`` of the Euler-Maruyama-discretised model
    (``VariationalPosterior.smooth_paths``): ``n_samples`` draws theta ~ q, one smoothed path per theta from the genealogy of the
    particle filter that estimated ``p^(y | theta)`` (``particle_smoother``), and the weights ``p(theta) p^(y | theta) / q(theta)`` of
    ``ParameterReweighting`` -- proper for the pair, because the path comes from the same filter that made ``p^``.  No network enters:
    set ``path_mean`` / ``path_std`` beside ``summary().diffusion_path_mean`` / ``diffusion_path_std``.

    * ``log_evidence``, ``standard_error``, ``effective_sample_size``, ``n_samples``, ``n_nonfinite``,
      ``filter_effective_sample_size [n]``: as in ``ParameterReweighting`` (the same numbers under the same seed);
    * ``times [T+1]``: the grid; ``path_mean``, ``path_std`` ``[T+1, S]`` and ``path_quantiles`` (each ``[T+1, S]``) of the paths
      under the normalised weights, by the weighted-quantile rule of ``ParameterReweighting``; NaN where no estimate exists;
    * ``paths [n, T+1, S]``, ``sde_parameters [n, P]``, ``log_weights [n]`` (float64) when asked for, else None.  The path of a
      draw whose filter died is NaN and its weight zero."""
    log_evidence: float
    standard_error: float
    effective_sample_size: float
    n_samples: int
    n_nonfinite: int
    filter_effective_sample_size: Tensor
    times: Tensor
    path_mean: Tensor
    path_std: Tensor
    path_quantiles: Quantiles
    paths: Optional[Tensor] = None
    sde_parameters: Optional[Tensor] = None
    log_weights: Optional[Tensor] = None


def _weighted_quantiles(values: Tensor, wn: Tensor) -> Tensor:
    """``[levels, C]``: per column of ``values [n, C]`` the smallest value whose cumulative normalised weight ``wn [n]``, in sorted
    order, reaches each of QUANTILE_LEVELS."""
    order = torch.argsort(values, dim=0)
    cdf = torch.cumsum(wn[order], dim=0)                                    # [n, C]: cumulative weight in each column's sorted order
    levels = torch.tensor(QUANTILE_LEVELS, device=values.device, dtype=values.dtype)
    first = (cdf[None, :, :] < levels[:, None, None]).sum(dim=1).clamp(max=values.shape[0] - 1)    # [levels, C]
    return torch.gather(torch.gather(values, 0, order), 0, first)


class VariationalPosteriorCheckpoint(BaseModel):
    model_config = ConfigDict(frozen=True, arbitrary_types_allowed=True)
    model_state: dict[str, Tensor]
    ema_state: dict[str, Tensor]
    time_horizon: float
    time_step: float
    state_positive_dims: list[int]
    evidence_lower_bound_history: list[float]


class VariationalPosterior:
    def __init__(self, model: VariationalSDEPosterior, exponential_moving_average: ExponentialMovingAverage,
                 prior: Prior, observations: Observations, time_horizon: float, time_step: float,
                 state_space: StateSpace, evidence_lower_bound_history: list[float], device: torch.device) -> None:
        self.model = model.to(device)
        self.exponential_moving_average = exponential_moving_average
        self.prior, self.observations = prior, observations.to(device)
        self.time_horizon, self.time_step, self.state_space = time_horizon, time_step, state_space
        self.evidence_lower_bound_history = evidence_lower_bound_history
        self.device = device
        self._calls: dict[tuple, int] = {}                                  # sample() calls seen per (n, autocast dtype)
        self._captured: dict[tuple, Optional[CapturedPathSampler]] = {}     # -> replayable call (None: capture failed, stay eager)
        self._capture_failure_logged = False
        # sample(n) is replayed from a HIP graph from its second call on, for n up to this many samples (a graph pins the call's
        # peak memory: ~0.5 GB at 512 Lotka-Volterra paths); 0 = always eager.  release_graphs() frees the pools.
        self.graph_max_samples = int(os.environ.get("VSDE_SAMPLE_GRAPH_MAX", "1024"))

    @torch.no_grad()
    def sample(self, n: int, mixed_precision: bool = False) -> VariationalPosteriorSamples:
        """n joint draws (theta, path) from the variational posterior using the EMA weights.

        On the GPU a repeated ``sample(n)`` with the same ``n`` (a serving loop) replays the call as ONE HIP graph from its
        second occurrence on (``CapturedPathSampler``: same kernels, same RNG stream order -- theta draw, then the path noise --
        fresh draws per call; ``VSDE_SAMPLE_GRAPH=0`` keeps every call eager).  The first call of a size runs eagerly.
        ``mixed_precision`` (not in the reference, whose ``sample`` always runs in the parameters' precision): run the encoder
        under bf16 autocast, i.e. in the precision a ``mixed_precision`` training run optimised it in -- the fused encoder
        kernels instead of fp32 library GEMMs (~5 x faster at the Lotka-Volterra size); the head stays fp32."""
        self.model.eval()
        amp = torch.bfloat16 if (mixed_precision and self.device.type == "cuda") else None
        with self.exponential_moving_average.apply():
            replay = self._replayable(n, amp)
            if replay is not None:
                theta, x, _ = replay()
                return VariationalPosteriorSamples(sde_parameters=theta.clone(), diffusion_paths=x.clone())
            theta = self.model.sde_parameter_posterior.rsample(n)
            x0 = self.observations.values[0].unsqueeze(0).expand(n, -1)
            with torch.autocast(device_type=self.device.type, dtype=amp, enabled=amp is not None):
                drawn = sample_diffusion_paths(self.model.encoder, self.model.head, self.observations, theta, x0,
                                               self.time_horizon, self.time_step, self.state_space)
            return VariationalPosteriorSamples(sde_parameters=theta, diffusion_paths=drawn.x)

    def _replayable(self, n: int, amp: Optional[torch.dtype] = None) -> Optional[CapturedPathSampler]:
        if self.device.type != "cuda" or not _sampler.SAMPLE_GRAPH:
            return None
        if self._captured and not getattr(self, "_range_flag_seen", False) and CapturedPathSampler.kernel_choice_outdated():
            self._range_flag_seen = True   # captured with the MFMA GRU kernels, which a weight has outgrown: capture again (fp32 kernels)
            self._captured.clear()
        key = (n, amp)
        self._calls[key] = self._calls.get(key, 0) + 1
        if self._calls[key] < 2:
            return None
        if n > self.graph_max_samples:     # a captured call pins the peak memory of one sampling call at this size for good
            return None
        if key not in self._captured:
            if len(self._captured) >= 2:   # each graph keeps a private memory pool: two sizes at most (oldest goes first)
                self._captured.pop(next(iter(self._captured)))
            try:
                self._captured[key] = CapturedPathSampler(self.model, self.observations, self.time_horizon, self.time_step,
                                                          self.state_space, n, autocast_dtype=amp, warmup=1)
            except Exception as err:   # capture is an optimisation, never a requirement -- but a persistent fallback must be visible
                self._captured[key] = None
                if not self._capture_failure_logged:
                    self._capture_failure_logged = True
                    import logging
                    logging.getLogger("viforsdes_amd").warning(
                        "VariationalPosterior.sample(%d): HIP graph capture failed (%s: %s); sampling eagerly", n, type(err).__name__, err)
        return self._captured[key]

    def release_graphs(self) -> None:
        """Drop the captured sampling calls and their private memory pools (they are re-captured on demand)."""
        self._captured.clear()
        self._calls.clear()
        if self.device.type == "cuda":
            torch.cuda.empty_cache()

    @torch.no_grad()
    def log_evidence(self, sde: SDE, observation_likelihood: ObservationLikelihood, n_samples: int = 4096, chunk_size: int = 512,
                     mixed_precision: bool = False, return_log_weights: bool = False) -> EvidenceEstimate:
        """Importance-sampled log evidence ``log p(y)`` of the model (``sde``, ``observation_likelihood``, the prior) with the
        variational posterior as proposal, for model comparison (``log_evidence`` +- ``standard_error``) and as a fit
        diagnostic (``effective_sample_size``).

        The evidence is that of the Euler-Maruyama-discretised model on this posterior's time grid, conditioned -- like the
        ELBO -- on the start state being the first observation (``x0 = y0``).  Draws use the EMA weights, as ``sample()`` does,
        ``chunk_size`` paths at a time (the last chunk is drawn in full; only the first ``n_samples`` weights count).  The first
        chunk is drawn eagerly, the others replay a captured sampling call that this call owns (``sample()``'s graphs are not
        touched).  Per chunk: draw, one log-weight kernel, one accumulate kernel into an fp64 state on the device; the host
        synchronises once, at the end.  ``mixed_precision``: run the encoder under bf16 autocast, as ``sample()`` does; the
        weights stay exact for the paths drawn, since they use the head's own transition means / Cholesky factors.
        ``return_log_weights``: keep the ``[n_samples]`` log-weights (device tensor) in the result."""
        from .. import _hip
        from ..inference.evidence import importance_log_weights
        if n_samples < 1 or chunk_size < 1:
            raise ValueError(f"n_samples and chunk_size must be >= 1 (got {n_samples}, {chunk_size})")
        state = _hip.log_weight_state(self.device)   # raises HipLibraryError off the GPU: there is no CPU implementation
        n_chunks = -(-n_samples // chunk_size)
        kept = torch.empty(n_samples, device=self.device, dtype=torch.float32) if return_log_weights else None
        self.model.eval()
        amp = torch.bfloat16 if mixed_precision else None
        model = self.model
        sampler = None
        with self.exponential_moving_average.apply():
            for c in range(n_chunks):
                count = min(chunk_size, n_samples - c * chunk_size)
                if c > 0 and sampler is None:
                    sampler = self._evidence_sampler(chunk_size, amp)
                if sampler:
                    theta, _, drawn = sampler()
                else:
                    theta = model.sde_parameter_posterior.rsample(chunk_size)
                    x0 = self.observations.values[0].unsqueeze(0).expand(chunk_size, -1)
                    with torch.autocast(device_type=self.device.type, dtype=amp, enabled=amp is not None):
                        drawn = sample_diffusion_paths(model.encoder, model.head, self.observations, theta, x0, self.time_horizon,
                                                       self.time_step, self.state_space)
                log_w = importance_log_weights(sde, self.observations, observation_likelihood, self.prior,
                                               model.sde_parameter_posterior, theta, drawn, self.time_step)
                _hip.log_weight_accumulate(log_w, count, state)
                if kept is not None:
                    kept[c * chunk_size:c * chunk_size + count].copy_(log_w[:count])
        del sampler
        return EvidenceEstimate.from_state(state.tolist(), kept)

    def _evidence_sampler(self, n: int, amp: Optional[torch.dtype], caller: str = "log_evidence"):
        """A captured sampling call of ``n`` paths owned by one ``log_evidence`` (or ``predict``) call (kept out of ``sample()``'s
        caches), or False when capture is off or fails (the chunks are then drawn eagerly: same kernels, same draws)."""
        if not _sampler.SAMPLE_GRAPH:
            return False
        try:
            return CapturedPathSampler(self.model, self.observations, self.time_horizon, self.time_step, self.state_space, n,
                                       autocast_dtype=amp, warmup=1)
        except Exception as err:
            import logging
            logging.getLogger("viforsdes_amd").warning(
                "VariationalPosterior.%s: HIP graph capture of %d paths failed (%s: %s); sampling eagerly", caller, n,
                type(err).__name__, err)
            return False

    @torch.no_grad()
    def predict(self, sde: SDE, times, n_samples: int = 1000, observation_likelihood: Optional[ObservationLikelihood] = None,
                chunk_size: int = 512, mixed_precision: bool = False) -> PosteriorPredictive:
        """Posterior predictive draws of the state at ``times`` (1-D, sorted, >= 0) and, with ``observation_likelihood``, of
        fresh observations of it: what the fitted model says about the process inside the data window and after it.

        Each of the ``n_samples`` draws pairs a theta with its own posterior path, as ``sample()`` does (EMA weights, same RNG
        order: the theta draw, then the path noise).  A time maps to the grid step ``round(t / time_step)`` (the rule of
        ``grid_index``).  Steps inside the horizon are read from the path; steps after it come from the model SDE ``sde``
        continued from the path's end state with the draw's theta (``forecast_states``: one launch over all draws for a built-in
        SDE; the positive state dims are clamped at 1e-6 as in ``euler_maruyama``).  Paths are drawn ``chunk_size`` at a time,
        as in ``log_evidence``: the first chunk eagerly, the others by replaying a captured sampling call that this call owns
        (``sample()``'s graphs are not touched).  Then one forecast key, then the observation noise, are drawn.
        ``observation_likelihood`` needs a ``sample(state)`` method (the package's Gaussian, Poisson and negative-binomial ones have one).
        ``mixed_precision``: run the encoder under bf16 autocast, as ``sample()`` does."""
        from .. import _hip
        from ..core.forecast import forecast_states
        times = times if isinstance(times, Tensor) else torch.as_tensor(times, dtype=torch.float32)
        if times.ndim != 1 or times.numel() < 1:
            raise ValueError(f"times must be a non-empty 1-D tensor, got shape {tuple(times.shape)}")
        times = times.detach().cpu()
        if not times.is_floating_point():
            times = times.float()
        if not bool(torch.isfinite(times).all()) or bool((times < 0).any()) or bool((times[1:] < times[:-1]).any()):
            raise ValueError("times must be finite, >= 0 and sorted in non-decreasing order")
        if n_samples < 1 or chunk_size < 1:
            raise ValueError(f"n_samples and chunk_size must be >= 1 (got {n_samples}, {chunk_size})")
        S, P = self.state_space.dim, self.model.sde_parameter_posterior.sde_param_dim
        if sde.state_dim != S or sde.sde_param_dim != P:
            raise ValueError(f"sde has state_dim {sde.state_dim}, sde_param_dim {sde.sde_param_dim}; the posterior has {S}, {P}")
        like = observation_likelihood
        if like is not None and not callable(getattr(like, "sample", None)):
            raise TypeError(f"{type(like).__name__} has no sample(state) method: observations cannot be drawn from it")
        if self.device.type != "cuda":
            raise _hip.HipLibraryError("VariationalPosterior.predict draws paths with the HIP kernels; there is no CPU implementation")
        dev, dt = self.device, self.time_step
        n_steps = round(self.time_horizon / dt)
        steps = torch.round(times / dt).long()
        n_in = int((steps <= n_steps).sum())
        rows_in = steps[:n_in].to(dev)
        chunk = min(chunk_size, n_samples)
        theta_all = torch.empty(n_samples, P, device=dev)
        ends = torch.empty(n_samples, S, device=dev)
        inside = torch.empty(n_samples, n_in, S, device=dev)
        self.model.eval()
        amp = torch.bfloat16 if mixed_precision else None
        model = self.model
        sampler = None
        with self.exponential_moving_average.apply():
            for c in range(-(-n_samples // chunk)):
                lo, count = c * chunk, min(chunk, n_samples - c * chunk)
                if c > 0 and sampler is None:
                    sampler = self._evidence_sampler(chunk, amp, caller="predict")
                if sampler:
                    theta, x, _ = sampler()
                else:
                    theta = model.sde_parameter_posterior.rsample(chunk)
                    x0 = self.observations.values[0].unsqueeze(0).expand(chunk, -1)
                    with torch.autocast(device_type=dev.type, dtype=amp, enabled=amp is not None):
                        x = sample_diffusion_paths(model.encoder, model.head, self.observations, theta, x0, self.time_horizon,
                                                   self.time_step, self.state_space).x
                theta_all[lo:lo + count] = theta[:count]
                ends[lo:lo + count] = x[:count, n_steps]
                if n_in:
                    inside[lo:lo + count] = x[:count, rows_in]
        del sampler
        states = inside
        if n_in < steps.numel():
            ahead = steps[n_in:] - n_steps
            after = forecast_states(sde, ends, theta_all, int(ahead[-1]), ahead, dt, self.state_space.positive_dims)
            states = torch.cat([inside, after.to(inside.dtype)], dim=1)
        observations = like.sample(states) if like is not None else None
        return PosteriorPredictive(times=times.to(dev), sde_parameters=theta_all, states=states, observations=observations)

    @torch.no_grad()
    def reweight_parameters(self, sde: SDE, observation_likelihood: ObservationLikelihood, n_samples: int = 1024,
                            n_particles: int = 512, chunk_size: int = 256, return_draws: bool = True,
                            proposal: str = "bootstrap", dynamics: str = "diffusion",
                            max_events: int = 2 ** 16) -> ParameterReweighting:
        """Is q(theta) any good?  Draws theta ~ q with the EMA weights as ``sample()`` draws them, estimates ``log p(y | theta)`` of
        the Euler-Maruyama-discretised model on this posterior's grid with a bootstrap particle filter (``particle_filter``:
        ``n_particles`` particles per theta, ``chunk_size`` thetas per call, start state = first observation as in
        ``log_evidence``), and weights the draws by ``p(theta) p^(y | theta) / q(theta)``.  Unlike ``log_evidence`` the variational
        paths do not enter, so a poor path posterior cannot hide a good theta posterior or the reverse; and unlike it this also
        runs on a CPU posterior (the filter's torch route).  It touches none of ``sample()``'s caches or graphs.
        ``proposal`` goes to ``particle_filter``: switch to ``"bridge"`` (the guided filter; Gaussian observation term only) when
        ``filter_effective_sample_size.min()`` of a bootstrap run is near 1 -- the observations are then too informative for a
        proposal that does not look at them, and ``log p^`` too noisy for the weights to mean much.  The bridge extrapolates the
        drift linearly to the next observation: it pays when observations are a few steps apart or the drift changes little between
        them, not across a long gap of a strongly nonlinear model (compare ``filter_effective_sample_size`` of the two); there
        ``"residual_bridge"`` (the same step around the noise-free Euler path of the segment) is the one to try.
        ``dynamics="jump"`` (a ``ReactionNetworkSDE``): ``log p(y | theta)`` is that of the exact jump process instead
        (``jump_particle_filter`` with ``max_events`` events per particle and segment; ``proposal`` must be ``"bootstrap"``); the
        start state is the first observation, which must hold integers.  ``dynamics="tau_leap"``: that of the tau-leap of the jump
        process on this posterior's grid (``tau_leap_particle_filter``), with the same conditions."""
        from ..inference import jump_filter as _jf
        from ..inference import particle_filter as _pf
        from ..inference.particle_mcmc import DYNAMICS
        if proposal not in _pf.PROPOSALS:
            raise ValueError(f"proposal must be one of {_pf.PROPOSALS}, got {proposal!r}")
        if dynamics not in DYNAMICS:
            raise ValueError(f"dynamics must be one of {DYNAMICS}, got {dynamics!r}")
        if dynamics != "diffusion" and proposal != "bootstrap":
            raise ValueError(f"dynamics={dynamics!r} runs the bootstrap filter on the jump process: proposal must be 'bootstrap', got {proposal!r}")
        if n_samples < 1 or chunk_size < 1 or n_particles < 1:
            raise ValueError(f"n_samples, n_particles and chunk_size must be >= 1 (got {n_samples}, {n_particles}, {chunk_size})")
        q = self.model.sde_parameter_posterior
        S, P = self.state_space.dim, q.sde_param_dim
        if sde.state_dim != S or sde.sde_param_dim != P:
            raise ValueError(f"sde has state_dim {sde.state_dim}, sde_param_dim {sde.sde_param_dim}; the posterior has {S}, {P}")
        self.model.eval()
        with self.exponential_moving_average.apply():
            theta = q.rsample(n_samples)
            log_q = q.log_prob(theta).double()
        log_prior = self.prior.log_prob(theta)
        if log_prior.ndim > 1:
            log_prior = log_prior.sum(dim=-1)
        x0 = self.observations.values[0]
        loglik = torch.empty(n_samples, device=theta.device, dtype=theta.dtype)
        min_ess = torch.empty(n_samples, device=theta.device, dtype=theta.dtype)
        for lo in range(0, n_samples, chunk_size):
            if dynamics == "jump":
                res = _jf.jump_particle_filter(sde, self.observations, observation_likelihood, theta[lo:lo + chunk_size],
                                               n_particles=n_particles, initial_state=x0, max_events=max_events)
            elif dynamics == "tau_leap":
                from ..inference.tau_leap_filter import tau_leap_particle_filter
                res = tau_leap_particle_filter(sde, self.observations, observation_likelihood, theta[lo:lo + chunk_size], self.time_step,
                                               n_particles=n_particles, initial_state=x0)
            else:
                res = _pf.particle_filter(sde, self.observations, observation_likelihood, theta[lo:lo + chunk_size], self.time_step,
                                          n_particles=n_particles, initial_state=x0, positive_dims=self.state_space.positive_dims,
                                          proposal=proposal)
            loglik[lo:lo + chunk_size] = res.log_likelihood
            min_ess[lo:lo + chunk_size] = res.effective_sample_size.min(dim=1).values
        log_w = log_prior.double() + loglik.double() - log_q
        th = theta.double()
        bad = int((torch.isnan(log_w) | torch.isposinf(log_w)).sum())
        draws = (theta, loglik, log_w) if return_draws else (None, None, None)
        v_mean, v_std = theta.mean(dim=0), theta.std(dim=0) if n_samples > 1 else torch.zeros_like(theta[0])
        nan_p = torch.full_like(v_mean, float("nan"))
        nan_q = Quantiles(*([nan_p] * len(QUANTILE_LEVELS)))
        m = float(log_w.max()) if bad == 0 else float("nan")
        if bad > 0 or m == float("-inf"):    # NaN weights: every estimate is NaN; all weights zero: -inf, as EvidenceEstimate says
            head = (float("nan"),) * 3 if bad > 0 else (float("-inf"), float("inf"), 0.0)
            return ParameterReweighting(*head, n_samples, bad, nan_p, nan_p, nan_q, v_mean, v_std, min_ess, *draws)
        w = torch.exp(log_w - m)
        s1, s2 = float(w.sum()), float((w * w).sum())
        ess = s1 * s1 / s2
        wn = w / s1
        mean = (wn[:, None] * th).sum(dim=0)
        std = (wn[:, None] * (th - mean) ** 2).sum(dim=0).sqrt()
        quant = _weighted_quantiles(th, wn)
        return ParameterReweighting(
            m + math.log(s1) - math.log(n_samples), math.sqrt(max(1.0 / ess - 1.0 / n_samples, 0.0)), ess, n_samples, 0,
            mean.to(theta.dtype), std.to(theta.dtype), Quantiles(*quant.to(theta.dtype).unbind(0)), v_mean, v_std, min_ess, *draws)

    @torch.no_grad()
    def smooth_paths(self, sde: SDE, observation_likelihood: ObservationLikelihood, n_samples: int = 1024, n_particles: int = 512,
                     chunk_size: int = 256, proposal: str = "bootstrap", return_draws: bool = True) -> PathReweighting:
        """Are the variational paths any good?  ``reweight_parameters`` with one smoothed path per theta draw
        (``particle_smoother``: the path is traced through the genealogy of the very filter that estimated ``p^(y | theta)``), so
        the weighted draws are a proper importance sample of the exact joint posterior ``p(theta, x_{0:T} | y)``: ``path_mean`` /
        ``path_std`` / ``path_quantiles`` are what ``summary().diffusion_path_mean`` / ``diffusion_path_std`` should match, and
        neither the encoder nor the head enters.  It consumes torch's generator exactly as ``reweight_parameters`` does (theta, then
        one key per chunk), so under the same seed both return the same ``log_evidence``.  It runs on a CPU posterior too (the
        torch routes) and touches none of ``sample()``'s caches or graphs.  ``proposal`` as in ``reweight_parameters``."""
        from ..inference import particle_filter as _pf
        from ..inference import particle_smoother as _ps
        if proposal not in _pf.PROPOSALS:
            raise ValueError(f"proposal must be one of {_pf.PROPOSALS}, got {proposal!r}")
        if n_samples < 1 or chunk_size < 1 or n_particles < 1:
            raise ValueError(f"n_samples, n_particles and chunk_size must be >= 1 (got {n_samples}, {n_particles}, {chunk_size})")
        q = self.model.sde_parameter_posterior
        S, P = self.state_space.dim, q.sde_param_dim
        if sde.state_dim != S or sde.sde_param_dim != P:
            raise ValueError(f"sde has state_dim {sde.state_dim}, sde_param_dim {sde.sde_param_dim}; the posterior has {S}, {P}")
        self.model.eval()
        with self.exponential_moving_average.apply():
            theta = q.rsample(n_samples)
            log_q = q.log_prob(theta).double()
        log_prior = self.prior.log_prob(theta)
        if log_prior.ndim > 1:
            log_prior = log_prior.sum(dim=-1)
        x0 = self.observations.values[0]
        loglik = torch.empty(n_samples, device=theta.device, dtype=theta.dtype)
        min_ess = torch.empty(n_samples, device=theta.device, dtype=theta.dtype)
        paths = None
        for lo in range(0, n_samples, chunk_size):
            res = _ps.particle_smoother(sde, self.observations, observation_likelihood, theta[lo:lo + chunk_size], self.time_step,
                                        n_particles=n_particles, n_draws=1, initial_state=x0,
                                        positive_dims=self.state_space.positive_dims, proposal=proposal)
            if paths is None:
                paths = torch.empty(n_samples, *res.paths.shape[2:], device=theta.device, dtype=res.paths.dtype)
            loglik[lo:lo + chunk_size] = res.log_likelihood
            min_ess[lo:lo + chunk_size] = res.effective_sample_size.min(dim=1).values
            paths[lo:lo + chunk_size] = res.paths[:, 0]
        T1 = paths.shape[1]
        times = torch.arange(T1, device=theta.device, dtype=theta.dtype) * self.time_step
        log_w = log_prior.double() + loglik.double() - log_q
        bad = int((torch.isnan(log_w) | torch.isposinf(log_w)).sum())
        draws = (paths, theta, log_w) if return_draws else (None, None, None)
        nan_x = torch.full((T1, S), float("nan"), device=theta.device, dtype=paths.dtype)
        nan_q = Quantiles(*([nan_x] * len(QUANTILE_LEVELS)))
        m = float(log_w.max()) if bad == 0 else float("nan")
        if bad > 0 or m == float("-inf"):    # as reweight_parameters: NaN weights, or all weights zero
            head = (float("nan"),) * 3 if bad > 0 else (float("-inf"), float("inf"), 0.0)
            return PathReweighting(*head, n_samples, bad, min_ess, times, nan_x, nan_x, nan_q, *draws)
        w = torch.exp(log_w - m)
        s1, s2 = float(w.sum()), float((w * w).sum())
        ess = s1 * s1 / s2
        wn = w / s1
        keep = wn > 0                                        # a dead filter's NaN path has weight zero: it enters no estimate
        x, wk = paths[keep].double().reshape(int(keep.sum()), T1 * S), wn[keep]
        mean = (wk[:, None] * x).sum(dim=0)
        std = (wk[:, None] * (x - mean) ** 2).sum(dim=0).sqrt()
        quant = _weighted_quantiles(x, wk)
        shape = lambda v: v.to(paths.dtype).reshape(T1, S)
        return PathReweighting(
            m + math.log(s1) - math.log(n_samples), math.sqrt(max(1.0 / ess - 1.0 / n_samples, 0.0)), ess, n_samples, 0, min_ess,
            times, shape(mean), shape(std), Quantiles(*(shape(v) for v in quant.unbind(0))), *draws)

    @torch.no_grad()
    def refine_parameters(self, sde: SDE, observation_likelihood: ObservationLikelihood, n_chains: int = 256,
                          n_iterations: int = 600, warmup: int = 300, n_particles: int = 512, filters_per_chain: int = 1,
                          thin: int = 1, proposal: str = "bootstrap", return_paths: bool = False, path_thin: int = 1,
                          dynamics: str = "diffusion", max_events: int = 2 ** 16, path_times=None):
        """When ``reweight_parameters`` says q(theta) is poor (a small ``effective_sample_size``: a mean-field q cannot follow a
        correlated posterior), this gives something better: ``n_chains`` independent particle-MCMC chains (``particle_mcmc``) started
        at draws of q under the EMA weights, as ``reweight_parameters`` draws them, which sample the exact theta posterior of the
        Euler-Maruyama-discretised model on this posterior's grid (prior, first observation as start state and
        ``state_space.positive_dims`` as everywhere here; q's positive mask says which dims walk in log space; the initial proposal
        scale is q's own ``exp(log_std)``).  Returns the ``ParticleMCMCResult`` with ``variational_mean`` / ``variational_std``, the
        plain moments of the starting draws, next to the chains' ``mean`` / ``std``; check ``r_hat`` and ``mean_standard_error``
        before trusting them.  ``return_paths=True``: every ``path_thin``-th kept state also gets the latent path accepted with it
        (``paths [n_path, C, T+1, S]`` and the ``path_*`` fields of the result): exact draws of the path to set beside
        ``summary().diffusion_path_mean``, where ``smooth_paths`` is an importance sample around q.  It runs on a CPU posterior too (the torch route) and touches none of ``sample()``'s caches or
        graphs.  ``dynamics="jump"`` (a ``ReactionNetworkSDE``): the chains target the theta posterior of the exact jump process
        (``particle_mcmc(..., dynamics="jump", max_events=...)``): the start state is the first observation, which must hold
        integers and ``proposal`` must be ``"bootstrap"``.  A jump process has no grid: with ``return_paths=True`` it needs
        ``path_times`` (float64 ``[Q]``, non-decreasing, inside ``[0, T_{K-1}]``), the instants the integer paths ``[n_path, C, Q, S]``
        are read at.  ``dynamics="tau_leap"`` (a ``ReactionNetworkSDE``): the chains target the theta posterior of the tau-leap of the
        jump process on this posterior's grid (``particle_mcmc(..., dynamics="tau_leap")``), with the same start state and
        ``proposal``; ``return_paths=True`` and ``path_times`` raise."""
        import dataclasses
        from ..inference import particle_mcmc as _mc
        if n_chains < 1:
            raise ValueError(f"n_chains must be >= 1, got {n_chains}")
        q = self.model.sde_parameter_posterior
        S, P = self.state_space.dim, q.sde_param_dim
        if sde.state_dim != S or sde.sde_param_dim != P:
            raise ValueError(f"sde has state_dim {sde.state_dim}, sde_param_dim {sde.sde_param_dim}; the posterior has {S}, {P}")
        self.model.eval()
        with self.exponential_moving_average.apply():
            theta = q.rsample(n_chains)
            scale = torch.diag(q.log_std.detach().exp())
        res = _mc.particle_mcmc(sde, self.observations, observation_likelihood, self.prior, self.time_step, theta, n_iterations,
                                warmup=warmup, n_particles=n_particles, filters_per_chain=filters_per_chain, thin=thin,
                                theta_positive_dims=q._positive_dims, positive_dims=self.state_space.positive_dims,
                                initial_state=self.observations.values[0], proposal=proposal, proposal_scale_tril=scale,
                                return_paths=return_paths, path_thin=path_thin, dynamics=dynamics, max_events=max_events,
                                path_times=path_times)
        v_std = theta.std(dim=0) if n_chains > 1 else torch.zeros_like(theta[0])
        return dataclasses.replace(res, variational_mean=theta.mean(dim=0), variational_std=v_std)

    def summary(self, n_samples: int = 1000, mixed_precision: bool = False) -> VariationalPosteriorSummary:
        s = self.sample(n_samples, mixed_precision)
        levels = torch.tensor(QUANTILE_LEVELS, device=self.device, dtype=s.sde_parameters.dtype)
        q = torch.quantile(s.sde_parameters, levels, dim=0)
        return VariationalPosteriorSummary(
            sde_parameter_mean=s.sde_parameters.mean(dim=0), sde_parameter_std=s.sde_parameters.std(dim=0),
            sde_parameter_quantiles=Quantiles(*q.unbind(0)), diffusion_path_mean=s.diffusion_paths.mean(dim=0),
            diffusion_path_std=s.diffusion_paths.std(dim=0))

    def diagnostics(self) -> InferenceDiagnostics:
        hist = self.evidence_lower_bound_history
        return InferenceDiagnostics(evidence_lower_bound_history=hist,
                                    final_evidence_lower_bound=hist[-1] if hist else float("nan"),
                                    n_iterations=len(hist))

    def plot(self, n_trajectories: int = 50, show: bool = True):
        from ..visualization import plot_posterior
        return plot_posterior(self.sample(n_trajectories), self.observations, self.time_horizon, show)

    def save(self, path: str | Path) -> None:
        torch.save({"model_state": self.model.state_dict(),
                    "ema_state": self.exponential_moving_average.state_dict(),
                    "time_horizon": self.time_horizon, "time_step": self.time_step,
                    "state_positive_dims": self.state_space.positive_dims,
                    "evidence_lower_bound_history": self.evidence_lower_bound_history}, Path(path))

    @classmethod
    def load(cls, path: str | Path, model: VariationalSDEPosterior, prior: Prior, observations: Observations,
             device: torch.device) -> "VariationalPosterior":
        ckpt = VariationalPosteriorCheckpoint.model_validate(torch.load(Path(path), map_location=device, weights_only=True))
        model.load_state_dict(ckpt.model_state)
        ema = ExponentialMovingAverage(model)
        ema.load_state_dict(ckpt.ema_state)
        space = StateSpace(observations.values.shape[-1], ckpt.state_positive_dims)
        return cls(model=model, exponential_moving_average=ema, prior=prior, observations=observations,
                   time_horizon=ckpt.time_horizon, time_step=ckpt.time_step, state_space=space,
                   evidence_lower_bound_history=ckpt.evidence_lower_bound_history, device=device)
