"""Importance log-weights of posterior draws: the per-sample ELBO integrand (``evidence_lower_bound.py``) before the batch mean,

    log w_b = obs_lp + sde_lp - gen_lp + log_jacobian + log p(theta_b) - log q(theta_b),

so that ``mean(log w)`` is the ELBO on the same draws and ``logsumexp(log w) - log n`` estimates the log evidence of the
Euler-Maruyama-discretised model (``VariationalPosterior.log_evidence``).  Not differentiable: the weights are diagnostics."""
from __future__ import annotations

import torch
from torch import Tensor

from ..core.observations import ObservationLikelihood, Observations, grid_index
from ..core.priors import Prior
from ..core.sde import SDE, builtin_sde_route, kernel_theta
from ..models.sde_parameter_posterior import SDEParameterPosterior
from .evidence_lower_bound import _fused_tail_config, path_log_terms, sde_coefficients, tail_log_terms
from .types import DiffusionPathSample


@torch.no_grad()
def importance_log_weights(sde: SDE, observations: Observations, observation_likelihood: ObservationLikelihood, prior: Prior,
                           sde_parameter_posterior: SDEParameterPosterior, sde_parameters: Tensor, sample: DiffusionPathSample,
                           time_step: float) -> Tensor:
    """``log w [B]`` of the draws ``(sde_parameters [B, P], sample)``.  ``sample`` must carry the transition means / Cholesky
    factors that generated its paths (the head's output), whatever precision the encoder ran in.

    * built-in SDE and closed-form tail (Gaussian likelihood, the package's Prior and posterior, dims <= 16): ONE kernel
      (csrc/vsde_elbo.hip: log_weight_kernel), drift / diffusion evaluated in registers;
    * user SDE with a closed-form tail: the SDE's Python drift / diffusion, then the same kernel reading them;
    * otherwise: the ELBO's path-term kernel plus the objects' own ``log_prob`` per sample."""
    z = sample.z
    n_steps = z.shape[1] - 1
    obs_idx = grid_index(observations.times, time_step, n_steps)
    cfg = _fused_tail_config(observations, observation_likelihood, prior, sde_parameter_posterior, z, sde_parameters)
    if cfg is not None:
        from .. import _hip
        obs_values, obs_matrix, variance, prior_type, prior_mean, prior_std, theta_pos = cfg
        kind, network = builtin_sde_route(sde)
        drift = diffusion = None
        if kind not in _hip.SDE_KINDS:
            kind = None
            drift, diffusion = sde_coefficients(sde, sample.x, sde_parameters)
        return _hip.log_weights(kind, z, sample.transition_means, sample.transition_cholesky, drift, diffusion, sde_parameters,
                                obs_idx, obs_values, obs_matrix, variance, prior_type, prior_mean, prior_std,
                                sde_parameter_posterior.mean, sde_parameter_posterior.log_std, sample.state_space.positive_dims,
                                theta_pos, time_step, network=network,
                                rates=None if kind is None else kernel_theta(network, sde_parameters))
    x = sample.x
    drift, diffusion = sde_coefficients(sde, x, sde_parameters)
    sde_lp, gen_lp, jac = path_log_terms(sample, drift, diffusion, time_step)
    obs_lp, prior_lp, post_lp = tail_log_terms(observations, observation_likelihood, prior, sde_parameter_posterior, x,
                                               sde_parameters, obs_idx)
    return obs_lp + sde_lp - gen_lp + jac + prior_lp - post_lp
