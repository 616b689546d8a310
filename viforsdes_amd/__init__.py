"""viforsdes_amd -- MI355X-native variational inference for SDEs.

Same user-facing surface as Tom-Ryder/VIforSDEs (``infer``, ``InferenceConfig``, ``SDE``,
``Observations``, ``Prior``, ``GaussianObservationLikelihood``, the configs and the
``VariationalSDEPosterior`` checkpoint layout); the hot path (fused GRU path sampler forward /
backward and the ELBO accumulation) runs as hand-written HIP kernels for gfx950 behind the C ABI
declared in ``include/vsde_hip.h``."""
import os as _os

# dmabuf IPC for multi-process GPU work (RCCL): read once when HSA initialises, so it is defaulted here, at import time
_os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

from .config import AmpDtype, EncoderConfig, HeadConfig, PretrainConfig, TrainingConfig, YamlConfig
from .core.observations import (GaussianObservationLikelihood, NegativeBinomialObservationLikelihood, ObservationLikelihood,
                                Observations, PoissonObservationLikelihood)
from .core.jump_process import (DiffusionApproximationCheck, JumpProcessResult, diffusion_approximation_check,
                                jump_process)
from .core.priors import Prior, PriorType
from .core.tau_leap import TauLeapResult, tau_leap_process
from .core.reaction_network import Hill, MichaelisMenten, ReactionNetworkSDE
from .core.sde import SDE, FunctionalSDE, make_sde
from .infer import InferenceConfig, infer
from .inference.jump_filter import JumpParticleFilterResult, jump_particle_filter
from .inference.jump_smoother import SmoothedJumpPaths, jump_particle_smoother
from .inference.particle_filter import ParticleFilterResult, particle_filter
from .inference.particle_mcmc import ParticleMCMCResult, particle_mcmc
from .inference.particle_smoother import SmoothedPaths, particle_smoother
from .inference.tau_leap_filter import TauLeapFilterResult, tau_leap_particle_filter
from .posterior.variational_posterior import (EvidenceEstimate, ParameterReweighting, PathReweighting, PosteriorPredictive,
                                              VariationalPosterior)

__all__ = ["AmpDtype", "EncoderConfig", "HeadConfig", "PretrainConfig", "TrainingConfig", "YamlConfig",
           "GaussianObservationLikelihood", "NegativeBinomialObservationLikelihood", "PoissonObservationLikelihood",
           "ObservationLikelihood", "Observations", "Prior", "PriorType", "SDE",
           "FunctionalSDE", "Hill", "MichaelisMenten", "ReactionNetworkSDE", "make_sde", "InferenceConfig", "infer", "VariationalPosterior",
           "EvidenceEstimate", "PosteriorPredictive", "ParameterReweighting", "ParticleFilterResult", "particle_filter",
           "PathReweighting", "SmoothedPaths", "particle_smoother", "ParticleMCMCResult", "particle_mcmc", "JumpProcessResult",
           "jump_process", "DiffusionApproximationCheck", "diffusion_approximation_check", "JumpParticleFilterResult",
           "jump_particle_filter", "SmoothedJumpPaths", "jump_particle_smoother", "TauLeapResult", "tau_leap_process",
           "TauLeapFilterResult", "tau_leap_particle_filter"]
__version__ = "0.1.0"
