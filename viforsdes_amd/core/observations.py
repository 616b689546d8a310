"""Observations and the observation models: Gaussian (reference: core/observations.py:12-74) and, for count data, Poisson and
negative binomial."""
from __future__ import annotations

import math
import weakref
from typing import Optional, Protocol, runtime_checkable

import torch
from pydantic import BaseModel, ConfigDict, model_validator
from torch import Tensor
from typing_extensions import Self


class Observations(BaseModel):
    """``times[T_obs]`` (sorted) and ``values[T_obs, obs_dim]``."""

    model_config = ConfigDict(frozen=True, arbitrary_types_allowed=True)
    times: Tensor
    values: Tensor

    @model_validator(mode="after")
    def _check(self) -> Self:
        t, v = self.times, self.values
        if t.ndim != 1:
            raise ValueError("times must be 1D tensor")
        if v.ndim != 2:
            raise ValueError("values must be 2D tensor [T_obs, obs_dim]")
        if t.shape[0] != v.shape[0]:
            raise ValueError(f"times and values must have same first dimension: got {t.shape[0]} vs {v.shape[0]}")
        if t.numel() > 1 and bool((t[1:] < t[:-1]).any()):
            raise ValueError("times must be sorted in non-decreasing order")
        return self

    def to(self, device: torch.device | str) -> "Observations":
        return Observations(times=self.times.to(device), values=self.values.to(device))


_GRID_INDEX_CACHE: dict = {}


def grid_index(times: Tensor, time_step: float, max_index: int) -> Tensor:
    """``round(times / time_step).long().clamp(max=max_index)``: the grid rows of the observation times (reference:
    evidence_lower_bound.py:45, encoder.py:74).  The observation times do not change during a run, so the index tensor is built
    once per (tensor, version, step, bound) instead of four small kernels at each of its two uses in every step."""
    key = (id(times), times._version, float(time_step), int(max_index))
    hit = _GRID_INDEX_CACHE.get(key)
    if hit is not None and hit[0]() is times:     # the id of a dead tensor can be reused: the weak reference pins the identity
        return hit[1]
    idx = torch.round(times / time_step).long().clamp(max=max_index)
    if times.is_cuda and torch.cuda.is_current_stream_capturing():
        return idx   # memory of a capturing graph's private pool: valid for that graph only
    if len(_GRID_INDEX_CACHE) >= 16:
        _GRID_INDEX_CACHE.clear()
    _GRID_INDEX_CACHE[key] = (weakref.ref(times), idx)
    return idx


@runtime_checkable
class ObservationLikelihood(Protocol):
    def log_prob(self, observations: Tensor, state: Tensor) -> Tensor: ...


class GaussianObservationLikelihood(BaseModel):
    """y ~ N(H x, variance * I); ``obs_matrix`` H is optional (identity when absent)."""

    model_config = ConfigDict(frozen=True, arbitrary_types_allowed=True)
    variance: float
    obs_matrix: Optional[Tensor] = None

    @model_validator(mode="after")
    def _check(self) -> Self:
        if self.variance <= 0:
            raise ValueError("variance must be positive")
        return self

    def predict(self, state: Tensor) -> Tensor:
        H = self.obs_matrix
        if H is None:
            return state
        if H.ndim != 2:
            raise ValueError("obs_matrix must be 2D [obs_dim, state_dim]")
        if H.shape[1] != state.shape[-1]:
            raise ValueError("obs_matrix second dim must match state")
        return state @ H.to(state).T

    def log_prob(self, observations: Tensor, state: Tensor) -> Tensor:
        pred = self.predict(state)
        if self.obs_matrix is not None and self.obs_matrix.shape[0] != observations.shape[-1]:
            raise ValueError("obs_matrix first dim must match observations")
        if observations.shape != pred.shape:
            raise ValueError(f"observation shape {observations.shape} does not match predicted shape {pred.shape}")
        resid = observations - pred
        per_dim = -0.5 * resid * resid / self.variance - 0.5 * math.log(2.0 * math.pi * self.variance)
        return per_dim.sum(dim=-1)

    def sample(self, state: Tensor) -> Tensor:
        """One draw y ~ N(H x, variance * I) per state row: ``predict(state) + sqrt(variance) * eps`` (torch's generator)."""
        pred = self.predict(state)
        return pred + math.sqrt(self.variance) * torch.randn_like(pred)


RATE_FLOOR = 1e-6   # floor of a count likelihood's rate (csrc/vsde_sde_coef.h: kRateFloor)
LIK_POISSON, LIK_NEGATIVE_BINOMIAL = 1, 2   # include/vsde_hip.h: VSDE_LIK_*


def check_counts(observations: Tensor) -> None:
    """Raise ``ValueError`` unless every observation is a non-negative integer value (reads the tensor: a device tensor syncs)."""
    bad = (observations < 0) | (observations != torch.floor(observations)) | torch.isnan(observations)
    if bool(bad.any()):
        raise ValueError("count observations must be non-negative integer values")


class _CountObservationLikelihood(BaseModel):
    """What the two count likelihoods share: the rate ``lambda = max(scale * H x, RATE_FLOOR)`` (``torch.clamp``: no gradient
    reaches the state where the floor binds) and the validation of the counts."""

    model_config = ConfigDict(frozen=True, arbitrary_types_allowed=True)
    scale: float = 1.0
    obs_matrix: Optional[Tensor] = None

    @model_validator(mode="after")
    def _check_scale(self) -> Self:
        if not self.scale > 0:
            raise ValueError("scale must be positive")
        return self

    def predict(self, state: Tensor) -> Tensor:
        """The rate ``lambda`` of every observed dim."""
        H = self.obs_matrix
        if H is None:
            pred = state
        else:
            if H.ndim != 2:
                raise ValueError("obs_matrix must be 2D [obs_dim, state_dim]")
            if H.shape[1] != state.shape[-1]:
                raise ValueError("obs_matrix second dim must match state")
            pred = state @ H.to(state).T
        return torch.clamp(self.scale * pred, min=RATE_FLOOR)

    def _rate(self, observations: Tensor, state: Tensor) -> Tensor:
        lam = self.predict(state)
        if self.obs_matrix is not None and self.obs_matrix.shape[0] != observations.shape[-1]:
            raise ValueError("obs_matrix first dim must match observations")
        if observations.shape != lam.shape:
            raise ValueError(f"observation shape {observations.shape} does not match predicted shape {lam.shape}")
        if not observations.is_cuda:   # the host copy only: reading a device tensor here would sync inside captured code
            check_counts(observations)
        return lam

    def kernel_terms(self, values: Tensor) -> "CountKernelTerms":
        """What the count kernels take in place of a variance: the likelihood's code and constants and ``row_constants(values)``."""
        return CountKernelTerms(self._kind, float(self.scale), float(getattr(self, "dispersion", 1.0)), count_row_constants(self, values))


class PoissonObservationLikelihood(_CountObservationLikelihood):
    """y_o ~ Poisson(lambda_o), ``lambda = max(scale * H x, RATE_FLOOR)``; ``obs_matrix`` H is optional (identity when absent).
    ``log_prob`` raises for a negative or fractional observation (checked on a CPU tensor; the kernel routes check the
    observations once per tensor)."""

    _kind = LIK_POISSON

    def log_prob(self, observations: Tensor, state: Tensor) -> Tensor:
        lam = self._rate(observations, state)
        return (torch.xlogy(observations, lam) - lam - torch.lgamma(observations + 1.0)).sum(dim=-1)

    def row_constants(self, values: Tensor) -> Tensor:
        """``sum_o [y log y - y - lgamma(y + 1)]`` of every observation row (float64 ``[K]``): ``log_prob`` minus the deviance
        form ``y log(lambda / y) - (lambda - y)`` the kernels evaluate."""
        y = values.double()
        return (torch.xlogy(y, y) - y - torch.lgamma(y + 1.0)).sum(dim=-1)

    def sample(self, state: Tensor) -> Tensor:
        """One draw y ~ Poisson(lambda) per state row (torch's generator)."""
        return torch.poisson(self.predict(state))


class NegativeBinomialObservationLikelihood(_CountObservationLikelihood):
    """y_o ~ NB(mean lambda_o, variance lambda_o + lambda_o^2 / dispersion), ``lambda = max(scale * H x, RATE_FLOOR)``: a Poisson
    whose rate is Gamma(dispersion, dispersion / lambda) distributed.  Otherwise as ``PoissonObservationLikelihood``."""

    dispersion: float
    _kind = LIK_NEGATIVE_BINOMIAL

    @model_validator(mode="after")
    def _check_dispersion(self) -> Self:
        if not self.dispersion > 0:
            raise ValueError("dispersion must be positive")
        return self

    def log_prob(self, observations: Tensor, state: Tensor) -> Tensor:
        lam = self._rate(observations, state)
        y, r = observations, float(self.dispersion)
        total = r + lam
        per_dim = (torch.lgamma(y + r) - math.lgamma(r) - torch.lgamma(y + 1.0) + r * torch.log(r / total)
                   + torch.xlogy(y, lam / total))
        return per_dim.sum(dim=-1)

    def row_constants(self, values: Tensor) -> Tensor:
        """``sum_o [lgamma(y + r) - lgamma(r) - lgamma(y + 1) + r log r + y log y - (r + y) log(r + y)]`` (float64 ``[K]``):
        ``log_prob`` minus the deviance form ``y log(lambda / y) - (r + y) log((r + lambda) / (r + y))``."""
        y, r = values.double(), float(self.dispersion)
        return (torch.lgamma(y + r) - math.lgamma(r) - torch.lgamma(y + 1.0) + r * math.log(r) + torch.xlogy(y, y)
                - (r + y) * torch.log(r + y)).sum(dim=-1)

    def sample(self, state: Tensor) -> Tensor:
        """One draw per state row: Poisson of a Gamma(dispersion, dispersion / lambda) draw (torch's generator)."""
        lam = self.predict(state)
        r = torch.full_like(lam, float(self.dispersion))
        return torch.poisson(torch._standard_gamma(r) * (lam / r))


COUNT_LIKELIHOODS = (PoissonObservationLikelihood, NegativeBinomialObservationLikelihood)


class CountKernelTerms(tuple):
    """``(lik_kind, scale, dispersion, row_const [K] fp32 on the observations' device)``: what a count kernel takes where the
    Gaussian one takes its variance."""

    def __new__(cls, lik_kind: int, scale: float, dispersion: float, row_const: Tensor):
        return super().__new__(cls, (lik_kind, scale, dispersion, row_const))


_ROW_CONSTANT_CACHE: dict = {}


def count_row_constants(like, values: Tensor) -> Tensor:
    """``like.row_constants(values)`` as fp32 ``[K]`` on ``values``' device, computed there in float64, and the validation of the
    counts (``check_counts``, one sync), both once per (likelihood constants, tensor, version) as ``grid_index`` does it.  Under
    stream capture nothing is read back: an unseen tensor is not validated there and its constants are not cached."""
    key = (type(like), float(getattr(like, "dispersion", 0.0)), id(values), values._version)
    hit = _ROW_CONSTANT_CACHE.get(key)
    if hit is not None and hit[0]() is values:
        return hit[1]
    capturing = values.is_cuda and torch.cuda.is_current_stream_capturing()
    if not capturing:
        check_counts(values)
    const = like.row_constants(values).to(torch.float32)
    if capturing:
        return const
    if len(_ROW_CONSTANT_CACHE) >= 16:
        _ROW_CONSTANT_CACHE.clear()
    _ROW_CONSTANT_CACHE[key] = (weakref.ref(values), const)
    return const
