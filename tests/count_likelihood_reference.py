"""float64 restatements of the count likelihoods for the tests, independent of torch: ``math.lgamma`` / ``math.log`` per element
(core/observations.py: PoissonObservationLikelihood, NegativeBinomialObservationLikelihood), and the log-weights of the filter's
particles in vectorised numpy."""
import math

import numpy as np

RATE_FLOOR = 1e-6
_lgamma = np.vectorize(math.lgamma, otypes=[np.float64])


def rates(x, scale=1.0, H=None):
    """lambda [..., O] = max(scale * H x, RATE_FLOOR) of states x [..., S] (float64)."""
    x = np.asarray(x, dtype=np.float64)
    pred = x if H is None else x @ np.asarray(H, dtype=np.float64).T
    return np.maximum(scale * pred, RATE_FLOOR)


def poisson_log_prob(y, x, scale=1.0, H=None):
    """sum_o [y log lambda - lambda - lgamma(y + 1)], one element at a time."""
    lam, y = rates(x, scale, H), np.broadcast_to(np.asarray(y, dtype=np.float64), rates(x, scale, H).shape)
    out = np.zeros(lam.shape[:-1])
    for idx in np.ndindex(*lam.shape):
        yv, lv = float(y[idx]), float(lam[idx])
        out[idx[:-1]] += (yv * math.log(lv) if yv > 0 else 0.0) - lv - math.lgamma(yv + 1.0)
    return out


def negative_binomial_log_prob(y, x, dispersion, scale=1.0, H=None):
    """sum_o [lgamma(y + r) - lgamma(r) - lgamma(y + 1) + r log(r / (r + lambda)) + y log(lambda / (r + lambda))]."""
    lam, r = rates(x, scale, H), float(dispersion)
    y = np.broadcast_to(np.asarray(y, dtype=np.float64), lam.shape)
    out = np.zeros(lam.shape[:-1])
    for idx in np.ndindex(*lam.shape):
        yv, lv = float(y[idx]), float(lam[idx])
        out[idx[:-1]] += (math.lgamma(yv + r) - math.lgamma(r) - math.lgamma(yv + 1.0) + r * math.log(r / (r + lv))
                          + (yv * math.log(lv / (r + lv)) if yv > 0 else 0.0))
    return out


def count_log_weights(y, x, dispersion=None, scale=1.0, H=None):
    """lw [..., N] of particles x [..., N, S] for one observation y [O] (float64; Poisson when ``dispersion`` is None); NaN
    counts as -inf.  Vectorised: the raw formulas in float64."""
    lam = rates(x, scale, H)
    y = np.asarray(y, dtype=np.float64)
    ylog = lambda v: np.where(y > 0, y * np.log(v), 0.0)
    if dispersion is None:
        lw = (ylog(lam) - lam - _lgamma(y + 1.0)).sum(axis=-1)
    else:
        r = float(dispersion)
        lw = (_lgamma(y + r) - math.lgamma(r) - _lgamma(y + 1.0) + r * np.log(r / (r + lam)) + ylog(lam / (r + lam))).sum(axis=-1)
    return np.where(np.isnan(lw), -np.inf, lw)
