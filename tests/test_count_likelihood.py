"""CPU: the count observation models (core/observations.py: PoissonObservationLikelihood, NegativeBinomialObservationLikelihood):
``log_prob`` against an independent float64 restatement (tests/count_likelihood_reference.py), the rate floor, sampling moments,
validation, and the torch route of the particle filter with them."""
import math

import numpy as np
import pytest
import torch

import count_likelihood_reference as ref

COUNTS = [0.0, 1.0, 7.0, 400.0, 5000.0]
SIR_TIMES = [0.0, 5.0, 10.0, 15.0, 20.0]
SIR_VALUES = [[95.0, 5.0], [85.0, 8.0], [72.0, 11.0], [60.0, 12.0], [50.0, 11.0]]


def _likes(H=None):
    from viforsdes_amd import NegativeBinomialObservationLikelihood, PoissonObservationLikelihood
    return [(PoissonObservationLikelihood(scale=1.7, obs_matrix=H), None, 1.7),
            (NegativeBinomialObservationLikelihood(dispersion=10.0, scale=0.6, obs_matrix=H), 10.0, 0.6),
            (NegativeBinomialObservationLikelihood(dispersion=0.5, obs_matrix=H), 0.5, 1.0)]


@pytest.mark.parametrize("with_matrix", [False, True])
def test_log_prob_matches_the_float64_restatement(with_matrix):
    """y in {0, 1, 7, 400, 5000}, lambda near y (within a few per cent) and far from it (a factor 0.01 .. 100): 1e-12 relative."""
    g = torch.Generator().manual_seed(3)
    H = torch.tensor([[1.0, 0.5, 0.0], [0.25, 0.0, 2.0]], dtype=torch.float64) if with_matrix else None
    worst = 0.0
    for like, r, scale in _likes(H):
        for factor in (1.0, 1.03, 0.97, 0.01, 0.3, 5.0, 100.0):
            y = torch.tensor(COUNTS, dtype=torch.float64)
            if with_matrix:       # rows of two observed counts; states solved so that scale * H x = factor * max(y, 0.5)
                y = torch.stack([y, y.flip(0)], dim=1)                                       # [5, 2]
                target = factor * y.clamp(min=0.5) / scale
                x = torch.linalg.lstsq(H.expand(5, 2, 3), target.unsqueeze(-1)).solution.squeeze(-1)
                x = x * (1.0 + 1e-3 * torch.rand(5, 3, generator=g, dtype=torch.float64))
            else:
                y = y.unsqueeze(-1)                                                          # [5, 1]
                x = factor * y.clamp(min=0.5) / scale * (1.0 + 1e-3 * torch.rand(5, 1, generator=g, dtype=torch.float64))
            got = like.log_prob(y, x).numpy()
            Hn = None if H is None else H.numpy()
            want = (ref.poisson_log_prob(y.numpy(), x.numpy(), scale, Hn) if r is None
                    else ref.negative_binomial_log_prob(y.numpy(), x.numpy(), r, scale, Hn))
            assert got.shape == want.shape == (5,)
            worst = max(worst, float(np.max(np.abs(got - want) / np.abs(want))))
            # the deviance form the kernels evaluate plus the row constants is the same function
            lam = like.predict(x)
            dev = torch.where(y > 0, torch.xlogy(y, lam / y.clamp(min=1.0)), torch.zeros_like(y))
            dev = dev - (lam - y) if r is None else dev - (r + y) * torch.log((r + lam) / (r + y))
            total = dev.sum(-1) + like.row_constants(y)
            assert float(np.max(np.abs(total.numpy() - want) / np.abs(want))) < 1e-11
    print(f"largest relative difference {worst:.2e}")
    assert worst <= 1e-12


def test_the_floor_gives_a_finite_value_and_an_exactly_zero_gradient():
    H = torch.tensor([[1.0, -2.0], [0.0, 1.0]], dtype=torch.float64)
    for like, r, scale in _likes(H):
        x = torch.tensor([[0.0, 0.0], [1.0, 3.0], [4.0, 1.0]], dtype=torch.float64, requires_grad=True)   # H x = (0, 0), (-5, 3), (2, 1)
        y = torch.tensor([[2.0, 0.0], [3.0, 1.0], [0.0, 4.0]], dtype=torch.float64)
        lp = like.log_prob(y, x)
        assert bool(torch.isfinite(lp).all())
        (gx,) = torch.autograd.grad(lp.sum(), x)
        assert torch.equal(gx[0], torch.zeros(2, dtype=torch.float64))          # both rates floored
        lam = like.predict(x.detach())
        assert float(lam[0, 0]) == 1e-6 and float(lam[1, 0]) == 1e-6 and float(lam[1, 1]) == scale * 3.0
        # row 1: the floored first observation sends nothing back; the gradient is the second observation's alone
        x2 = x.detach().clone().requires_grad_(True)
        lam2 = scale * (x2[1] @ H[1])
        second = (y[1, 1] * torch.log(lam2) - lam2) if r is None else (y[1, 1] * torch.log(lam2 / (r + lam2)) + r * torch.log(r / (r + lam2)))
        (g2,) = torch.autograd.grad(second, x2)
        assert torch.allclose(gx[1], g2[1], rtol=1e-12, atol=0.0)
        assert bool((gx[2] != 0).any())
    from viforsdes_amd import PoissonObservationLikelihood
    like = PoissonObservationLikelihood()
    x = torch.zeros(1, 2, requires_grad=True)
    lp = like.log_prob(torch.tensor([[0.0, 3.0]]), x)
    assert bool(torch.isfinite(lp).all()) and torch.equal(torch.autograd.grad(lp.sum(), x)[0], torch.zeros(1, 2))


def test_sampling_moments():
    """200 000 draws: mean within 5 standard errors of lambda, variance within 5 standard errors of lambda + lambda^2 / r (the
    standard error of a sample variance from the sample's own fourth central moment)."""
    n = 200_000
    for like, r, scale in _likes():
        for level in (0.7, 12.0, 300.0):
            torch.manual_seed(17)
            lam = scale * level
            s = like.sample(torch.full((n, 1), level, dtype=torch.float64)).squeeze(-1)
            assert s.shape == (n,) and bool((s >= 0).all()) and bool((s == s.round()).all())
            var = lam if r is None else lam + lam * lam / r
            mean_se = math.sqrt(var / n)
            d = s - s.mean()
            var_se = math.sqrt(max(float((d ** 4).mean()) - float((d ** 2).mean()) ** 2, 0.0) / n)
            print(f"{type(like).__name__} lambda {lam:g}: mean {float(s.mean()):.4f} (se {mean_se:.4f}), variance {float(s.var()):.4f} "
                  f"vs {var:.4f} (se {var_se:.4f})")
            assert abs(float(s.mean()) - lam) < 5.0 * mean_se
            assert abs(float(s.var()) - var) < 5.0 * var_se


def test_validation():
    from viforsdes_amd import NegativeBinomialObservationLikelihood, PoissonObservationLikelihood
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="scale"):
            PoissonObservationLikelihood(scale=bad)
        with pytest.raises(ValueError, match="scale"):
            NegativeBinomialObservationLikelihood(dispersion=1.0, scale=bad)
        with pytest.raises(ValueError, match="dispersion"):
            NegativeBinomialObservationLikelihood(dispersion=bad)
    x = torch.ones(1, 2)
    for like, _, _ in _likes():
        for y in ([[1.0, -1.0]], [[0.5, 2.0]]):
            with pytest.raises(ValueError, match="non-negative integer"):
                like.log_prob(torch.tensor(y), x)
        with pytest.raises(ValueError, match="shape"):
            like.log_prob(torch.ones(1, 3), x)
    H = torch.ones(2, 3)
    for like, _, _ in _likes(H):
        with pytest.raises(ValueError, match="second dim"):
            like.predict(x)
        with pytest.raises(ValueError, match="first dim"):
            like.log_prob(torch.ones(1, 3), torch.ones(1, 3))
        assert like.predict(torch.ones(4, 3)).shape == (4, 2)
    with pytest.raises(ValueError, match="2D"):
        PoissonObservationLikelihood(obs_matrix=torch.ones(3)).predict(torch.ones(1, 3))


def _sir():
    from viforsdes_amd import Observations, ReactionNetworkSDE
    sde = ReactionNetworkSDE(reactants=[[1, 1], [0, 1]], products=[[0, 2], [0, 0]], species=["S", "I"], reactions=["infection", "removal"])
    obs = Observations(times=torch.tensor(SIR_TIMES, dtype=torch.float64), values=torch.tensor(SIR_VALUES, dtype=torch.float64))
    return sde, obs


def test_the_bridge_proposal_still_needs_a_gaussian_likelihood():
    from viforsdes_amd import particle_filter
    sde, obs = _sir()
    for like, _, _ in _likes():
        with pytest.raises(ValueError, match="GaussianObservationLikelihood"):
            particle_filter(sde, obs, like, torch.tensor([[0.004, 0.15]], dtype=torch.float64), 0.1, n_particles=8, proposal="bridge")


def test_torch_route_filter_with_count_likelihoods():
    from viforsdes_amd import particle_filter
    sde, obs = _sir()
    M, N = 8, 64
    g = torch.Generator().manual_seed(0)
    th = torch.tensor([0.004, 0.15], dtype=torch.float64) * (1.0 + 0.1 * torch.rand(M, 2, generator=g, dtype=torch.float64))
    for like, _, _ in _likes():
        res = particle_filter(sde, obs, like, th, 0.1, n_particles=N, positive_dims=(0, 1), return_particles=True,
                              key=torch.tensor([7, 9], dtype=torch.int32))
        assert res.log_likelihood.dtype == torch.float64 and res.increments.shape == (M, 5)
        assert bool(torch.isfinite(res.log_likelihood).all()) and bool(torch.isfinite(res.increments).all())
        assert torch.equal(res.increments.sum(1), res.log_likelihood)
        assert bool((res.effective_sample_size > 1.0).all()) and bool((res.effective_sample_size <= N).all())
        # the stored log-weights are the likelihood's own
        lw = like.log_prob(obs.values[3].expand(N, 2), res.particles[2, 3])
        assert torch.equal(res.log_weights[2, 3], lw)
