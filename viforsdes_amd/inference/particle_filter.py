"""Bootstrap particle filter: an unbiased estimate of the marginal likelihood ``p(y | theta)`` of the Euler-Maruyama-discretised
model, for a batch of parameter vectors at once.  It is the yardstick that does not depend on the variational paths: profile
likelihoods, a pseudo-marginal sampler, and the theta-only check of a fit (``VariationalPosterior.reweight_parameters``).

The torch code below is the specification and runs anywhere (any SDE, any likelihood, CPU or GPU).  Built-in SDEs with a
``GaussianObservationLikelihood`` (or, for the bootstrap proposal, a ``PoissonObservationLikelihood`` /
``NegativeBinomialObservationLikelihood``) on the GPU in fp32 and ``n_particles`` a multiple of 64 up to 1024 (512 for a reaction network
of 5..8 species) run as ONE kernel (csrc/vsde_filter.hip: a workgroup per theta, a thread per particle) that reproduces it; every
other case falls back to the torch route silently, as ``forecast_states`` does.

The algorithm, for filter ``m`` (parameters ``theta_m``, ``N`` particles, all started at ``initial_state``):

* grid rows of the observations ``rows = round(times / time_step)`` (the rule of ``grid_index``); ``rows[K-1]`` Euler steps in all,
  several observations may share a row;
* between observations the step of ``euler_maruyama`` (``positive_dims`` clamped at 1e-6 after every step);
* at observation ``k``: ``lw_j = log p(y_k | x_j)`` (NaN counts as -inf), ``increment_k = max lw + log sum_j exp(lw_j - max) -
  log N``; then systematic resampling, at every observation: ``w_j = exp(lw_j - max)``, inclusive cumulative sums ``C_j`` in particle
  order (made non-decreasing by a running maximum, which is the identity in exact arithmetic), one uniform ``u`` in (0, 1],
  thresholds ``tau_j = (j + u) / N * C_{N-1}``, ``ancestor_j = min(#{i : C_i <= tau_j}, N - 1)``; particle ``j`` continues from the
  state of ``ancestor_j``.  If no weight is positive the increment is -inf, the ESS 0, the filtered moments NaN and the particles
  stay as they are (ancestors = identity);
* randomness is the forecast kernel's stream (include/vsde_hip.h): the normal of filter m, particle slot j, GLOBAL grid step t,
  dim i is the normal of path ``b = m N + j``, step t, dim i for the call's key; the resampling uniform of (m, k) is
  ``((w0 >> 8) + 0.5) 2^-24`` with ``w0`` the first word of ``philox4x32_10({k, 0, m, 1}, key)``.  A slot keeps its own noise
  stream across resampling.  Same key => same result.

``proposal="bridge"`` (a guided filter: the modified diffusion bridge of Durham-Gallant, in Golightly-Wilkinson's form for noisy
linear-Gaussian observations) draws every Euler step from a Gaussian pulled towards the next observation and carries the ratio
model / proposal in the weight, so ``exp(log_likelihood)`` stays unbiased while the particles arrive where the observation is: the
filter to use when the bootstrap filter's ``effective_sample_size.min()`` is near 1 (sharply informative observations) and the drift
changes little between observations (the proposal extrapolates it linearly over the steps that are left: across a long gap of a
strongly nonlinear model it can be worse than the bootstrap filter; the particle ESS of the two runs tells).  It needs a
``GaussianObservationLikelihood`` (the proposal is derived from its H and variance), no trained network, and exactly the normals the
bootstrap filter uses.  With D = time_step, f = drift(x, theta), L = diffusion(x, theta) [S, S], H = obs_matrix (identity when
absent, O = S) and v = variance, the Euler step t -> t + 1 of a particle at x is:

* k = the first observation with ``rows[k] > t``, n = ``rows[k] - t``;
* A = sqrt(D) H L [O, S];  psi = n A A^T + v I [O, O];  e = y_k - H (x + n D f);
* with psi = R R^T (lower Cholesky factor), W = R^-1 A and r = R^-1 e:  m = W^T r (= A^T psi^-1 e) and C = I_S - W^T W
  (= I - A^T psi^-1 A);
* M = the lower Cholesky factor of C with every pivot floored at ``BRIDGE_PIVOT_FLOOR`` before its square root (in exact arithmetic
  the pivots are >= v / (lambda_max(A A^T) + v) for n = 1 and >= 1 - 1 / n otherwise; any invertible M gives a valid weight because
  the same M makes the draw and its density);
* z [S] = the stream's normals of (path b = m N + j, global step t), eps = m + M z, x' = x + f D + sqrt(D) L eps, then the 1e-6
  clamp of the positive dims;
* the particle's running log-ratio:  ``lr += -|eps|^2 / 2 + |z|^2 / 2 + sum_j log M_jj``  (model over proposal in noise space, so
  it stays valid where the diffusion factor is floored or singular, and under the clamp).

At observation k ``lw_j = lr_j + log p(y_k | x_j)`` (NaN counts as -inf) and everything after that is the bootstrap rule with this
``lw``; ``lr`` is zero after every observation, so later observations on the same grid row get the plain Gaussian weight.  For n = 1
the step ratio plus the observation term is ``log N(y; H (x + f D), D H L L^T H^T + v I)`` whatever z is (the fully adapted filter).
The kernel takes the bridge for built-in SDEs with S <= 4 and O <= 4 (``_hip.particle_filter_max_particles(kind, S, proposal)``
particles at most); everything else runs the torch route.

``proposal="residual_bridge"`` (the residual bridge of Whitaker, Golightly, Boys and Sherlock 2017) is the bridge with ONE quantity
replaced, for gaps over which the drift turns: the bridge's predicted state at the observation's row, ``x + n D f(x)``, extrapolates
the drift at x linearly over all n steps that are left, which across an oscillation of a nonlinear model points nowhere near the
path.  The residual bridge carries a deterministic companion path eta per particle and extrapolates only the difference from it:

* at the start of every segment (row 0, and the row of observation k - 1 after resampling, when there are steps towards observation
  k) ``eta <- x``, and a first pass runs the noise-free Euler scheme from x over the segment's ``n0 = rows[k] - t0`` steps,
  ``eta <- clamp(eta + D f(eta, theta))`` with the state's own clamp; its result is ``eta_end``, nothing else of the pass is kept;
* at every step of the segment, with ``f_eta = f(eta, theta)``:  ``e = y_k - H (eta_end + (x - eta) + n D (f(x) - f_eta))``;
  A, psi, R, W, r, m, C, M, eps, x', the clamp and ``lr`` are the bridge's, with the same normals;
* after the step ``eta <- clamp(eta + D f_eta)``.

eta and eta_end are deterministic functions of the segment's start state and theta, and the proposal is still a Gaussian in noise
space with the same M for the draw and its density, so the weights and the unbiasedness are the bridge's.  At the last step of a
segment eta + D f_eta = eta_end, so the predicted state is ``x + D f(x)`` in exact arithmetic whenever eta's clamp does not bind on
that step, and the fully adapted n = 1 identity above holds under that condition.  Same requirements, same kernel coverage and the
same normals as the bridge."""
from __future__ import annotations

import math
from collections.abc import Sequence
from dataclasses import dataclass
from typing import Optional

import torch
from torch import Tensor

from ..core.euler_maruyama import _floor_vector
from ..core.observations import COUNT_LIKELIHOODS, GaussianObservationLikelihood, ObservationLikelihood, Observations
from ..core.sde import SDE, builtin_sde_route, kernel_theta

HIP_FILTER = True   # set False to force the torch route (A/B tests)
PROPOSALS = ("bootstrap", "bridge", "residual_bridge")
BRIDGE_PIVOT_FLOOR = 1e-6   # floor of the pivots of C = I - A^T psi^-1 A before their square root (csrc/vsde_filter.hip: kPfPivotFloor)

_M0, _M1, _W0, _W1, _MASK = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 0xFFFFFFFF


@dataclass(frozen=True)
class ParticleFilterResult:
    """``log_likelihood [M]``: log p^(y | theta_m) given the start state; ``increments [M, K]``: log p^(y_k | y_<k, theta_m), whose sum
    over k it is; ``effective_sample_size [M, K]``: (sum w)^2 / sum w^2 of the weights at observation k, in [0, N];
    ``filtered_mean`` / ``filtered_std [M, K, S]``: weighted moments of the particles before resampling; ``particles [M, K, N, S]``
    (those states) and ``ancestors [M, K, N]`` (int32), or None unless asked for; ``log_weights [M, K, N]``: the log-weights ``lw`` of
    those states (bootstrap: the observation term; bridge: plus the running log-ratio), filled with ``particles``."""
    log_likelihood: Tensor
    increments: Tensor
    effective_sample_size: Tensor
    filtered_mean: Tensor
    filtered_std: Tensor
    particles: Optional[Tensor] = None
    ancestors: Optional[Tensor] = None
    log_weights: Optional[Tensor] = None


def _mul_hi_lo(m: int, c: Tensor) -> tuple[Tensor, Tensor]:
    """High and low 32-bit words of the 64-bit product m * c (m, c < 2^32) in int64 arithmetic that never overflows."""
    ph, pl = m * (c >> 16), m * (c & 0xFFFF)
    return (ph + (pl >> 16)) >> 16, (((ph & 0xFFFF) << 16) + (pl & _MASK)) & _MASK


def philox4x32_10(c0: Tensor, c1: Tensor, c2: Tensor, c3: Tensor, k0: Tensor, k1: Tensor) -> list[Tensor]:
    """The four output words (int64 tensors holding uint32 values) of Philox4x32-10 for counter (c0..c3) and key (k0, k1), all int64
    tensors of uint32 values, broadcast together."""
    c = list(torch.broadcast_tensors(c0, c1, c2, c3))
    for _ in range(10):
        hi0, lo0 = _mul_hi_lo(_M0, c[0])
        hi1, lo1 = _mul_hi_lo(_M1, c[2])
        c = [hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0]
        k0, k1 = (k0 + _W0) & _MASK, (k1 + _W1) & _MASK
    return c


def _uniform(w: Tensor) -> Tensor:
    """u = ((w >> 8) + 0.5) 2^-24 in (0, 1], formed in fp32 as the kernels form it."""
    return ((w >> 8).to(torch.float32) + 0.5) * 2.0 ** -24


def _key_words(key: Tensor) -> tuple[Tensor, Tensor]:
    k = key.to(torch.int64) & _MASK
    return k[0], k[1]


def _box_muller(w: Sequence[Tensor]) -> Tensor:
    """Four normals per counter (float64, on a new last dim) from the four Philox words: Box-Muller on the word pairs (w0, w1),
    (w2, w3); u in fp32, log / sqrt / cos / sin in float64."""
    out = []
    for wa, wb in ((w[0], w[1]), (w[2], w[3])):
        r = torch.sqrt(-2.0 * torch.log(_uniform(wa).double()))
        ang = 2.0 * math.pi * _uniform(wb).double()
        out += [r * torch.cos(ang), r * torch.sin(ang)]
    return torch.stack(out, dim=-1)


def path_normals(paths: Tensor, block: int, state_dim: int, key: Tensor) -> Tensor:
    """The stream's normals of grid steps ``4 block .. 4 block + 3`` for the path indices ``paths [B]`` (int64) under ``key``, two
    words ``[2]`` for all paths or ``[B, 2]``, path b under ``key[b]``: float64 ``[B, S, 4]`` (``_box_muller`` of
    ``philox4x32_10({block, i, path, 0}, key)``)."""
    dev = paths.device
    k = key.to(torch.int64) & _MASK
    i = torch.arange(state_dim, device=dev, dtype=torch.int64)[None, :]
    blk = torch.full((1, 1), int(block), device=dev, dtype=torch.int64)
    return _box_muller(philox4x32_10(blk, i, paths[:, None], torch.zeros_like(blk), k[..., 0:1], k[..., 1:2]))


def stream_normals(n_paths: int, block: int, state_dim: int, key: Tensor) -> Tensor:
    """``path_normals`` for paths ``0 .. n_paths - 1``: float64 ``[n_paths, S, 4]``."""
    return path_normals(torch.arange(n_paths, device=key.device, dtype=torch.int64), block, state_dim, key)


def resampling_uniforms(n_filters: int, k: int, key: Tensor) -> Tensor:
    """The uniform of (filter m, observation k) for m = 0 .. n_filters - 1: fp32 ``[n_filters]``."""
    dev = key.device
    k0, k1 = _key_words(key)
    m = torch.arange(n_filters, device=dev, dtype=torch.int64)
    kk = torch.full((1,), int(k), device=dev, dtype=torch.int64)
    return _uniform(philox4x32_10(kk, torch.zeros_like(kk), m, torch.ones_like(kk), k0, k1)[0])


def systematic_ancestors(weights: Tensor, u: Tensor) -> Tensor:
    """Ancestors ``[M, N]`` (int64) of systematic resampling with the weights ``[M, N]`` (>= 0, not all zero in a row) and one
    uniform ``u [M]`` per row: ``min(#{i : C_i <= (j + u) / N * C_{N-1}}, N - 1)``."""
    N = weights.shape[1]
    cum = torch.cummax(torch.cumsum(weights, dim=1), dim=1).values
    j = torch.arange(N, device=weights.device, dtype=weights.dtype)
    tau = (j[None, :] + u.to(weights.dtype)[:, None]) / N * cum[:, -1:]
    return torch.searchsorted(cum.contiguous(), tau.contiguous(), right=True).clamp(max=N - 1)


def _validate(sde, observations, theta, time_step, n_particles, initial_state):
    if n_particles < 1:
        raise ValueError(f"n_particles must be >= 1, got {n_particles}")
    if time_step <= 0:
        raise ValueError(f"time_step must be positive, got {time_step}")
    if theta.ndim == 1:
        theta = theta.unsqueeze(0)
    S, P = int(sde.state_dim), int(sde.sde_param_dim)
    if theta.ndim != 2 or theta.shape[0] < 1 or theta.shape[1] != P:
        raise ValueError(f"theta [M, {P}] or [{P}] expected (sde_param_dim {P}), got {tuple(theta.shape)}")
    M = theta.shape[0]
    if M * n_particles >= 2 ** 32:
        raise ValueError(f"M * n_particles = {M * n_particles} paths: the noise stream indexes fewer than 2^32")
    if observations.values.shape[0] < 1:
        raise ValueError("observations must not be empty")
    if initial_state is None:
        if observations.values.shape[1] != S:
            raise ValueError(f"initial_state is required: the observations have dim {observations.values.shape[1]}, the state {S}")
        initial_state = observations.values[0]
    x0 = initial_state.to(device=theta.device, dtype=theta.dtype)
    if x0.ndim == 1:
        x0 = x0.unsqueeze(0).expand(M, -1)
    if tuple(x0.shape) != (M, S):
        raise ValueError(f"initial_state [{S}] or [{M}, {S}] expected (state_dim {S}), got {tuple(initial_state.shape)}")
    return theta, x0


def particle_filter(sde: SDE, observations: Observations, observation_likelihood: ObservationLikelihood, theta: Tensor,
                    time_step: float, n_particles: int = 1024, initial_state: Optional[Tensor] = None,
                    positive_dims: Sequence[int] = (), return_particles: bool = False,
                    key: Optional[Tensor] = None, proposal: str = "bootstrap") -> ParticleFilterResult:
    """Particle filters with ``n_particles`` particles, one per row of ``theta`` (``[M, P]``, or ``[P]`` for M = 1), all
    started at ``initial_state`` (``[S]`` or ``[M, S]``; default: the first observation).  The observation at the start row counts
    like any other, so ``log_likelihood`` targets what ``VariationalPosterior.log_evidence`` conditions on.  ``key``: two int32
    words (a tensor); default: drawn from torch's generator on theta's device, so ``torch.manual_seed`` makes the call repeatable
    and a call captured in a HIP graph draws a fresh key per replay.  ``proposal``: "bootstrap", or "bridge" / "residual_bridge" for
    the guided filters of the module docstring.  No gradients."""
    bridge, residual = _proposal_flags(proposal, observation_likelihood)
    theta, x0 = _validate(sde, observations, theta, time_step, n_particles, initial_state)
    dev = theta.device
    obs = observations if observations.values.device == dev else observations.to(dev)
    key = _call_key(key, dev)
    pos = tuple(positive_dims)
    with torch.no_grad():
        route = _kernel_route(sde, obs, observation_likelihood, theta, n_particles, proposal)
        if route is not None:
            kind, network = route
            rows, model = _launch_model(obs, observation_likelihood, theta, time_step)
            out = _kernel_call("particle_filter", proposal, (kind, x0, kernel_theta(network, theta), rows), model,
                               key.to(torch.int32) if key.dtype != torch.int32 else key, float(time_step), n_particles, pos,
                               network=network, return_particles=return_particles)
            if bridge:
                return ParticleFilterResult(*out)
            lw = _gaussian_log_weights(observation_likelihood, obs.values, out[5]) if return_particles else None
            return ParticleFilterResult(*out, lw)
        return _torch_filter(sde, obs, observation_likelihood, theta, float(time_step), n_particles, x0, pos, return_particles, key,
                             bridge, residual)


def _proposal_flags(proposal, like) -> tuple[bool, bool]:
    """``(bridge, residual)`` of a valid ``proposal``: whether the steps are guided, and by the residual bridge."""
    if proposal not in PROPOSALS:
        raise ValueError(f"proposal must be one of {PROPOSALS}, got {proposal!r}")
    if proposal != "bootstrap" and not isinstance(like, GaussianObservationLikelihood):
        raise ValueError(f"proposal='{proposal}' needs a GaussianObservationLikelihood: the proposal is derived from its obs_matrix and "
                         f"variance (got {type(like).__name__})")
    return proposal != "bootstrap", proposal == "residual_bridge"


def _call_key(key, dev) -> Tensor:
    """A call's two key words ``[2]`` on ``dev``: the caller's, or drawn from torch's generator there."""
    if key is None:
        return torch.randint(-2 ** 31, 2 ** 31, (2,), device=dev, dtype=torch.int32)
    key = torch.as_tensor(key).to(dev)
    if key.numel() != 2 or key.is_floating_point():
        raise ValueError("key must hold two 32-bit integer words")
    return key.reshape(2)


def _launch_model(obs, like, like_theta, time_step):
    """The fixed arguments of the kernel launches: ``(rows [K] int32, (observed values, obs_matrix cast to theta's dtype and device
    or None, the Gaussian variance or the count likelihood's kernel terms))``."""
    H = like.obs_matrix
    rows = torch.round(obs.times / time_step).to(torch.int32)
    term = like.kernel_terms(obs.values) if type(like) in COUNT_LIKELIHOODS else float(like.variance)
    return rows, (obs.values, None if H is None else H.to(like_theta), term)


def _kernel_call(name, proposal, head, model, *tail, **keywords):
    """``_hip.<name>(*head, *tail)`` for the bootstrap proposal, ``_hip.guided_<name>(*head, *model, *tail, residual=...)`` for the
    guided ones: the bindings are looked up in ``_hip`` at every call.  The plain filter takes the observation model as well (it
    weighs with it); the plain replays have no use for it."""
    from .. import _hip
    if proposal != "bootstrap":
        return getattr(_hip, "guided_" + name)(*head, *model, *tail, residual=proposal == "residual_bridge", **keywords)
    return getattr(_hip, name)(*head, *(model if name == "particle_filter" else ()), *tail, **keywords)


def _gaussian_log_weights(like, values, particles):
    """``lw [M, K, N]`` of the bootstrap kernel's stored particles [M, K, N, S]: the observation term (any likelihood), NaN as
    -inf."""
    M, K, N, S = particles.shape
    y = values[None, :, None, :].expand(M, K, N, -1).reshape(M * K * N, -1)
    lw = like.log_prob(y, particles.reshape(M * K * N, S)).reshape(M, K, N)
    return torch.where(torch.isnan(lw), torch.full_like(lw, float("-inf")), lw)


def _kernel_route(sde, obs, like, theta, n_particles, proposal="bootstrap"):
    """``builtin_sde_route(sde)`` when the filter kernel takes the call, else None."""
    if not (HIP_FILTER and theta.is_cuda and theta.dtype == torch.float32 and obs.values.dtype == torch.float32):
        return None
    count = type(like) in COUNT_LIKELIHOODS
    if not (count or type(like) is GaussianObservationLikelihood) or (count and proposal != "bootstrap"):
        return None
    kind, network = builtin_sde_route(sde)
    if kind is None:
        return None
    from .. import _hip
    S, O, H = int(sde.state_dim), obs.values.shape[1], like.obs_matrix
    if S > _hip.PF_MAX_STATE or O > _hip.PF_MAX_OBS or (H is None and O != S) or (H is not None and tuple(H.shape) != (O, S)):
        return None
    if proposal != "bootstrap" and (S > _hip.PF_GUIDED_MAX_STATE or O > _hip.PF_GUIDED_MAX_OBS):
        return None
    if n_particles % 64 != 0 or n_particles > _hip.particle_filter_max_particles(kind, S, proposal=proposal):
        return None
    return kind, network


def _floored_cholesky(a: Tensor, floor: Optional[float] = None) -> Tensor:
    """Lower Cholesky factor of a [B, n, n] (its lower triangle is read), column by column; ``floor``: every pivot is clamped there
    before its square root.  Never raises: a NaN or indefinite matrix gives NaN entries."""
    n = a.shape[-1]
    out = torch.zeros_like(a)
    for j in range(n):
        s = a[:, j, j] - (out[:, j, :j] * out[:, j, :j]).sum(dim=-1)
        if floor is not None:
            s = s.clamp(min=floor)
        d = s.sqrt()
        out[:, j, j] = d
        if j + 1 < n:
            out[:, j + 1:, j] = (a[:, j + 1:, j] - (out[:, j + 1:, :j] * out[:, j:j + 1, :j]).sum(dim=-1)) / d[:, None]
    return out


def _bridge_step(sde, x, th, z, y, H, variance, n, dt, root_dt, residual=None):
    """One guided Euler step of the module docstring: (x' before the clamp [B, S], the step's log-ratio [B]).  ``residual``: (eta,
    f(eta), eta_end) of the residual bridge, each [B, S]."""
    f, L = sde.drift(x, th), sde.diffusion(x, th)
    A = root_dt * (L if H is None else torch.einsum("ok,bki->boi", H, L))
    if residual is None:
        ahead = x + (n * dt) * f
    else:
        eta, f_eta, eta_end = residual
        ahead = eta_end + (x - eta) + (n * dt) * (f - f_eta)
    e = y[None, :] - (ahead if H is None else ahead @ H.T)
    O = A.shape[1]
    psi = n * (A @ A.transpose(1, 2)) + variance * torch.eye(O, device=x.device, dtype=x.dtype)
    R = _floored_cholesky(psi)
    sol = torch.linalg.solve_triangular(R, torch.cat([A, e[..., None]], dim=-1), upper=False)
    W, r = sol[..., :-1], sol[..., -1]
    m = torch.einsum("boi,bo->bi", W, r)
    C = torch.eye(x.shape[1], device=x.device, dtype=x.dtype) - W.transpose(1, 2) @ W
    Mf = _floored_cholesky(C, BRIDGE_PIVOT_FLOOR)
    eps = m + torch.einsum("bij,bj->bi", Mf, z)
    lr = -0.5 * (eps * eps).sum(dim=-1) + 0.5 * (z * z).sum(dim=-1) + torch.log(torch.diagonal(Mf, dim1=1, dim2=2)).sum(dim=-1)
    return x + f * dt + torch.einsum("bij,bj->bi", L, eps) * root_dt, lr


def _ode_step(eta, f_eta, dt, floor):
    """One noise-free Euler step of the residual bridge's companion path, with the state's own clamp."""
    eta = eta + f_eta * dt
    return eta if floor is None else torch.maximum(eta, floor)


def _ode_endpoint(sde, x, th, n_steps, dt, floor):
    """``eta_end``: the companion path ``n_steps`` steps after a segment's start state x (the first pass of the residual bridge)."""
    for _ in range(n_steps):
        x = _ode_step(x, sde.drift(x, th), dt, floor)
    return x


def _segment_propagator(sde, obs, like, theta, dt, pos, bridge, residual):
    """The step of the module docstring, stated once for the filter and the two replays (``particle_smoother``, ``particle_mcmc``).
    Returns ``advance(x, th, t0, k, row, paths, key, out=None)``: the states ``x [B, S]`` with parameters ``th [B, P]`` taken over the
    grid steps ``t0 .. row - 1`` towards observation ``k`` at grid row ``row`` (the guided steps look ``row - t`` steps ahead), path b
    on the normals of ``path_normals(paths [B], ., S, key)``; ``out [B, row - t0, S]``: where every state after a step is kept as
    well.  It gives (the end state, the summed log-ratio ``lr [B]`` of the guided steps or None); a segment without steps returns x
    as it is."""
    dev, dtype = theta.device, theta.dtype
    S = int(sde.state_dim)
    floor = _floor_vector(list(pos), S, dev, dtype) if pos else None
    root_dt = dt ** 0.5
    H = like.obs_matrix if bridge else None
    H = None if H is None else H.to(device=dev, dtype=dtype)

    def advance(x, th, t0, k, row, paths, key, out=None):
        lr = torch.zeros(x.shape[0], device=dev, dtype=dtype) if bridge else None
        if residual and t0 < row:
            # a segment starts from a state both the filter and the replays hold, so eta and eta_end are the same in all of them
            eta, eta_end = x, _ode_endpoint(sde, x, th, row - t0, dt, floor)
        z, z_block = None, -1
        for t in range(t0, row):
            if t // 4 != z_block:
                z_block = t // 4
                z = path_normals(paths, z_block, S, key).to(dtype)
            if bridge:
                f_eta = sde.drift(eta, th) if residual else None
                x, step_lr = _bridge_step(sde, x, th, z[..., t % 4], obs.values[k].to(dtype), H, float(like.variance), row - t, dt,
                                          root_dt, (eta, f_eta, eta_end) if residual else None)
                lr = lr + step_lr
                if residual:
                    eta = _ode_step(eta, f_eta, dt, floor)
            else:
                shock = torch.einsum("bij,bj->bi", sde.diffusion(x, th), z[..., t % 4])
                x = x + sde.drift(x, th) * dt + shock * root_dt
            if floor is not None:
                x = torch.maximum(x, floor)
            if out is not None:
                out[:, t - t0] = x
        return x, lr

    return advance


def observation_stage(lw: Tensor, xm: Tensor, k: int, key: Tensor) -> tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    """What a filter does at observation ``k`` once the log-weights ``lw [M, N]`` (no NaN) of its particles ``xm [M, N, S]`` (in the
    dtype of ``lw``) are formed, stated once for ``particle_filter`` and ``jump_particle_filter``: ``(increment [M], ESS [M],
    weighted mean [M, S], weighted std [M, S], ancestors [M, N] int64)`` by the rule of the module docstring, with the dead-filter
    rule (increment -inf, ESS 0, NaN moments, ancestors = identity)."""
    M, N = lw.shape
    neg_inf = torch.tensor(float("-inf"), device=lw.device, dtype=lw.dtype)
    slot = torch.arange(N, device=lw.device)
    mx = lw.max(dim=1, keepdim=True).values
    dead = torch.isneginf(mx)
    w = torch.exp(lw - torch.where(dead, torch.zeros_like(mx), mx))
    s1, s2 = w.sum(dim=1), (w * w).sum(dim=1)
    has = (w > 0)[..., None]
    mean = torch.where(has, w[..., None] * xm, torch.zeros_like(xm)).sum(dim=1) / s1[:, None]
    dx = xm - mean[:, None, :]
    var = torch.where(has, w[..., None] * dx * dx, torch.zeros_like(xm)).sum(dim=1) / s1[:, None]
    incr = torch.where(dead[:, 0], neg_inf, mx[:, 0] + torch.log(s1) - math.log(N))
    ess = torch.where(dead[:, 0], torch.zeros_like(s1), s1 * s1 / s2)
    safe = torch.where(dead, torch.ones_like(w), w)          # a dead filter keeps its particles: its row is overwritten below
    anc = systematic_ancestors(safe, resampling_uniforms(M, k, key))
    return incr, ess, mean, var.sqrt(), torch.where(dead, slot[None, :], anc)


def _torch_filter(sde, obs, like, theta, dt, N, x0, pos, return_particles, key, bridge=False, residual=False) -> ParticleFilterResult:
    dev, dtype = theta.device, theta.dtype
    M, P = theta.shape
    S = x0.shape[1]
    rows = torch.round(obs.times / dt).long().tolist()
    K = len(rows)
    x = x0[:, None, :].expand(M, N, S).reshape(M * N, S).clone()
    th = theta[:, None, :].expand(M, N, P).reshape(M * N, P)
    advance = _segment_propagator(sde, obs, like, theta, dt, pos, bridge, residual)
    b = torch.arange(M * N, device=dev, dtype=torch.int64)          # slot j of filter m draws the normals of path m N + j
    neg_inf = torch.tensor(float("-inf"), device=dev, dtype=dtype)
    incr, ess, means, stds, parts, ancs, lws = [], [], [], [], [], [], []
    t = 0
    for k in range(K):
        x, lr = advance(x, th, t, k, rows[k], b, key)
        t = max(t, rows[k])
        lw = like.log_prob(obs.values[k].to(dtype).unsqueeze(0).expand(M * N, -1), x)
        if bridge:
            lw = lw + lr
        lw = lw.reshape(M, N)
        lw = torch.where(torch.isnan(lw), neg_inf, lw)
        xm = x.reshape(M, N, S)
        inc_k, ess_k, mean, std, anc = observation_stage(lw, xm, k, key)
        incr.append(inc_k)
        ess.append(ess_k)
        means.append(mean)
        stds.append(std)
        if return_particles:
            parts.append(xm)
            ancs.append(anc.to(torch.int32))
            lws.append(lw)
        x = torch.gather(xm, 1, anc[..., None].expand(-1, -1, S)).reshape(M * N, S)
    increments = torch.stack(incr, dim=1)
    return ParticleFilterResult(
        log_likelihood=increments.sum(dim=1), increments=increments, effective_sample_size=torch.stack(ess, dim=1),
        filtered_mean=torch.stack(means, dim=1), filtered_std=torch.stack(stds, dim=1),
        particles=torch.stack(parts, dim=1) if return_particles else None,
        ancestors=torch.stack(ancs, dim=1) if return_particles else None,
        log_weights=torch.stack(lws, dim=1) if return_particles else None)
