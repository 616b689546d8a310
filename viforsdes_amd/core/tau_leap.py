"""Tau-leaping for the jump process of a reaction network: a fixed step ``tau`` with Poisson-many firings of every reaction, on an
integer state.  It stands between the two propagators the package already has: the chemical Langevin SDE cannot represent an
extinction or a handful of individuals, and the exact jump process (``core/jump_process.py``) costs as much as there are events.
A tau-leap costs ``steps x reactions`` whatever the population, and on a GPU every path takes the same steps.

The rule.

Grid: ``rows = round(times / time_step)`` (the rule of ``grid_index``).  Steps ``t = 0, 1, ..`` are global: a path that is read
at row ``r`` has taken steps ``0 .. r - 1``.

Step t of path b from the integer state x:

* ``a_j = jump_propensities(net, x, rates)`` in theta's dtype: the jump process's falling factorials and Hill gates, unchanged.  A
  NaN, infinite or negative ``a_j`` stops the path with status 2, as in ``jump_process``;
* ``lam_j = a_j * tau`` with tau cast to theta's dtype; this one product is then converted to float64.  ``lam_j > 2^30`` gives
  status 2;
* ``n_j = poisson_draw(lam_j, words of (t, j, b))`` for every j: all draws use the propensities at the start of the step.  A draw
  that fails (below) gives status 2;
* the reactions are applied in reaction order with a cap, on the running state (int64):
  ``n_j <- min(n_j, min over the species i with r_ji > 0 of floor(x_i / r_ji))``, ``x <- x + n_j nu_j``.  A reduced ``n_j`` adds
  1 to the path's ``capped`` count.  The state cannot go negative, since ``nu_ji >= -r_ji``;
* any ``x_i > 2^30`` after the step (after the last reaction) gives status 2.

A path that stops at step t keeps the state from before step t, its ``capped`` count does not include step t, and the outputs
it has not reached are -1.

Stream: fourth Philox counter word 8 (0..7 are taken: ``core/jump_process.py`` lists them).  Attempt q of reaction j at step t
uses ``w = philox4x32_10({t, j | ((q >> 1) << 16), b, 8}, key)``, ``u1 = U(w[2 (q & 1)])``, ``u2 = U(w[2 (q & 1) + 1])`` with the
package's ``U(w) = ((w >> 8) + 0.5) 2^-24`` formed in fp32.  A particle slot of ``tau_leap_particle_filter`` keeps its stream
across resampling, as in ``particle_filter``.

``poisson_draw`` runs entirely in float64 on every route; only ``lam`` carries theta's precision.

* ``lam == 0``: the draw is 0 and no words are read;
* ``lam < 10``: inversion by sequential search with ``u1`` of attempt 0: ``p = F = exp(-lam)``, ``n = 0``; while ``u1 > F and n <
  63``: ``n += 1; p = p * (lam / n); F = F + p``.  ``U`` can be exactly 1.0, hence the bound;
* ``lam >= 10``: Hoermann's PTRS (1993) with the published constants ``b = 0.931 + 2.53 sqrt(lam)``, ``a = -0.059 + 0.02483 b``,
  ``1/alpha = 1.1239 + 1.1328 / (b - 3.4)``, ``v_r = 0.9277 - 3.6224 / (b - 2)``.  Attempt q: ``Uc = u1 - 0.5``, ``V = u2``,
  ``us = 0.5 - |Uc|``; reject if ``us < 0.013 and V > us`` (first, before n is formed: ``us`` can be 0); ``n = floor(((2 a) / us +
  b) Uc + lam + 0.43)``; accept if ``us >= 0.07 and V <= v_r``; reject if ``n < 0``; accept if ``(log V + log(1/alpha)) - log(a /
  (us us) + b) <= (-lam + n log lam) - lgamma(n + 1)``.  At most 32 attempts: after the 32nd the draw fails.  (An accepted n is
  far below 2^31 for ``lam <= 2^30``: the last test cannot pass at ``n >= 2 lam``.)

Why float64 in the sampler: the accept test subtracts terms of size ``n log lam``, about 1e5 at ``lam = 1e4``, to get an O(1)
result; in fp32 that decides about a percent of the attempts wrongly.  A step costs R draws, not events, and most attempts are
accepted by the squeeze and never reach ``log`` and ``lgamma``.

How to choose tau: ``capped`` must be 0 or rare (a capped draw is a reaction that ran out of reactants inside a step: the leap
was too long for that state), and where the copy numbers allow it, set ``tau_leap_process`` beside ``jump_process`` at the same
instants with ``ks_two_sample``.

The torch code below is the specification and runs on any device and dtype.  A ``kernel_compatible`` network with CUDA fp32
theta runs ONE HIP kernel instead (csrc/vsde_tau_leap.hip: a thread per trajectory; state, constants and draws in registers)."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import torch
from torch import Tensor

from .jump_process import MAX_COPY_NUMBER, _call_key, _key_words, _rows, _uniform, jump_propensities, philox4x32_10
from .reaction_network import ReactionNetworkSDE

STREAM_WORD = 8                # fourth Philox counter word of the tau-leap draws
MAX_RATE = 2 ** 30             # lam_j above it stops the path
MAX_ATTEMPTS = 32              # PTRS attempts per draw
INVERSION_BELOW = 10.0         # lam below it: inversion; from it on: PTRS
INVERSION_MAX = 63             # the largest draw of the inversion
MAX_ROW = 2 ** 31 - 1          # the step index is a 32-bit counter word (and an int32 of the kernel)
STATUS_COMPLETE, STATUS_INVALID = 0, 2


@dataclass(frozen=True)
class TauLeapResult:
    """Trajectories of ``tau_leap_process``: ``states`` int32 [B, K, S] (-1 where the path stopped before the row), ``status`` int32
    [B] (0 complete, 2 stopped: an invalid propensity, a rate above 2^30, a failed draw or a copy number above 2^30), ``capped``
    int32 [B]: the draws reduced because a reactant would have run out, and with ``record_steps = E > 0`` the raw draws (before the
    cap) of steps 0 .. E - 1: ``draws`` int32 [B, E, R], -1 from the step at which the path stopped (or that it never took) on."""
    states: Tensor
    status: Tensor
    capped: Tensor
    draws: Optional[Tensor] = None

    @property
    def complete(self) -> Tensor:
        return self.status == STATUS_COMPLETE


def _words(key) -> tuple[int, int]:
    if isinstance(key, Tensor):
        return _key_words(key)
    k0, k1 = key
    return int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF


def poisson_draw(lam: Tensor, step, reaction: int, paths: Tensor, key) -> tuple[Tensor, Tensor, Tensor]:
    """The draws of the module docstring for the rates ``lam [B]`` (converted to float64; finite, >= 0) on the words of (``step``:
    an int or int64 ``[B]``, ``reaction``, ``paths [B]`` int64) under ``key`` (two words: a tensor or a pair of ints).  Returns ``(n
    [B] int64, attempts [B] int64, ok [B] bool)``: ``attempts`` is 0 where ``lam == 0`` (no words read), 1 for the inversion, and
    the attempts PTRS made; ``ok`` is False where the 32nd attempt was rejected (``n`` is 0 there)."""
    dev = lam.device
    lam = lam.to(torch.float64)
    k0, k1 = _words(key)
    paths = paths.to(device=dev, dtype=torch.int64)
    zero = torch.zeros_like(paths)
    step = zero + (step.to(device=dev, dtype=torch.int64) if isinstance(step, Tensor) else int(step))
    n, attempts = zero.clone(), zero.clone()
    small, big = (lam > 0) & (lam < INVERSION_BELOW), lam >= INVERSION_BELOW
    ok = torch.ones_like(small)
    if not bool((small | big).any()):
        return n, attempts, ok
    w = philox4x32_10(step, zero + int(reaction), paths, zero + STREAM_WORD, k0, k1)
    if bool(small.any()):
        u1 = _uniform(w[0], torch.float64)
        p = torch.exp(-lam)
        F = p.clone()
        for i in range(1, INVERSION_MAX + 1):
            go = small & (u1 > F) & (n < INVERSION_MAX)         # n == i - 1 where it holds; F is frozen once it fails
            if not bool(go.any()):
                break
            n = n + go.to(torch.int64)
            p = torch.where(go, p * (lam / i), p)
            F = torch.where(go, F + p, F)
        attempts = torch.where(small, attempts + 1, attempts)
    if bool(big.any()):
        b = 0.931 + 2.53 * torch.sqrt(lam)
        a = -0.059 + 0.02483 * b
        inv_alpha = 1.1239 + 1.1328 / (b - 3.4)
        v_r = 0.9277 - 3.6224 / (b - 2.0)
        log_lam, log_inv_alpha = torch.log(lam), torch.log(inv_alpha)
        pending = big.clone()
        for q in range(MAX_ATTEMPTS):
            if not bool(pending.any()):
                break
            if q and q % 2 == 0:
                w = philox4x32_10(step, zero + (int(reaction) | ((q >> 1) << 16)), paths, zero + STREAM_WORD, k0, k1)
            u1, V = _uniform(w[2 * (q & 1)], torch.float64), _uniform(w[2 * (q & 1) + 1], torch.float64)
            Uc = u1 - 0.5
            us = 0.5 - Uc.abs()
            early_reject = (us < 0.013) & (V > us)
            m = torch.floor(((2.0 * a) / us + b) * Uc + lam + 0.43)
            squeeze = ~early_reject & (us >= 0.07) & (V <= v_r)
            rest = ~early_reject & ~squeeze & ~(m < 0)
            lhs = (torch.log(V) + log_inv_alpha) - torch.log(a / (us * us) + b)
            rhs = (-lam + m * log_lam) - torch.lgamma(m + 1.0)
            accept = pending & (squeeze | (rest & (lhs <= rhs)))
            n = torch.where(accept, torch.where(accept, m, torch.zeros_like(m)).to(torch.int64), n)
            attempts = torch.where(pending, zero + (q + 1), attempts)
            pending = pending & ~accept
        ok = ~pending
    return n, attempts, ok


def tau_leap_segment(net, x: Tensor, rates: Tensor, time_step: float, step_begin: int, step_end: int, paths: Tensor, key,
                     draws: Optional[Tensor] = None, live: Optional[Tensor] = None) -> tuple[Tensor, Tensor, Tensor]:
    """Steps ``step_begin .. step_end - 1`` of the module docstring for the integer states ``x [B, S]`` (int64) with the effective
    constants ``rates`` (``[B, 2R]``, or ``[B, R]`` for a plain network), path b = ``paths [B]`` (int64).  ``live [B]`` (bool,
    default all): the paths that step at all.  Returns ``(x [B, S] int64, status [B] int32: 0 or 2, capped [B] int32)``; a stopped
    path keeps the state from before the step it stopped at.  ``draws`` (int32 ``[B, E, R]``, written in place): row t takes the
    raw draws of step t < E of the paths that complete it."""
    dev, dtype = rates.device, rates.dtype
    B, R = x.shape[0], net.num_reactions
    words = _words(key)
    nu = torch.tensor(net.change, dtype=torch.int64, device=dev)
    tau = torch.tensor(float(time_step), dtype=dtype, device=dev)
    status = torch.zeros(B, dtype=torch.int32, device=dev)
    capped = torch.zeros(B, dtype=torch.int32, device=dev)
    live = torch.ones(B, dtype=torch.bool, device=dev) if live is None else live.clone()
    for t in range(int(step_begin), int(step_end)):
        if not bool(live.any()):
            break
        a = jump_propensities(net, x, rates)
        lam = (a * tau).to(torch.float64)
        bad = (~(a >= 0) | torch.isinf(a)).any(dim=-1) | (lam > MAX_RATE).any(dim=-1)
        go = live & ~bad
        raw = []
        for j in range(R):
            n_j, _, ok = poisson_draw(torch.where(go, lam[:, j], torch.zeros_like(lam[:, j])), t, j, paths, words)
            bad = bad | ~ok
            raw.append(n_j)
        xn, reduced = x, torch.zeros(B, dtype=torch.int32, device=dev)
        for j, row in enumerate(net.reactants):
            n_j = raw[j]
            for i, r in enumerate(row):
                if r > 0:
                    n_j = torch.minimum(n_j, torch.div(xn[:, i], int(r), rounding_mode="floor"))
            reduced = reduced + (n_j < raw[j]).to(torch.int32)
            xn = xn + n_j[:, None] * nu[j]
        bad = bad | (xn > MAX_COPY_NUMBER).any(dim=-1)
        done = live & ~bad
        x = torch.where(done[:, None], xn, x)
        capped = capped + torch.where(done, reduced, torch.zeros_like(reduced))
        status = torch.where(live & bad, torch.full_like(status, STATUS_INVALID), status)
        if draws is not None and t < draws.shape[1]:
            draws[:, t] = torch.where(done[:, None], torch.stack(raw, dim=-1).to(torch.int32), draws[:, t])
        live = done
    return x, status, capped


def grid_rows(times, time_step: float, what: str = "times") -> Tensor:
    """``round(times / time_step)`` as int64 on the host for the float64 ``times`` (finite, >= 0, non-decreasing)."""
    host = torch.as_tensor(times, dtype=torch.float64).detach().cpu()
    if host.ndim != 1 or host.numel() < 1:
        raise ValueError(f"{what} must be a non-empty 1-D tensor, got shape {tuple(host.shape)}")
    if not bool(torch.isfinite(host).all()) or bool((host < 0).any()) or bool((host[1:] < host[:-1]).any()):
        raise ValueError(f"{what} must be finite, >= 0 and non-decreasing")
    if not (isinstance(time_step, (int, float)) and time_step > 0 and time_step < float("inf")):
        raise ValueError(f"time_step must be positive and finite, got {time_step}")
    rows = torch.round(host / float(time_step))
    if float(rows[-1]) > MAX_ROW:
        raise ValueError(f"{what} / time_step reaches row {float(rows[-1]):.3g}: at most 2^31 - 1 steps")
    return rows.to(torch.int64)


def _tau_leap_process_torch(net, x0: Tensor, rates: Tensor, rows: Tensor, time_step: float, key: Tensor, E: int):
    dev = rates.device
    B, S = x0.shape
    K, R = rows.shape[0], net.num_reactions
    x = x0.to(torch.int64).clone()
    paths = torch.arange(B, dtype=torch.int64, device=dev)
    states = torch.full((B, K, S), -1, dtype=torch.int32, device=dev)
    status = torch.zeros(B, dtype=torch.int32, device=dev)
    capped = torch.zeros(B, dtype=torch.int32, device=dev)
    draws = torch.full((B, E, R), -1, dtype=torch.int32, device=dev) if E else None
    words = _key_words(key)
    t = 0
    for k, row in enumerate(rows.tolist()):
        live = status == STATUS_COMPLETE
        x, st, cap = tau_leap_segment(net, x, rates, time_step, t, row, paths, words, draws=draws, live=live)
        status = torch.where(live, st, status)
        capped = capped + cap
        t = row
        ok = status == STATUS_COMPLETE
        states[:, k] = torch.where(ok[:, None], x.to(torch.int32), states[:, k])
    return states, status, capped, draws


def tau_leap_process(net: ReactionNetworkSDE, x0, theta: Tensor, times, time_step: float, n_paths: Optional[int] = None, key=None,
                     record_steps: int = 0) -> TauLeapResult:
    """B tau-leap trajectories of the jump process of ``net`` (module docstring) with the step ``time_step``, read at the grid rows
    ``round(times / time_step)``.

    ``x0``, ``theta``, ``n_paths``, ``times`` and ``key`` are those of ``jump_process`` and are validated in the same way; in
    addition ``time_step > 0``.  ``record_steps = E > 0`` also returns the raw draws of the first E steps.  No gradients.

    A ``kernel_compatible()`` network with CUDA fp32 theta runs the HIP kernel; everything else (any network, CPU, float64) runs
    the torch specification.  Both follow the same rules on the same words; the kernel forms its propensities in fp32."""
    if not isinstance(net, ReactionNetworkSDE):
        raise ValueError("tau_leap_process needs a ReactionNetworkSDE: the jump process is defined by its reactions")
    theta = torch.as_tensor(theta)
    if not theta.is_floating_point():
        raise ValueError("theta must be a floating-point tensor")
    dev = theta.device
    theta = _rows("theta", theta.detach(), net.sde_param_dim, "P")
    x0 = _rows("x0", torch.as_tensor(x0).detach(), net.state_dim, "S")
    if x0.is_floating_point() and not bool((torch.isfinite(x0) & (x0 == x0.round())).all()):
        raise ValueError("x0 must hold integers (copy numbers)")
    x0 = x0.to(torch.int64)
    if bool((x0 < 0).any()) or bool((x0 > MAX_COPY_NUMBER).any()):
        raise ValueError(f"x0 must lie in 0 .. 2^30, got {int(x0.min())} .. {int(x0.max())}")
    x0 = x0.to(dev)
    n_rows = {x0.shape[0], theta.shape[0]} - {1}
    if len(n_rows) > 1:
        raise ValueError(f"x0 has {x0.shape[0]} rows but theta has {theta.shape[0]}")
    B = n_rows.pop() if n_rows else (1 if n_paths is None else int(n_paths))
    if n_paths is not None and int(n_paths) != B:
        raise ValueError(f"n_paths = {n_paths} but x0 / theta have {B} rows")
    if not 1 <= B < 2 ** 32:
        raise ValueError(f"the number of paths must be in 1 .. 2^32 - 1, got {B}")
    E = int(record_steps)
    if E < 0:
        raise ValueError(f"record_steps must be >= 0, got {record_steps}")
    rows = grid_rows(times, time_step)
    x0, theta = x0.expand(B, -1), theta.expand(B, -1)
    key = _call_key(key, dev)
    if net.kernel_compatible() and theta.is_cuda and theta.dtype == torch.float32:
        from .. import _hip
        from .sde import kernel_theta
        network = net.kernel_descriptor()
        out = _hip.tau_leap_process(x0.to(torch.int32).contiguous(), kernel_theta(network, theta).contiguous(),
                                    rows.to(device=dev, dtype=torch.int32), key.to(torch.int32), float(time_step), E, network=network)
    else:
        out = _tau_leap_process_torch(net, x0, theta if net.plain else net.kernel_parameters(theta), rows, float(time_step), key, E)
    return TauLeapResult(*out)
