"""The Markov jump process of a reaction network on integer copy numbers, simulated exactly (Gillespie's direct method), and a
check of its diffusion approximation.

``ReactionNetworkSDE`` runs the chemical Langevin SDE of a network: the diffusion approximation of a jump process whose state
``x`` counts molecules, cases or animals.  ``jump_process`` simulates that process itself, so that synthetic count data need not
come from the approximation being fitted, and ``diffusion_approximation_check`` runs both from the same start and compares
them: the one diagnostic that asks whether the SDE is adequate at these copy numbers, not whether q fits the SDE.

The process.  With the effective constants ``k_0..k_{R-1}, K_0..K_{R-1}`` of theta (``kernel_parameters``; theta itself for a
plain network), the propensity of reaction j at the state x is

* mass action: ``a_j = k_j * prod_i x_i (x_i - 1) .. (x_i - r_ji + 1)``, the falling factorial, by repeated multiplication in
  species order on x converted to theta's dtype.  As everywhere in the package there is no ``1 / r!`` factor (such constants
  belong in k_j).  It is 0 once ``x_i < r_ji``, so the state never goes negative.  For orders <= 1 it is the propensity of the
  SDE; for orders 2 and 3 it differs from the SDE's ``x^r`` by a relative ``O(1 / x)``;
* Hill laws: the SDE's expression (``reaction_network.propensities``, the same operation order) with ``u = x_s``, multiplied by
  the gate ``1[x_i >= r_ji for all i]``: the reactant row of a rate-law reaction still consumes.

Event e (0-based) of path b: ``c_j = a_0 + .. + a_j`` in reaction order and in theta's dtype, ``a0 = c_{R-1}``.  A propensity
that is NaN, infinite or negative (a negative theta), or an infinite a0, ends the path with status 2.  ``a0 = 0``: the state is
absorbed and fills every remaining output (status 0).  Otherwise ``tau = -log(u1) / a0``, ``t <- t + tau`` with the clock t in
float64 whatever theta's dtype (an fp32 clock drops increments below half an ulp of t: a bias, and without the event cap a loop
that never ends), the reaction is the smallest j with ``u2 * a0 < c_j`` (none after rounding: the last j with ``a_j > 0``) and
``x <- x + nu_j``.  Output time ``T_k`` receives the state after every event with time <= ``T_k``.

Stream: ``w = philox4x32_10(counter {e >> 1, 0, b, 7}, key)``, ``u1 = U(w[2 (e & 1)])``, ``u2 = U(w[2 (e & 1) + 1])`` with
``U(w) = ((w >> 8) + 0.5) * 2^-24`` formed in fp32.  Fourth counter words 0..6 are the path normals, the resampling uniforms, the
smoother's final draw and the four PMMH draws; 7 is this stream.  The same key gives the same result on a route.  The free second
counter word carries the segment index of the jump-process particle filter (``jump_segment``, inference/jump_filter.py), whose
segment 0 is this process.

The torch code below is the specification.  It is vectorised over the B paths with a live mask, one Python iteration per event,
and runs on any device in theta's dtype.  A ``kernel_compatible`` network with CUDA fp32 theta runs ONE HIP kernel instead
(csrc/vsde_jump.hip: a thread per trajectory, state, constants and clock in registers)."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Sequence

import torch
from torch import Tensor

from .forecast import forecast_states
from .reaction_network import LAW_HILL_ACTIVATION, ReactionNetworkSDE

MAX_EVENTS_LIMIT = 2 ** 23     # csrc/vsde_jump.hip: kJumpMaxEvents
MAX_COPY_NUMBER = 2 ** 30      # 2^30 + 127 * 2^23 < 2^31: with int8 net changes an int32 state cannot overflow
STREAM_WORD = 7                # fourth Philox counter word of the jump process
STATUS_COMPLETE, STATUS_EVENT_CAP, STATUS_INVALID = 0, 1, 2

_M0, _M1, _W0, _W1, _MASK = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 0xFFFFFFFF


@dataclass(frozen=True)
class JumpProcessResult:
    """Trajectories of ``jump_process``: ``states`` int32 [B, K, S] (-1 where the path stopped early), ``n_events`` int32 [B],
    ``status`` int32 [B] (0 complete, 1 event cap, 2 invalid propensity), and with ``record_events = E > 0`` the first E events
    of each path: ``event_times`` float64 [B, E] (NaN past the last one) and ``event_reactions`` int32 [B, E] (-1 past it)."""
    states: Tensor
    n_events: Tensor
    status: Tensor
    event_times: Optional[Tensor] = None
    event_reactions: Optional[Tensor] = None

    @property
    def complete(self) -> Tensor:
        return self.status == STATUS_COMPLETE


def _mulhilo(m: int, c: Tensor) -> tuple[Tensor, Tensor]:
    """(high, low) 32-bit words of m * c for a 32-bit constant m and 32-bit values c held in int64 (split: no int64 overflow)."""
    p_lo, p_hi = m * (c & 0xFFFF), m * (c >> 16)              # each < 2^48; the product is p_hi * 2^16 + p_lo
    s = ((p_hi & 0xFFFF) << 16) + (p_lo & _MASK)
    return (p_hi >> 16) + (p_lo >> 32) + (s >> 32), s & _MASK


def philox4x32_10(c0: Tensor, c1: Tensor, c2: Tensor, c3: Tensor, k0: int, k1: int) -> list:
    """The four output words (int64 tensors holding 32-bit values) of Philox4x32-10 for counters c0..c3 and key (k0, k1)."""
    c = [c0, c1, c2, c3]
    k0, k1 = k0 & _MASK, k1 & _MASK
    for _ in range(10):
        hi0, lo0 = _mulhilo(_M0, c[0])
        hi1, lo1 = _mulhilo(_M1, c[2])
        c = [hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0]
        k0, k1 = (k0 + _W0) & _MASK, (k1 + _W1) & _MASK
    return c


def _uniform(w: Tensor, dtype) -> Tensor:
    """``((w >> 8) + 0.5) * 2^-24`` in fp32 (in (0, 1]: the sum rounds to even once w >> 8 needs all 24 bits), then cast."""
    return (((w >> 8).to(torch.float32) + 0.5) * (2.0 ** -24)).to(dtype)


def jump_propensities(net: ReactionNetworkSDE, x: Tensor, rates: Tensor) -> Tensor:
    """``a [B, R]`` of the jump process at the integer states ``x [B, S]`` for the effective constants ``rates`` ``[B, 2R]``
    (``[B, R]`` serves a network without rate laws), in the dtype of ``rates``; see the module docstring."""
    R = net.num_reactions
    xf = x.to(rates.dtype)
    cols = []
    for j, row in enumerate(net.reactants):
        law = net.laws[j]
        if law is not None:
            code, s, n = law[:3]
            u, K = xf[:, s], rates[:, R + j]
            a, c = u, K
            for _ in range(n - 1):
                a, c = a * u, c * K
            gate = torch.ones_like(u)
            for i, r in enumerate(row):
                if r > 0:
                    gate = gate * (x[:, i] >= r).to(rates.dtype)
            cols.append(rates[:, j] * ((a if code == LAW_HILL_ACTIVATION else c) / (c + a)) * gate)
            continue
        m = None
        for i, r in enumerate(row):
            for q in range(r):
                fac = xf[:, i] - q if q else xf[:, i]
                m = fac if m is None else m * fac
        cols.append(rates[:, j] if m is None else rates[:, j] * m)
    return torch.stack(cols, dim=-1)


def _key_words(key: Tensor) -> tuple[int, int]:
    k = key.reshape(2).to("cpu", torch.int64) & _MASK
    return int(k[0]), int(k[1])


def _jump_process_torch(net, x0: Tensor, rates: Tensor, times: Tensor, key: Tensor, max_events: int, E: int):
    dev, dtype = rates.device, rates.dtype
    B, S = x0.shape
    K, R = times.shape[0], net.num_reactions
    k0, k1 = _key_words(key)
    nu = torch.tensor(net.change, dtype=torch.int64, device=dev)
    x = x0.to(torch.int64).clone()
    t = torch.zeros(B, dtype=torch.float64, device=dev)
    k = torch.zeros(B, dtype=torch.int64, device=dev)
    n_events = torch.zeros(B, dtype=torch.int32, device=dev)
    status = torch.zeros(B, dtype=torch.int32, device=dev)
    states = torch.full((B, K, S), -1, dtype=torch.int32, device=dev)
    ev_t = torch.full((B, E), float("nan"), dtype=torch.float64, device=dev) if E else None
    ev_r = torch.full((B, E), -1, dtype=torch.int32, device=dev) if E else None
    live = torch.ones(B, dtype=torch.bool, device=dev)
    path = torch.arange(B, dtype=torch.int64, device=dev)
    zero = torch.zeros_like(path)
    inf = torch.full((B,), float("inf"), dtype=torch.float64, device=dev)
    w = None
    for e in range(max_events):
        if not bool(live.any()):
            break
        a = jump_propensities(net, x, rates)
        c = [a[:, 0]]
        for j in range(1, R):
            c.append(c[-1] + a[:, j])
        c = torch.stack(c, dim=-1)
        a0 = c[:, -1]
        bad = live & ((~(a >= 0) | torch.isinf(a)).any(dim=-1) | torch.isinf(a0))
        status[bad] = STATUS_INVALID
        live = live & ~bad
        if e % 2 == 0:
            w = philox4x32_10(zero + (e >> 1), zero, path, zero + STREAM_WORD, k0, k1)
        u1, u2 = _uniform(w[2 * (e & 1)], dtype), _uniform(w[2 * (e & 1) + 1], dtype)
        t_next = torch.where(a0 == 0, inf, t + (-torch.log(u1) / a0).to(torch.float64))
        for _ in range(K):                   # outputs before the event take the state before it
            due = live & (k < K)
            due = due & (times[k.clamp(max=K - 1)] < t_next)
            if not bool(due.any()):
                break
            states[path[due], k[due]] = x[due].to(torch.int32)
            k = k + due.to(torch.int64)
        live = live & (k < K)
        below = (u2 * a0).unsqueeze(-1) < c
        first = below.to(torch.int8).argmax(dim=-1)
        last_positive = (R - 1) - (a > 0).flip(-1).to(torch.int8).argmax(dim=-1)
        j = torch.where(below.any(dim=-1), first, last_positive)
        x = torch.where(live.unsqueeze(-1), x + nu[j], x)
        t = torch.where(live, t_next, t)
        if e < E:
            ev_t[:, e] = torch.where(live, t, ev_t[:, e])
            ev_r[:, e] = torch.where(live, j.to(torch.int32), ev_r[:, e])
        n_events = n_events + live.to(torch.int32)
    status[live] = STATUS_EVENT_CAP
    return states, n_events, status, ev_t, ev_r


def jump_segment(net, x: Tensor, rates: Tensor, t_start: float, t_end: float, segment: int, paths: Tensor, key: Tensor,
                 max_events: int) -> tuple[Tensor, Tensor, Tensor]:
    """The event rule of the module docstring over ONE segment ``(t_start, t_end]``, for the jump-process particle filter
    (inference/jump_filter.py): the integer states ``x [B, S]`` (int64) with the effective constants ``rates``, path b = ``paths
    [B]`` (int64) on the uniforms of ``philox4x32_10({e >> 1, segment, paths[b], 7}, key)``.  The float64 clock starts at exactly
    ``t_start`` (the waiting times are memoryless) and the event counter at 0; a path ends the segment as soon as ``t_end < t +
    tau`` (``a0 == 0``: at once, absorbed), stops with status 2 at an invalid propensity and with status 1 once it has fired
    ``max_events`` events short of ``t_end``; a stopped path keeps the state it stopped in.  Returns ``(x [B, S] int64, n_events
    [B] int32, status [B] int32)``.  Segment 0 from ``t_start = 0`` is ``jump_process`` read at ``[t_end]``."""
    dev, dtype = rates.device, rates.dtype
    B, R = x.shape[0], net.num_reactions
    k0, k1 = _key_words(key)
    nu = torch.tensor(net.change, dtype=torch.int64, device=dev)
    t = torch.full((B,), float(t_start), dtype=torch.float64, device=dev)
    n_events = torch.zeros(B, dtype=torch.int32, device=dev)
    status = torch.zeros(B, dtype=torch.int32, device=dev)
    live = torch.ones(B, dtype=torch.bool, device=dev)
    zero = torch.zeros_like(paths)
    inf = torch.full((B,), float("inf"), dtype=torch.float64, device=dev)
    w = None
    for e in range(max_events):
        if not bool(live.any()):
            break
        a = jump_propensities(net, x, rates)
        c = [a[:, 0]]
        for j in range(1, R):
            c.append(c[-1] + a[:, j])
        c = torch.stack(c, dim=-1)
        a0 = c[:, -1]
        bad = live & ((~(a >= 0) | torch.isinf(a)).any(dim=-1) | torch.isinf(a0))
        status[bad] = STATUS_INVALID
        live = live & ~bad
        if e % 2 == 0:
            w = philox4x32_10(zero + (e >> 1), zero + int(segment), paths, zero + STREAM_WORD, k0, k1)
        u1, u2 = _uniform(w[2 * (e & 1)], dtype), _uniform(w[2 * (e & 1) + 1], dtype)
        t_next = torch.where(a0 == 0, inf, t + (-torch.log(u1) / a0).to(torch.float64))
        live = live & ~(t_end < t_next)
        below = (u2 * a0).unsqueeze(-1) < c
        first = below.to(torch.int8).argmax(dim=-1)
        last_positive = (R - 1) - (a > 0).flip(-1).to(torch.int8).argmax(dim=-1)
        j = torch.where(below.any(dim=-1), first, last_positive)
        x = torch.where(live.unsqueeze(-1), x + nu[j], x)
        t = torch.where(live, t_next, t)
        n_events = n_events + live.to(torch.int32)
    status[live] = STATUS_EVENT_CAP
    return x, n_events, status


def jump_segment_states(net, x: Tensor, rates: Tensor, t_start: float, t_end: float, segment: int, paths: Tensor, key: Tensor,
                        max_events: int, out_times) -> tuple[Tensor, Tensor, Tensor, Tensor]:
    """``jump_segment`` (the same loop on the same uniforms, the same three results bit for bit) that also reads the path at the
    instants ``out_times`` (non-decreasing floats or a float64 tensor ``[Q]``, inside the segment): output ``t_q`` receives the state
    after every event with time ``<= t_q``, the rule of ``jump_process``: before the event at ``t_next`` is applied, every ``t_q <
    t_next`` not yet written takes the current state.  A path that ends the segment (status 0) has written all of them by then; a
    stopped one (status 1 or 2) leaves -1 in those it did not reach.  Returns ``(x [B, S] int64, n_events [B] int32, status [B]
    int32, states [B, Q, S] int32)``; the replay of the jump-process smoother and of PMMH paths (inference/jump_smoother.py).
    ``key`` may also be ``[B, 2]``: a key per path (the records of PMMH come from filters of different iterations)."""
    dev, dtype = rates.device, rates.dtype
    B, R, S = x.shape[0], net.num_reactions, x.shape[1]
    if key.ndim == 2:
        k0, k1 = (key.to(device=dev, dtype=torch.int64) & _MASK).unbind(dim=1)
    else:
        k0, k1 = _key_words(key)
    nu = torch.tensor(net.change, dtype=torch.int64, device=dev)
    out_times = torch.as_tensor(out_times, dtype=torch.float64).reshape(-1).to(dev)
    Q = out_times.shape[0]
    states = torch.full((B, Q, S), -1, dtype=torch.int32, device=dev)
    q = torch.zeros(B, dtype=torch.int64, device=dev)
    row = torch.arange(B, dtype=torch.int64, device=dev)
    t = torch.full((B,), float(t_start), dtype=torch.float64, device=dev)
    n_events = torch.zeros(B, dtype=torch.int32, device=dev)
    status = torch.zeros(B, dtype=torch.int32, device=dev)
    live = torch.ones(B, dtype=torch.bool, device=dev)
    zero = torch.zeros_like(paths)
    inf = torch.full((B,), float("inf"), dtype=torch.float64, device=dev)
    w = None
    for e in range(max_events):
        if not bool(live.any()):
            break
        a = jump_propensities(net, x, rates)
        c = [a[:, 0]]
        for j in range(1, R):
            c.append(c[-1] + a[:, j])
        c = torch.stack(c, dim=-1)
        a0 = c[:, -1]
        bad = live & ((~(a >= 0) | torch.isinf(a)).any(dim=-1) | torch.isinf(a0))
        status[bad] = STATUS_INVALID
        live = live & ~bad
        if e % 2 == 0:
            w = philox4x32_10(zero + (e >> 1), zero + int(segment), paths, zero + STREAM_WORD, k0, k1)
        u1, u2 = _uniform(w[2 * (e & 1)], dtype), _uniform(w[2 * (e & 1) + 1], dtype)
        t_next = torch.where(a0 == 0, inf, t + (-torch.log(u1) / a0).to(torch.float64))
        for _ in range(Q):                   # outputs before the event take the state before it
            due = live & (q < Q)
            due = due & (out_times[q.clamp(max=Q - 1)] < t_next)
            if not bool(due.any()):
                break
            states[row[due], q[due]] = x[due].to(torch.int32)
            q = q + due.to(torch.int64)
        live = live & ~(t_end < t_next)
        below = (u2 * a0).unsqueeze(-1) < c
        first = below.to(torch.int8).argmax(dim=-1)
        last_positive = (R - 1) - (a > 0).flip(-1).to(torch.int8).argmax(dim=-1)
        j = torch.where(below.any(dim=-1), first, last_positive)
        x = torch.where(live.unsqueeze(-1), x + nu[j], x)
        t = torch.where(live, t_next, t)
        n_events = n_events + live.to(torch.int32)
    status[live] = STATUS_EVENT_CAP
    if Q:
        # status 0 wrote every output on the way (t_q <= t_end < t_next) unless an output lies past t_end: the final state
        rest = (torch.arange(Q, device=dev)[None, :] >= q[:, None]) & (status == STATUS_COMPLETE)[:, None]
        states = torch.where(rest[:, :, None], x.to(torch.int32)[:, None, :], states)
    return x, n_events, status, states


def _rows(name: str, t: Tensor, width: int, what: str) -> Tensor:
    if t.ndim == 1:
        t = t.unsqueeze(0)
    if t.ndim != 2 or t.shape[1] != width or t.shape[0] < 1:
        raise ValueError(f"{name} must be [{what}] or [B, {what}] with {what} = {width}, got {tuple(t.shape)}")
    return t


def _call_key(key, dev) -> Tensor:
    from ..inference.particle_filter import _call_key as call_key
    return call_key(key, dev)


def jump_process(net: ReactionNetworkSDE, x0, theta: Tensor, times, n_paths: Optional[int] = None, key=None,
                 max_events: int = 2 ** 20, record_events: int = 0) -> JumpProcessResult:
    """B exact trajectories of the jump process of ``net`` (module docstring) read at ``times``.

    ``x0`` is ``[S]`` or ``[B, S]``, of any dtype but holding integers in ``0 .. 2^30``; ``theta`` is ``[P]`` or ``[B, P]``;
    ``n_paths`` gives B when both are single rows (default 1).  ``times``: 1-D, non-decreasing, >= 0 (duplicates and 0 are
    allowed), taken as float64.  ``key``: two 32-bit integer words, or None to draw them from torch's generator on theta's
    device.  A path that has fired ``max_events`` (``1 .. 2^23``) events before its last output time stops with status 1; the
    outputs it did not reach are -1.  ``record_events = E > 0`` also returns the first E events of each path.  No gradients.

    A ``kernel_compatible()`` network with CUDA fp32 theta runs the HIP kernel; everything else (any network, CPU, float64)
    runs the torch specification.  Both follow the same rules on the same uniforms; the kernel forms its propensities in fp32."""
    if not isinstance(net, ReactionNetworkSDE):
        raise ValueError("jump_process needs a ReactionNetworkSDE: the jump process is defined by its reactions")
    theta = torch.as_tensor(theta)
    if not theta.is_floating_point():
        raise ValueError("theta must be a floating-point tensor")
    dev = theta.device
    theta = _rows("theta", theta.detach(), net.sde_param_dim, "P")
    x0 = _rows("x0", torch.as_tensor(x0).detach(), net.state_dim, "S")      # checked where it lives: a host x0 costs no sync
    if x0.is_floating_point() and not bool((torch.isfinite(x0) & (x0 == x0.round())).all()):
        raise ValueError("x0 must hold integers (copy numbers)")
    x0 = x0.to(torch.int64)
    if bool((x0 < 0).any()) or bool((x0 > MAX_COPY_NUMBER).any()):
        raise ValueError(f"x0 must lie in 0 .. 2^30, got {int(x0.min())} .. {int(x0.max())}")
    x0 = x0.to(dev)
    rows = {x0.shape[0], theta.shape[0]} - {1}
    if len(rows) > 1:
        raise ValueError(f"x0 has {x0.shape[0]} rows but theta has {theta.shape[0]}")
    B = rows.pop() if rows else (1 if n_paths is None else int(n_paths))
    if n_paths is not None and int(n_paths) != B:
        raise ValueError(f"n_paths = {n_paths} but x0 / theta have {B} rows")
    if not 1 <= B < 2 ** 32:
        raise ValueError(f"the number of paths must be in 1 .. 2^32 - 1, got {B}")
    max_events, E = int(max_events), int(record_events)
    if not 1 <= max_events <= MAX_EVENTS_LIMIT:
        raise ValueError(f"max_events must be in 1 .. 2^23, got {max_events}")
    if E < 0:
        raise ValueError(f"record_events must be >= 0, got {record_events}")
    times = torch.as_tensor(times, dtype=torch.float64).detach()
    if times.ndim != 1 or times.numel() < 1:
        raise ValueError(f"times must be a non-empty 1-D tensor, got shape {tuple(times.shape)}")
    host = times.cpu()
    if not bool(torch.isfinite(host).all()) or bool((host < 0).any()) or bool((host[1:] < host[:-1]).any()):
        raise ValueError("times must be finite, >= 0 and non-decreasing")
    times = times.to(dev)
    x0, theta = x0.expand(B, -1), theta.expand(B, -1)
    key = _call_key(key, dev)
    if net.kernel_compatible() and theta.is_cuda and theta.dtype == torch.float32:
        from .. import _hip
        from .sde import kernel_theta
        network = net.kernel_descriptor()
        out = _hip.jump_process(x0.to(torch.int32).contiguous(), kernel_theta(network, theta).contiguous(), times,
                                key.to(torch.int32), max_events, E, network=network)
    else:
        out = _jump_process_torch(net, x0, theta if net.plain else net.kernel_parameters(theta), times, key, max_events, E)
    return JumpProcessResult(*out)


@dataclass(frozen=True)
class DiffusionApproximationCheck:
    """The jump process of a network against its chemical Langevin SDE from the same start, at the same instants and with the
    same theta rows (``diffusion_approximation_check``).  Moments are over the n complete jump paths (and the SDE paths of the
    same rows); K instants, S species.

    ``times [K]`` (the grid instants read), ``jump_states`` / ``diffusion_states [n, K, S]``, ``jump_mean``, ``jump_std``,
    ``diffusion_mean``, ``diffusion_std [K, S]`` (population standard deviations), ``mean_shift`` = (diffusion_mean -
    jump_mean) / jump_std (NaN where jump_std is 0), ``std_ratio`` = diffusion_std / jump_std (NaN there too), ``ks_distance
    [K, S]``: the two-sample Kolmogorov statistic, ``zero_fraction [K, S]``: the share of jump paths with the species at 0,
    where the SDE sits on its clamp instead, and ``n_incomplete``: the jump paths left out."""
    times: Tensor
    jump_states: Tensor
    diffusion_states: Tensor
    jump_mean: Tensor
    jump_std: Tensor
    diffusion_mean: Tensor
    diffusion_std: Tensor
    mean_shift: Tensor
    std_ratio: Tensor
    ks_distance: Tensor
    zero_fraction: Tensor
    n_incomplete: int


def ks_two_sample(a: Tensor, b: Tensor) -> Tensor:
    """The two-sample Kolmogorov statistic ``sup_v |F_a(v) - F_b(v)|`` along dim 0 of ``a [n, ...]`` and ``b [m, ...]``, by one
    sort of the pooled sample: F_a - F_b is read after the last of every run of equal values."""
    n, m = a.shape[0], b.shape[0]
    pooled = torch.cat([a, b], dim=0)
    is_a = torch.cat([torch.ones_like(a), torch.zeros_like(b)], dim=0)
    v, order = torch.sort(pooled, dim=0, stable=True)
    from_a = torch.gather(is_a, 0, order)
    diff = torch.cumsum(from_a / n - (1 - from_a) / m, dim=0)
    end_of_run = torch.ones_like(v, dtype=torch.bool)
    end_of_run[:-1] = v[1:] != v[:-1]
    return torch.where(end_of_run, diff.abs(), torch.zeros_like(diff)).amax(dim=0)


def diffusion_approximation_check(net: ReactionNetworkSDE, x0, theta: Tensor, times, time_step: float, n_paths: int = 4096,
                                  positive_dims: Optional[Sequence[int]] = None, key=None,
                                  max_events: int = 2 ** 20) -> DiffusionApproximationCheck:
    """Run the jump process (``jump_process``) and the Euler-Maruyama discretised SDE (``forecast_states``, ``time_step``) of
    ``net`` from the same integer ``x0`` with the same theta rows and compare them at ``times``.

    A time maps to the grid step ``round(t / time_step)`` (the rule of ``grid_index``), which must be >= 1; both processes are
    read at ``step * time_step``.  ``theta`` is ``[P]`` (``n_paths`` paths) or ``[n, P]``, for example
    ``post.sample(n).sde_parameters``.  ``positive_dims`` (the SDE's clamped dims) defaults to all species."""
    if time_step <= 0:
        raise ValueError(f"time_step must be positive, got {time_step}")
    theta = torch.as_tensor(theta).detach()
    if theta.ndim == 1:
        theta = theta.unsqueeze(0).expand(int(n_paths), -1)
    B = theta.shape[0]
    t_in = torch.as_tensor(times, dtype=torch.float64).reshape(-1).cpu()
    if t_in.numel() < 1:
        raise ValueError("times must not be empty")
    steps = torch.round(t_in / time_step).long()
    if bool((steps < 1).any()) or bool((steps[1:] < steps[:-1]).any()):
        raise ValueError("times must be non-decreasing and each map to a grid step round(t / time_step) >= 1")
    grid_times = steps.to(torch.float64) * time_step
    key = _call_key(key, theta.device)
    jump = jump_process(net, x0, theta, grid_times, n_paths=B, key=key, max_events=max_events)
    x_start = _rows("x0", torch.as_tensor(x0).detach(), net.state_dim, "S").to(theta).expand(B, -1).contiguous()
    pos = tuple(range(net.state_dim)) if positive_dims is None else tuple(positive_dims)
    diff = forecast_states(net, x_start, theta.contiguous(), int(steps[-1]), steps.tolist(), float(time_step), pos)
    ok = jump.complete
    js, ds = jump.states[ok].to(torch.float64), diff[ok].to(torch.float64)
    nan = torch.full(js.shape[1:], float("nan"), dtype=torch.float64, device=js.device)
    if js.shape[0] == 0:
        stats = [nan] * 8
    else:
        jm, dm = js.mean(dim=0), ds.mean(dim=0)
        jsd, dsd = js.std(dim=0, unbiased=False), ds.std(dim=0, unbiased=False)
        flat = jsd == 0
        stats = [jm, jsd, dm, dsd, torch.where(flat, nan, (dm - jm) / jsd), torch.where(flat, nan, dsd / jsd),
                 ks_two_sample(js, ds), (js == 0).to(torch.float64).mean(dim=0)]
    return DiffusionApproximationCheck(grid_times.to(theta.device), jump.states[ok], diff[ok], *stats,
                                       n_incomplete=int((~ok).sum()))
