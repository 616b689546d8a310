"""ctypes binding of libvsde_hip.so (see include/vsde_hip.h for the C ABI).

This is the only place the package touches native code.  There is deliberately NO CPU or
PyTorch fallback: if the library is missing, or tensors are not on a HIP device, the call
raises.  Tensors are passed as raw device pointers + the current torch stream handle.
"""
from __future__ import annotations

import ctypes
import os
from typing import Optional, Sequence

import torch

from .build import LIB_PATH

VSDE_ABI_VERSION = 1
MAX_LAYERS = 4      # reference: kernels/constants.py:13
MAX_HIDDEN = 1024
MAX_STATE = 32
DIAG_MIN = 1e-2     # reference: inference/constants.py:6


class HipLibraryError(RuntimeError):
    pass


class _Dims(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int) for n in ("B", "T", "S", "P", "C", "H", "L")]


class _Weights(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in (
        "W_ih_l0", "W_hh_l0", "b_ih_l0", "b_hh_l0", "W_ih_stack", "W_hh_stack",
        "b_ih_stack", "b_hh_stack", "out_weight", "out_bias")]


class _CtxView(ctypes.Structure):
    _fields_ = [("base", ctypes.c_void_p), ("dtype", ctypes.c_int),
                ("batch_stride", ctypes.c_int64), ("step_stride", ctypes.c_int64)]


class _Grads(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in (
        "x0", "context", "theta", "W_ih_l0", "W_hh_l0", "b_ih_l0", "b_hh_l0",
        "W_ih_stack", "W_hh_stack", "b_ih_stack", "b_hh_stack", "out_weight", "out_bias")] + [
        ("context_dtype", ctypes.c_int), ("context_batch_stride", ctypes.c_int64)]


EXPORTS = (
    "vsde_abi_version", "vsde_build_ablations", "vsde_last_error",
    "vsde_head_forward_workspace_bytes", "vsde_head_forward",
    "vsde_head_backward_workspace_bytes", "vsde_head_backward",
    "vsde_elbo_path_terms", "vsde_elbo_path_terms_bwd", "vsde_elbo_tail_fwd", "vsde_elbo_tail_bwd",
    "vsde_count_elbo_tail_fwd", "vsde_count_elbo_tail_bwd",
    "vsde_log_weights", "vsde_log_weight_accumulate", "vsde_count_log_weights", "vsde_crn_count_log_weights",
    "vsde_crn_kinetic_count_log_weights", "vsde_count_particle_filter", "vsde_crn_count_particle_filter",
    "vsde_crn_kinetic_count_particle_filter",
    "vsde_profile_enable", "vsde_profile_elapsed_ms", "vsde_debug_force_v1", "vsde_debug_head_mp", "vsde_head_mfma_range_exceeded",
    "vsde_debug_head_context_projection", "vsde_debug_head_backward_gemms",
    "vsde_ln_modulate_fwd", "vsde_ln_modulate_bwd", "vsde_gated_residual_fwd", "vsde_gated_residual_bwd",
    "vsde_swiglu_fwd", "vsde_swiglu_bwd", "vsde_gate_merge_fwd", "vsde_gate_merge_bwd",
    "vsde_qk_norm_rope_fwd", "vsde_qk_norm_rope_bwd_partials", "vsde_qk_norm_rope_bwd",
    "vsde_residual_ln_fwd", "vsde_residual_ln_bwd", "vsde_colsum_workspace_bytes", "vsde_linear_wgrad_workspace_bytes", "vsde_linear_wgrad_bf16", "vsde_linear_wgrad_bf16_rows", "vsde_linear_wgrad_group_workspace_bytes", "vsde_linear_wgrad_group_bf16",
    "vsde_attention_max_tokens", "vsde_attention_fwd_bf16", "vsde_attention_bwd_bf16",
    "vsde_attention_fused_supported", "vsde_attention_fwd_gated_bf16", "vsde_gate_bwd_delta", "vsde_attention_bwd_fused_partials",
    "vsde_attention_bwd_fused_bf16",
    "vsde_euler_maruyama_fwd", "vsde_euler_maruyama_bwd", "vsde_forecast", "vsde_sde_coefficients_fwd", "vsde_sde_coefficients_bwd",
    "vsde_crn_sde_coefficients_fwd", "vsde_crn_sde_coefficients_bwd", "vsde_crn_euler_maruyama_fwd", "vsde_crn_euler_maruyama_bwd",
    "vsde_crn_forecast", "vsde_crn_log_weights", "vsde_crn_kinetic_sde_coefficients_fwd", "vsde_crn_kinetic_sde_coefficients_bwd",
    "vsde_crn_kinetic_euler_maruyama_fwd", "vsde_crn_kinetic_euler_maruyama_bwd", "vsde_crn_kinetic_forecast",
    "vsde_crn_kinetic_log_weights", "vsde_particle_filter", "vsde_crn_particle_filter", "vsde_crn_kinetic_particle_filter",
    "vsde_guided_particle_filter", "vsde_crn_guided_particle_filter", "vsde_crn_kinetic_guided_particle_filter",
    "vsde_filter_replay", "vsde_crn_filter_replay", "vsde_crn_kinetic_filter_replay",
    "vsde_guided_filter_replay", "vsde_crn_guided_filter_replay", "vsde_crn_kinetic_guided_filter_replay", "vsde_pmmh_step",
    "vsde_pmmh_step_paths", "vsde_anchored_replay", "vsde_crn_anchored_replay", "vsde_crn_kinetic_anchored_replay",
    "vsde_guided_anchored_replay", "vsde_crn_guided_anchored_replay", "vsde_crn_kinetic_guided_anchored_replay",
    "vsde_residual_particle_filter", "vsde_crn_residual_particle_filter", "vsde_crn_kinetic_residual_particle_filter",
    "vsde_residual_filter_replay", "vsde_crn_residual_filter_replay", "vsde_crn_kinetic_residual_filter_replay",
    "vsde_residual_anchored_replay", "vsde_crn_residual_anchored_replay", "vsde_crn_kinetic_residual_anchored_replay",
    "vsde_crn_jump_process", "vsde_crn_kinetic_jump_process", "vsde_crn_jump_particle_filter", "vsde_crn_kinetic_jump_particle_filter",
    "vsde_crn_jump_filter_replay", "vsde_crn_kinetic_jump_filter_replay", "vsde_crn_jump_anchored_replay", "vsde_crn_kinetic_jump_anchored_replay",
    "vsde_crn_tau_leap_process", "vsde_crn_kinetic_tau_leap_process", "vsde_crn_tau_leap_particle_filter", "vsde_crn_kinetic_tau_leap_particle_filter",
    "vsde_linear_bf16_supported", "vsde_linear_bf16", "vsde_linear_qknorm_bf16", "vsde_linear_gated_bf16", "vsde_linear_gate_bwd_bf16",
    "vsde_mlp_image_bytes", "vsde_mlp_fwd_bf16", "vsde_mlp_block_fwd_bf16", "vsde_mlp_attn_block_fwd_bf16", "vsde_linear_deep256_bf16", "vsde_mlp_debug_trace", "vsde_wgrad_debug_trace", "vsde_attn_debug_trace", "vsde_mlp_bwd_image_bytes", "vsde_mlp_bwd_bf16",
    "vsde_pack_tile_bytes", "vsde_pack_refresh", "vsde_optim_chunk_bytes", "vsde_optim_chunk_elems", "vsde_optim_step",
)

_lib: Optional[ctypes.CDLL] = None
_loaded_path: Optional[str] = None


def library_path() -> str:
    """The library file in use (the in-tree build unless VSDE_HIP_LIB names another one)."""
    return _loaded_path or os.environ.get("VSDE_HIP_LIB") or LIB_PATH


def has_ablations() -> bool:
    """Whether the loaded library is an ablation build (``python -m viforsdes_amd.build --ablations`` + VSDE_HIP_LIB): A/B switches are
    read from the environment and the losing kernel variants exist.  The shipped library says False."""
    return bool(load().vsde_build_ablations())


ABL_LIB_PATH = os.path.join(os.path.dirname(LIB_PATH), "libvsde_hip_abl.so")


def load() -> ctypes.CDLL:
    """Load the shared library (fails loudly if it was never built)."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("VSDE_HIP_LIB") or LIB_PATH   # VSDE_HIP_LIB: an A/B build of the same sources (tools only)
    if not os.path.exists(path):
        raise HipLibraryError(
            f"{path} is missing: build it with `python -m viforsdes_amd.build` "
            "(there is no CPU fallback for the fused head / ELBO kernels)")
    lib = ctypes.CDLL(path)
    for name in EXPORTS:
        if not hasattr(lib, name):
            raise HipLibraryError(f"{path} does not export {name}")
    global _loaded_path
    _loaded_path = path
    lib.vsde_abi_version.restype = ctypes.c_int
    if lib.vsde_abi_version() != VSDE_ABI_VERSION:
        raise HipLibraryError(f"{path}: ABI version mismatch; rebuild it")
    lib.vsde_last_error.restype = ctypes.c_char_p
    lib.vsde_head_forward_workspace_bytes.restype = ctypes.c_size_t
    lib.vsde_head_backward_workspace_bytes.restype = ctypes.c_size_t
    for f in (lib.vsde_head_forward, lib.vsde_head_backward, lib.vsde_elbo_path_terms, lib.vsde_elbo_path_terms_bwd):
        f.restype = ctypes.c_int
    lib.vsde_qk_norm_rope_bwd_partials.restype = ctypes.c_int64
    lib.vsde_attention_bwd_fused_partials.restype = ctypes.c_int64
    lib.vsde_linear_wgrad_workspace_bytes.restype = ctypes.c_size_t
    lib.vsde_linear_wgrad_group_workspace_bytes.restype = ctypes.c_size_t
    lib.vsde_colsum_workspace_bytes.restype = ctypes.c_size_t
    lib.vsde_mlp_bwd_image_bytes.restype = ctypes.c_int64
    _lib = lib
    return lib


def _raise(rc: int) -> None:
    msg = load().vsde_last_error().decode("utf-8", "replace")
    if rc < 0:
        raise ValueError(msg)          # argument errors, like the reference's ValueError (models/head.py:33-36)
    raise HipLibraryError(f"HIP error {rc}: {msg}")


def _ptr(t: Optional[torch.Tensor]):
    return ctypes.c_void_p(None if t is None or t.numel() == 0 else t.data_ptr())


def _require_hip(*tensors: torch.Tensor) -> torch.device:
    dev = None
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise HipLibraryError(
                "the fused head / ELBO kernels only run on a HIP (cuda) device; got a "
                f"{t.device} tensor and there is no CPU fallback")
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise ValueError("all tensors must live on the same device")
    assert dev is not None
    return dev


def _stream(dev: torch.device):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _f32c(t: torch.Tensor) -> torch.Tensor:
    if t.dtype != torch.float32:
        t = t.float()
    return t if t.is_contiguous() else t.contiguous()


def context_view(ctx: torch.Tensor):
    """Describe a [B, T, C] context (fp32 or bf16, last dim contiguous) without copying."""
    if ctx.dtype not in (torch.float32, torch.bfloat16):
        ctx = ctx.float()
    if ctx.stride(2) != 1:
        ctx = ctx.contiguous()
    v = _CtxView(ctypes.c_void_p(ctx.data_ptr()), 1 if ctx.dtype == torch.bfloat16 else 0,
                 ctx.stride(0), ctx.stride(1))
    return ctx, v


def _weights_struct(ws: Sequence[torch.Tensor]):
    keep = [_f32c(w) for w in ws]
    return keep, _Weights(*[_ptr(w) for w in keep])


def _dims(x0, ctx, theta, ws) -> _Dims:
    B, S = x0.shape
    T, C = ctx.shape[1], ctx.shape[2]
    P = theta.shape[1]
    H = ws[1].shape[1]
    L = 1 + (ws[4].shape[0] if ws[4].numel() > 0 else 0)
    if tuple(ws[0].shape) != (3 * H, S + C + P):
        raise ValueError(f"W_ih_l0 has shape {tuple(ws[0].shape)}, expected {(3 * H, S + C + P)}")
    return _Dims(B, T, S, P, C, H, L)


def head_forward(x0, ctx, theta, eps, ws, time_step: float, save: bool, diag_min: float = DIAG_MIN):
    """-> (paths[B,T+1,S], means[B,T,S], chol[B,T,S,S], chol_raw|None, acts|None), all fp32."""
    lib = load()
    dev = _require_hip(x0, ctx, theta, eps, *ws)
    x0 = _f32c(x0); theta = _f32c(theta); eps = _f32c(eps)
    ctx, cview = context_view(ctx)
    keep, wstruct = _weights_struct(ws)
    d = _dims(x0, ctx, theta, keep)
    B, T, S, H, L = d.B, d.T, d.S, d.H, d.L
    ntril = S * (S + 1) // 2
    with torch.cuda.device(dev):
        paths = torch.empty(B, T + 1, S, device=dev, dtype=torch.float32)
        means = torch.empty(B, T, S, device=dev, dtype=torch.float32)
        chol = torch.empty(B, T, S, S, device=dev, dtype=torch.float32)
        chol_raw = torch.empty(B, T, ntril, device=dev, dtype=torch.float32) if save else None
        acts = torch.empty(B, T, L, 5, H, device=dev, dtype=torch.float32) if save else None
        nbytes = lib.vsde_head_forward_workspace_bytes(ctypes.byref(d))
        if nbytes == 0:
            _raise(-1)
        wsbuf = torch.empty(nbytes, device=dev, dtype=torch.uint8)
        rc = lib.vsde_head_forward(
            ctypes.byref(d), _ptr(x0), ctypes.byref(cview), _ptr(theta), _ptr(eps), ctypes.byref(wstruct),
            ctypes.c_double(time_step), ctypes.c_double(diag_min), ctypes.c_int(1 if save else 0),
            _ptr(paths), _ptr(means), _ptr(chol), _ptr(chol_raw), _ptr(acts),
            _ptr(wsbuf), ctypes.c_size_t(nbytes), _stream(dev))
    if rc != 0:
        _raise(rc)
    return paths, means, chol, chol_raw, acts


def head_backward(g_paths, g_means, g_chol, ctx, theta, eps, paths, chol_raw, acts, ws,
                  time_step: float, diag_min: float = DIAG_MIN, context_grad_out=None, workspace=None):
    """-> 13 fp32 gradients in launch_bwd order (reference kernels/backward.py:766-784).

    ``context_grad_out``: optional contiguous [B, T+1, C] (f32 or bf16) tensor; the context gradient is then written
    straight into its first T steps (in its dtype) and returned in place of the fp32 [B,T,C] tensor; its last step is
    the caller's to zero.  ``workspace``: optional uint8 tensor of at least ``head_backward_workspace_bytes`` to run in (tests read the
    sweep's pre-activation gradients back from it)."""
    lib = load()
    dev = _require_hip(g_paths, g_means, g_chol, ctx, theta, eps, paths, chol_raw, acts, *ws)
    g_paths = _f32c(g_paths); g_means = _f32c(g_means); g_chol = _f32c(g_chol)
    theta = _f32c(theta); eps = _f32c(eps)
    ctx, cview = context_view(ctx)
    keep, wstruct = _weights_struct(ws)
    B, T1, S = paths.shape
    d = _dims(paths[:, 0], ctx, theta, keep)
    T, C, P, H, L = d.T, d.C, d.P, d.H, d.L
    NO = S + S * (S + 1) // 2
    with torch.cuda.device(dev):
        mk = lambda *shape: torch.empty(*shape, device=dev, dtype=torch.float32)
        g = [mk(B, S), mk(B, T, C), mk(B, P), mk(3 * H, S + C + P), mk(3 * H, H), mk(3 * H), mk(3 * H),
             mk(L - 1, 3 * H, H), mk(L - 1, 3 * H, H), mk(L - 1, 3 * H), mk(L - 1, 3 * H), mk(NO, H), mk(NO)]
        cdt, cbs = 0, 0
        if context_grad_out is not None:
            o = context_grad_out
            if (not o.is_contiguous() or o.ndim != 3 or o.shape[0] != B or o.shape[1] < T or o.shape[2] != C
                    or o.dtype not in (torch.float32, torch.bfloat16) or o.device != dev):
                raise ValueError("context_grad_out must be a contiguous [B, >=T, C] f32/bf16 tensor on the same device")
            g[1] = o
            cdt, cbs = int(o.dtype == torch.bfloat16), o.shape[1] * C
        gstruct = _Grads(*[_ptr(t) for t in g], cdt, cbs)
        nbytes = lib.vsde_head_backward_workspace_bytes(ctypes.byref(d))
        if nbytes == 0:
            _raise(-1)
        wsbuf = torch.empty(nbytes, device=dev, dtype=torch.uint8) if workspace is None else workspace
        if wsbuf.dtype != torch.uint8 or wsbuf.numel() < nbytes or not wsbuf.is_contiguous() or wsbuf.device != dev:
            raise ValueError(f"workspace must be a contiguous uint8 tensor of at least {nbytes} bytes on the same device")
        rc = lib.vsde_head_backward(
            ctypes.byref(d), _ptr(g_paths), _ptr(g_means), _ptr(g_chol), ctypes.byref(cview), _ptr(theta),
            _ptr(eps), _ptr(paths), _ptr(chol_raw), _ptr(acts), ctypes.byref(wstruct),
            ctypes.c_double(time_step), ctypes.c_double(diag_min), ctypes.byref(gstruct),
            _ptr(wsbuf), ctypes.c_size_t(nbytes), _stream(dev))
    if rc != 0:
        _raise(rc)
    return tuple(g)


def _mask_bytes(positive_dims, S: int):
    m = (ctypes.c_uint8 * S)()
    for dd in positive_dims or []:
        m[dd] = 1
    return m


def elbo_path_terms(z, x, means, chol, drift, diffusion, positive_dims, time_step: float):
    lib = load()
    dev = _require_hip(z, x, means, chol, drift, diffusion)
    z, x, means, chol, drift, diffusion = (_f32c(t) for t in (z, x, means, chol, drift, diffusion))
    B, T1, S = z.shape
    with torch.cuda.device(dev):
        outs = [torch.empty(B, device=dev, dtype=torch.float32) for _ in range(3)]
        rc = lib.vsde_elbo_path_terms(
            ctypes.c_int(B), ctypes.c_int(T1 - 1), ctypes.c_int(S), _ptr(z), _ptr(x), _ptr(means), _ptr(chol),
            _ptr(drift), _ptr(diffusion), _mask_bytes(positive_dims, S), ctypes.c_double(time_step),
            *[_ptr(o) for o in outs], _stream(dev))
    if rc != 0:
        _raise(rc)
    return tuple(outs)


def elbo_path_terms_bwd(z, x, means, chol, drift, diffusion, positive_dims, time_step: float, g_sde, g_gen, g_jac):
    lib = load()
    dev = _require_hip(z, x, means, chol, drift, diffusion, g_sde, g_gen, g_jac)
    z, x, means, chol, drift, diffusion, g_sde, g_gen, g_jac = (
        _f32c(t) for t in (z, x, means, chol, drift, diffusion, g_sde, g_gen, g_jac))
    B, T1, S = z.shape
    with torch.cuda.device(dev):
        outs = [torch.empty_like(z), torch.empty_like(x), torch.empty_like(means), torch.empty_like(chol),
                torch.empty_like(drift), torch.empty_like(diffusion)]
        rc = lib.vsde_elbo_path_terms_bwd(
            ctypes.c_int(B), ctypes.c_int(T1 - 1), ctypes.c_int(S), _ptr(z), _ptr(x), _ptr(means), _ptr(chol),
            _ptr(drift), _ptr(diffusion), _mask_bytes(positive_dims, S), ctypes.c_double(time_step),
            _ptr(g_sde), _ptr(g_gen), _ptr(g_jac), *[_ptr(o) for o in outs], _stream(dev))
    if rc != 0:
        _raise(rc)
    return tuple(outs)


SDE_KINDS = {"ornstein_uhlenbeck": 1, "lotka_volterra": 2, "linear_diagonal": 3, "reaction_network": 4}
CRN_MAX_SPECIES, CRN_MAX_REACTIONS, CRN_MAX_ORDER, CRN_MAX_HILL = 8, 16, 3, 4
CRN_LAW_MASS_ACTION, CRN_LAW_HILL_ACTIVATION, CRN_LAW_HILL_REPRESSION = 0, 1, 2


class CrnNetwork(ctypes.Structure):
    """``vsde_crn_network`` (include/vsde_hip.h): a reaction network's reactant orders and net changes, passed by pointer to
    host memory and copied into the kernel arguments at launch."""
    _fields_ = [("S", ctypes.c_int32), ("R", ctypes.c_int32),
                ("order", (ctypes.c_int8 * CRN_MAX_SPECIES) * CRN_MAX_REACTIONS),
                ("change", (ctypes.c_int8 * CRN_MAX_SPECIES) * CRN_MAX_REACTIONS)]


def crn_network(order, change) -> CrnNetwork:
    """The descriptor of a network with reactant orders ``order`` and net changes ``change`` (both [R][S] integers)."""
    R, S = len(order), len(order[0])
    if not (1 <= S <= CRN_MAX_SPECIES and 1 <= R <= CRN_MAX_REACTIONS) or len(change) != R:
        raise ValueError(f"reaction-network descriptor: {S} species / {R} reactions outside 1..{CRN_MAX_SPECIES} / 1..{CRN_MAX_REACTIONS}")
    net = CrnNetwork()
    net.S, net.R = S, R
    for j in range(R):
        if len(order[j]) != S or len(change[j]) != S:
            raise ValueError(f"reaction-network descriptor: row {j} does not have {S} entries")
        for i in range(S):
            if not 0 <= order[j][i] <= CRN_MAX_ORDER or not -128 <= change[j][i] <= 127:
                raise ValueError(f"reaction-network descriptor: reaction {j}, species {i}: order {order[j][i]} / change "
                                 f"{change[j][i]} outside 0..{CRN_MAX_ORDER} / int8")
            net.order[j][i], net.change[j][i] = order[j][i], change[j][i]
    return net


class CrnKinetics(ctypes.Structure):
    """``vsde_crn_kinetics`` (include/vsde_hip.h): per reaction the law code (CRN_LAW_*), the modifier species and the Hill
    coefficient of its rate law; host memory, copied into the kernel arguments at launch."""
    _fields_ = [("law", ctypes.c_int8 * CRN_MAX_REACTIONS), ("modifier", ctypes.c_int8 * CRN_MAX_REACTIONS),
                ("hill_n", ctypes.c_int8 * CRN_MAX_REACTIONS)]


def crn_kinetics(laws) -> CrnKinetics:
    """The rate-law descriptor of ``laws``: per reaction None (mass action) or ``(law code, modifier species, n)``."""
    if not 1 <= len(laws) <= CRN_MAX_REACTIONS:
        raise ValueError(f"rate-law descriptor: {len(laws)} reactions outside 1..{CRN_MAX_REACTIONS}")
    kin = CrnKinetics()
    for j, law in enumerate(laws):
        code, s, n = (CRN_LAW_MASS_ACTION, 0, 1) if law is None else law
        if code not in (CRN_LAW_MASS_ACTION, CRN_LAW_HILL_ACTIVATION, CRN_LAW_HILL_REPRESSION) or not (
                0 <= s < CRN_MAX_SPECIES and 1 <= n <= CRN_MAX_HILL):
            raise ValueError(f"rate-law descriptor: reaction {j}: law {code}, modifier {s}, n {n} outside 0..2 / "
                             f"0..{CRN_MAX_SPECIES - 1} / 1..{CRN_MAX_HILL}")
        kin.law[j], kin.modifier[j], kin.hill_n[j] = code, s, n
    return kin


class CrnKineticRoute:
    """The kernel route of a reaction network with rate laws, shared or fixed constants (ReactionNetworkSDE.kernel_descriptor):
    the network and rate-law descriptors, dispatched to the ``vsde_crn_kinetic_*`` entry points, and ``kernel_parameters``,
    the network's differentiable map from theta [.., P] to the effective constants [.., 2R] those entry points take."""

    def __init__(self, network: CrnNetwork, kinetics: CrnKinetics, kernel_parameters) -> None:
        self.network, self.kinetics, self.kernel_parameters = network, kinetics, kernel_parameters


def _sde_entry(lib, name: str, kind: str, network):
    """(entry point, leading arguments) of a built-in SDE: ``vsde_<name>(kind, ...)``, or for a reaction network the mirrored
    ``vsde_crn_<name>(&descriptor, ...)`` (``vsde_crn_kinetic_<name>(&descriptor, &rate laws, ...)`` for a CrnKineticRoute,
    whose theta are the effective constants [B, 2R])."""
    if kind == "reaction_network":
        if isinstance(network, CrnKineticRoute):
            return getattr(lib, "vsde_crn_kinetic_" + name), ctypes.byref(network.network), ctypes.byref(network.kinetics)
        if not isinstance(network, CrnNetwork):
            raise ValueError("the reaction-network kernels need the network's descriptor (ReactionNetworkSDE.network_descriptor())")
        return getattr(lib, "vsde_crn_" + name), ctypes.byref(network)
    return getattr(lib, "vsde_" + name), ctypes.c_int(SDE_KINDS[kind])


def euler_maruyama_fwd(kind: str, x0, theta, noise, time_step: float, positive_dims=(), network=None):
    """Trajectory [B, T+1, S] of a built-in model SDE (``kind`` in SDE_KINDS; a reaction network also needs its ``network``
    descriptor) for given noise [B, T, S]."""
    lib = load()
    dev = _require_hip(x0, theta, noise)
    x0, theta, noise = _f32c(x0), _f32c(theta), _f32c(noise)
    B, T, S = noise.shape
    with torch.cuda.device(dev):
        traj = torch.empty(B, T + 1, S, device=dev, dtype=torch.float32)
        _call(*_sde_entry(lib, "euler_maruyama_fwd", kind, network), ctypes.c_int(B), ctypes.c_int(T), ctypes.c_int(S),
              ctypes.c_int(theta.shape[1]), _ptr(x0), _ptr(theta), _ptr(noise), ctypes.c_double(time_step),
              _mask_bytes(positive_dims, S), _ptr(traj), _stream(dev))
    return traj


def euler_maruyama_bwd(kind: str, theta, noise, traj, g_traj, time_step: float, positive_dims=(), network=None):
    """(g_x0 [B,S], g_theta [B,P]) of ``euler_maruyama_fwd`` for the upstream gradient g_traj [B, T+1, S]."""
    lib = load()
    dev = _require_hip(theta, noise, traj, g_traj)
    theta, noise, traj, g_traj = _f32c(theta), _f32c(noise), _f32c(traj), _f32c(g_traj)
    B, T, S = noise.shape
    with torch.cuda.device(dev):
        g_x0 = torch.empty(B, S, device=dev, dtype=torch.float32)
        g_theta = torch.empty_like(theta)
        _call(*_sde_entry(lib, "euler_maruyama_bwd", kind, network), ctypes.c_int(B), ctypes.c_int(T), ctypes.c_int(S),
              ctypes.c_int(theta.shape[1]), _ptr(theta), _ptr(noise), _ptr(traj), _ptr(g_traj), ctypes.c_double(time_step),
              _mask_bytes(positive_dims, S), _ptr(g_x0), _ptr(g_theta), _stream(dev))
    return g_x0, g_theta


def forecast(kind: str, x_start, theta, n_steps: int, out_steps, key, time_step: float, positive_dims=(), network=None):
    """States [B, K, S] of a built-in model SDE (``kind`` in SDE_KINDS) after the grid steps ``out_steps`` (int32 device tensor
    [K], non-decreasing, values in 1..n_steps) of an ``n_steps``-step Euler-Maruyama run from x_start [B, S] with theta [B, P]; the
    increments come from the Philox stream of ``key`` (2 int32 words on the device; see include/vsde_hip.h: vsde_forecast)."""
    lib = load()
    dev = _require_hip(x_start, theta, out_steps, key)
    x_start, theta = _f32c(x_start), _f32c(theta)
    if out_steps.dtype != torch.int32 or out_steps.ndim != 1 or key.dtype not in (torch.int32, torch.uint32) or key.numel() != 2:
        raise ValueError("forecast: out_steps must be an int32 [K] tensor and key two int32 words")
    out_steps, key = out_steps.contiguous(), key.contiguous()
    B, S = x_start.shape
    K = out_steps.shape[0]
    if theta.shape[0] != B:
        raise ValueError(f"forecast: theta has {theta.shape[0]} rows for {B} start states")
    with torch.cuda.device(dev):
        out = torch.empty(B, K, S, device=dev, dtype=torch.float32)
        _call(*_sde_entry(lib, "forecast", kind, network), ctypes.c_int(B), ctypes.c_int(n_steps), ctypes.c_int(S),
              ctypes.c_int(theta.shape[1]), ctypes.c_int(K), _ptr(x_start), _ptr(theta), _ptr(out_steps), _ptr(key),
              ctypes.c_double(time_step), _mask_bytes(positive_dims, S), _ptr(out), _stream(dev))
    return out


def jump_process(x0, theta, out_times, key, max_events: int, record_events: int = 0, network=None):
    """Gillespie trajectories of a reaction network (include/vsde_hip.h: vsde_crn_jump_process): x0 int32 [B, S], theta fp32
    [B, P] (the effective constants [B, 2R] for a CrnKineticRoute), out_times float64 [K] and key (2 int32 words), all on the
    device.  Returns ``(states int32 [B, K, S], n_events int32 [B], status int32 [B], event_times float64 [B, E] or None,
    event_reactions int32 [B, E] or None)`` with E = ``record_events``."""
    lib = load()
    dev = _require_hip(x0, theta, out_times, key)
    if x0.dtype != torch.int32 or x0.ndim != 2 or out_times.dtype != torch.float64 or out_times.ndim != 1:
        raise ValueError("jump_process: x0 must be an int32 [B, S] tensor and out_times a float64 [K] tensor")
    if key.dtype not in (torch.int32, torch.uint32) or key.numel() != 2:
        raise ValueError("jump_process: key must be two int32 words")
    x0, theta, out_times, key = x0.contiguous(), _f32c(theta), out_times.contiguous(), key.contiguous()
    B, S = x0.shape
    K, E = out_times.shape[0], int(record_events)
    if theta.ndim != 2 or theta.shape[0] != B:
        raise ValueError(f"jump_process: theta {tuple(theta.shape)} does not have one row for each of the {B} start states")
    if B < 1 or K < 1 or E < 0:
        raise ValueError(f"jump_process: bad dims B={B} K={K} E={E}")
    with torch.cuda.device(dev):
        states = torch.empty(B, K, S, device=dev, dtype=torch.int32)
        n_events = torch.empty(B, device=dev, dtype=torch.int32)
        status = torch.empty(B, device=dev, dtype=torch.int32)
        ev_t = torch.empty(B, E, device=dev, dtype=torch.float64) if E else None
        ev_r = torch.empty(B, E, device=dev, dtype=torch.int32) if E else None
        _call(*_sde_entry(lib, "jump_process", "reaction_network", network), ctypes.c_int(B), ctypes.c_int(S),
              ctypes.c_int(theta.shape[1]), ctypes.c_int(K), ctypes.c_int(E), _ptr(x0), _ptr(theta), _ptr(out_times), _ptr(key),
              ctypes.c_int(int(max_events)), _ptr(states), _ptr(n_events), _ptr(status), _ptr(ev_t), _ptr(ev_r), _stream(dev))
    return states, n_events, status, ev_t, ev_r


def _observation_term(variance, n_rows: int, dev):
    """(prefix of the entry point's name, its arguments) for the observation term of a tail / log-weight / filter call:
    ``variance`` is the Gaussian variance (a number) or the ``CountKernelTerms`` (lik_kind, scale, dispersion, row_const [K]) of a
    Poisson / negative-binomial likelihood, which select the ``vsde_*count_*`` form of the entry point."""
    if not isinstance(variance, tuple):
        return "", (ctypes.c_double(variance),)
    lik_kind, scale, dispersion, row_const = variance
    if not isinstance(row_const, torch.Tensor) or row_const.device != dev or row_const.numel() != n_rows:
        raise ValueError(f"count likelihood: row constants [{n_rows}] on {dev} expected")
    row_const = _f32c(row_const)
    return "count_", (ctypes.c_int(int(lik_kind)), ctypes.c_double(scale), ctypes.c_double(dispersion), _ptr(row_const))


PF_MAX_STATE, PF_MAX_OBS, PF_MAX_PARTICLES = 16, 16, 1024
PF_GUIDED_MAX_STATE, PF_GUIDED_MAX_OBS = 4, 4
PF_RESIDUAL_FULL_STATE = 3   # csrc/vsde_filter_step.h: kPfResidualFullS


def particle_filter_max_particles(kind: str, state_dim: int, proposal: str = "bootstrap") -> int:
    """The largest ``n_particles`` (a multiple of 64) the filter kernel of a built-in SDE takes (csrc/vsde_filter.hip: pf_max_n):
    1024, and 512 for a reaction network of 5..8 species (its step needs more than the 128 registers of a 1024-thread workgroup).
    ``proposal="bridge"``: the guided step fits those registers up to state_dim 3; at state_dim 4 its instantiations are built
    for 512 threads: 512.  ``proposal="residual_bridge"``: its own rule (pf_max_n's residual argument), which today gives the
    bridge's limits: the companion path still fits the 128 registers up to state_dim 3."""
    if proposal not in ("bootstrap", "bridge", "residual_bridge"):
        raise ValueError(f"proposal must be 'bootstrap', 'bridge' or 'residual_bridge', got {proposal!r}")
    if proposal == "bridge" and state_dim > 3:
        return PF_MAX_PARTICLES // 2
    if proposal == "residual_bridge" and state_dim > PF_RESIDUAL_FULL_STATE:
        return PF_MAX_PARTICLES // 2
    return PF_MAX_PARTICLES // 2 if kind == "reaction_network" and state_dim > 4 else PF_MAX_PARTICLES


def _particle_filter(entry: str, want_lw: bool, kind, x0, theta, obs_rows, obs_values, obs_matrix, variance, key, time_step,
                     n_particles, positive_dims, network, return_particles, store=None):
    lib = load()
    dev = _require_hip(x0, theta, obs_rows, obs_values, obs_matrix, key)
    x0, theta, obs_values = _f32c(x0), _f32c(theta), _f32c(obs_values)
    obs_matrix = None if obs_matrix is None else _f32c(obs_matrix)
    if obs_rows.dtype != torch.int32 or obs_rows.ndim != 1 or key.dtype not in (torch.int32, torch.uint32) or key.numel() != 2:
        raise ValueError("particle_filter: obs_rows must be an int32 [K] tensor and key two int32 words")
    obs_rows, key = obs_rows.contiguous(), key.contiguous()
    if x0.ndim != 2 or theta.ndim != 2 or theta.shape[0] != x0.shape[0] or obs_values.ndim != 2 \
            or obs_values.shape[0] != obs_rows.shape[0]:
        raise ValueError(f"particle_filter: x0 [M, S], theta [M, P], obs_values [K, O], obs_rows [K] expected, got "
                         f"{tuple(x0.shape)}, {tuple(theta.shape)}, {tuple(obs_values.shape)}, {tuple(obs_rows.shape)}")
    M, S = x0.shape
    K, O = obs_values.shape
    N = int(n_particles)
    if obs_matrix is not None and tuple(obs_matrix.shape) != (O, S):
        raise ValueError(f"particle_filter: obs_matrix must be [{O}, {S}], got {tuple(obs_matrix.shape)}")
    with torch.cuda.device(dev):
        f32 = dict(device=dev, dtype=torch.float32)
        loglik, incr, ess = torch.empty(M, **f32), torch.empty(M, K, **f32), torch.empty(M, K, **f32)
        mean, std = torch.empty(M, K, S, **f32), torch.empty(M, K, S, **f32)
        keep = return_particles and 0 < N <= PF_MAX_PARTICLES   # a bad N is the entry point's to refuse: allocate nothing for it
        particles = torch.empty(M, K, N, S, **f32) if keep else None
        ancestors = torch.empty(M, K, N, device=dev, dtype=torch.int32) if keep else None
        extra = ()
        if want_lw:
            extra = (torch.empty(M, K, N, **f32) if keep else None,)
        if store is not None:
            particles, ancestors = store
            if not (particles.is_contiguous() and ancestors.is_contiguous() and particles.dtype == torch.float32
                    and ancestors.dtype == torch.int32 and particles.device == ancestors.device == dev
                    and tuple(particles.shape) == (M, K, N, S) and tuple(ancestors.shape) == (M, K, N)):
                raise ValueError(f"particle_filter: store = (particles fp32 [{M}, {K}, {N}, {S}], ancestors int32 [{M}, {K}, {N}]), "
                                 "contiguous on the call's device, expected")
            extra = (None,) if want_lw else ()
        prefix, term = _observation_term(variance, K, dev)
        if prefix and want_lw:
            raise ValueError("the guided particle filter needs a Gaussian observation term")
        _call(*_sde_entry(lib, prefix + entry, kind, network), ctypes.c_int(M), ctypes.c_int(N), ctypes.c_int(S),
              ctypes.c_int(theta.shape[1]), ctypes.c_int(K), ctypes.c_int(O), _ptr(x0), _ptr(theta), _ptr(obs_rows), _ptr(obs_values),
              _ptr(obs_matrix), *term, _ptr(key), ctypes.c_double(time_step), _mask_bytes(positive_dims, S),
              _ptr(loglik), _ptr(incr), _ptr(ess), _ptr(mean), _ptr(std), _ptr(particles), _ptr(ancestors),
              *[_ptr(t) for t in extra], _stream(dev))
    return (loglik, incr, ess, mean, std, particles, ancestors) + extra


def particle_filter(kind: str, x0, theta, obs_rows, obs_values, obs_matrix, variance: float, key, time_step: float,
                    n_particles: int, positive_dims=(), network=None, return_particles: bool = False, store=None):
    """Bootstrap particle filters of a built-in model SDE (``kind`` in SDE_KINDS), one per row of theta [M, P] (the effective
    constants [M, 2R] for a CrnKineticRoute) from the start states x0 [M, S], against obs_values [K, O] at the grid rows obs_rows
    (int32 device tensor [K]) with a Gaussian observation term (obs_matrix [O, S] or None; ``variance``: a number) or a count term
    (``variance``: the likelihood's ``CountKernelTerms``: vsde_count_particle_filter); noise and resampling uniforms come from
    the Philox stream of ``key`` (2 int32 words on the device).  See include/vsde_hip.h: vsde_particle_filter.  Returns
    (log_likelihood [M], increments [M, K], effective_sample_size [M, K], filtered_mean [M, K, S], filtered_std [M, K, S],
    particles [M, K, N, S] or None, ancestors [M, K, N] int32 or None).  ``store``: (particles, ancestors) buffers of those shapes
    to write into instead of ``return_particles`` (a caller that runs the filter in a loop allocates them once)."""
    return _particle_filter("particle_filter", False, kind, x0, theta, obs_rows, obs_values, obs_matrix, variance, key, time_step,
                            n_particles, positive_dims, network, return_particles, store)


def guided_particle_filter(kind: str, x0, theta, obs_rows, obs_values, obs_matrix, variance: float, key, time_step: float,
                           n_particles: int, positive_dims=(), network=None, return_particles: bool = False, store=None,
                           residual: bool = False):
    """``particle_filter`` with the bridge proposal (include/vsde_hip.h: vsde_guided_particle_filter; S <= 4, O <= 4): the same
    arguments, and the same 7 outputs followed by log_weights [M, K, N] or None (None with ``store``).  ``residual``: the residual
    bridge (vsde_residual_particle_filter)."""
    return _particle_filter("residual_particle_filter" if residual else "guided_particle_filter", True, kind, x0, theta, obs_rows, obs_values, obs_matrix, variance, key,
                            time_step, n_particles, positive_dims, network, return_particles, store)


def jump_filter_max_particles(state_dim: int, n_reactions: int, kinetic: bool = False) -> int:
    """The largest ``n_particles`` (a multiple of 64) the jump-process filter kernel takes for a network of ``state_dim`` species
    and ``n_reactions`` reactions, with rate laws or without (csrc/vsde_jump_filter.hip: jf_max_n): every instantiation fits the
    128 registers of a 1024-thread workgroup, so 1024 throughout today."""
    if not (1 <= state_dim <= CRN_MAX_SPECIES and 1 <= n_reactions <= CRN_MAX_REACTIONS):
        raise ValueError(f"jump_filter_max_particles: {state_dim} species / {n_reactions} reactions outside 1..{CRN_MAX_SPECIES} / "
                         f"1..{CRN_MAX_REACTIONS}")
    return PF_MAX_PARTICLES


def jump_particle_filter(x0, theta, obs_times, obs_values, obs_matrix, variance, key, max_events: int, n_particles: int,
                         network=None, return_particles: bool = False, store=None):
    """Bootstrap particle filters on the exact jump process of a reaction network (include/vsde_hip.h:
    vsde_crn_jump_particle_filter), one per row of theta fp32 [M, P] (the effective constants [M, 2R] for a CrnKineticRoute) from
    the start states x0 int32 [M, S], against obs_values fp32 [K, O] at obs_times float64 [K], with a Gaussian observation term
    (obs_matrix [O, S] or None; ``variance``: a number) or a count term (``variance``: the likelihood's ``CountKernelTerms``); key:
    2 int32 words; everything on the device.  Returns (log_likelihood [M], increments [M, K], effective_sample_size [M, K],
    filtered_mean [M, K, S], filtered_std [M, K, S], stopped int32 [M, K], mean_events [M, K], and with ``return_particles``, else
    None: particles int32 [M, K, N, S], ancestors int32 [M, K, N], log_weights [M, K, N], events int32 [M, K, N]).  ``store``:
    ``(particles, ancestors)``, contiguous int32 device buffers of those shapes to write into instead (particle MCMC with paths: no
    allocation per launch); they are returned in their places, log_weights and events stay None."""
    lib = load()
    dev = _require_hip(x0, theta, obs_times, obs_values, obs_matrix, key)
    if x0.dtype != torch.int32 or x0.ndim != 2 or obs_times.dtype != torch.float64 or obs_times.ndim != 1:
        raise ValueError("jump_particle_filter: x0 must be an int32 [M, S] tensor and obs_times a float64 [K] tensor")
    if key.dtype not in (torch.int32, torch.uint32) or key.numel() != 2:
        raise ValueError("jump_particle_filter: key must be two int32 words")
    x0, theta, obs_times, obs_values, key = x0.contiguous(), _f32c(theta), obs_times.contiguous(), _f32c(obs_values), key.contiguous()
    obs_matrix = None if obs_matrix is None else _f32c(obs_matrix)
    if theta.ndim != 2 or theta.shape[0] != x0.shape[0] or obs_values.ndim != 2 or obs_values.shape[0] != obs_times.shape[0]:
        raise ValueError(f"jump_particle_filter: x0 [M, S], theta [M, P], obs_values [K, O], obs_times [K] expected, got "
                         f"{tuple(x0.shape)}, {tuple(theta.shape)}, {tuple(obs_values.shape)}, {tuple(obs_times.shape)}")
    M, S = x0.shape
    K, O = obs_values.shape
    N = int(n_particles)
    if obs_matrix is not None and tuple(obs_matrix.shape) != (O, S):
        raise ValueError(f"jump_particle_filter: obs_matrix must be [{O}, {S}], got {tuple(obs_matrix.shape)}")
    with torch.cuda.device(dev):
        f32, i32 = dict(device=dev, dtype=torch.float32), dict(device=dev, dtype=torch.int32)
        loglik, incr, ess = torch.empty(M, **f32), torch.empty(M, K, **f32), torch.empty(M, K, **f32)
        mean, std = torch.empty(M, K, S, **f32), torch.empty(M, K, S, **f32)
        stopped, mean_events = torch.empty(M, K, **i32), torch.empty(M, K, **f32)
        keep = return_particles and 0 < N <= PF_MAX_PARTICLES   # a bad N is the entry point's to refuse: allocate nothing for it
        particles = torch.empty(M, K, N, S, **i32) if keep else None
        ancestors, events = (torch.empty(M, K, N, **i32), torch.empty(M, K, N, **i32)) if keep else (None, None)
        log_weights = torch.empty(M, K, N, **f32) if keep else None
        if store is not None:
            particles, ancestors = store
            for t, shape in ((particles, (M, K, N, S)), (ancestors, (M, K, N))):
                if not isinstance(t, torch.Tensor) or t.device != dev or t.dtype != torch.int32 or not t.is_contiguous() \
                        or tuple(t.shape) != shape:
                    raise ValueError(f"jump_particle_filter: store must be contiguous int32 device tensors [{M}, {K}, {N}, {S}] and "
                                     f"[{M}, {K}, {N}]")
        prefix, term = _observation_term(variance, K, dev)
        if prefix:      # (lik_kind, scale, dispersion, row_const) -> lik_kind, variance, scale, dispersion, row_const
            term = (term[0], ctypes.c_double(1.0)) + term[1:]
        else:
            term = (ctypes.c_int(0),) + term + (ctypes.c_double(1.0), ctypes.c_double(1.0), _ptr(None))
        _call(*_sde_entry(lib, "jump_particle_filter", "reaction_network", network), ctypes.c_int(M), ctypes.c_int(N), ctypes.c_int(S),
              ctypes.c_int(theta.shape[1]), ctypes.c_int(K), ctypes.c_int(O), _ptr(x0), _ptr(theta), _ptr(obs_times), _ptr(obs_values),
              _ptr(obs_matrix), *term, _ptr(key), ctypes.c_int(int(max_events)), _ptr(loglik), _ptr(incr), _ptr(ess), _ptr(mean),
              _ptr(std), _ptr(stopped), _ptr(mean_events), _ptr(particles), _ptr(ancestors), _ptr(log_weights), _ptr(events),
              _stream(dev))
    return loglik, incr, ess, mean, std, stopped, mean_events, particles, ancestors, log_weights, events


def tau_leap_process(x0, theta, out_rows, key, time_step: float, record_steps: int = 0, network=None):
    """Tau-leap trajectories of a reaction network (include/vsde_hip.h: vsde_crn_tau_leap_process): x0 int32 [B, S], theta fp32
    [B, P] (the effective constants [B, 2R] for a CrnKineticRoute), out_rows int32 [K] (non-decreasing grid rows >= 0) and key (2
    int32 words), all on the device.  Returns ``(states int32 [B, K, S], status int32 [B], capped int32 [B], draws int32 [B, E, R]
    or None)`` with E = ``record_steps``."""
    lib = load()
    dev = _require_hip(x0, theta, out_rows, key)
    if x0.dtype != torch.int32 or x0.ndim != 2 or out_rows.dtype != torch.int32 or out_rows.ndim != 1:
        raise ValueError("tau_leap_process: x0 must be an int32 [B, S] tensor and out_rows an int32 [K] tensor")
    if key.dtype not in (torch.int32, torch.uint32) or key.numel() != 2:
        raise ValueError("tau_leap_process: key must be two int32 words")
    x0, theta, out_rows, key = x0.contiguous(), _f32c(theta), out_rows.contiguous(), key.contiguous()
    B, S = x0.shape
    K, E = out_rows.shape[0], int(record_steps)
    if theta.ndim != 2 or theta.shape[0] != B:
        raise ValueError(f"tau_leap_process: theta {tuple(theta.shape)} does not have one row for each of the {B} start states")
    if B < 1 or K < 1 or E < 0:
        raise ValueError(f"tau_leap_process: bad dims B={B} K={K} E={E}")
    net = network.network if isinstance(network, CrnKineticRoute) else network
    R = int(net.R) if isinstance(net, CrnNetwork) else 0
    with torch.cuda.device(dev):
        i32 = dict(device=dev, dtype=torch.int32)
        states, status, capped = torch.empty(B, K, S, **i32), torch.empty(B, **i32), torch.empty(B, **i32)
        draws = torch.empty(B, E, R, **i32) if E and R else None
        _call(*_sde_entry(lib, "tau_leap_process", "reaction_network", network), ctypes.c_int(B), ctypes.c_int(S),
              ctypes.c_int(theta.shape[1]), ctypes.c_int(K), ctypes.c_int(E), _ptr(x0), _ptr(theta), _ptr(out_rows), _ptr(key),
              ctypes.c_double(time_step), _ptr(states), _ptr(status), _ptr(capped), _ptr(draws), _stream(dev))
    return states, status, capped, draws


TAU_LEAP_FILTER_MAX_PARTICLES = PF_MAX_PARTICLES // 2


def tau_leap_filter_max_particles(state_dim: int, n_reactions: int, kinetic: bool = False) -> int:
    """The largest ``n_particles`` (a multiple of 64) the tau-leap filter kernel takes for a network of ``state_dim`` species and
    ``n_reactions`` reactions, with rate laws or without (csrc/vsde_tau_leap.hip: tlf_max_n): the float64 Poisson sampler takes
    118 .. 171 VGPRs, more than the 128 a lane has in a 1024-thread workgroup, so every instantiation is built for 512."""
    if not (1 <= state_dim <= CRN_MAX_SPECIES and 1 <= n_reactions <= CRN_MAX_REACTIONS):
        raise ValueError(f"tau_leap_filter_max_particles: {state_dim} species / {n_reactions} reactions outside 1..{CRN_MAX_SPECIES} / "
                         f"1..{CRN_MAX_REACTIONS}")
    return TAU_LEAP_FILTER_MAX_PARTICLES


def tau_leap_particle_filter(x0, theta, obs_rows, obs_values, obs_matrix, variance, key, time_step: float, n_particles: int,
                             network=None, return_particles: bool = False, store=None):
    """Bootstrap particle filters on the tau-leap of a reaction network (include/vsde_hip.h: vsde_crn_tau_leap_particle_filter), one
    per row of theta fp32 [M, P] (the effective constants [M, 2R] for a CrnKineticRoute) from the start states x0 int32 [M, S],
    against obs_values fp32 [K, O] at the grid rows obs_rows int32 [K], with a Gaussian observation term (obs_matrix [O, S] or
    None; ``variance``: a number) or a count term (``variance``: the likelihood's ``CountKernelTerms``); key: 2 int32 words;
    everything on the device.  Returns (log_likelihood [M], increments [M, K], effective_sample_size [M, K], filtered_mean [M, K,
    S], filtered_std [M, K, S], stopped int32 [M, K], capped int32 [M, K], and with ``return_particles``, else None: particles int32
    [M, K, N, S], ancestors int32 [M, K, N], log_weights [M, K, N]).  ``store``: ``(particles, ancestors)``, contiguous int32
    device buffers of those shapes to write into instead (no allocation per launch); they are returned in their places,
    log_weights stays None."""
    lib = load()
    dev = _require_hip(x0, theta, obs_rows, obs_values, obs_matrix, key)
    if x0.dtype != torch.int32 or x0.ndim != 2 or obs_rows.dtype != torch.int32 or obs_rows.ndim != 1:
        raise ValueError("tau_leap_particle_filter: x0 must be an int32 [M, S] tensor and obs_rows an int32 [K] tensor")
    if key.dtype not in (torch.int32, torch.uint32) or key.numel() != 2:
        raise ValueError("tau_leap_particle_filter: key must be two int32 words")
    x0, theta, obs_rows, obs_values, key = x0.contiguous(), _f32c(theta), obs_rows.contiguous(), _f32c(obs_values), key.contiguous()
    obs_matrix = None if obs_matrix is None else _f32c(obs_matrix)
    if theta.ndim != 2 or theta.shape[0] != x0.shape[0] or obs_values.ndim != 2 or obs_values.shape[0] != obs_rows.shape[0]:
        raise ValueError(f"tau_leap_particle_filter: x0 [M, S], theta [M, P], obs_values [K, O], obs_rows [K] expected, got "
                         f"{tuple(x0.shape)}, {tuple(theta.shape)}, {tuple(obs_values.shape)}, {tuple(obs_rows.shape)}")
    M, S = x0.shape
    K, O = obs_values.shape
    N = int(n_particles)
    if obs_matrix is not None and tuple(obs_matrix.shape) != (O, S):
        raise ValueError(f"tau_leap_particle_filter: obs_matrix must be [{O}, {S}], got {tuple(obs_matrix.shape)}")
    with torch.cuda.device(dev):
        f32, i32 = dict(device=dev, dtype=torch.float32), dict(device=dev, dtype=torch.int32)
        loglik, incr, ess = torch.empty(M, **f32), torch.empty(M, K, **f32), torch.empty(M, K, **f32)
        mean, std = torch.empty(M, K, S, **f32), torch.empty(M, K, S, **f32)
        stopped, capped = torch.empty(M, K, **i32), torch.empty(M, K, **i32)
        keep = return_particles and 0 < N <= PF_MAX_PARTICLES   # a bad N is the entry point's to refuse: allocate nothing for it
        particles = torch.empty(M, K, N, S, **i32) if keep else None
        ancestors = torch.empty(M, K, N, **i32) if keep else None
        log_weights = torch.empty(M, K, N, **f32) if keep else None
        if store is not None:
            particles, ancestors = store
            for t, shape in ((particles, (M, K, N, S)), (ancestors, (M, K, N))):
                if not isinstance(t, torch.Tensor) or t.device != dev or t.dtype != torch.int32 or not t.is_contiguous() \
                        or tuple(t.shape) != shape:
                    raise ValueError(f"tau_leap_particle_filter: store must be contiguous int32 device tensors [{M}, {K}, {N}, {S}] "
                                     f"and [{M}, {K}, {N}]")
        prefix, term = _observation_term(variance, K, dev)
        if prefix:      # (lik_kind, scale, dispersion, row_const) -> lik_kind, variance, scale, dispersion, row_const
            term = (term[0], ctypes.c_double(1.0)) + term[1:]
        else:
            term = (ctypes.c_int(0),) + term + (ctypes.c_double(1.0), ctypes.c_double(1.0), _ptr(None))
        _call(*_sde_entry(lib, "tau_leap_particle_filter", "reaction_network", network), ctypes.c_int(M), ctypes.c_int(N),
              ctypes.c_int(S), ctypes.c_int(theta.shape[1]), ctypes.c_int(K), ctypes.c_int(O), _ptr(x0), _ptr(theta), _ptr(obs_rows),
              _ptr(obs_values), _ptr(obs_matrix), *term, _ptr(key), ctypes.c_double(time_step), _ptr(loglik), _ptr(incr), _ptr(ess),
              _ptr(mean), _ptr(std), _ptr(stopped), _ptr(capped), _ptr(particles), _ptr(ancestors), _ptr(log_weights), _stream(dev))
    return loglik, incr, ess, mean, std, stopped, capped, particles, ancestors, log_weights


def _jump_replay_inputs(who: str, x0, theta, obs_times, path_times, q_begin, max_events):
    """What the two jump replays check alike; returns the contiguous (x0, theta, obs_times, path_times, q_begin on the device)."""
    if x0.dtype != torch.int32 or x0.ndim != 2 or obs_times.dtype != torch.float64 or obs_times.ndim != 1 \
            or path_times.dtype != torch.float64 or path_times.ndim != 1:
        raise ValueError(f"{who}: x0 must be an int32 [rows, S] tensor, obs_times and path_times float64 [K] and [Q] tensors")
    theta = _f32c(theta)
    if theta.ndim != 2 or theta.shape[0] != x0.shape[0]:
        raise ValueError(f"{who}: theta {tuple(theta.shape)} does not have one row for each of the {x0.shape[0]} start states")
    K, Q = obs_times.shape[0], path_times.shape[0]
    if not isinstance(q_begin, torch.Tensor) or q_begin.dtype != torch.int32 or q_begin.device.type != "cpu" or tuple(q_begin.shape) != (K + 1,):
        raise ValueError(f"{who}: q_begin must be an int32 CPU tensor [{K + 1}]")
    if K < 1 or Q < 1 or int(q_begin[0]) != 0 or int(q_begin[K]) != Q or bool((q_begin[1:] < q_begin[:-1]).any()):
        raise ValueError(f"{who}: q_begin must be non-decreasing from 0 to Q = {Q} >= 1")
    if not 1 <= int(max_events) <= 2 ** 23:
        raise ValueError(f"{who}: max_events must be in 1 .. 2^23, got {max_events}")
    return x0.contiguous(), theta, obs_times.contiguous(), path_times.contiguous(), q_begin.to(x0.device)


def jump_filter_replay(x0, theta, obs_times, path_times, q_begin, key, max_events: int, particles, ancestors, last_slot, network=None):
    """Smoothed jump-process paths from the genealogy of ``jump_particle_filter`` (include/vsde_hip.h: vsde_crn_jump_filter_replay):
    x0 int32 [M, S], theta [M, P], obs_times float64 [K], key and network as given to the filter, its particles int32 [M, K, N, S]
    and ancestors int32 [M, K, N], last_slot int32 [M, D] (-1: no sample), the output times path_times float64 [Q] on the device and
    their ownership ranges q_begin, an int32 CPU tensor [K + 1] (checked here: from 0 to Q, non-decreasing).  Returns (paths int32
    [M, D, Q, S], lineage int32 [M, D, K], n_events int32 [M, D, K], status int32 [M, D, K])."""
    lib = load()
    dev = _require_hip(x0, theta, obs_times, path_times, key, particles, ancestors, last_slot)
    x0, theta, obs_times, path_times, q_dev = _jump_replay_inputs("jump_filter_replay", x0, theta, obs_times, path_times, q_begin, max_events)
    if key.dtype not in (torch.int32, torch.uint32) or key.numel() != 2:
        raise ValueError("jump_filter_replay: key must be two int32 words")
    if particles.dtype != torch.int32 or ancestors.dtype != torch.int32 or last_slot.dtype != torch.int32:
        raise ValueError("jump_filter_replay: particles, ancestors and last_slot must be int32 tensors")
    key, particles, ancestors, last_slot = key.contiguous(), particles.contiguous(), ancestors.contiguous(), last_slot.contiguous()
    M, S = x0.shape
    K, Q = obs_times.shape[0], path_times.shape[0]
    if particles.ndim != 4 or last_slot.ndim != 2 or tuple(particles.shape[:2]) != (M, K) or particles.shape[3] != S \
            or tuple(ancestors.shape) != tuple(particles.shape[:3]) or last_slot.shape[0] != M or last_slot.shape[1] < 1:
        raise ValueError(f"jump_filter_replay: particles [M, K, N, S], ancestors [M, K, N], last_slot [M, D >= 1] expected for M = {M}, "
                         f"K = {K}, S = {S}, got {tuple(particles.shape)}, {tuple(ancestors.shape)}, {tuple(last_slot.shape)}")
    N, D = particles.shape[2], last_slot.shape[1]
    with torch.cuda.device(dev):
        i32 = dict(device=dev, dtype=torch.int32)
        paths = torch.empty(M, D, Q, S, **i32)
        lineage, n_events, status = torch.empty(M, D, K, **i32), torch.empty(M, D, K, **i32), torch.empty(M, D, K, **i32)
        _call(*_sde_entry(lib, "jump_filter_replay", "reaction_network", network), ctypes.c_int(M), ctypes.c_int(N), ctypes.c_int(S),
              ctypes.c_int(theta.shape[1]), ctypes.c_int(K), ctypes.c_int(D), ctypes.c_int(Q), _ptr(x0), _ptr(theta), _ptr(obs_times),
              _ptr(path_times), _ptr(q_dev), _ptr(key), ctypes.c_int(int(max_events)), _ptr(particles), _ptr(ancestors), _ptr(last_slot),
              _ptr(paths), _ptr(lineage), _ptr(n_events), _ptr(status), _stream(dev))
    return paths, lineage, n_events, status


def jump_anchored_replay(x0, theta, obs_times, path_times, q_begin, anchors, noise_path, keys, max_events: int, network=None):
    """Jump-process paths of B path records of particle MCMC (include/vsde_hip.h: vsde_crn_jump_anchored_replay): per record its
    start state x0 int32 [B, S], theta [B, P] (the effective constants for a CrnKineticRoute), anchors int32 [B, K, S], noise_path
    [B, K] and filter key keys [B, 2] (int32); obs_times, path_times and q_begin as in ``jump_filter_replay``.  Returns (paths int32
    [B, Q, S], n_events int32 [B, K], status int32 [B, K])."""
    lib = load()
    dev = _require_hip(x0, theta, obs_times, path_times, anchors, noise_path, keys)
    x0, theta, obs_times, path_times, q_dev = _jump_replay_inputs("jump_anchored_replay", x0, theta, obs_times, path_times, q_begin, max_events)
    ints = (torch.int32, torch.uint32)
    if anchors.dtype != torch.int32 or noise_path.dtype not in ints or keys.dtype not in ints:
        raise ValueError("jump_anchored_replay: anchors [B, K, S], noise_path [B, K] and keys [B, 2] must be int32 tensors")
    anchors, noise_path, keys = anchors.contiguous(), noise_path.contiguous(), keys.contiguous()
    B, S = x0.shape
    K, Q = obs_times.shape[0], path_times.shape[0]
    if tuple(anchors.shape) != (B, K, S) or tuple(noise_path.shape) != (B, K) or tuple(keys.shape) != (B, 2):
        raise ValueError(f"jump_anchored_replay: anchors [{B}, {K}, {S}], noise_path [{B}, {K}], keys [{B}, 2] expected, got "
                         f"{tuple(anchors.shape)}, {tuple(noise_path.shape)}, {tuple(keys.shape)}")
    with torch.cuda.device(dev):
        i32 = dict(device=dev, dtype=torch.int32)
        paths, n_events, status = torch.empty(B, Q, S, **i32), torch.empty(B, K, **i32), torch.empty(B, K, **i32)
        _call(*_sde_entry(lib, "jump_anchored_replay", "reaction_network", network), ctypes.c_int(B), ctypes.c_int(S),
              ctypes.c_int(theta.shape[1]), ctypes.c_int(K), ctypes.c_int(Q), _ptr(x0), _ptr(theta), _ptr(obs_times), _ptr(path_times),
              _ptr(q_dev), _ptr(anchors), _ptr(noise_path), _ptr(keys), ctypes.c_int(int(max_events)), _ptr(paths), _ptr(n_events),
              _ptr(status), _stream(dev))
    return paths, n_events, status


def _replay_inputs(who: str, obs_rows, words_ok: bool, words: str, guided: bool, model, state_dim: int):
    """What the two replays check alike: obs_rows is an int32 [K] tensor and the caller's integer words are what ``words`` says
    (``words_ok``); then, for a guided form, the observation model (obs_values [K, O], obs_matrix [O, S] or None, variance) of the
    filter launches.  Returns (O, the entry point's extra arguments, the fp32 casts they point into: the caller holds them until
    the launch is queued)."""
    if obs_rows.dtype != torch.int32 or obs_rows.ndim != 1 or not words_ok:
        raise ValueError(f"{who}: obs_rows must be an int32 [K] tensor{words}")
    if not guided:
        return state_dim, (), None
    obs_values, obs_matrix, variance = model
    obs_values = _f32c(obs_values)
    obs_matrix = None if obs_matrix is None else _f32c(obs_matrix)
    if obs_values.ndim != 2 or obs_values.shape[0] != obs_rows.shape[0] \
            or (obs_matrix is not None and tuple(obs_matrix.shape) != (obs_values.shape[1], state_dim)):
        raise ValueError(f"{who}: obs_values [{obs_rows.shape[0]}, O] and obs_matrix [O, {state_dim}] expected")
    return obs_values.shape[1], (_ptr(obs_values), _ptr(obs_matrix), ctypes.c_double(variance)), (obs_values, obs_matrix)


def _filter_replay(entry: str, guided: bool, kind, x0, theta, obs_rows, model, key, time_step, particles, ancestors, last_slot,
                   n_steps, positive_dims, network):
    lib = load()
    dev = _require_hip(x0, theta, obs_rows, key, particles, ancestors, last_slot, *model[:2])
    x0, theta, particles = _f32c(x0), _f32c(theta), _f32c(particles)
    O, extra, held = _replay_inputs("filter_replay", obs_rows, key.dtype in (torch.int32, torch.uint32) and key.numel() == 2,
                                    " and key two int32 words", guided, model, x0.shape[-1])
    if ancestors.dtype != torch.int32 or last_slot.dtype != torch.int32:
        raise ValueError("filter_replay: ancestors and last_slot must be int32 tensors")
    obs_rows, key, ancestors, last_slot = obs_rows.contiguous(), key.contiguous(), ancestors.contiguous(), last_slot.contiguous()
    K = obs_rows.shape[0]
    if x0.ndim != 2 or theta.ndim != 2 or theta.shape[0] != x0.shape[0] or particles.ndim != 4 or last_slot.ndim != 2 \
            or tuple(particles.shape[:2]) != (x0.shape[0], K) or particles.shape[3] != x0.shape[1] \
            or tuple(ancestors.shape) != tuple(particles.shape[:3]) or last_slot.shape[0] != x0.shape[0]:
        raise ValueError(f"filter_replay: x0 [M, S], theta [M, P], obs_rows [K], particles [M, K, N, S], ancestors [M, K, N], "
                         f"last_slot [M, D] expected, got {tuple(x0.shape)}, {tuple(theta.shape)}, {tuple(obs_rows.shape)}, "
                         f"{tuple(particles.shape)}, {tuple(ancestors.shape)}, {tuple(last_slot.shape)}")
    M, S = x0.shape
    N, D = particles.shape[2], last_slot.shape[1]
    T = int(obs_rows[-1]) if n_steps is None and K else int(n_steps or 0)
    with torch.cuda.device(dev):
        ok = D >= 1 and T >= 0    # bad sizes are the entry point's to refuse: allocate nothing for them
        paths = torch.empty(M, D, T + 1, S, device=dev, dtype=torch.float32) if ok else None
        lineage = torch.empty(M, D, K, device=dev, dtype=torch.int32) if ok else None
        _call(*_sde_entry(lib, entry, kind, network), ctypes.c_int(M), ctypes.c_int(N), ctypes.c_int(S), ctypes.c_int(theta.shape[1]),
              ctypes.c_int(K), ctypes.c_int(O), ctypes.c_int(D), ctypes.c_int(T), _ptr(x0), _ptr(theta), _ptr(obs_rows), *extra,
              _ptr(key), ctypes.c_double(time_step), _mask_bytes(positive_dims, S), _ptr(particles), _ptr(ancestors),
              _ptr(last_slot), _ptr(paths), _ptr(lineage), _stream(dev))
    return paths, lineage


def filter_replay(kind: str, x0, theta, obs_rows, key, time_step: float, particles, ancestors, last_slot, positive_dims=(),
                  network=None, n_steps: Optional[int] = None):
    """Smoothed paths from a bootstrap filter's genealogy (include/vsde_hip.h: vsde_filter_replay): ``kind``, x0, theta, obs_rows,
    key, time_step, positive_dims and network as given to ``particle_filter``, its particles [M, K, N, S] and ancestors [M, K, N],
    and last_slot [M, D] (int32; -1: no sample), the slot of each draw at the last observation.  ``n_steps``: obs_rows[K-1] when
    the caller knows it (saves reading it back from the device).  Returns (paths [M, D, T+1, S], lineage [M, D, K] int32)."""
    return _filter_replay("filter_replay", False, kind, x0, theta, obs_rows, (None, None, None), key, time_step, particles, ancestors,
                          last_slot, n_steps, positive_dims, network)


def guided_filter_replay(kind: str, x0, theta, obs_rows, obs_values, obs_matrix, variance: float, key, time_step: float, particles,
                         ancestors, last_slot, positive_dims=(), network=None, n_steps: Optional[int] = None, residual: bool = False):
    """``filter_replay`` for the stored particles of ``guided_particle_filter`` (vsde_guided_filter_replay; S <= 4, O <= 4): the
    bridge steps need the observations, obs_matrix and variance of that call as well, and its ``residual``
    (vsde_residual_filter_replay)."""
    return _filter_replay("residual_filter_replay" if residual else "guided_filter_replay", True, kind, x0, theta, obs_rows,
                          (obs_values, obs_matrix, variance), key, time_step, particles, ancestors, last_slot, n_steps, positive_dims,
                          network)


PMMH_MAX_PARAMS = 16


def pmmh_step(iteration: int, scale_tril, step_size: float, prior_type: int, prior_mean: float, prior_std: float,
              theta_positive_dims, key, loglik_prop, cur_u, cur_log_target, cur_loglik, prop_u, prop_log_prior, theta_prop,
              filter_key, n_accept, sample_row=None, loglik_row=None, target_row=None, _paths=None) -> None:
    """One Metropolis step of particle MCMC, in place (include/vsde_hip.h: vsde_pmmh_step): closes iteration ``iteration - 1`` with
    the filter estimates ``loglik_prop [C, R]`` (None: nothing to close) and opens iteration ``iteration``.  ``scale_tril``: a
    contiguous fp32 CPU tensor [P, P]; ``key`` / ``filter_key``: 2 int32 words on the device; chain state ``cur_u [C, P]``,
    ``cur_log_target [C]``, ``cur_loglik [C]``, the pending proposal ``prop_u [C, P]``, ``prop_log_prior [C]``, the filter's input
    ``theta_prop [C R, P]`` and ``n_accept [C]`` (int32) are contiguous device tensors written in place; ``sample_row [C, P]``,
    ``loglik_row [C]``, ``target_row [C]``: where the closed state is kept, or None.  C, P are prop_u's shape, R = rows of
    theta_prop / C."""
    lib = load()
    dev = _require_hip(key, prop_u, theta_prop)
    if not (isinstance(scale_tril, torch.Tensor) and scale_tril.device.type == "cpu" and scale_tril.dtype == torch.float32
            and scale_tril.is_contiguous() and prop_u.ndim == 2 and tuple(scale_tril.shape) == (prop_u.shape[1],) * 2):
        raise ValueError("pmmh_step: prop_u [C, P] and scale_tril, a contiguous fp32 CPU tensor [P, P], expected")
    for t, dt in ((key, None), (filter_key, None), (n_accept, torch.int32), (loglik_prop, torch.float32), (cur_u, torch.float32),
                  (cur_log_target, torch.float32), (cur_loglik, torch.float32), (prop_u, torch.float32),
                  (prop_log_prior, torch.float32), (theta_prop, torch.float32), (sample_row, torch.float32),
                  (loglik_row, torch.float32), (target_row, torch.float32)):
        if t is not None and (t.device != dev or not t.is_contiguous() or (t.dtype != dt if dt else t.dtype not in (torch.int32, torch.uint32))):
            raise ValueError("pmmh_step: contiguous fp32 tensors (int32: key, filter_key, n_accept) on one device expected")
    C, P = prop_u.shape
    R = theta_prop.shape[0] // C if C else 1
    sizes = ((key, 2), (filter_key, 2), (n_accept, C), (loglik_prop, C * R), (cur_u, C * P), (cur_log_target, C), (cur_loglik, C),
             (prop_log_prior, C), (theta_prop, C * R * P), (sample_row, C * P), (loglik_row, C), (target_row, C))
    if any(t is not None and t.numel() != n for t, n in sizes):
        raise ValueError(f"pmmh_step: a tensor does not have the size that C = {C}, P = {P}, R = {R} give it")
    entry, tail = lib.vsde_pmmh_step, ()
    if _paths is not None:
        particles, ancestors, cur_anchor, cur_noise_path, cur_path_iteration, anchor_row, noise_row, iteration_row = _paths
        bad = "pmmh_step_paths: particles fp32 [C R, K, N, S], ancestors int32 [C R, K, N], cur_anchor fp32 [C, K, S], cur_noise_path " \
              "int32 [C, K], cur_path_iteration int32 [C] and rows of the records' shapes or None, contiguous on one device, expected"
        if not (isinstance(particles, torch.Tensor) and particles.ndim == 4 and particles.shape[0] == C * R):
            raise ValueError(bad)
        _, K, N, S = particles.shape
        for t, dt, shape in ((particles, torch.float32, (C * R, K, N, S)), (ancestors, torch.int32, (C * R, K, N)),
                             (cur_anchor, torch.float32, (C, K, S)), (cur_noise_path, None, (C, K)),
                             (cur_path_iteration, torch.int32, (C,)), (anchor_row, torch.float32, (C, K, S)), (noise_row, None, (C, K)),
                             (iteration_row, torch.int32, (C,))):
            required = t is particles or t is ancestors or t is cur_anchor or t is cur_noise_path or t is cur_path_iteration
            if t is None and not required:
                continue
            if not isinstance(t, torch.Tensor) or t.device != dev or not t.is_contiguous() or tuple(t.shape) != shape \
                    or (t.dtype != dt if dt else t.dtype not in (torch.int32, torch.uint32)):
                raise ValueError(bad)
        entry = lib.vsde_pmmh_step_paths
        tail = (ctypes.c_int(N), ctypes.c_int(K), ctypes.c_int(S), _ptr(particles), _ptr(ancestors), _ptr(cur_anchor),
                _ptr(cur_noise_path), _ptr(cur_path_iteration), _ptr(anchor_row), _ptr(noise_row), _ptr(iteration_row))
    with torch.cuda.device(dev):
        _call(entry, ctypes.c_int(C), ctypes.c_int(P), ctypes.c_int(R), ctypes.c_int(int(iteration)),
              ctypes.c_void_p(scale_tril.data_ptr()), ctypes.c_double(step_size), ctypes.c_int(int(prior_type)),
              ctypes.c_double(prior_mean), ctypes.c_double(prior_std), _mask_bytes(theta_positive_dims, P), _ptr(key),
              _ptr(loglik_prop), _ptr(cur_u), _ptr(cur_log_target), _ptr(cur_loglik), _ptr(prop_u), _ptr(prop_log_prior),
              _ptr(theta_prop), _ptr(filter_key), _ptr(sample_row), _ptr(loglik_row), _ptr(target_row), _ptr(n_accept), *tail,
              _stream(dev))


def pmmh_step_paths(iteration: int, scale_tril, step_size: float, prior_type: int, prior_mean: float, prior_std: float,
                    theta_positive_dims, key, loglik_prop, cur_u, cur_log_target, cur_loglik, prop_u, prop_log_prior, theta_prop,
                    filter_key, n_accept, particles, ancestors, cur_anchor, cur_noise_path, cur_path_iteration, sample_row=None,
                    loglik_row=None, target_row=None, anchor_row=None, noise_row=None, iteration_row=None) -> None:
    """``pmmh_step`` for chains that carry a latent path (include/vsde_hip.h: vsde_pmmh_step_paths): the same step, and for every
    chain it accepts the record of the proposal's path drawn from ``particles [C R, K, N, S]`` and ``ancestors [C R, K, N]`` (int32),
    what the filter launch of the closed iteration stored.  The records ``cur_anchor [C, K, S]``, ``cur_noise_path [C, K]`` (int32
    holding the uint32 path indices; all ones: dead) and ``cur_path_iteration [C]`` (int32) are written in place; ``anchor_row``,
    ``noise_row``, ``iteration_row``: where the carried records are kept, or None."""
    pmmh_step(iteration, scale_tril, step_size, prior_type, prior_mean, prior_std, theta_positive_dims, key, loglik_prop, cur_u,
              cur_log_target, cur_loglik, prop_u, prop_log_prior, theta_prop, filter_key, n_accept, sample_row, loglik_row, target_row,
              _paths=(particles, ancestors, cur_anchor, cur_noise_path, cur_path_iteration, anchor_row, noise_row, iteration_row))


def _anchored_replay(entry: str, guided: bool, kind, x0, theta, obs_rows, model, anchors, noise_path, keys, time_step, n_steps,
                     positive_dims, network):
    lib = load()
    dev = _require_hip(x0, theta, obs_rows, anchors, noise_path, keys, *model[:2])
    x0, theta, anchors = _f32c(x0), _f32c(theta), _f32c(anchors)
    ints = (torch.int32, torch.uint32)
    O, extra, held = _replay_inputs("anchored_replay", obs_rows, noise_path.dtype in ints and keys.dtype in ints,
                                    ", noise_path [B, K] and keys [B, 2] int32 tensors", guided, model, x0.shape[-1])
    obs_rows, noise_path, keys = obs_rows.contiguous(), noise_path.contiguous(), keys.contiguous()
    K = obs_rows.shape[0]
    if x0.ndim != 2 or theta.ndim != 2 or theta.shape[0] != x0.shape[0] or tuple(anchors.shape) != (x0.shape[0], K, x0.shape[1]) \
            or tuple(noise_path.shape) != (x0.shape[0], K) or tuple(keys.shape) != (x0.shape[0], 2):
        raise ValueError(f"anchored_replay: x0 [B, S], theta [B, P], obs_rows [K], anchors [B, K, S], noise_path [B, K], keys [B, 2] "
                         f"expected, got {tuple(x0.shape)}, {tuple(theta.shape)}, {tuple(obs_rows.shape)}, {tuple(anchors.shape)}, "
                         f"{tuple(noise_path.shape)}, {tuple(keys.shape)}")
    B, S = x0.shape
    T = int(obs_rows[-1]) if n_steps is None and K else int(n_steps or 0)
    with torch.cuda.device(dev):
        paths = torch.empty(B, T + 1, S, device=dev, dtype=torch.float32) if T >= 0 else None   # a bad T is the entry point's to refuse
        _call(*_sde_entry(lib, entry, kind, network), ctypes.c_int(B), ctypes.c_int(S), ctypes.c_int(theta.shape[1]), ctypes.c_int(K),
              ctypes.c_int(O), ctypes.c_int(T), _ptr(x0), _ptr(theta), _ptr(obs_rows), *extra, _ptr(anchors), _ptr(noise_path),
              _ptr(keys), ctypes.c_double(time_step), _mask_bytes(positive_dims, S), _ptr(paths), _stream(dev))
    return paths


def anchored_replay(kind: str, x0, theta, obs_rows, anchors, noise_path, keys, time_step: float, positive_dims=(), network=None,
                    n_steps: Optional[int] = None):
    """Paths [B, T+1, S] of B path records of ``pmmh_step_paths`` (include/vsde_hip.h: vsde_anchored_replay): per record its start
    state x0 [B, S], theta [B, P] (the effective constants for a CrnKineticRoute), anchors [B, K, S], noise_path [B, K] and filter
    key keys [B, 2] (int32); ``kind``, obs_rows, time_step, positive_dims and network as given to the filter launches the records
    were drawn from.  ``n_steps``: obs_rows[K-1] when the caller knows it (saves reading it back from the device)."""
    return _anchored_replay("anchored_replay", False, kind, x0, theta, obs_rows, (None, None, None), anchors, noise_path, keys, time_step,
                            n_steps, positive_dims, network)


def guided_anchored_replay(kind: str, x0, theta, obs_rows, obs_values, obs_matrix, variance: float, anchors, noise_path, keys,
                           time_step: float, positive_dims=(), network=None, n_steps: Optional[int] = None, residual: bool = False):
    """``anchored_replay`` for records drawn from ``guided_particle_filter`` launches (vsde_guided_anchored_replay; S <= 4, O <= 4):
    the bridge steps need the observations, obs_matrix and variance of those launches as well, and their ``residual``
    (vsde_residual_anchored_replay)."""
    return _anchored_replay("residual_anchored_replay" if residual else "guided_anchored_replay", True, kind, x0, theta, obs_rows,
                            (obs_values, obs_matrix, variance), anchors, noise_path, keys, time_step, n_steps, positive_dims, network)


def _tail_args(x_obs, obs_values, obs_matrix, variance, theta, prior_type, prior_mean, prior_std, post_mean, post_log_std, theta_positive_dims):
    """(prefix of the entry point's name, the leading arguments); ``variance``: see ``_observation_term``."""
    B, K, S = x_obs.shape
    O, P = obs_values.shape[1], theta.shape[1]
    prefix, term = _observation_term(variance, K, x_obs.device)
    return prefix, (ctypes.c_int(B), ctypes.c_int(K), ctypes.c_int(S), ctypes.c_int(O), ctypes.c_int(P), _ptr(x_obs), _ptr(obs_values),
            _ptr(obs_matrix), *term, _ptr(theta), ctypes.c_int(prior_type), ctypes.c_double(prior_mean),
            ctypes.c_double(prior_std), _ptr(post_mean), _ptr(post_log_std), _mask_bytes(theta_positive_dims, P))


def elbo_tail_fwd(x_obs, obs_values, obs_matrix, variance: float, theta, prior_type: int, prior_mean: float, prior_std: float,
                  post_mean, post_log_std, theta_positive_dims, sde_lp, gen_lp, log_jac):
    """[elbo, obs, sde, gen, prior, post] batch means (see include/vsde_hip.h: vsde_elbo_tail_fwd)."""
    lib = load()
    dev = _require_hip(x_obs, obs_values, theta, post_mean, post_log_std, sde_lp, gen_lp, log_jac)
    x_obs, obs_values, theta, post_mean, post_log_std, sde_lp, gen_lp, log_jac = (
        _f32c(t) for t in (x_obs, obs_values, theta, post_mean, post_log_std, sde_lp, gen_lp, log_jac))
    obs_matrix = None if obs_matrix is None else _f32c(obs_matrix)
    with torch.cuda.device(dev):
        out = torch.empty(6, device=dev, dtype=torch.float32)
        prefix, args = _tail_args(x_obs, obs_values, obs_matrix, variance, theta, prior_type, prior_mean, prior_std, post_mean,
                                  post_log_std, theta_positive_dims)
        _call(getattr(lib, f"vsde_{prefix}elbo_tail_fwd"), *args, _ptr(sde_lp), _ptr(gen_lp), _ptr(log_jac), _ptr(out), _stream(dev))
    return out


def elbo_tail_bwd(x_obs, obs_values, obs_matrix, variance: float, theta, prior_type: int, prior_mean: float, prior_std: float,
                  post_mean, post_log_std, theta_positive_dims, g_out):
    """Gradients of ``elbo_tail_fwd``: (g_x_obs, g_theta, g_post_mean, g_post_log_std, g_sde, g_gen, g_jac)."""
    lib = load()
    dev = _require_hip(x_obs, obs_values, theta, post_mean, post_log_std, g_out)
    x_obs, obs_values, theta, post_mean, post_log_std, g_out = (
        _f32c(t) for t in (x_obs, obs_values, theta, post_mean, post_log_std, g_out))
    obs_matrix = None if obs_matrix is None else _f32c(obs_matrix)
    B = theta.shape[0]
    with torch.cuda.device(dev):
        g_x = torch.empty_like(x_obs); g_theta = torch.empty_like(theta)
        g_mean = torch.empty_like(post_mean); g_ls = torch.empty_like(post_log_std)
        g_paths = torch.empty(3, B, device=dev, dtype=torch.float32)
        prefix, args = _tail_args(x_obs, obs_values, obs_matrix, variance, theta, prior_type, prior_mean, prior_std, post_mean,
                                  post_log_std, theta_positive_dims)
        _call(getattr(lib, f"vsde_{prefix}elbo_tail_bwd"), *args, _ptr(g_out), _ptr(g_x), _ptr(g_theta), _ptr(g_mean), _ptr(g_ls), _ptr(g_paths[0]), _ptr(g_paths[1]), _ptr(g_paths[2]),
              _stream(dev))
    return g_x, g_theta, g_mean, g_ls, g_paths[0], g_paths[1], g_paths[2]


def log_weights(kind: str | None, z, means, chol, drift, diffusion, theta, obs_rows, obs_values, obs_matrix, variance: float,
                prior_type: int, prior_mean: float, prior_std: float, post_mean, post_log_std, state_positive_dims,
                theta_positive_dims, time_step: float, network=None, rates=None):
    """Per-sample importance log-weights [B] (see include/vsde_hip.h: vsde_log_weights).  ``kind`` in SDE_KINDS evaluates the
    built-in drift / diffusion in the kernel (``drift`` / ``diffusion`` None; a reaction network also needs its ``network``
    descriptor: vsde_crn_log_weights, and for a CrnKineticRoute the effective constants ``rates`` [B, 2R] of the drift /
    diffusion: vsde_crn_kinetic_log_weights); ``kind`` None reads the given tensors."""
    lib = load()
    dev = _require_hip(z, means, chol, drift, diffusion, theta, rates, obs_rows, obs_values, post_mean, post_log_std)
    z, means, chol, theta, obs_values, post_mean, post_log_std = (
        _f32c(t) for t in (z, means, chol, theta, obs_values, post_mean, post_log_std))
    drift, diffusion, obs_matrix = (None if t is None else _f32c(t) for t in (drift, diffusion, obs_matrix))
    obs_rows = obs_rows.to(torch.int32).contiguous()
    B, T1, S = z.shape
    K, O, P = obs_rows.shape[0], obs_values.shape[1], theta.shape[1]
    if tuple(means.shape) != (B, T1 - 1, S) or tuple(chol.shape) != (B, T1 - 1, S, S) or theta.shape[0] != B \
            or obs_values.shape[0] != K or post_mean.numel() != P or post_log_std.numel() != P \
            or (obs_matrix is not None and tuple(obs_matrix.shape) != (O, S)) or (obs_matrix is None and O != S):
        raise ValueError("log_weights: inconsistent shapes")
    if kind is None and (drift is None or tuple(drift.shape) != (B, T1 - 1, S) or tuple(diffusion.shape) != (B, T1 - 1, S, S)):
        raise ValueError("log_weights: drift [B, T, S] and diffusion [B, T, S, S] are required without a built-in kind")
    dims = (ctypes.c_int(B), ctypes.c_int(T1 - 1), ctypes.c_int(S), ctypes.c_int(K), ctypes.c_int(O), ctypes.c_int(P),
            _ptr(z), _ptr(means), _ptr(chol))
    prefix, term = _observation_term(variance, K, dev)
    tail = (_ptr(theta), _ptr(obs_rows), _ptr(obs_values), _ptr(obs_matrix), *term,
            ctypes.c_int(prior_type), ctypes.c_double(prior_mean), ctypes.c_double(prior_std), _ptr(post_mean),
            _ptr(post_log_std), _mask_bytes(state_positive_dims, S), _mask_bytes(theta_positive_dims, P),
            ctypes.c_double(time_step))
    with torch.cuda.device(dev):
        out = torch.empty(B, device=dev, dtype=torch.float32)
        if kind == "reaction_network" and isinstance(network, CrnKineticRoute):
            if rates is None or rates.ndim != 2 or rates.shape[0] != B:
                raise ValueError("log_weights: a reaction network with rate laws needs its effective constants rates [B, 2R]")
            rates = _f32c(rates)
            fn, net, kin = _sde_entry(lib, prefix + "log_weights", kind, network)
            _call(fn, net, kin, *dims[:6], ctypes.c_int(rates.shape[1]), *dims[6:], _ptr(theta), _ptr(rates), *tail[1:],
                  _ptr(out), _stream(dev))
        elif kind == "reaction_network":
            fn, net = _sde_entry(lib, prefix + "log_weights", kind, network)
            _call(fn, net, *dims, *tail, _ptr(out), _stream(dev))
        else:
            _call(getattr(lib, f"vsde_{prefix}log_weights"), ctypes.c_int(0 if kind is None else SDE_KINDS[kind]), *dims, _ptr(drift), _ptr(diffusion),
                  *tail, _ptr(out), _stream(dev))
    return out


def log_weight_state(device) -> torch.Tensor:
    """A fresh accumulator state for ``log_weight_accumulate``: fp64 [M, S1, S2, sum lw, n, n_nonfinite] = [-inf, 0, ...] on
    ``device`` (a HIP device: the accumulator has no CPU implementation)."""
    state = torch.zeros(6, device=device, dtype=torch.float64)
    _require_hip(state)
    state[0] = float("-inf")
    return state


def log_weight_accumulate(log_w, n: int, state) -> None:
    """Merge the first ``n`` entries of ``log_w`` [>= n] into ``state`` in place, in stream order (no host synchronisation)."""
    lib = load()
    dev = _require_hip(log_w, state)
    log_w = _f32c(log_w)
    if log_w.ndim != 1 or not 0 < n <= log_w.shape[0]:
        raise ValueError(f"log_weight_accumulate: need 0 < n <= {log_w.shape[0] if log_w.ndim == 1 else '?'} (got {n})")
    if state.dtype != torch.float64 or tuple(state.shape) != (6,) or not state.is_contiguous():
        raise ValueError("log_weight_accumulate: state must be a contiguous float64 [6] tensor")
    with torch.cuda.device(dev):
        _call(lib.vsde_log_weight_accumulate, ctypes.c_int(n), _ptr(log_w), _ptr(state), _stream(dev))


def sde_coefficients_fwd(kind: str, x, theta, network=None):
    """(drift [B,T,S], diffusion [B,T,S,S]) of a built-in SDE on the first T points of every path x [B, T+1, S]."""
    lib = load()
    dev = _require_hip(x, theta)
    x, theta = _f32c(x), _f32c(theta)
    B, T1, S = x.shape
    T = T1 - 1
    with torch.cuda.device(dev):
        drift = torch.empty(B, T, S, device=dev, dtype=torch.float32)
        diffusion = torch.empty(B, T, S, S, device=dev, dtype=torch.float32)
        _call(*_sde_entry(lib, "sde_coefficients_fwd", kind, network), ctypes.c_int(B), ctypes.c_int(T), ctypes.c_int(S),
              ctypes.c_int(theta.shape[1]), _ptr(x), _ptr(theta), _ptr(drift), _ptr(diffusion), _stream(dev))
    return drift, diffusion


def sde_coefficients_bwd(kind: str, x, theta, g_drift, g_diffusion, network=None):
    """(g_x [B,T+1,S], g_theta [B,P]) of ``sde_coefficients_fwd``."""
    lib = load()
    dev = _require_hip(x, theta, g_drift, g_diffusion)
    x, theta, g_drift, g_diffusion = _f32c(x), _f32c(theta), _f32c(g_drift), _f32c(g_diffusion)
    B, T1, S = x.shape
    with torch.cuda.device(dev):
        g_x = torch.empty_like(x)
        g_theta = torch.empty_like(theta)
        _call(*_sde_entry(lib, "sde_coefficients_bwd", kind, network), ctypes.c_int(B), ctypes.c_int(T1 - 1), ctypes.c_int(S),
              ctypes.c_int(theta.shape[1]), _ptr(x), _ptr(theta), _ptr(g_drift), _ptr(g_diffusion), _ptr(g_x), _ptr(g_theta),
              _stream(dev))
    return g_x, g_theta


def pack_refresh(table: torch.Tensor) -> None:
    """One launch that re-fills the cached bf16 GEMM operands (and their transposes) from the fp32 parameters; ``table`` is
    the int64 [n_tiles, 8] device tensor built by ``primitives.fused.PackedWeight.refresh_all``."""
    lib = load()
    dev = _require_hip(table)
    if table.dtype != torch.int64 or table.ndim != 2 or table.shape[1] * 8 != lib.vsde_pack_tile_bytes() or not table.is_contiguous():
        raise ValueError("pack-refresh table must be a contiguous int64 [n_tiles, 8] tensor")
    with torch.cuda.device(dev):
        _call(lib.vsde_pack_refresh, _ptr(table), ctypes.c_int(table.shape[0]), _stream(dev))


def optim_chunk_elems() -> int:
    return int(load().vsde_optim_chunk_elems())


def optim_step(table: torch.Tensor, grad_ptrs: torch.Tensor, scale: Optional[torch.Tensor], partials: torch.Tensor, tstate: torch.Tensor,
               groups: torch.Tensor, max_norm: float, ema_weight: float, out: torch.Tensor) -> None:
    """unscale + global-norm clip + AdamW + EMA of every parameter as two launches (csrc/vsde_optim.hip).  ``table``: int64
    [n_chunks, 8] chunk records; ``grad_ptrs``: int64 [n_params] device pointers of this step's gradients; ``scale``: the loss
    scale (fp32 device scalar) or None; ``groups``: float64 [n_groups, 5]; ``out``: fp32 [2] <- (gradient norm, found_inf)."""
    lib = load()
    dev = _require_hip(table, grad_ptrs, partials, tstate, groups, out)
    if (table.dtype != torch.int64 or table.ndim != 2 or table.shape[1] * 8 != lib.vsde_optim_chunk_bytes() or not table.is_contiguous()
            or grad_ptrs.dtype != torch.int64 or groups.dtype != torch.float64 or partials.numel() < table.shape[0]
            or tstate.dtype != torch.float32 or out.dtype != torch.float32):
        raise ValueError("bad optimizer-step buffers")
    with torch.cuda.device(dev):
        _call(lib.vsde_optim_step, _ptr(table), ctypes.c_int(table.shape[0]), _ptr(grad_ptrs), _ptr(scale), _ptr(partials), _ptr(tstate),
              _ptr(groups), ctypes.c_double(max_norm), ctypes.c_double(ema_weight), _ptr(out), _stream(dev))


def profile_enable(on: bool) -> None:
    load().vsde_profile_enable(ctypes.c_int(1 if on else 0))


def profile_elapsed_ms(which: int) -> float:
    """Duration of the last timed serial kernel (0 = forward/train, 1 = backward), HIP events."""
    ms = ctypes.c_float(0.0)
    rc = load().vsde_profile_elapsed_ms(ctypes.c_int(which), ctypes.byref(ms))
    if rc != 0:
        _raise(rc)
    return float(ms.value)


def debug_force_v1(on: bool) -> None:
    """Test hook: run 1-2 layer heads through the kernels that normally serve 3-4 layers."""
    load().vsde_debug_force_v1(ctypes.c_int(1 if on else 0))


def debug_head_mp(mode: int) -> None:
    """Forward time-stepping kernel for hidden_dim 64 / L <= 2 / state_dim <= 2: 1 = the multi-path MFMA kernel whenever
    applicable, 0 = the four-waves-per-path kernel, -1 = default (VSDE_HEAD_MP, else by batch size)."""
    load().vsde_debug_head_mp(ctypes.c_int(mode))


def head_backward_workspace_bytes(B: int, T: int, S: int, P: int, C: int, H: int, L: int) -> int:
    """Size query of ``vsde_head_backward`` (host only, no GPU needed); 0 = dims the kernels refuse."""
    return int(load().vsde_head_backward_workspace_bytes(ctypes.byref(_Dims(B, T, S, P, C, H, L))))


def head_forward_workspace_bytes(B: int, T: int, S: int, P: int, C: int, H: int, L: int) -> int:
    return int(load().vsde_head_forward_workspace_bytes(ctypes.byref(_Dims(B, T, S, P, C, H, L))))


def debug_head_context_projection(ctx, ws, state_dim: int, param_dim: int):
    """Test hook: G [B*T, 3H] = ctx W_ih_l0[:, S:S+C]^T + b_ih_l0 through the weight packing and the projection dispatch of
    ``head_forward`` alone.  ``ctx`` [B, T, C] (f32 / bf16) is passed as the view it is (strides and alignment are what the dispatch
    looks at); G is pre-filled with NaN."""
    lib = load()
    dev = _require_hip(ctx, *ws)
    if ctx.dtype not in (torch.float32, torch.bfloat16) or ctx.stride(2) != 1:
        raise ValueError("ctx must be an f32 / bf16 [B, T, C] view with a contiguous last dimension")
    ctx, cview = context_view(ctx)
    keep, wstruct = _weights_struct(ws)
    B, T, C = ctx.shape
    H = keep[1].shape[1]
    L = 1 + (keep[4].shape[0] if keep[4].numel() > 0 else 0)
    if tuple(keep[0].shape) != (3 * H, state_dim + C + param_dim):
        raise ValueError(f"W_ih_l0 has shape {tuple(keep[0].shape)}, expected {(3 * H, state_dim + C + param_dim)}")
    d = _Dims(B, T, state_dim, param_dim, C, H, L)
    with torch.cuda.device(dev):
        G = torch.full((B * T, 3 * H), float("nan"), device=dev, dtype=torch.float32)
        nbytes = lib.vsde_head_forward_workspace_bytes(ctypes.byref(d))
        if nbytes == 0:
            _raise(-1)
        wsbuf = torch.empty(nbytes, device=dev, dtype=torch.uint8)
        rc = lib.vsde_debug_head_context_projection(ctypes.byref(d), ctypes.byref(cview), ctypes.byref(wstruct), _ptr(G),
                                                    _ptr(wsbuf), ctypes.c_size_t(nbytes), _stream(dev))
    if rc != 0:
        _raise(rc)
    return G


def debug_head_backward_gemms(ctx, theta, paths, acts, D4, DO, ws, context_grad_out=None):
    """Test hook: grad_context and the ten weight / bias gradients from GIVEN pre-activation gradients ``D4`` [B, T, L, 4, H] and
    emission gradients ``DO`` [B, T, NO], through the weight packing, the grad_context dispatch and the grouped weight-gradient
    launch of ``head_backward`` alone.  -> (context, W_ih_l0, W_hh_l0, b_ih_l0, b_hh_l0, W_ih_stack, W_hh_stack, b_ih_stack,
    b_hh_stack, out_weight, out_bias), the ones allocated here pre-filled with NaN.  ``context_grad_out`` as in ``head_backward``."""
    lib = load()
    dev = _require_hip(ctx, theta, paths, acts, D4, DO, *ws)
    if ctx.dtype not in (torch.float32, torch.bfloat16) or ctx.stride(2) != 1:
        raise ValueError("ctx must be an f32 / bf16 [B, T, C] view with a contiguous last dimension")
    ctx, cview = context_view(ctx)
    keep, wstruct = _weights_struct(ws)
    theta, paths, acts, D4, DO = (_f32c(t) for t in (theta, paths, acts, D4, DO))
    B, T1, S = paths.shape
    d = _dims(paths[:, 0], ctx, theta, keep)
    T, C, P, H, L = d.T, d.C, d.P, d.H, d.L
    NO = S + S * (S + 1) // 2
    if T1 != T + 1 or tuple(acts.shape) != (B, T, L, 5, H) or tuple(D4.shape) != (B, T, L, 4, H) or tuple(DO.shape) != (B, T, NO):
        raise ValueError("paths / acts / D4 / DO do not have the shapes [B, T+1, S] / [B, T, L, 5, H] / [B, T, L, 4, H] / [B, T, NO]")
    with torch.cuda.device(dev):
        mk = lambda *shape: torch.full(shape, float("nan"), device=dev, dtype=torch.float32)
        g = [None, mk(B, T, C), None, mk(3 * H, S + C + P), mk(3 * H, H), mk(3 * H), mk(3 * H),
             mk(L - 1, 3 * H, H), mk(L - 1, 3 * H, H), mk(L - 1, 3 * H), mk(L - 1, 3 * H), mk(NO, H), mk(NO)]
        cdt, cbs = 0, 0
        if context_grad_out is not None:
            o = context_grad_out
            if (not o.is_contiguous() or o.ndim != 3 or o.shape[0] != B or o.shape[1] < T or o.shape[2] != C
                    or o.dtype not in (torch.float32, torch.bfloat16) or o.device != dev):
                raise ValueError("context_grad_out must be a contiguous [B, >=T, C] f32/bf16 tensor on the same device")
            g[1] = o
            cdt, cbs = int(o.dtype == torch.bfloat16), o.shape[1] * C
        gstruct = _Grads(*[_ptr(t) for t in g], cdt, cbs)
        nbytes = lib.vsde_head_backward_workspace_bytes(ctypes.byref(d))
        if nbytes == 0:
            _raise(-1)
        wsbuf = torch.empty(nbytes, device=dev, dtype=torch.uint8)
        rc = lib.vsde_debug_head_backward_gemms(
            ctypes.byref(d), ctypes.byref(cview), _ptr(theta), _ptr(paths), _ptr(acts), _ptr(D4), _ptr(DO), ctypes.byref(wstruct),
            ctypes.byref(gstruct), _ptr(wsbuf), ctypes.c_size_t(nbytes), _stream(dev))
    if rc != 0:
        _raise(rc)
    return tuple(t for t in g if t is not None)


def head_mfma_range_exceeded(clear: bool = False) -> bool:
    """True once a GRU head weight has left the f16 range of the multi-path MFMA kernels (|W| > 2.2e4): the launch that found it returned
    non-finite paths and every later launch takes the fp32 kernels.  Host-mapped flag written in stream order, no synchronisation: callers
    that replay captured graphs poll it after a replay.  ``clear=True`` resets it (tests)."""
    return bool(load().vsde_head_mfma_range_exceeded(ctypes.c_int(1 if clear else 0)))


# ---------------------------------------------------------------------------------------------
# fused encoder operators (csrc/vsde_encoder.hip)
def _dt(t: torch.Tensor) -> int:
    if t.dtype == torch.float32:
        return 0
    if t.dtype == torch.bfloat16:
        return 1
    raise ValueError(f"fused encoder ops support float32/bfloat16, got {t.dtype}")


def _call(fn, *args):
    rc = fn(*args)
    if rc != 0:
        _raise(rc)


def _i64(v):
    return ctypes.c_int64(int(v))


def _mod_pitch(C, *vecs):
    """Common row pitch of per-batch-row vectors [B, C] (contiguous, or column ranges of one [B, pitch] buffer)."""
    pitch = None
    for v in vecs:
        if v is None:
            continue
        if v.ndim != 2 or v.shape[1] != C or v.stride(1) != 1 or v.stride(0) < C:
            raise ValueError(f"expected a [B,{C}] row-pitched vector, got shape {tuple(v.shape)} strides {v.stride()}")
        if pitch is None:
            pitch = v.stride(0)
        elif v.stride(0) != pitch:
            raise ValueError("scale / shift / gate and their gradient outputs must share one row pitch")
    return pitch


def _like_vec(v):
    return torch.empty_strided(v.shape, v.stride(), device=v.device, dtype=v.dtype)


def ln_modulate_fwd(x, scale, shift, eps):
    lib = load(); dev = _require_hip(x, scale, shift)
    B, N, C = x.shape
    y = torch.empty_like(x)
    mean = torch.empty(B, N, device=dev, dtype=torch.float32); rstd = torch.empty_like(mean)
    with torch.cuda.device(dev):
        _call(lib.vsde_ln_modulate_fwd, _dt(x), _ptr(x), _ptr(scale), _ptr(shift), _ptr(y), _ptr(mean), _ptr(rstd), _i64(B),
              ctypes.c_int(N), ctypes.c_int(C), ctypes.c_double(eps), _i64(_mod_pitch(C, scale, shift)), _stream(dev))
    return y, mean, rstd


def _colsum_workspace(lib, B, C, dev):
    nbytes = lib.vsde_colsum_workspace_bytes(_i64(B), ctypes.c_int(C))
    return torch.empty(max(int(nbytes), 1), device=dev, dtype=torch.uint8)


def ln_modulate_bwd(x, scale, dy, mean, rstd, dres=None, dscale=None, dshift=None):
    """dres (optional, same shape as x) is added to dx inside the kernel; dscale / dshift: optional destinations with the row
    pitch of ``scale`` (column ranges of a shared gradient buffer)."""
    lib = load(); dev = _require_hip(x, scale, dy)
    B, N, C = x.shape
    dx = torch.empty_like(x)
    dscale = _like_vec(scale) if dscale is None else dscale
    dshift = _like_vec(scale) if dshift is None else dshift
    ws = _colsum_workspace(lib, B, C, dev)
    with torch.cuda.device(dev):
        _call(lib.vsde_ln_modulate_bwd, _dt(x), _ptr(x), _ptr(scale), _ptr(dy), _ptr(mean), _ptr(rstd), _ptr(dres), _ptr(dx),
              _ptr(dscale), _ptr(dshift), _i64(B), ctypes.c_int(N), ctypes.c_int(C), _i64(_mod_pitch(C, scale, dscale, dshift)),
              _ptr(ws), ctypes.c_size_t(ws.numel()), _stream(dev))
    return dx, dscale, dshift


def residual_ln_fwd(x, y, gate, scale, shift, eps):
    """(xnew, h, mean, rstd) with xnew = x + gate*y and h = LN(xnew)*(1+scale)+shift."""
    lib = load(); dev = _require_hip(x, y, gate, scale, shift)
    B, N, C = x.shape
    xnew = torch.empty_like(x); h = torch.empty_like(x)
    mean = torch.empty(B * N, device=dev, dtype=torch.float32); rstd = torch.empty_like(mean)
    with torch.cuda.device(dev):
        _call(lib.vsde_residual_ln_fwd, _dt(x), _ptr(x), _ptr(y), _ptr(gate), _ptr(scale), _ptr(shift), _ptr(xnew), _ptr(h),
              _ptr(mean), _ptr(rstd), _i64(B), ctypes.c_int(N), ctypes.c_int(C), ctypes.c_double(eps),
              _i64(_mod_pitch(C, gate, scale, shift)), _stream(dev))
    return xnew, h, mean, rstd


def residual_ln_bwd(xnew, y, gate, scale, dh, dxnew, mean, rstd, dgate=None, dscale=None, dshift=None):
    """(dx, dy, dgate, dscale, dshift); dxnew may be None; optional preallocated d-vector destinations (pitch of ``gate``)."""
    lib = load(); dev = _require_hip(xnew, y, gate, scale, dh)
    B, N, C = xnew.shape
    dx = torch.empty_like(xnew); dy = torch.empty_like(xnew)
    dgate = _like_vec(gate) if dgate is None else dgate
    dscale = _like_vec(scale) if dscale is None else dscale
    dshift = _like_vec(scale) if dshift is None else dshift
    ws = _colsum_workspace(lib, B, C, dev)
    with torch.cuda.device(dev):
        _call(lib.vsde_residual_ln_bwd, _dt(xnew), _ptr(xnew), _ptr(y), _ptr(gate), _ptr(scale), _ptr(dh), _ptr(dxnew),
              _ptr(mean), _ptr(rstd), _ptr(dx), _ptr(dy), _ptr(dgate), _ptr(dscale), _ptr(dshift), _i64(B), ctypes.c_int(N),
              ctypes.c_int(C), _i64(_mod_pitch(C, gate, scale, dgate, dscale, dshift)), _ptr(ws), ctypes.c_size_t(ws.numel()),
              _stream(dev))
    return dx, dy, dgate, dscale, dshift


def gated_residual_fwd(x, y, gate):
    lib = load(); dev = _require_hip(x, y, gate)
    B, N, C = x.shape
    out = torch.empty_like(x)
    with torch.cuda.device(dev):
        _call(lib.vsde_gated_residual_fwd, _dt(x), _ptr(x), _ptr(y), _ptr(gate), _ptr(out), _i64(B), ctypes.c_int(N),
              ctypes.c_int(C), _i64(_mod_pitch(C, gate)), _stream(dev))
    return out


def gated_residual_bwd(y, gate, dout, dgate=None):
    lib = load(); dev = _require_hip(y, gate, dout)
    B, N, C = y.shape
    dy = torch.empty_like(y)
    dgate = _like_vec(gate) if dgate is None else dgate
    ws = _colsum_workspace(lib, B, C, dev)
    with torch.cuda.device(dev):
        _call(lib.vsde_gated_residual_bwd, _dt(y), _ptr(y), _ptr(gate), _ptr(dout), _ptr(dy), _ptr(dgate), _i64(B),
              ctypes.c_int(N), ctypes.c_int(C), _i64(_mod_pitch(C, gate, dgate)), _ptr(ws), ctypes.c_size_t(ws.numel()),
              _stream(dev))
    return dy, dgate


def swiglu_fwd(u):
    lib = load(); dev = _require_hip(u)
    H2 = u.shape[-1] // 2
    out = torch.empty(*u.shape[:-1], H2, device=dev, dtype=u.dtype)
    with torch.cuda.device(dev):
        _call(lib.vsde_swiglu_fwd, _dt(u), _ptr(u), _ptr(out), _i64(u.numel() // (2 * H2)), ctypes.c_int(H2), _stream(dev))
    return out


def swiglu_bwd(u, dout):
    lib = load(); dev = _require_hip(u, dout)
    H2 = u.shape[-1] // 2
    du = torch.empty_like(u)
    with torch.cuda.device(dev):
        _call(lib.vsde_swiglu_bwd, _dt(u), _ptr(u), _ptr(dout), _ptr(du), _i64(u.numel() // (2 * H2)), ctypes.c_int(H2), _stream(dev))
    return du


def _head_dims(t, token_major):
    """(B, heads, N, d) of a per-head tensor stored [B,heads,N,d] (token_major False) or [B,N,heads,d] (True)."""
    if token_major:
        B, N, h, d = t.shape
    else:
        B, h, N, d = t.shape
    return B, h, N, d


def _row_pitch(t, width):
    """Row pitch (elements) of a [B,N,width] tensor that is either contiguous or a column range of a contiguous
    [B,N,W] buffer (the merged [qkv | gate] projection)."""
    B, N, w = t.shape
    pitch = t.stride(1)
    if w != width or t.stride(2) != 1 or pitch < width or t.stride(0) != N * pitch:
        raise ValueError(f"expected a [B,N,{width}] row-pitched tensor, got shape {tuple(t.shape)} strides {t.stride()}")
    return pitch


def gate_merge_fwd(attn, glog, token_major=False):
    lib = load(); dev = _require_hip(attn, glog)
    B, h, N, d = _head_dims(attn, token_major)
    out = torch.empty(B, N, h * d, device=dev, dtype=attn.dtype)
    with torch.cuda.device(dev):
        _call(lib.vsde_gate_merge_fwd, _dt(attn), _ptr(attn), _ptr(glog), _ptr(out), _i64(B), ctypes.c_int(N), ctypes.c_int(h),
              ctypes.c_int(d), ctypes.c_int(int(token_major)), _i64(_row_pitch(glog, d)), _stream(dev))
    return out


def gate_merge_bwd(attn, glog, dout, token_major=False, dglog=None):
    """dglog: optional preallocated destination with the same row pitch as glog (a column range of a shared buffer)."""
    lib = load(); dev = _require_hip(attn, glog, dout)
    B, h, N, d = _head_dims(attn, token_major)
    dattn = torch.empty_like(attn)
    if dglog is None:
        dglog = torch.empty_like(glog) if glog.is_contiguous() else torch.empty_strided(glog.shape, glog.stride(), device=dev, dtype=glog.dtype)
    pitch = _row_pitch(glog, d)
    if _row_pitch(dglog, d) != pitch:
        raise ValueError("dglog must have the row pitch of glog")
    with torch.cuda.device(dev):
        _call(lib.vsde_gate_merge_bwd, _dt(attn), _ptr(attn), _ptr(glog), _ptr(dout), _ptr(dattn), _ptr(dglog), _i64(B),
              ctypes.c_int(N), ctypes.c_int(h), ctypes.c_int(d), ctypes.c_int(int(token_major)), _i64(pitch), _stream(dev))
    return dattn, dglog


def qk_norm_rope_fwd(qkv, cos, sin, wq, wk, v0, lam, heads, eps, token_major=False):
    lib = load(); dev = _require_hip(qkv, cos, sin, wq, wk)
    B, N, C3 = qkv.shape
    d = C3 // 3 // heads
    pitch = _row_pitch(qkv, C3)
    shape = (B, N, heads, d) if token_major else (B, heads, N, d)
    q = torch.empty(shape, device=dev, dtype=qkv.dtype); k = torch.empty_like(q); v = torch.empty_like(q)
    with torch.cuda.device(dev):
        _call(lib.vsde_qk_norm_rope_fwd, _dt(qkv), _ptr(qkv), _ptr(cos), _ptr(sin), _ptr(wq), _ptr(wk), _ptr(v0), _ptr(lam),
              _ptr(q), _ptr(k), _ptr(v), _i64(B), ctypes.c_int(N), ctypes.c_int(heads), ctypes.c_int(d), ctypes.c_double(eps),
              ctypes.c_int(int(token_major)), _i64(pitch), _stream(dev))
    return q, k, v


def qk_norm_rope_bwd(qkv, cos, sin, wq, wk, v0, lam, dq, dk, dv, heads, eps, token_major=False, dqkv=None, dv0=None,
                     dv_extra=None):
    """dqkv: optional preallocated destination with the same row pitch as qkv (a column range of a shared buffer);
    dv0: optional existing buffer to ACCUMULATE the value-residual gradient into; dv_extra: added to dv first."""
    lib = load(); dev = _require_hip(qkv, dq, dk, dv)
    B, N, C3 = qkv.shape
    d = C3 // 3 // heads
    pitch = _row_pitch(qkv, C3)
    if dqkv is None:
        dqkv = torch.empty_like(qkv) if qkv.is_contiguous() else torch.empty_strided(qkv.shape, qkv.stride(), device=dev, dtype=qkv.dtype)
    if _row_pitch(dqkv, C3) != pitch:
        raise ValueError("dqkv must have the row pitch of qkv")
    accumulate = dv0 is not None
    if v0 is not None and dv0 is None:
        dv0 = torch.empty_like(dv)
    nparts = lib.vsde_qk_norm_rope_bwd_partials(_i64(B), ctypes.c_int(N), ctypes.c_int(heads), ctypes.c_int(d))
    parts = torch.empty(nparts, device=dev, dtype=torch.float32) if v0 is not None else None
    with torch.cuda.device(dev):
        _call(lib.vsde_qk_norm_rope_bwd, _dt(qkv), _ptr(qkv), _ptr(cos), _ptr(sin), _ptr(wq), _ptr(wk), _ptr(v0), _ptr(lam),
              _ptr(dq), _ptr(dk), _ptr(dv), _ptr(dqkv), _ptr(dv0), _ptr(parts), _i64(B), ctypes.c_int(N), ctypes.c_int(heads),
              ctypes.c_int(d), ctypes.c_double(eps), ctypes.c_int(int(token_major)), _i64(pitch), ctypes.c_int(int(accumulate)),
              _ptr(dv_extra), _stream(dev))
    dlam = parts.sum() if parts is not None else None
    return dqkv, dv0, dlam


def attention_max_tokens() -> int:
    return int(load().vsde_attention_max_tokens())


def attention_fwd(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, scale: float):
    """softmax(scale q k^T) v for token-major bf16 heads [B,N,H,d], d in (64, 128); returns (o, lse [B,H,N] fp32)."""
    lib = load(); dev = _require_hip(q, k, v)
    B, N, H, d = q.shape
    if q.dtype != torch.bfloat16 or not (q.is_contiguous() and k.is_contiguous() and v.is_contiguous()):
        raise ValueError("attention_fwd needs contiguous bf16 [B,N,H,d] tensors")
    o = torch.empty_like(q)
    lse = torch.empty(B, H, N, device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        _call(lib.vsde_attention_fwd_bf16, _ptr(q), _ptr(k), _ptr(v), _ptr(o), _ptr(lse), _i64(B), ctypes.c_int(N),
              ctypes.c_int(H), ctypes.c_int(d), ctypes.c_double(scale), _stream(dev))
    return o, lse


def attention_bwd(dout, q, k, v, o, lse, scale: float):
    """(dq, dk, dv) token-major bf16 for ``attention_fwd``'s inputs/outputs."""
    lib = load(); dev = _require_hip(dout, q, k, v, o, lse)
    B, N, H, d = q.shape
    for t in (dout, q, k, v, o):
        if t.dtype != torch.bfloat16 or not t.is_contiguous() or t.shape != q.shape:
            raise ValueError("attention_bwd needs contiguous bf16 [B,N,H,d] tensors of one shape")
    dq, dk, dv = torch.empty_like(q), torch.empty_like(q), torch.empty_like(q)
    delta = torch.empty(B, H, N, device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        _call(lib.vsde_attention_bwd_bf16, _ptr(dout), _ptr(q), _ptr(k), _ptr(v), _ptr(o), _ptr(lse), _ptr(dq), _ptr(dk),
              _ptr(dv), _ptr(delta), _i64(B), ctypes.c_int(N), ctypes.c_int(H), ctypes.c_int(d), ctypes.c_double(scale),
              _stream(dev))
    return dq, dk, dv


def linear_wgrad(dy: torch.Tensor, x: torch.Tensor, want_bias: bool, row_map: Optional[torch.Tensor] = None,
                 out_rows: Optional[int] = None, out: Optional[torch.Tensor] = None, out_bias: Optional[torch.Tensor] = None):
    """dW[N,K] = dy^T x and db[N] = colsum(dy) in fp32 for bf16 dy [M,N], x [M,K].  ``row_map`` (int32 [N] on the device):
    product row n is stored at output row ``row_map[n]`` (negative: dropped) of an ``[out_rows, K]`` result.
    ``out`` / ``out_bias``: contiguous fp32 buffers [rows, K] / [rows] to write into instead of fresh ones."""
    lib = load(); dev = _require_hip(dy, x)
    M, N = dy.shape
    K = x.shape[1]
    rows = N if row_map is None else int(out_rows)
    dW = torch.empty(rows, K, device=dev, dtype=torch.float32) if out is None else _given(out, (rows, K), torch.float32)
    db = None
    if want_bias:
        db = torch.empty(rows, device=dev, dtype=torch.float32) if out_bias is None else _given(out_bias, (rows,), torch.float32)
    nbytes = lib.vsde_linear_wgrad_workspace_bytes(_i64(M), ctypes.c_int(N), ctypes.c_int(K))
    ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    with torch.cuda.device(dev):
        _call(lib.vsde_linear_wgrad_bf16_rows, _ptr(dy), _ptr(x), _i64(M), ctypes.c_int(N), ctypes.c_int(K), _ptr(dW), _ptr(db),
              _ptr(row_map), _ptr(ws), ctypes.c_size_t(nbytes), _stream(dev))
    return dW, db


class _WgradItem(ctypes.Structure):
    _fields_ = [("dy", ctypes.c_void_p), ("x", ctypes.c_void_p), ("M", ctypes.c_int64), ("N", ctypes.c_int32), ("K", ctypes.c_int32),
                ("dW", ctypes.c_void_p), ("db", ctypes.c_void_p), ("row_map", ctypes.c_void_p)]


def linear_wgrad_group(problems, group_plan: bool = False, outs=None):
    """``[(dy, x, want_bias, row_map, out_rows), ...]`` -> ``[(dW, db), ...]``: every problem as ``linear_wgrad`` computes it, all of
    them in a handful of launches (csrc/vsde_wgrad.hip, ``vsde_linear_wgrad_group_bf16``).  ``group_plan=False``: bit-identical to
    one call per problem; ``True``: split counts chosen for the group as a whole (other summation order, less partial traffic).
    ``outs``: ``[(dW, db or None), ...]`` contiguous fp32 buffers to write into instead of fresh ones."""
    lib = load()
    dev = _require_hip(*[t for pr in problems for t in pr[:2]])
    n = len(problems)
    items = (_WgradItem * n)()
    given, outs = outs, []
    for i, (dy, x, want_bias, row_map, out_rows) in enumerate(problems):
        M, N = dy.shape
        K = x.shape[1]
        rows = N if row_map is None else int(out_rows)
        if given is None:
            dW = torch.empty(rows, K, device=dev, dtype=torch.float32)
            db = torch.empty(rows, device=dev, dtype=torch.float32) if want_bias else None
        else:
            dW = _given(given[i][0], (rows, K), torch.float32)
            db = _given(given[i][1], (rows,), torch.float32) if want_bias else None
        items[i] = _WgradItem(dy.data_ptr(), x.data_ptr(), M, N, K, dW.data_ptr(), None if db is None else db.data_ptr(),
                              None if row_map is None else row_map.data_ptr())
        outs.append((dW, db))
    nbytes = lib.vsde_linear_wgrad_group_workspace_bytes(ctypes.c_int(n), ctypes.byref(items))
    ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    with torch.cuda.device(dev):
        _call(lib.vsde_linear_wgrad_group_bf16, ctypes.c_int(n), ctypes.byref(items), ctypes.c_int(1 if group_plan else 0), _ptr(ws),
              ctypes.c_size_t(nbytes), _stream(dev))
    return outs


EPI_PLAIN, EPI_SWIGLU, EPI_SWIGLU_BWD = 0, 1, 2


def linear_variant(M: int, N: int, K: int, epilogue: int = EPI_PLAIN) -> int:
    """0 = shape not covered, 1 = rows kernel (K in {128, 256, 512}), 2 = cols kernel, 3 = persistent deep-reduction kernel
    (K >= 512, N % 256 == 0, N <= K, M >= 32768)."""
    return int(load().vsde_linear_bf16_supported(_i64(M), ctypes.c_int(N), ctypes.c_int(K), ctypes.c_int(epilogue)))


def linear_supported(M: int, N: int, K: int, epilogue: int = EPI_PLAIN) -> bool:
    return linear_variant(M, N, K, epilogue) != 0


def _given(t: torch.Tensor, shape, dtype, pitched: bool = False):
    """A caller's output buffer: the expected shape and type, contiguous (``pitched``: rows contiguous, any row pitch)."""
    ok = t.dtype == dtype and tuple(t.shape) == tuple(shape) and (t.is_contiguous() or (pitched and t.ndim == 2 and t.stride(1) == 1))
    if not ok:
        raise ValueError(f"output buffer: expected {dtype} {tuple(shape)}, got {t.dtype} {tuple(t.shape)} strides {t.stride()}")
    return t


def _rows2d(t: torch.Tensor):
    """(tensor, row pitch) of a bf16 matrix whose rows are contiguous (a column range of a wider buffer is fine)."""
    if t.dtype != torch.bfloat16 or t.ndim != 2 or t.stride(1) != 1:
        raise ValueError(f"expected a row-pitched bf16 matrix, got {t.dtype} {tuple(t.shape)} strides {t.stride()}")
    return t, t.stride(0)


def linear_bf16(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], out: Optional[torch.Tensor] = None):
    """y = x w^T + bias on the MFMA kernels: x [M,K] (row-pitched), w [N,K] contiguous, bias [N] or None -> y [M,N] bf16."""
    lib = load(); dev = _require_hip(x, w)
    x, ldx = _rows2d(x)
    M, K = x.shape
    N = w.shape[0]
    y = torch.empty(M, N, device=dev, dtype=torch.bfloat16) if out is None else out
    with torch.cuda.device(dev):
        _call(lib.vsde_linear_bf16, _ptr(x), _i64(ldx), _ptr(w), _ptr(bias), _ptr(y), _i64(y.stride(0)), _i64(M), ctypes.c_int(N),
              ctypes.c_int(K), ctypes.c_int(EPI_PLAIN), None, _i64(0), None, _i64(0), _stream(dev))
    return y


def linear_swiglu_bf16(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], want_u: bool = True,
                       out_u: Optional[torch.Tensor] = None, out_s: Optional[torch.Tensor] = None):
    """(u [M,N] or None, s [M,N/2]) for the interleaved-packed SwiGLU input projection w [N,K].  ``out_u`` / ``out_s``: row-pitched
    bf16 buffers to write into instead of fresh ones."""
    lib = load(); dev = _require_hip(x, w)
    x, ldx = _rows2d(x)
    M, K = x.shape
    N = w.shape[0]
    u = None
    if want_u:
        u = torch.empty(M, N, device=dev, dtype=torch.bfloat16) if out_u is None else _given(out_u, (M, N), torch.bfloat16, True)
    s = torch.empty(M, N // 2, device=dev, dtype=torch.bfloat16) if out_s is None else _given(out_s, (M, N // 2), torch.bfloat16, True)
    with torch.cuda.device(dev):
        _call(lib.vsde_linear_bf16, _ptr(x), _i64(ldx), _ptr(w), _ptr(bias), _ptr(u), _i64(N if u is None else u.stride(0)), _i64(M),
              ctypes.c_int(N), ctypes.c_int(K), ctypes.c_int(EPI_SWIGLU), _ptr(s), _i64(s.stride(0)), None, _i64(0), _stream(dev))
    return u, s


def linear_qknorm_bf16(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], heads: int, tokens: int, cos, sin, wq, wk,
                       v0: Optional[torch.Tensor], lam: Optional[torch.Tensor], eps: float, save: bool = False):
    """Attention projection: x [M,256] against the packed [q | k | v | gate] weight w [3*heads*64 + G, 256] with the
    QK-RMS-norm + RoPE + value mix in the GEMM epilogue -> (q, k, v [M, heads*64] token-major, gate logits [M, G] or None).
    ``save`` (training): the gate block is returned as sigmoid(logits) and (rinv [M, 2*heads] fp32, vdiff [M, heads*64] bf16 or
    None) are returned for the fused backward."""
    lib = load(); dev = _require_hip(x, w, cos, sin, wq, wk)
    x, ldx = _rows2d(x)
    M, K = x.shape
    C = heads * 64
    G = w.shape[0] - 3 * C
    q = torch.empty(M, C, device=dev, dtype=torch.bfloat16); k = torch.empty_like(q); v = torch.empty_like(q)
    gate = torch.empty(M, G, device=dev, dtype=torch.bfloat16) if G > 0 else None
    rinv = torch.empty(M, 2 * heads, device=dev, dtype=torch.float32) if save else None
    vdiff = torch.empty(M, C, device=dev, dtype=torch.bfloat16) if (save and v0 is not None) else None
    with torch.cuda.device(dev):
        _call(lib.vsde_linear_qknorm_bf16, _ptr(x), _i64(ldx), _ptr(w), _ptr(bias), _i64(M), ctypes.c_int(K), ctypes.c_int(heads),
              ctypes.c_int(G), ctypes.c_int(tokens), _ptr(cos), _ptr(sin), _ptr(wq), _ptr(wk), _ptr(v0), _ptr(lam),
              ctypes.c_double(eps), _ptr(q), _ptr(k), _ptr(v), _ptr(gate), _i64(G), ctypes.c_int(int(save)), _ptr(rinv), _ptr(vdiff),
              _stream(dev))
    if save:
        return q, k, v, gate, rinv, vdiff
    return q, k, v, gate


def attention_fused_supported(N: int, head_dim: int) -> bool:
    return bool(load().vsde_attention_fused_supported(ctypes.c_int(N), ctypes.c_int(head_dim)))


def attention_fwd_gated(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, gate: torch.Tensor, scale: float):
    """softmax(scale q k^T) v * gate for token-major bf16 heads [B,N,H,64] and the gate factors s = sigmoid(logits) [B*N, >=64]
    (row-pitched; ``linear_qknorm_bf16(save=True)`` produces them): returns (the merged rows og [B,N,H,64], lse [B,H,N] fp32)."""
    lib = load(); dev = _require_hip(q, k, v, gate)
    B, N, H, d = q.shape
    if q.dtype != torch.bfloat16 or d != 64 or not (q.is_contiguous() and k.is_contiguous() and v.is_contiguous()):
        raise ValueError("attention_fwd_gated needs contiguous bf16 [B,N,H,64] tensors")
    gate, ldg = _rows2d(gate)
    o = torch.empty_like(q)
    lse = torch.empty(B, H, N, device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        _call(lib.vsde_attention_fwd_gated_bf16, _ptr(q), _ptr(k), _ptr(v), _ptr(gate), _i64(ldg), _ptr(o), _ptr(lse), _i64(B),
              ctypes.c_int(N), ctypes.c_int(H), ctypes.c_double(scale), _stream(dev))
    return o, lse


def gate_bwd_delta(dout: torch.Tensor, og: torch.Tensor, gate: torch.Tensor, dgate: torch.Tensor):
    """Backward of the gate folded into ``attention_fwd_gated``: dout, og [B,N,H,64] bf16, gate factors s [B*N, >=64]; ``dgate``
    (row-pitched [B*N, 64], e.g. the gate columns of the projection's gradient buffer) receives the gradient of the LOGITS.
    Returns (dattn [B,N,H,64] = the gradient of the ungated attention output, delta [B,H,N] fp32 = <dattn, o>)."""
    lib = load(); dev = _require_hip(dout, og, gate, dgate)
    B, N, H, d = og.shape
    if d != 64 or not (dout.is_contiguous() and og.is_contiguous()) or dout.dtype != torch.bfloat16:
        raise ValueError("gate_bwd_delta needs contiguous bf16 [B,N,H,64] tensors")
    gate, ldg = _rows2d(gate); dgate, ldd = _rows2d(dgate)
    dattn = torch.empty_like(og)
    delta = torch.empty(B, H, N, device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        _call(lib.vsde_gate_bwd_delta, _ptr(dout), _ptr(og), _ptr(gate), _i64(ldg), _ptr(dattn), _ptr(dgate), _i64(ldd), _ptr(delta),
              _i64(B), ctypes.c_int(N), ctypes.c_int(H), _stream(dev))
    return dattn, delta


def mlp_image_bytes(C: int) -> tuple[int, int, int]:
    """Bytes per 16-unit tile of the fused SwiGLU MLP's weight images (W1, W2, b1) for width C."""
    a, b, c = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
    rc = load().vsde_mlp_image_bytes(ctypes.c_int(C), ctypes.byref(a), ctypes.byref(b), ctypes.byref(c))
    if rc != 0:
        _raise(rc)
    return int(a.value), int(b.value), int(c.value)


def mlp_fwd(x: torch.Tensor, w1_img: torch.Tensor, w2_img: torch.Tensor, b1_img: torch.Tensor, b2: Optional[torch.Tensor], H: int,
            want_s: bool = False, out_y: Optional[torch.Tensor] = None, out_s: Optional[torch.Tensor] = None):
    """Fused SwiGLU MLP forward (csrc/vsde_mlp.hip): x [M,C] bf16 (row-pitched) -> (y [M,C] bf16, s [M,H] bf16 or None).
    ``out_y`` / ``out_s``: row-pitched bf16 buffers to write into instead of fresh ones."""
    lib = load(); dev = _require_hip(x, w1_img, w2_img, b1_img)
    x, ldx = _rows2d(x)
    M, C = x.shape
    y = torch.empty(M, C, device=dev, dtype=torch.bfloat16) if out_y is None else _given(out_y, (M, C), torch.bfloat16, True)
    s = None
    if want_s:
        s = torch.empty(M, H, device=dev, dtype=torch.bfloat16) if out_s is None else _given(out_s, (M, H), torch.bfloat16, True)
    with torch.cuda.device(dev):
        _call(lib.vsde_mlp_fwd_bf16, _ptr(x), _i64(ldx), _ptr(w1_img), _ptr(w2_img), _ptr(b1_img), _ptr(b2), _ptr(y), _i64(y.stride(0)), _ptr(s),
              _i64(H if s is None else s.stride(0)), _i64(M), ctypes.c_int(C), ctypes.c_int(H), _stream(dev))
    return y, s


def mlp_block_fwd(x, yin, ga, sc, sh, gm, sn, hs, eps: float, eps_next: float, w1_img, w2_img, b1_img, b2, H: int):
    """Block form of the fused SwiGLU MLP (no-grad): x, yin [B,N,C] bf16 contiguous, modulation vectors [B,C] views of one
    [B,pitch] buffer -> (tok [B,N,C], hnext [B,N,C] or None when sn / hs are None).  See include/vsde_hip.h."""
    lib = load(); dev = _require_hip(x, yin, ga, sc, sh, gm, w1_img, w2_img, b1_img)
    B, N, C = x.shape
    if not (x.is_contiguous() and yin.is_contiguous() and x.dtype == torch.bfloat16 and yin.dtype == torch.bfloat16 and yin.shape == x.shape):
        raise ValueError("mlp_block_fwd: x and yin must be contiguous bf16 tensors of one shape")
    mp = _mod_pitch(C, ga, sc, sh, gm, sn, hs)
    tok = torch.empty_like(x)
    hnext = torch.empty_like(x) if sn is not None else None
    with torch.cuda.device(dev):
        _call(lib.vsde_mlp_block_fwd_bf16, _ptr(x), _ptr(yin), _ptr(ga), _ptr(sc), _ptr(sh), _ptr(gm), _ptr(sn), _ptr(hs), _i64(mp),
              ctypes.c_int(N), ctypes.c_double(eps), ctypes.c_double(eps_next), _ptr(w1_img), _ptr(w2_img), _ptr(b1_img), _ptr(b2),
              _ptr(tok), _ptr(hnext), _i64(B * N), ctypes.c_int(C), ctypes.c_int(H), _stream(dev))
    return tok, hnext


def mlp_attn_block_fwd(x, attn, glog, wo_img, bo, ga, sc, sh, gm, sn, hs, eps: float, eps_next: float, w1_img, w2_img, b1_img, b2, H: int):
    """``mlp_block_fwd`` with the attention out projection in front: attn [B,N,C] bf16 contiguous (merged heads), glog [B*N,64]
    gate logits (row pitch free), wo_img the out projection's weight in the w2 image format.  See include/vsde_hip.h."""
    lib = load(); dev = _require_hip(x, attn, glog, wo_img, ga, sc, sh, gm, w1_img, w2_img, b1_img)
    B, N, C = x.shape
    if not (x.is_contiguous() and attn.is_contiguous() and x.dtype == torch.bfloat16 and attn.dtype == torch.bfloat16 and attn.numel() == x.numel()):
        raise ValueError("mlp_attn_block_fwd: x and attn must be contiguous bf16 tensors of one size")
    if not (glog.ndim == 2 and glog.shape == (B * N, 64) and glog.dtype == torch.bfloat16 and glog.stride(1) == 1):
        raise ValueError("mlp_attn_block_fwd: glog must be [B*N, 64] bf16 with unit column stride")
    mp = _mod_pitch(C, ga, sc, sh, gm, sn, hs)
    tok = torch.empty_like(x)
    hnext = torch.empty_like(x) if sn is not None else None
    with torch.cuda.device(dev):
        _call(lib.vsde_mlp_attn_block_fwd_bf16, _ptr(x), _ptr(attn), _ptr(glog), _i64(glog.stride(0)), _ptr(wo_img), _ptr(bo), _ptr(ga), _ptr(sc),
              _ptr(sh), _ptr(gm), _ptr(sn), _ptr(hs), _i64(mp), ctypes.c_int(N), ctypes.c_double(eps), ctypes.c_double(eps_next), _ptr(w1_img),
              _ptr(w2_img), _ptr(b1_img), _ptr(b2), _ptr(tok), _ptr(hnext), _i64(B * N), ctypes.c_int(C), ctypes.c_int(H), _stream(dev))
    return tok, hnext


def linear_deep256(x: torch.Tensor, w_img: torch.Tensor, bias: Optional[torch.Tensor]) -> torch.Tensor:
    """y [M,256] = x [M,K] W^T (+ bias) for K % 64 == 0, K >= 256: ``w_img`` = W as K/16 k-step images [K/16, 2, 256, 8] bf16
    (``fused.DeepImage``).  See include/vsde_hip.h."""
    lib = load(); dev = _require_hip(x, w_img)
    x, ldx = _rows2d(x)
    M, K = x.shape
    if w_img.dtype != torch.bfloat16 or w_img.numel() != 256 * K or not w_img.is_contiguous():
        raise ValueError("linear_deep256: w_img must be a contiguous bf16 image of 256 x K elements")
    y = torch.empty(M, 256, device=dev, dtype=torch.bfloat16)
    with torch.cuda.device(dev):
        _call(lib.vsde_linear_deep256_bf16, _ptr(x), _i64(ldx), _ptr(w_img), _ptr(bias), _ptr(y), _i64(256), _i64(M), ctypes.c_int(K), _stream(dev))
    return y


def mlp_bwd_image_bytes(C: int) -> int:
    """Bytes per pair tile (32 hidden units) of the fused MLP backward's weight image; 0 = width not built."""
    return int(load().vsde_mlp_bwd_image_bytes(ctypes.c_int(C)))


def mlp_bwd(dy: torch.Tensor, u: torch.Tensor, img: torch.Tensor, H: int):
    """Fused SwiGLU MLP backward (csrc/vsde_mlp.hip): dy [M,C], saved u [M,2H] (interleaved layout) -> (du [M,2H], dx [M,C])."""
    lib = load(); dev = _require_hip(dy, u, img)
    dy, lddy = _rows2d(dy); u, ldu = _rows2d(u)
    M, C = dy.shape
    du = torch.empty(M, 2 * H, device=dev, dtype=torch.bfloat16)
    dx = torch.empty(M, C, device=dev, dtype=torch.bfloat16)
    with torch.cuda.device(dev):
        _call(lib.vsde_mlp_bwd_bf16, _ptr(dy), _i64(lddy), _ptr(u), _i64(ldu), _ptr(img), _ptr(du), _i64(2 * H), _ptr(dx), _i64(C), _i64(M),
              ctypes.c_int(C), ctypes.c_int(H), _stream(dev))
    return du, dx


def linear_gate_bwd(dy: torch.Tensor, w_t: torch.Tensor, og: torch.Tensor, s: torch.Tensor, dgate: torch.Tensor, tokens: int):
    """Input gradient of the attention output projection fused with the gate backward: dy [M,K] (gradient of the projection
    output), w_t [H*64, K] (its weight transposed), og [B,N,H,64] the merged gated rows, s / dgate row-pitched [M, >=64] (gate
    factors in, gate-logit gradient out).  Returns (dattn [B,N,H,64], delta [B,H,N] fp32) like ``gate_bwd_delta``."""
    lib = load(); dev = _require_hip(dy, w_t, og, s, dgate)
    dy, ldy = _rows2d(dy); s, lds = _rows2d(s); dgate, ldd = _rows2d(dgate)
    B, N, H, d = og.shape
    M, K = dy.shape
    if d != 64 or N != tokens or M != B * N or tuple(w_t.shape) != (H * 64, K) or not (og.is_contiguous() and w_t.is_contiguous()):
        raise ValueError("linear_gate_bwd: inconsistent shapes")
    dattn = torch.empty_like(og)
    delta = torch.empty(B, H, N, device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        _call(lib.vsde_linear_gate_bwd_bf16, _ptr(dy), _i64(ldy), _ptr(w_t), _ptr(og), _ptr(s), _i64(lds), _ptr(dattn), _ptr(dgate),
              _i64(ldd), _ptr(delta), _i64(M), ctypes.c_int(K), ctypes.c_int(H), ctypes.c_int(N), _stream(dev))
    return dattn, delta


def attention_bwd_fused(dattn, q, k, v, lse, delta, rinv, cos, sin, wq, wk, vdiff, lam, dv0, dv_extra, dy, scale: float):
    """Attention backward whose epilogues apply the RoPE / RMS-norm / value-mix backward and write the q, k, v columns of ``dy``
    ([B*N, >= 192 H] bf16, the gradient of the [q | k | v | gate] projection).  ``dv0``: existing buffer to accumulate the
    residual-value gradient into (a new one is made when ``vdiff`` is given and ``dv0`` is None).  Returns (dv0, dlam)."""
    lib = load(); dev = _require_hip(dattn, q, k, v, lse, delta, rinv, dy)
    B, N, H, d = q.shape
    dy2, ldy = _rows2d(dy)
    accumulate = dv0 is not None
    parts = None
    if vdiff is not None:
        if dv0 is None:
            dv0 = torch.empty_like(v)
        parts = torch.empty(int(lib.vsde_attention_bwd_fused_partials(_i64(B), ctypes.c_int(N), ctypes.c_int(H))), device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        _call(lib.vsde_attention_bwd_fused_bf16, _ptr(dattn), _ptr(q), _ptr(k), _ptr(v), _ptr(lse), _ptr(delta), _ptr(rinv), _ptr(cos),
              _ptr(sin), _ptr(wq), _ptr(wk), _ptr(vdiff), _ptr(lam if vdiff is not None else None),
              _ptr(dv0 if vdiff is not None else None), ctypes.c_int(int(accumulate)), _ptr(dv_extra), _ptr(dy2), _i64(ldy), _ptr(parts),
              _i64(B), ctypes.c_int(N), ctypes.c_int(H), ctypes.c_double(scale), _stream(dev))
    return (dv0 if vdiff is not None else None), (parts.sum() if parts is not None else None)


def linear_gated_bf16(attn: torch.Tensor, gate: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor]):
    """y [M,N] = (attn [M,K] * sigmoid(gate [M,64] broadcast over the heads)) w^T + bias: gate_merge folded into the GEMM."""
    lib = load(); dev = _require_hip(attn, gate, w)
    attn, ldx = _rows2d(attn); gate, ldg = _rows2d(gate)
    M, K = attn.shape
    N = w.shape[0]
    y = torch.empty(M, N, device=dev, dtype=torch.bfloat16)
    with torch.cuda.device(dev):
        _call(lib.vsde_linear_gated_bf16, _ptr(attn), _i64(ldx), _ptr(gate), _i64(ldg), _ptr(w), _ptr(bias), _ptr(y), _i64(N), _i64(M),
              ctypes.c_int(N), ctypes.c_int(K), _stream(dev))
    return y


def linear_swiglu_bwd_bf16(dy: torch.Tensor, w_t: torch.Tensor, u: torch.Tensor, out: Optional[torch.Tensor] = None):
    """du [M,2H] (interleaved, like u) from dy [M,K] and w_t [H,K] = the SwiGLU output projection transposed: the product
    ds = dy w_t^T never leaves the registers.  ``out``: a row-pitched bf16 buffer to write into instead of a fresh one."""
    lib = load(); dev = _require_hip(dy, w_t, u)
    dy, ldx = _rows2d(dy)
    M, K = dy.shape
    H = w_t.shape[0]
    du = torch.empty(M, 2 * H, device=dev, dtype=torch.bfloat16) if out is None else _given(out, (M, 2 * H), torch.bfloat16, True)
    with torch.cuda.device(dev):
        _call(lib.vsde_linear_bf16, _ptr(dy), _i64(ldx), _ptr(w_t), None, _ptr(du), _i64(du.stride(0)), _i64(M), ctypes.c_int(H),
              ctypes.c_int(K), ctypes.c_int(EPI_SWIGLU_BWD), None, _i64(0), _ptr(u), _i64(u.stride(0)), _stream(dev))
    return du
