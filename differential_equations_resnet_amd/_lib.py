"""ctypes binding of libasr.so (include/asr.h).

This is the ONLY way the package computes: every public operation ends in one
of these C entry points, which launch the hand-written gfx950 kernels.  If the
library is missing or cannot be loaded the package raises — there is no
CPU or PyTorch fallback for the hot path.
"""
from __future__ import annotations

import ctypes as ct
import os

try:  # torch must own the HIP runtime before libasr binds to it (one runtime per process)
    import torch  # noqa: F401
except ImportError:  # pragma: no cover - torch is part of the image
    torch = None

from . import _build

ASR_OK = 0
ASR_E_ARG = -1
ASR_E_UNSUPPORTED = -2
ASR_E_WORKSPACE = -3
ASR_E_HIP = -4
ASR_E_DEVICE = -5

ASR_F32 = 0
ASR_BF16 = 1
ASR_PARAM_3BY3 = 0
ASR_PARAM_GENERAL = 1
ASR_PARAM_REGULAR = 2
ABI_VERSION = 13
ASR_MODE_EULER = 0
ASR_MODE_CONV = 1
ASR_INTEGRATOR_EULER = 0
ASR_INTEGRATOR_RK2 = 1
ASR_VARIANT_NO_FOLD = 1
ASR_VARIANT_STEM_FWD_VALU = 2
ASR_VARIANT_STEM_WGRAD_VALU = 4
ASR_VARIANT_PER_BLOCK_FWD = 8
ASR_VARIANT_PER_BLOCK_BWD = 16
ASR_VARIANT_INFERENCE = 32
ASR_VARIANT_TIMED = 64
ASR_VARIANT_FULL_DXL = 128
ASR_VARIANT_FULL_SLABS = 256
ASR_VARIANT_W_BF16 = 512
ASR_DIST_UNIQUE_ID_BYTES = 128
ASR_U8 = 2
ASR_AUG_RESIZE_NONE, ASR_AUG_RESIZE_BILINEAR, ASR_AUG_RESIZE_PAD = 0, 1, 2
ASR_AUG_NONE, ASR_AUG_BRIGHTNESS, ASR_AUG_SATURATION = 0, 1, 2
ASR_STAGES_MAX = 8


class AsrError(RuntimeError):
    pass


class AsrUnsupported(AsrError, NotImplementedError):
    pass


class NetConfig(ct.Structure):
    _fields_ = [
        ("N", ct.c_int), ("H", ct.c_int), ("W", ct.c_int), ("Cin", ct.c_int), ("C", ct.c_int), ("L", ct.c_int),
        ("num_classes", ct.c_int), ("h", ct.c_float), ("gamma", ct.c_float), ("subtract_mean", ct.c_float),
        ("divide_by_stddev", ct.c_float), ("use_norm", ct.c_int), ("dtype", ct.c_int), ("input_u8", ct.c_int),
        ("param_kind", ct.c_int), ("antisymmetric", ct.c_int), ("integrator", ct.c_int), ("variant", ct.c_int),
        ("kernel_size", ct.c_int), ("conv1_kernel_size", ct.c_int),  # 0 means 3 (ABI 10)
    ]


class StagesConfig(ct.Structure):
    """asr_stages_config (include/asr.h, ABI 7)."""
    _fields_ = [
        ("N", ct.c_int), ("H", ct.c_int), ("W", ct.c_int), ("Cin", ct.c_int), ("num_classes", ct.c_int),
        ("n_stages", ct.c_int), ("C", ct.c_int * 8), ("L", ct.c_int * 8), ("stride", ct.c_int * 8),
        ("h", ct.c_float), ("gamma", ct.c_float), ("subtract_mean", ct.c_float), ("divide_by_stddev", ct.c_float),
        ("use_norm", ct.c_int), ("input_u8", ct.c_int), ("param_kind", ct.c_int), ("antisymmetric", ct.c_int),
        ("dtype", ct.c_int),
    ]


class AugItem(ct.Structure):
    """asr_aug_item (include/asr.h, ABI 11): 32 bytes, one per output image."""
    _fields_ = [("src", ct.c_int32), ("y0", ct.c_int32), ("x0", ct.c_int32), ("ch", ct.c_int32), ("cw", ct.c_int32),
                ("flip", ct.c_int32), ("brightness", ct.c_float), ("saturation", ct.c_float)]


class AugPlanConfig(ct.Structure):
    """asr_aug_plan (include/asr.h, ABI 11)."""
    _fields_ = [("Hs", ct.c_int), ("Ws", ct.c_int), ("Cch", ct.c_int), ("src_dtype", ct.c_int), ("Ho", ct.c_int),
                ("Wo", ct.c_int), ("dst_dtype", ct.c_int), ("resize", ct.c_int), ("rh", ct.c_int), ("rw", ct.c_int),
                ("pad_top", ct.c_int), ("pad_left", ct.c_int), ("flip_src", ct.c_int), ("color", ct.c_int * 2)]


ASR_OPT_SGD, ASR_OPT_ADAM, ASR_OPT_RMSPROP = 0, 1, 2
ASR_OPT_NESTEROV, ASR_OPT_AMSGRAD = 1, 2


class OptimizerConfig(ct.Structure):
    """asr_optimizer_config (include/asr.h)."""
    _fields_ = [("kind", ct.c_int), ("flags", ct.c_int), ("lr", ct.c_float), ("a", ct.c_float), ("b", ct.c_float),
                ("eps", ct.c_float), ("step", ct.c_long), ("grad_scale", ct.c_float)]


ASR_REG_MAX_SEGMENTS = 256


class RegSegment(ct.Structure):
    """asr_reg_segment (include/asr.h)."""
    _fields_ = [("offset", ct.c_long), ("count", ct.c_long), ("layer_stride", ct.c_long), ("layers", ct.c_int),
                ("l2", ct.c_float), ("smooth", ct.c_float)]


_P = ct.c_void_p
_I = ct.c_int
_L = ct.c_long
_F = ct.c_float
_S = ct.c_size_t

# (name, restype, argtypes) — exactly the declarations of include/asr.h
SIGNATURES = [
    ("asr_last_error", ct.c_char_p, []),
    ("asr_abi_version", _I, []),
    ("asr_device_cu_count", _I, []),
    ("asr_theta_count", _L, [_I, _I, _I]),
    ("asr_param_map", _I, [_I, _I, _I, _P, _P]),
    ("asr_param_is_antisymmetric", _I, [_I, _I]),
    ("asr_param_map_transpose", _I, [_I, _P, _P]),
    ("asr_param_map_pair", _I, [_I, _P, ct.c_long, _P]),
    ("asr_theta_count_k", _L, [_I, _I, _I, _I]),
    ("asr_param_map_k", _I, [_I, _I, _I, _I, _P, _P]),
    ("asr_param_map_transpose_k", _I, [_I, _I, _P, _P]),
    ("asr_theta_to_w_k", _I, [_P, _L, _I, _I, _I, _P, _F, _P, _L, _P]),
    ("asr_conv_forward_k", _I, [_I, _I, _P, _P, _P, _P, _P, _F, _I, _I, _I, _I, _P]),
    ("asr_conv_backward_workspace_bytes_k", _S, [_I, _I, _I, _I, _I]),
    ("asr_conv_backward_k", _I, [_I, _I, _P, _P, _P, _P, _P, _L, _F, _F, _I, _I, _I, _I, _P, _P, _P, _P, _P, _S, _P]),
    ("asr_wpack_elems_k", _L, [_I, _I]),
    ("asr_theta_to_w_k_bf16", _I, [_P, _L, _I, _I, _I, _P, _F, _P, _L, _P]),
    ("asr_conv_forward_k_bf16", _I, [_I, _I, _P, _P, _P, _P, _P, _F, _I, _I, _I, _I, _P]),
    ("asr_conv_backward_workspace_bytes_k_bf16", _S, [_I, _I, _I, _I, _I]),
    ("asr_conv_backward_k_bf16", _I, [_I, _I, _P, _P, _P, _P, _P, _L, _F, _F, _I, _I, _I, _I, _P, _P, _P, _P, _P, _S,
                                      _P]),
    ("asr_wpack_elems", _L, [_I]),
    ("asr_theta_to_w", _I, [_P, _L, _I, _I, _P, _F, _P, _L, _I, _P]),
    ("asr_theta_to_w_mirror", _I, [_P, _L, _I, _I, _P, _P, _L, _I, _P]),
    ("asr_conv_forward", _I, [_I, _P, _P, _P, _P, _P, _F, _I, _I, _I, _I, _I, _P]),
    ("asr_mask_bytes", _L, [_I, _I, _I, _I]),
    ("asr_block_stack_forward", _I, [_P, _P, _L, _P, _L, _P, _L, _P, _L, _F, _I, _I, _I, _I, _I, _I, _I, _P]),
    ("asr_block_stack_backward_workspace_bytes", _S, [_I, _I, _I, _I, _I, _I]),
    ("asr_block_stack_backward", _I, [_P, _P, _L, _P, _L, _P, _L, _P, _L, _F, _F, _I, _I, _I, _I, _I, _I, _P, _P, _P,
                                      _S, _P]),
    ("asr_conv_backward_workspace_bytes", _S, [_I, _I, _I, _I, _I]),
    ("asr_conv_backward", _I, [_I, _P, _P, _P, _P, _P, _L, _F, _F, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _S, _P]),
    ("asr_rk2_forward", _I, [_P, _P, _P, _P, _P, _P, _P, _F, _I, _I, _I, _I, _I, _P]),
    ("asr_rk2_backward_workspace_bytes", _S, [_I, _I, _I, _I, _I]),
    ("asr_rk2_backward", _I, [_P, _P, _P, _P, _P, _P, _P, _L, _F, _F, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _S,
                              _P]),
    ("asr_net_param_count", _L, [ct.POINTER(NetConfig)]),
    ("asr_net_workspace_bytes", _S, [ct.POINTER(NetConfig)]),
    ("asr_net_prepare", _I, [ct.POINTER(NetConfig), _P, _S]),
    ("asr_net_forward", _I, [ct.POINTER(NetConfig), _P, _P, _P, _P, _S, _P]),
    ("asr_net_forward_backward", _I, [ct.POINTER(NetConfig), _P, _P, _P, _P, _P, _P, _P, _S, _P]),
    ("asr_net_check_status", _I, [ct.POINTER(NetConfig), _P, _S, _P]),
    ("asr_net_kernel_times", _I, [_P]),
    ("asr_stack_status", _I, [_I]),
    ("asr_debug_stack_backward", _I, [_I]),
    ("asr_rk2_stack_forward", _I, [_P, _P, _P, _L, _P, _P, _L, _P, _L, _P, _L, _F, _I, _I, _I, _I, _I, _I, _P]),
    ("asr_rk2_stack_backward_workspace_bytes", _S, [_I, _I, _I, _I, _I, _I]),
    ("asr_rk2_stack_backward", _I, [_P, _P, _P, _L, _P, _P, _L, _P, _L, _P, _L, _F, _F, _I, _I, _I, _I, _I, _I, _P,
                                    _P, _P, _S, _P]),
    ("asr_transition_forward", _I, [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    ("asr_transition_backward_workspace_bytes", _S, [_I, _I, _I, _I, _I, _I]),
    ("asr_transition_backward", _I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _P, _P, _S, _P]),
    ("asr_stages_check", ct.c_int, [ct.POINTER(StagesConfig)]),
    ("asr_stages_param_count", _L, [ct.POINTER(StagesConfig)]),
    ("asr_stages_workspace_bytes", _S, [ct.POINTER(StagesConfig)]),
    ("asr_stages_prepare", _I, [ct.POINTER(StagesConfig), _P, _S]),
    ("asr_stages_forward", _I, [ct.POINTER(StagesConfig), _P, _P, _P, _P, _S, _P]),
    ("asr_stages_forward_backward", _I, [ct.POINTER(StagesConfig), _P, _P, _P, _P, _P, _P, _P, _S, _P]),
    ("asr_adam_update", _I, [_P, _P, _P, _P, _L, _F, _F, _F, _F, _L, _F, _P]),
    ("asr_optimizer_slots", _I, [_I, _I]),
    ("asr_optimizer_update", _I, [ct.POINTER(OptimizerConfig), _P, _P, _P, _L, _P]),
    ("asr_regularize_check", _I, [_P, _I, _L]),
    ("asr_regularize_workspace_bytes", _S, [_I, _L]),
    ("asr_regularize", _I, [_P, _I, _P, _P, _F, _P, _P, _P, _S, _P]),
    ("asr_segment_sq_norms", _I, [_P, _P, _I, _P, _P]),
    ("asr_batch_metrics", _I, [_P, _P, _P, _I, _I, _P, _P]),
    ("asr_augment_batch", _I, [_P, _L, ct.POINTER(AugPlanConfig), _P, _I, _P, _P]),
    ("asr_dist_unique_id", _I, [_P]),
    ("asr_dist_init", _I, [_I, _I, _P]),
    ("asr_dist_allreduce_sum", _I, [_P, _S, _I, _P]),
    ("asr_dist_broadcast", _I, [_P, _S, _I, _I, _P]),
    ("asr_dist_world_size", _I, []),
    ("asr_dist_finalize", _I, []),
]

_lib = None


def lib_path() -> str:
    return _build.LIB


def load(build_if_missing: bool = True, path: str | None = None):
    """Load (building first if needed) libasr.so and bind its C ABI.

    `path` (development tools only: A/B timing of variant builds) loads
    another build of the same sources; it must be given before the first
    load of the process."""
    global _lib
    if _lib is not None:
        if path is not None and getattr(_lib, "_asr_path", None) != path:
            raise AsrError(f"libasr already loaded from {_lib._asr_path}")
        return _lib
    path = path or _build.LIB
    if not os.path.exists(path):
        if not build_if_missing:
            raise AsrError(f"libasr.so not found at {path}; run differential_equations_resnet_amd._build.build()")
        _build.build()
    lib = ct.CDLL(path, mode=ct.RTLD_GLOBAL)
    lib._asr_path = path
    for name, res, args in SIGNATURES:
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def last_error() -> str:
    msg = load().asr_last_error()
    return msg.decode() if msg else ""


def check(rc: int, what: str = "") -> None:
    if rc == ASR_OK:
        return
    msg = f"{what}: {last_error()} (code {rc})"
    if rc == ASR_E_UNSUPPORTED:
        raise AsrUnsupported(msg)
    if rc == ASR_E_ARG:
        raise ValueError(msg)
    raise AsrError(msg)


def call(name: str, *args):
    rc = getattr(load(), name)(*args)
    check(rc, name)
    return rc
