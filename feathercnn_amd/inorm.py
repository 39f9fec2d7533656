"""Python host-side mirror of include/feather_hip/feather_inorm.h (``libfeather_inorm.so``): InstanceNorm and the element-wise activations
of generative nets on torch CUDA tensors.  Every call goes through the C-ABI on the current stream; there is no fallback path.
"""
from __future__ import annotations

import ctypes

from . import _lib
from .booster import _ptr, _stream

ACT_NONE, ACT_RELU, ACT_LEAKY = 0, 1, 2
LEAKY_RELU, PRELU, SIGMOID, TANH, CLIP = range(5)
KINDS = {"leaky_relu": LEAKY_RELU, "prelu": PRELU, "sigmoid": SIGMOID, "tanh": TANH, "clip": CLIP}
FLT_MAX = 3.4028234663852886e38


_check = _lib.checker(_lib.load_inorm_library, "fhip_inorm_last_error")


def _act(act, slope):
    if act in (None, 0, "none"):
        return ACT_NONE, 0.0
    if act in (1, "relu"):
        return ACT_RELU, 0.0
    if act in (2, "leaky_relu"):
        return ACT_LEAKY, float(slope)
    raise ValueError(f"unknown activation {act!r}")


def scratch_bytes(shape) -> int:
    """Bytes of scratch instance_norm needs for an [N][C][H][W] tensor (0 unless the shape takes the split-plane route)."""
    n, c, h, w = shape
    b = ctypes.c_size_t()
    _check(_lib.load_inorm_library().fhip_instance_norm_get_buffer_size(n, c, h, w, ctypes.byref(b)), "fhip_instance_norm_get_buffer_size")
    return b.value


def instance_norm_route(x, out=None) -> str:
    """The kernel instantiation instance_norm launches for these tensors (fhip_instance_norm_route)."""
    n, c, h, w = x.shape
    name = ctypes.create_string_buffer(96)
    _check(_lib.load_inorm_library().fhip_instance_norm_route(n, c, h, w, _ptr(x if out is None else out), _ptr(x), name, len(name)),
           "fhip_instance_norm_route")
    return name.value.decode()


ROUTES = {"wave": 0, "block256": 1, "block1024": 2, "split": 3}
CHUNK = 4096  # floats per block of the split-plane route


def instance_norm(x, gamma=None, beta=None, eps: float = 1e-3, act=None, slope: float = 0.0, out=None, scratch=None, route=None):
    """y = act(instance_norm(x)) for a contiguous float32 [N][C][H][W] CUDA tensor; gamma / beta are [C] or None (1 / 0).  `scratch` (a
    float32 tensor of at least scratch_bytes(x.shape) bytes) is allocated here when the route needs one and none is given.  `route` (a key
    of ROUTES) runs that route instead of the selected one (fhip_instance_norm_forward_route: measurements and tests)."""
    import torch
    if x.dim() != 4 or x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError("instance_norm needs a contiguous float32 [N][C][H][W] tensor")
    n, c, h, w = x.shape
    for v in (gamma, beta):
        if v is not None and (v.dtype != torch.float32 or v.numel() != c or not v.is_contiguous()):
            raise ValueError("gamma / beta must be contiguous float32 [C]")
    if out is None:
        out = torch.empty_like(x)
    need = scratch_bytes(x.shape) if route is None else (n * c * -(-h * w // CHUNK) * 8 if route == "split" else 0)
    if need and scratch is None:
        scratch = torch.empty(need // 4, dtype=torch.float32, device=x.device)
    if need and (scratch.dtype != torch.float32 or scratch.device != x.device or not scratch.is_contiguous() or scratch.numel() * 4 < need
                 or scratch.data_ptr() % 8):
        raise ValueError(f"scratch must be a contiguous, 8-byte aligned float32 tensor of at least {need} bytes on {x.device}")
    code, slope = _act(act, slope)
    if route is not None:
        _check(_lib.load_inorm_library().fhip_instance_norm_forward_route(ROUTES[route], n, c, h, w, _ptr(out), _ptr(x), _ptr(gamma), _ptr(beta), float(eps),
                                                                          code, slope, _ptr(scratch), _stream()), "fhip_instance_norm_forward_route")
        return out
    _check(_lib.load_inorm_library().fhip_instance_norm_forward(n, c, h, w, _ptr(out), _ptr(x), _ptr(gamma), _ptr(beta), float(eps), code, slope,
                                                                _ptr(scratch), _stream()), "fhip_instance_norm_forward")
    return out


def activation(x, kind, slope: float = 0.0, min: float = -FLT_MAX, max: float = FLT_MAX, slopes=None, out=None):
    """Element-wise `kind` ("leaky_relu", "prelu", "sigmoid", "tanh", "clip") of a contiguous float32 [N][C][...] CUDA tensor; `slopes` is
    PReLU's per-channel [C] vector (None: the shared `slope`).  out may be x."""
    import torch
    if x.dim() < 2 or x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError("activation needs a contiguous float32 [N][C][...] tensor")
    k = KINDS[kind] if isinstance(kind, str) else int(kind)
    n, c = x.shape[:2]
    hw = x.numel() // (n * c) if x.numel() else 0
    if slopes is not None and (slopes.dtype != torch.float32 or slopes.numel() != c):
        raise ValueError("slopes must be float32 [C]")
    if out is None:
        out = torch.empty_like(x)
    p0 = float(min) if k == CLIP else float(slope)
    _check(_lib.load_inorm_library().fhip_activation_forward(k, _ptr(out), _ptr(x), n, c, hw, p0, float(max), _ptr(slopes), _stream()),
           "fhip_activation_forward")
    return out
