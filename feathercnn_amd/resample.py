"""Python host-side mirror of include/feather_hip/feather_resample.h (``libfeather_resample.so``): Interp (nearest / bilinear resize) and
HardSwish on torch CUDA tensors.  Every call goes through the C-ABI on the current stream; there is no fallback path.
"""
from __future__ import annotations

import ctypes

from . import _lib
from .booster import _ptr, _stream

NEAREST, BILINEAR = 1, 2
MODES = {"nearest": NEAREST, "bilinear": BILINEAR}


_check = _lib.checker(_lib.load_resample_library, "fhip_resample_last_error")


def _f32(t, what, dims=None):
    import torch
    if t.dtype != torch.float32 or not t.is_contiguous() or (dims is not None and t.dim() != dims):
        raise ValueError(f"{what} must be a contiguous float32 tensor" + (f" of {dims} dimensions" if dims else ""))


def _mode(mode) -> int:
    return MODES[mode] if isinstance(mode, str) else int(mode)


def interp_output_dim(in_h: int, in_w: int, scale=None, size=None):
    """(out_h, out_w) of an Interp layer (fhip_interp_output_dim): `size` = (h, w) where given (an entry of 0 leaves that axis to the scale),
    else `scale` = (height_scale, width_scale) or one value for both; out = int(in * scale) with the product in float32."""
    hs, ws = (scale, scale) if not isinstance(scale, (tuple, list)) else scale
    oh, ow = (0, 0) if size is None else size
    h, w = ctypes.c_int(), ctypes.c_int()
    _check(_lib.load_resample_library().fhip_interp_output_dim(int(in_h), int(in_w), float(hs or 0), float(ws or 0), int(oh), int(ow), ctypes.byref(h),
                                                               ctypes.byref(w)), "fhip_interp_output_dim")
    return h.value, w.value


def _geometry(x, scale, size):
    n, c, ih, iw = x.shape
    if size is not None and all(size):
        return n, c, ih, iw, int(size[0]), int(size[1]), 0.0, 0.0
    hs, ws = (scale, scale) if not isinstance(scale, (tuple, list)) else scale
    oh, ow = interp_output_dim(ih, iw, (hs, ws), size)
    # a scale is handed on only where it decided the size (the header: hs = 1 / scale there, in / out where the size was given)
    return n, c, ih, iw, oh, ow, 0.0 if size is not None and size[0] else float(hs), 0.0 if size is not None and size[1] else float(ws)


def interp(x, mode="bilinear", scale=None, size=None, align_corner: bool = False, residual=None, relu: bool = False, out=None):
    """Resize every plane of a contiguous float32 [N][C][H][W] CUDA tensor: mode "nearest" or "bilinear"; the output size from `size` =
    (h, w) or from `scale`; then `+ residual` (of the output's shape) and ReLU, each rounded on its own.  out may be residual."""
    import torch
    _f32(x, "x", 4)
    n, c, ih, iw, oh, ow, hs, ws = _geometry(x, scale, size)
    if residual is not None:
        _f32(residual, "residual", 4)
        if tuple(residual.shape) != (n, c, oh, ow):
            raise ValueError("residual must have the output's shape")
    if out is None:
        out = torch.empty((n, c, oh, ow), dtype=torch.float32, device=x.device)
    else:
        _f32(out, "out", 4)
        if tuple(out.shape) != (n, c, oh, ow):
            raise ValueError("out must have the output's shape")
    _check(_lib.load_resample_library().fhip_interp_forward(_mode(mode), int(bool(align_corner)), n, c, ih, iw, oh, ow, hs, ws, _ptr(out), _ptr(x),
                                                            _ptr(residual), int(bool(relu)), _stream()), "fhip_interp_forward")
    return out


def interp_route(x, mode="bilinear", scale=None, size=None, out=None, residual=None) -> str:
    """The kernel instantiation interp launches for these tensors (fhip_interp_route); without `out`, an aligned one is assumed."""
    n, c, ih, iw, oh, ow, hs, ws = _geometry(x, scale, size)
    name = ctypes.create_string_buffer(96)
    _check(_lib.load_resample_library().fhip_interp_route(_mode(mode), n, c, ih, iw, oh, ow, hs, ws, _ptr(out), _ptr(x), _ptr(residual), name, len(name)),
           "fhip_interp_route")
    return name.value.decode()


def hard_swish(x, alpha: float = 0.2, beta: float = 0.5, out=None):
    """ncnn's HardSwish(alpha, beta) of a contiguous float32 [N][C][...] CUDA tensor, element by element; out may be x."""
    import torch
    if x.dim() < 2:
        raise ValueError("hard_swish needs a contiguous float32 [N][C][...] tensor")
    _f32(x, "x")
    n, c = x.shape[:2]
    hw = x.numel() // (n * c) if x.numel() else 0
    if out is None:
        out = torch.empty_like(x)
    _check(_lib.load_resample_library().fhip_hardswish_forward(_ptr(out), _ptr(x), n, c, hw, float(alpha), float(beta), _stream()), "fhip_hardswish_forward")
    return out


def hard_swish_route(x, out=None) -> str:
    """The instantiation hard_swish launches for these tensors (fhip_hardswish_route)."""
    n, c = x.shape[:2]
    name = ctypes.create_string_buffer(96)
    _check(_lib.load_resample_library().fhip_hardswish_route(_ptr(x if out is None else out), _ptr(x), n, c, x.numel() // (n * c), name, len(name)),
           "fhip_hardswish_route")
    return name.value.decode()
