"""Python host-side mirror of include/feather_hip/feather_frame.h (``libfeather_frame.so``): the layers that frame an image-to-image net --
ncnn's Padding and Crop (one operation, the window) and PixelShuffle -- on torch CUDA tensors.  Every device call goes through the C-ABI on
the current stream; there is no fallback path.
"""
from __future__ import annotations

import ctypes

from . import _lib
from .booster import _ptr, _stream

NET_ROUTE = 112  # FHIP_FRAME_NET_ROUTE
TILE, TILE_MIN = 4096, 1024  # FHIP_FRAME_TILE, FHIP_FRAME_TILE_MIN
CONSTANT, REPLICATE, REFLECT = range(3)  # the window types (ncnn's Padding 4=type)
RELU_NONE, RELU_SLOPE, RELU_PLAIN = range(3)  # `relu` of pixel_shuffle
WINDOW, SHUFFLE = range(2)  # fhip_frame_op

_check = _lib.checker(_lib.load_frame_library, "fhip_frame_last_error")


def _f32(t, what):
    import torch
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous() or t.dim() != 4:
        raise ValueError(f"{what} must be a contiguous float32 CUDA tensor [N][C][H][W]")


def _out(out, x, shape):
    import torch
    if out is None:
        return torch.empty(shape, device=x.device, dtype=torch.float32)
    if not out.is_cuda or out.dtype != torch.float32 or not out.is_contiguous() or tuple(out.shape) != tuple(shape):
        raise ValueError(f"out must be a contiguous float32 CUDA tensor of shape {tuple(shape)}")
    return out


def window_output_dim(c: int, h: int, w: int, front: int = 0, behind: int = 0, top: int = 0, bottom: int = 0, left: int = 0, right: int = 0):
    """(c, h, w) of the window of an input (c, h, w) (fhip_frame_window_output_dim): positive margins pad, negative ones crop."""
    o = [ctypes.c_int() for _ in range(3)]
    _check(_lib.load_frame_library().fhip_frame_window_output_dim(int(c), int(h), int(w), int(front), int(behind), int(top), int(bottom), int(left), int(right),
                                                                  *[ctypes.byref(v) for v in o]), "fhip_frame_window_output_dim")
    return tuple(v.value for v in o)


def window(x, type: int = CONSTANT, value: float = 0.0, per_channel=None, front: int = 0, behind: int = 0, top: int = 0, bottom: int = 0, left: int = 0,
           right: int = 0, out=None):
    """The window of a contiguous float32 CUDA tensor [N][C][H][W] (fhip_frame_window_forward): six signed margins, type CONSTANT (`value`, or
    `per_channel`, a CUDA tensor of C floats), REPLICATE or REFLECT.  Every output element is a bit copy of an input element or the constant."""
    _f32(x, "x")
    n, c, h, w = x.shape
    shape = (n,) + window_output_dim(c, h, w, front, behind, top, bottom, left, right)
    if per_channel is not None and (not per_channel.is_cuda or per_channel.dtype != x.dtype or not per_channel.is_contiguous() or per_channel.numel() != c):
        raise ValueError("per_channel must be a contiguous float32 CUDA tensor of C values")
    out = _out(out, x, shape)
    _check(_lib.load_frame_library().fhip_frame_window_forward(int(type), float(value), None if per_channel is None else _ptr(per_channel), n, c, h, w, int(front),
                                                               int(behind), int(top), int(bottom), int(left), int(right), _ptr(out), _ptr(x), _stream()),
           "fhip_frame_window_forward")
    return out


def pad(x, top: int = 0, bottom: int = 0, left: int = 0, right: int = 0, type: int = CONSTANT, value: float = 0.0, per_channel=None, front: int = 0,
        behind: int = 0, out=None):
    """ncnn's Padding (0=top 1=bottom 2=left 3=right 4=type 5=value, per-channel values, 7=front 8=behind): the window with margins >= 0."""
    if min(top, bottom, left, right, front, behind) < 0:
        raise ValueError("Padding margins are >= 0 (crop() takes a part of a blob)")
    return window(x, type, value, per_channel, front, behind, top, bottom, left, right, out)


def crop(x, woffset: int = 0, hoffset: int = 0, coffset: int = 0, outw: int = -233, outh: int = -233, outc: int = -233, woffset2: int = 0, hoffset2: int = 0,
         coffset2: int = 0, out=None):
    """ncnn's Crop (0=woffset 1=hoffset 2=coffset 3=outw 4=outh 5=outc 6=woffset2 7=hoffset2 8=coffset2; a size of -233 is dim - offset -
    offset2): the window with margins <= 0."""
    _f32(x, "x")
    margins = []
    for dim, off, size, off2 in ((x.shape[1], coffset, outc, coffset2), (x.shape[2], hoffset, outh, hoffset2), (x.shape[3], woffset, outw, woffset2)):
        size = dim - off - off2 if size == -233 else size
        if off < 0 or off2 < 0 or size < 1 or off + size > dim:
            raise ValueError(f"the window (offset {off}, size {size}) leaves the dimension of {dim}")
        margins += [-off, off + size - dim]
    return window(x, CONSTANT, 0.0, None, *margins, out=out)


def pixel_shuffle_output_dim(r: int, c: int, h: int, w: int):
    """(c, h, w) of PixelShuffle's output for an input (c, h, w) (fhip_pixel_shuffle_output_dim)."""
    o = [ctypes.c_int() for _ in range(3)]
    _check(_lib.load_frame_library().fhip_pixel_shuffle_output_dim(int(r), int(c), int(h), int(w), *[ctypes.byref(v) for v in o]), "fhip_pixel_shuffle_output_dim")
    return tuple(v.value for v in o)


def pixel_shuffle(x, r: int, mode: int = 0, relu: int = RELU_NONE, slope: float = 0.0, out=None):
    """ncnn's PixelShuffle of a contiguous float32 CUDA tensor [N][C * r^2][H][W]: [N][C][H * r][W * r] (fhip_pixel_shuffle_forward); mode 0 is
    torch's pixel_shuffle, mode 1 the inverse of Reorg mode 1; relu: RELU_SLOPE (x > 0 ? x : x * slope) or RELU_PLAIN (fmaxf(x, 0))."""
    _f32(x, "x")
    n, c, h, w = x.shape
    out = _out(out, x, (n,) + pixel_shuffle_output_dim(r, c, h, w))
    _check(_lib.load_frame_library().fhip_pixel_shuffle_forward(int(r), int(mode), int(relu), float(slope), n, c, h, w, _ptr(out), _ptr(x), _stream()),
           "fhip_pixel_shuffle_forward")
    return out


def frame_route(what: int, a: int = 0, w: int = 0, b: int = 0, out_w: int = 0, aligned16: int = 1) -> str:
    """The kernel instantiation a call would launch (fhip_frame_route): what = WINDOW (a = type, b = some margin is positive, out_w,
    aligned16 = `out` is 16-byte aligned) or SHUFFLE (a = r, w and b = the input's w and h)."""
    name = ctypes.create_string_buffer(128)
    _check(_lib.load_frame_library().fhip_frame_route(int(what), int(a), int(w), int(b), int(out_w), int(aligned16), name, 128), "fhip_frame_route")
    return name.value.decode()
