"""Python host-side mirror of include/feather_hip/feather_conv1d.h (``libfeather_conv1d.so``): ncnn's Convolution1D, ConvolutionDepthWise1D
and Pooling1D on torch CUDA tensors.  Every device call goes through the C-ABI on the current stream; there is no fallback path.
"""
from __future__ import annotations

import ctypes

from . import _lib
from .booster import _stream

NET_ROUTE = 115  # FHIP_CONV1D_NET_ROUTE
SAME_UPPER, SAME_LOWER = -233, -234  # FHIP_CONV1D_SAME_UPPER, _SAME_LOWER
TILE_K, TILE_L, MFMA_MIN_C = 64, 64, 3  # FHIP_CONV1D_TILE_K, _TILE_L, _MFMA_MIN_C
LDS_SMALL, LDS_LARGE = 8192, 24576  # FHIP_CONV1D_LDS_SMALL, _LDS_LARGE
DIRECT_K, DW_SEGMENT, DW_LANE, DW_LDS = 4, 1024, 4, 8192  # FHIP_CONV1D_DIRECT_K, _DW_SEGMENT, _DW_LANE, _DW_LDS

_check = _lib.checker(_lib.load_conv1d_library, "fhip_conv1d_last_error")


def chunk(kw: int, s: int, d: int, lds_floats: int) -> int:
    """fhip_conv1d_chunk restated: the input channels per chunk of the matrix kernel for a budget, or 0."""
    slab = 63 * s + (kw - 1) * d + 1
    sp = (slab + s - 1) // s * s
    for cc in (16, 8, 4, 2):
        if 2 * (64 * ((cc * kw) | 1) + cc * sp) <= lds_floats:
            return cc
    return 0


def route_rule(c: int, k: int, kw: int, d: int = 1, s: int = 1, group: int = 1) -> str:
    """The rule of fhip_conv1d_route restated for a convolution the library accepts."""
    if group > 1 and group == c == k and (DW_SEGMENT - 1) * s + (kw - 1) * d + 9 <= DW_LDS:
        return "fhip::conv1d_depthwise_kernel"
    for lds in (LDS_SMALL, LDS_LARGE):
        if c // group >= MFMA_MIN_C and chunk(kw, s, d, lds):
            return "fhip::conv1d_mfma_kernel<%d>" % lds
    return "fhip::conv1d_direct_kernel"


def _rows(t, what):
    """(n, channels, length, row stride) of a [n][C][L] float32 CUDA tensor with unit column stride and equally spaced rows."""
    import torch
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32:
        raise ValueError(f"{what} must be a float32 CUDA tensor")
    if t.dim() != 3 or t.stride(2) != 1 or (t.shape[0] > 1 and t.stride(0) != t.shape[1] * t.stride(1)):
        raise ValueError(f"{what} must be [n][C][L] with unit column stride and equally spaced rows")
    return t.shape[0], t.shape[1], t.shape[2], t.stride(1)


def _dim(fn, what, *args):
    left, right, lo = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    _check(fn(*args, ctypes.byref(left), ctypes.byref(right), ctypes.byref(lo)), what)
    return left.value, right.value, lo.value


def conv1d_output_dim(l: int, kw: int, d: int = 1, s: int = 1, pad_left: int = 0, pad_right=None):
    """-> (pad_left, pad_right, Lo) with -233 / -234 resolved (fhip_conv1d_output_dim)."""
    return _dim(_lib.load_conv1d_library().fhip_conv1d_output_dim, "fhip_conv1d_output_dim", l, kw, d, s, pad_left, pad_left if pad_right is None else pad_right)


def pool1d_output_dim(l: int, kw: int, s: int = 1, pad_left: int = 0, pad_right=None, pad_mode: int = 0):
    """-> (pad_left, pad_right, Lo) by ncnn's pad_mode (fhip_pool1d_output_dim)."""
    return _dim(_lib.load_conv1d_library().fhip_pool1d_output_dim, "fhip_pool1d_output_dim", l, kw, s, pad_left, pad_left if pad_right is None else pad_right, pad_mode)


def conv1d(x, w, bias=None, stride: int = 1, dilation: int = 1, pad_left: int = 0, pad_right=None, pad_value: float = 0.0, group: int = 1, activation: int = 0,
           a0: float = 0.0, a1: float = 0.0, out=None):
    """ncnn's Convolution1D / ConvolutionDepthWise1D of x [n][C][L] (a view with a larger row stride is read in place) with w
    [K][C / group][kw] -> [n][K][Lo] (fhip_conv1d_forward).  pad_left -233 / -234: SAME_UPPER / SAME_LOWER."""
    import torch
    n, c, l, xs = _rows(x, "x")
    if not isinstance(w, torch.Tensor) or not w.is_cuda or w.dtype != torch.float32 or w.dim() != 3 or not w.is_contiguous():
        raise ValueError("w must be a contiguous float32 CUDA tensor [K][C / group][kw]")
    k, kw = w.shape[0], w.shape[2]
    if group < 1 or c % group or w.shape[1] != c // group:
        raise ValueError("x, w and group do not fit each other")
    if bias is not None and (not isinstance(bias, torch.Tensor) or not bias.is_cuda or bias.dtype != torch.float32 or tuple(bias.shape) != (k,) or not bias.is_contiguous()):
        raise ValueError("bias must be a contiguous float32 CUDA tensor [K]")
    left, right, lo = conv1d_output_dim(l, kw, dilation, stride, pad_left, pad_right)
    if out is None:
        out = torch.empty((n, k, lo), device=x.device, dtype=torch.float32)
    on, ok, ol, ys = _rows(out, "out")
    if (on, ok, ol) != (n, k, lo):
        raise ValueError(f"out must be [{n}][{k}][{lo}]")
    at = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    _check(_lib.load_conv1d_library().fhip_conv1d_forward(n, c, l, k, kw, int(dilation), int(stride), left, right, float(pad_value), int(group), int(activation), float(a0),
                                                          float(a1), at(x), xs, at(w), at(bias), at(out), ys, lo, _stream()), "fhip_conv1d_forward")
    return out


def pool1d(x, kernel_w: int = 0, stride: int = 1, pad_left: int = 0, pad_right=None, pad_mode: int = 0, avg: bool = False, count_include_pad: bool = False,
           global_: bool = False, out_w=None, out=None):
    """ncnn's Pooling1D of x [n][C][L] -> [n][C][Lo] (fhip_pool1d_forward).  global_: Lo = 1; out_w: adaptive pooling onto that many cells."""
    import torch
    n, c, l, xs = _rows(x, "x")
    if global_ or out_w is not None:
        kernel_w, left, right, lo = 0, 0, 0, 1 if global_ else int(out_w)
    else:
        left, right, lo = pool1d_output_dim(l, kernel_w, stride, pad_left, pad_right, pad_mode)
    if out is None:
        out = torch.empty((n, c, lo), device=x.device, dtype=torch.float32)
    on, oc, ol, ys = _rows(out, "out")
    if (on, oc, ol) != (n, c, lo):
        raise ValueError(f"out must be [{n}][{c}][{lo}]")
    _check(_lib.load_conv1d_library().fhip_pool1d_forward(int(bool(avg)), n * c, l, int(kernel_w), int(stride), left, right, int(bool(count_include_pad)),
                                                          ctypes.c_void_p(x.data_ptr()), xs, ctypes.c_void_p(out.data_ptr()), ys, lo, _stream()), "fhip_pool1d_forward")
    return out


def conv1d_route(c: int, k: int, kw: int, d: int = 1, s: int = 1, group: int = 1) -> str:
    """The kernel instantiation a convolution would launch (fhip_conv1d_route); kw == 0 asks for the pooling."""
    name = ctypes.create_string_buffer(128)
    _check(_lib.load_conv1d_library().fhip_conv1d_route(int(c), int(k), int(kw), int(d), int(s), int(group), name, 128), "fhip_conv1d_route")
    return name.value.decode()
