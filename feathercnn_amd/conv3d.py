"""Python host-side mirror of include/feather_hip/feather_conv3d.h (``libfeather_conv3d.so``): ncnn's Convolution3D, ConvolutionDepthWise3D
and Pooling3D on torch CUDA tensors.  Every device call goes through the C-ABI on the current stream; there is no fallback path.
"""
from __future__ import annotations

import ctypes

from . import _lib
from .booster import _stream

NET_ROUTE = 117  # FHIP_CONV3D_NET_ROUTE
SAME_UPPER, SAME_LOWER = -233, -234  # FHIP_CONV3D_SAME_UPPER, _SAME_LOWER
TILE_K_SMALL, TILE_K_LARGE, TILE_H, TILE_W, CHUNK, MAX_TAPS, MAX_PLANE = 64, 128, 8, 8, 8, 9, 320  # FHIP_CONV3D_*

_check = _lib.checker(_lib.load_conv3d_library, "fhip_conv3d_last_error")


def _three(v):
    return (int(v),) * 3 if isinstance(v, int) else tuple(int(e) for e in v)


def route_rule(c: int, k: int, kernel, dilation=1, stride=1, group: int = 1, direct: bool = False) -> str:
    """The rule of fhip_conv3d_route restated for a convolution the library accepts."""
    (_, kh, kw), (_, dh, dw), (_, sh, sw) = _three(kernel), _three(dilation), _three(stride)
    plane = ((TILE_H - 1) * sh + (kh - 1) * dh + 1) * ((TILE_W - 1) * sw + (kw - 1) * dw + 1)
    if direct or group != 1 or kh * kw > MAX_TAPS or plane > MAX_PLANE:
        return "fhip::conv3d_direct_kernel"
    return "fhip::conv3d_mfma_kernel<%d>" % (TILE_K_SMALL if k <= TILE_K_SMALL else TILE_K_LARGE)


def _dims(fn, what, extents, *per_axis):
    """One call of an output_dim entry per axis -> ((lo, hi) per axis, out per axis)."""
    pads, outs = [], []
    for axis, e in enumerate(extents):
        lo, hi, out = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        _check(fn(int(e), *[int(a[axis]) if isinstance(a, tuple) else int(a) for a in per_axis], ctypes.byref(lo), ctypes.byref(hi), ctypes.byref(out)), what)
        pads.append((lo.value, hi.value))
        outs.append(out.value)
    return pads, outs


def _pads(pads):
    """pads: an int, (d, h, w) or (front, behind, top, bottom, left, right); -233 / -234 first: SAME on every axis -> (lo per axis, hi per axis)."""
    if isinstance(pads, int):
        pads = (pads,) * 6
    elif len(pads) == 3:
        pads = tuple(p for p in pads for _ in (0, 1))
    if pads[0] in (SAME_UPPER, SAME_LOWER):
        return (pads[0],) * 3, (0,) * 3
    return tuple(int(p) for p in pads[0::2]), tuple(int(p) for p in pads[1::2])


def conv3d_output_dim(extents, kernel, dilation=1, stride=1, pads=0):
    """-> ([(front, behind), (top, bottom), (left, right)], (Do, Ho, Wo)) with -233 / -234 resolved (fhip_conv3d_output_dim per axis)."""
    lo, hi = _pads(pads)
    return _dims(_lib.load_conv3d_library().fhip_conv3d_output_dim, "fhip_conv3d_output_dim", extents, _three(kernel), _three(dilation), _three(stride), lo, hi)


def pool3d_output_dim(extents, kernel, stride=1, pads=0, pad_mode: int = 0):
    """-> (pads per axis, (Do, Ho, Wo)) by ncnn's pad_mode (fhip_pool3d_output_dim per axis)."""
    lo, hi = _pads(pads)
    return _dims(_lib.load_conv3d_library().fhip_pool3d_output_dim, "fhip_pool3d_output_dim", extents, _three(kernel), _three(stride), lo, hi, int(pad_mode))


def _dense(t, rank, what):
    import torch
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or t.dim() != rank or not t.is_contiguous():
        raise ValueError(f"{what} must be a contiguous float32 CUDA tensor of rank {rank}")
    return tuple(t.shape)


def _at(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def pack_weights(w):
    """[K][C][kd][kh][kw] -> the packed buffer of the matrix kernel (fhip_conv3d_pack_weights)."""
    import torch
    k, c, kd, kh, kw = _dense(w, 5, "w")
    packed = torch.empty(kd * kh * kw * k * ((c + CHUNK - 1) // CHUNK * CHUNK), device=w.device, dtype=torch.float32)
    _check(_lib.load_conv3d_library().fhip_conv3d_pack_weights(c, k, kd, kh, kw, _at(w), _at(packed), _stream()), "fhip_conv3d_pack_weights")
    return packed


def conv3d(x, w, bias=None, stride=1, dilation=1, pads=0, pad_value: float = 0.0, group: int = 1, activation: int = 0, a0: float = 0.0, a1: float = 0.0,
           direct: bool = False, out=None, packed=None):
    """ncnn's Convolution3D / ConvolutionDepthWise3D of x [n][C][D][H][W] with w [K][C / group][kd][kh][kw] -> [n][K][Do][Ho][Wo]
    (fhip_conv3d_forward).  pads as _pads takes them; direct: run on the direct kernel whatever the route rule says; packed: what pack_weights gave for
    w (packed here, per call, without it)."""
    import torch
    n, c, d, h, wd = _dense(x, 5, "x")
    k, cg, kd, kh, kw = _dense(w, 5, "w")
    if group < 1 or c % group or cg != c // group:
        raise ValueError("x, w and group do not fit each other")
    if bias is not None and _dense(bias, 1, "bias") != (k,):
        raise ValueError("bias must be [K]")
    (dd, dh, dw), (sd, sh, sw) = _three(dilation), _three(stride)
    resolved, (od, oh, ow) = conv3d_output_dim((d, h, wd), (kd, kh, kw), dilation, stride, pads)
    if out is None:
        out = torch.empty((n, k, od, oh, ow), device=x.device, dtype=torch.float32)
    if _dense(out, 5, "out") != (n, k, od, oh, ow):
        raise ValueError(f"out must be [{n}][{k}][{od}][{oh}][{ow}]")
    lib = _lib.load_conv3d_library()
    if direct:
        packed = None
    elif packed is None and lib.fhip_conv3d_packed_floats(c, k, kd, kh, kw, dh, dw, sh, sw, group):
        packed = pack_weights(w)
    _check(lib.fhip_conv3d_forward(n, c, d, h, wd, k, kd, kh, kw, dd, dh, dw, sd, sh, sw, *[p for pair in resolved for p in pair], float(pad_value), int(group),
                                   int(activation), float(a0), float(a1), _at(x), _at(w), _at(packed), _at(bias), _at(out), od, oh, ow, _stream()), "fhip_conv3d_forward")
    return out


def pool3d(x, kernel=0, stride=1, pads=0, pad_mode: int = 0, avg: bool = False, count_include_pad: bool = False, global_: bool = False, out_dhw=None, out=None):
    """ncnn's Pooling3D of x [n][C][D][H][W] -> [n][C][Do][Ho][Wo] (fhip_pool3d_forward).  global_: one cell; out_dhw: adaptive onto that volume."""
    import torch
    n, c, d, h, w = _dense(x, 5, "x")
    if global_ or out_dhw is not None:
        kernel, resolved, outs = 0, [(0, 0)] * 3, [1, 1, 1] if global_ else [int(v) for v in out_dhw]
    else:
        resolved, outs = pool3d_output_dim((d, h, w), kernel, stride, pads, pad_mode)
    if out is None:
        out = torch.empty((n, c, *outs), device=x.device, dtype=torch.float32)
    if _dense(out, 5, "out") != (n, c, *outs):
        raise ValueError(f"out must be [{n}][{c}]{outs}")
    _check(_lib.load_conv3d_library().fhip_pool3d_forward(int(bool(avg)), n * c, d, h, w, *_three(kernel), *_three(stride), *[p for pair in resolved for p in pair],
                                                          int(bool(count_include_pad)), _at(x), _at(out), *outs, _stream()), "fhip_pool3d_forward")
    return out


def conv3d_route(c: int, k: int, kernel=1, dilation=1, stride=1, group: int = 1, direct: bool = False) -> str:
    """The kernel instantiation a convolution would launch (fhip_conv3d_route); k == 0 asks for the pooling."""
    name = ctypes.create_string_buffer(128)
    (kd, kh, kw), (_, dh, dw), (_, sh, sw) = _three(kernel), _three(dilation), _three(stride)
    _check(_lib.load_conv3d_library().fhip_conv3d_route(int(c), int(k), kd, kh, kw, dh, dw, sh, sw, int(group), int(bool(direct)), name, 128), "fhip_conv3d_route")
    return name.value.decode()
