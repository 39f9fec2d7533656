"""Python host-side mirror of include/feather_hip/feather_dcn.h (``libfeather_dcn.so``): deformable convolution (DCN v1 / v2, ncnn's
DeformableConv2D) on torch CUDA tensors.  Every device call goes through the C-ABI on the current stream; there is no fallback path.
"""
from __future__ import annotations

import ctypes

from . import _lib
from .booster import _stream

NET_ROUTE = 116  # FHIP_DCN_NET_ROUTE
TILE_P, TILE_K_SMALL, TILE_K_LARGE, CHUNK_C = 64, 64, 128, 16  # FHIP_DCN_TILE_P, _TILE_K_SMALL, _TILE_K_LARGE, _CHUNK_C

_check = _lib.checker(_lib.load_dcn_library, "fhip_dcn_last_error")


def route_rule(c: int, k: int, kh: int = 3, kw: int = 3, g: int = 1) -> str:
    """The rule of fhip_dcn_route restated: the tile of 64 output channels where K <= 64, of 128 otherwise."""
    return "fhip::dcn_mfma_kernel<%d>" % (TILE_K_SMALL if k <= TILE_K_SMALL else TILE_K_LARGE)


def dcn_route(c: int, k: int, kh: int = 3, kw: int = 3, g: int = 1) -> str:
    """The kernel instantiation a forward would launch (fhip_dcn_route)."""
    name = ctypes.create_string_buffer(128)
    _check(_lib.load_dcn_library().fhip_dcn_route(int(c), int(k), int(kh), int(kw), int(g), name, 128), "fhip_dcn_route")
    return name.value.decode()


def _pair(v):
    return (int(v), int(v)) if isinstance(v, int) else (int(v[0]), int(v[1]))


def _pads(p):
    """(top, bottom, left, right) of an int, (vertical, horizontal) or the four."""
    if isinstance(p, int):
        return (p,) * 4
    return (p[0], p[0], p[1], p[1]) if len(p) == 2 else tuple(int(v) for v in p)


def dcn_output_dim(h: int, w: int, kernel, dilation=1, stride=1, pads=0):
    """-> (Ho, Wo) (fhip_dcn_output_dim).  kernel, dilation, stride: an int or (vertical, horizontal); pads: see deform_conv2d."""
    (kh, kw), (dh, dw), (sh, sw), (pt, pb, pl, pr) = _pair(kernel), _pair(dilation), _pair(stride), _pads(pads)
    ho, wo = ctypes.c_int(), ctypes.c_int()
    _check(_lib.load_dcn_library().fhip_dcn_output_dim(int(h), int(w), kh, kw, dh, dw, sh, sw, pt, pb, pl, pr, ctypes.byref(ho), ctypes.byref(wo)), "fhip_dcn_output_dim")
    return ho.value, wo.value


def _dense(t, what, dims):
    import torch
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or t.dim() != dims or not t.is_contiguous():
        raise ValueError(f"{what} must be a contiguous float32 CUDA tensor of {dims} dimensions")
    return t


def dcn_pack(w, offset_groups: int = 1):
    """ncnn's weights [K][C][kh][kw] -> the packed layout the kernel reads, [kh * kw][K][G][C / G rounded up to 16] (fhip_dcn_pack_weights)."""
    import torch
    k, c, kh, kw = _dense(w, "w", 4).shape
    lib = _lib.load_dcn_library()
    floats = lib.fhip_dcn_packed_floats(c, k, kh, kw, int(offset_groups))
    _check(0 if floats else -2, "fhip_dcn_packed_floats")  # 0 floats: refused (FHIP_E_BADARG), the reason in the last-error slot
    packed = torch.empty((floats,), device=w.device, dtype=torch.float32)
    _check(lib.fhip_dcn_pack_weights(c, k, kh, kw, int(offset_groups), ctypes.c_void_p(w.data_ptr()), ctypes.c_void_p(packed.data_ptr()), _stream()), "fhip_dcn_pack_weights")
    return packed


def deform_conv2d(x, offset, mask, w, bias=None, stride=1, dilation=1, pads=0, offset_groups: int = 1, activation: int = 0, a0: float = 0.0, a1: float = 0.0,
                  out=None, packed=None):
    """The deformable convolution of x [n][C][H][W] with w [K][C][kh][kw] at offset [n][G * 2 * kh * kw][Ho][Wo] and mask
    [n][G * kh * kw][Ho][Wo] (None: DCN v1) -> [n][K][Ho][Wo] (fhip_dcn_forward).  stride, dilation: an int or (vertical, horizontal); pads: an
    int, (vertical, horizontal) or (top, bottom, left, right).  packed: dcn_pack(w, offset_groups) from an earlier call, which is then not
    repeated."""
    import torch
    n, c, h, wd = _dense(x, "x", 4).shape
    k, cw, kh, kw = _dense(w, "w", 4).shape
    g = int(offset_groups)
    if cw != c:
        raise ValueError("w must be [K][C][kh][kw] for the C of x: the convolution group is 1")
    ho, wo = dcn_output_dim(h, wd, (kh, kw), dilation, stride, pads)
    if tuple(_dense(offset, "offset", 4).shape) != (n, g * 2 * kh * kw, ho, wo):
        raise ValueError(f"offset must be [{n}][{g * 2 * kh * kw}][{ho}][{wo}]")
    if mask is not None and tuple(_dense(mask, "mask", 4).shape) != (n, g * kh * kw, ho, wo):
        raise ValueError(f"mask must be [{n}][{g * kh * kw}][{ho}][{wo}]")
    if bias is not None and tuple(_dense(bias, "bias", 1).shape) != (k,):
        raise ValueError("bias must be [K]")
    if packed is None:
        packed = dcn_pack(w, g)
    if out is None:
        out = torch.empty((n, k, ho, wo), device=x.device, dtype=torch.float32)
    if tuple(_dense(out, "out", 4).shape) != (n, k, ho, wo):
        raise ValueError(f"out must be [{n}][{k}][{ho}][{wo}]")
    (dh, dw), (sh, sw), (pt, pb, pl, pr) = _pair(dilation), _pair(stride), _pads(pads)
    at = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    _check(_lib.load_dcn_library().fhip_dcn_forward(n, c, h, wd, k, kh, kw, dh, dw, sh, sw, pt, pb, pl, pr, g, int(activation), float(a0), float(a1), at(x), at(offset),
                                                    at(mask), at(_dense(packed, "packed", 1)), at(bias), at(out), ho, wo, _stream()), "fhip_dcn_forward")
    return out
