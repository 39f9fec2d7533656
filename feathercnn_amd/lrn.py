"""Python host-side mirror of include/feather_hip/feather_lrn.h (``libfeather_lrn.so``): local response normalisation, alone and with the
Pooling layer behind it, on torch CUDA tensors.  Every call goes through the C-ABI on the current stream; there is no fallback path.
"""
from __future__ import annotations

import ctypes

from . import _lib
from .booster import FeatherHipError, _ptr, _stream

ACROSS_CHANNELS, WITHIN_CHANNEL = 0, 1
CHUNK = 16  # FHIP_LRN_CHUNK
POOL_LDS_FLOATS = 8192  # FHIP_LRN_POOL_LDS_FLOATS


_check = _lib.checker(_lib.load_lrn_library, "fhip_lrn_last_error")


def _f32(t, what):
    import torch
    if t.dtype != torch.float32 or not t.is_contiguous() or t.dim() != 4:
        raise ValueError(f"{what} must be a contiguous float32 tensor of 4 dimensions")


def _pool(x, pool):
    """(fhip_pool_param for x, output height, output width); `pool` = a fhip_pool_param (feathercnn_amd.net.pool_param) or a dict of
    pool_param's arguments after (c, h, w)."""
    from .net import pool_param
    n, c, h, w = x.shape
    q = pool_param(c, h, w, **pool) if isinstance(pool, dict) else pool
    oh, ow = ctypes.c_int(), ctypes.c_int()
    rc = _lib.load_library().fhip_pooling_output_dim(ctypes.byref(q), ctypes.byref(oh), ctypes.byref(ow))
    if rc != 0:
        raise FeatherHipError(f"fhip_pooling_output_dim failed with code {rc}")
    return q, oh.value, ow.value


def lrn(x, local_size: int = 5, alpha: float = 1.0, beta: float = 0.75, bias: float = 1.0, region: int = ACROSS_CHANNELS, out=None, chunk=None):
    """ncnn's LRN of a contiguous float32 [N][C][H][W] CUDA tensor (fhip_lrn_forward); not in place.  `chunk` (across channels only) gives
    the channel split instead of leaving it to the library (fhip_lrn_forward_chunked; 0 = no split): same bits."""
    import torch
    _f32(x, "x")
    n, c, h, w = x.shape
    if out is None:
        out = torch.empty_like(x)
    else:
        _f32(out, "out")
        if out.shape != x.shape:
            raise ValueError("out must have x's shape")
    lib = _lib.load_lrn_library()
    if chunk is None:
        _check(lib.fhip_lrn_forward(int(region), int(local_size), float(alpha), float(beta), float(bias), n, c, h, w, _ptr(out), _ptr(x), _stream()),
               "fhip_lrn_forward")
    else:
        if region != ACROSS_CHANNELS:
            raise ValueError("chunk applies across channels only")
        _check(lib.fhip_lrn_forward_chunked(int(local_size), float(alpha), float(beta), float(bias), n, c, h, w, int(chunk), _ptr(out), _ptr(x), _stream()),
               "fhip_lrn_forward_chunked")
    return out


def lrn_route(x, local_size: int = 5, region: int = ACROSS_CHANNELS, out=None) -> str:
    """The kernel instantiation lrn launches for these tensors (fhip_lrn_route); without `out`, an aligned one is assumed."""
    n, c, h, w = x.shape
    name = ctypes.create_string_buffer(96)
    _check(_lib.load_lrn_library().fhip_lrn_route(int(region), int(local_size), n, c, h, w, _ptr(out), _ptr(x), name, len(name)), "fhip_lrn_route")
    return name.value.decode()


def lrn_pool(x, pool, local_size: int = 5, alpha: float = 1.0, beta: float = 0.75, bias: float = 1.0, region: int = ACROSS_CHANNELS, out=None):
    """pooling(lrn(x)) in one launch that never writes the normalised tensor (fhip_lrn_pool_forward), bit for bit the two calls.  `pool`: see
    _pool; global pooling is refused."""
    import torch
    _f32(x, "x")
    n, c, h, w = x.shape
    q, oh, ow = _pool(x, pool)
    if out is None:
        out = torch.empty((n, c, max(oh, 0), max(ow, 0)), dtype=torch.float32, device=x.device)
    else:
        _f32(out, "out")
        if tuple(out.shape) != (n, c, oh, ow):
            raise ValueError("out must have the pooled shape")
    _check(_lib.load_lrn_library().fhip_lrn_pool_forward(int(region), int(local_size), float(alpha), float(beta), float(bias), n, c, h, w, ctypes.byref(q),
                                                         _ptr(out), _ptr(x), _stream()), "fhip_lrn_pool_forward")
    return out


def lrn_pool_route(x, pool, local_size: int = 5, region: int = ACROSS_CHANNELS, out=None) -> str:
    """The kernel instantiation lrn_pool launches for these tensors (fhip_lrn_pool_route)."""
    n, c, h, w = x.shape
    q, _, _ = _pool(x, pool)
    name = ctypes.create_string_buffer(96)
    _check(_lib.load_lrn_library().fhip_lrn_pool_route(int(region), int(local_size), n, c, h, w, ctypes.byref(q), _ptr(out), _ptr(x), name, len(name)),
           "fhip_lrn_pool_route")
    return name.value.decode()
