"""Python host-side mirror of include/feather_hip/feather_stft.h (``libfeather_stft.so``): ncnn's Spectrogram (the short-time Fourier
transform on the matrix pipe) and UnaryOp on torch CUDA tensors.  Every device call goes through the C-ABI on the current stream; there is
no fallback path.
"""
from __future__ import annotations

import ctypes
import functools

import numpy as np

from . import _lib
from .booster import _stream

NET_ROUTE = 118  # FHIP_STFT_NET_ROUTE
MAX_NFFT, TILE_F, TILE_J, CHUNK = 4096, 64, 128, 32  # FHIP_STFT_MAX_NFFT, _TILE_F, _TILE_J, _CHUNK
UNARY_OPS = {"abs": 0, "neg": 1, "square": 4, "sqrt": 5, "rsqrt": 6, "exp": 7, "log": 8, "reciprocal": 15, "log10": 17}  # FHIP_UNARY_*

_check = _lib.checker(_lib.load_stft_library, "fhip_stft_last_error")


def route_rule(what: int, a: int, b: int) -> str:
    """The rule of fhip_stft_route restated for a call the library accepts: what 0 a Spectrogram (n_fft a, hoplen b), 1 a UnaryOp (op a,
    b: both pointers 16-byte aligned)."""
    return "fhip::stft_mfma_kernel" if what == 0 else "fhip::unary_kernel<%d>" % (1 if b else 0)


def stft_route(what: int, a: int, b: int) -> str:
    """The kernel instantiation a call would launch (fhip_stft_route)."""
    name = ctypes.create_string_buffer(128)
    _check(_lib.load_stft_library().fhip_stft_route(int(what), int(a), int(b), name, 128), "fhip_stft_route")
    return name.value.decode()


def output_shape(n: int, l: int, n_fft: int, power: int = 0, hoplen=None, center: bool = True, pad_type: int = 2, onesided: bool = True):
    """The shape of spectrogram()'s result (fhip_stft_output_dim): (n, freqs, frames, 2) for power 0, else (n, freqs, frames)."""
    freqs, frames = ctypes.c_int(), ctypes.c_int()
    hop = n_fft // 4 if hoplen is None else hoplen
    _check(_lib.load_stft_library().fhip_stft_output_dim(int(l), int(n_fft), int(hop), int(bool(center)), int(pad_type), int(bool(onesided)), ctypes.byref(freqs),
                                                         ctypes.byref(frames)), "fhip_stft_output_dim")
    return (n, freqs.value, frames.value, 2) if power == 0 else (n, freqs.value, frames.value)


def basis(n_fft: int, winlen=None, window_type: int = 0, normalized: int = 0, onesided: bool = True) -> np.ndarray:
    """The host basis [2 freqs][n_fft] in float32 (fhip_stft_basis): no device call."""
    freqs = n_fft // 2 + 1 if onesided else n_fft
    out = np.empty((2 * max(freqs, 1), max(n_fft, 1)), np.float32)
    _check(_lib.load_stft_library().fhip_stft_basis(int(n_fft), int(n_fft if winlen is None else winlen), int(window_type), int(normalized), int(bool(onesided)),
                                                    out.ctypes.data_as(ctypes.c_void_p), out.size), "fhip_stft_basis")
    return out


@functools.lru_cache(maxsize=8)
def _device_basis(device, *key):
    import torch
    return torch.from_numpy(basis(*key)).to(device)


def _floats(t, what, dim=None):
    import torch
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous() or (dim is not None and t.dim() != dim):
        raise ValueError(f"{what} must be a contiguous float32 CUDA tensor" + (f" of rank {dim}" if dim else ""))
    return ctypes.c_void_p(t.data_ptr())


def spectrogram(x, n_fft: int, power: int = 0, hoplen=None, winlen=None, window_type: int = 0, center: bool = True, pad_type: int = 2, normalized: int = 0,
                onesided: bool = True, device_basis=None, out=None):
    """ncnn's Spectrogram of x [n][L] -> [n][freqs][frames][2] (power 0) or [n][freqs][frames] (fhip_stft_forward).  device_basis: the device
    copy of basis(...) for the same window; made and kept (the last eight) where it is not given."""
    import torch
    px = _floats(x, "x", 2)
    n, l = x.shape
    hop = n_fft // 4 if hoplen is None else hoplen
    shape = output_shape(n, l, n_fft, power, hop, center, pad_type, onesided)
    if device_basis is None:
        device_basis = _device_basis(x.device, int(n_fft), None if winlen is None else int(winlen), int(window_type), int(normalized), bool(onesided))
    if out is None:
        out = torch.empty(shape, device=x.device, dtype=torch.float32)
    if tuple(out.shape) != shape:
        raise ValueError(f"out must be {shape}")
    _check(_lib.load_stft_library().fhip_stft_forward(n, l, int(n_fft), int(power), int(hop), int(bool(center)), int(pad_type), int(bool(onesided)), px,
                                                      _floats(device_basis, "device_basis", 2), _floats(out, "out"), shape[2], _stream()), "fhip_stft_forward")
    return out


def unary(op, x, out=None):
    """ncnn's UnaryOp (fhip_unary_forward): op an id or a name of UNARY_OPS; out may be x (in place)."""
    import torch
    op = UNARY_OPS.get(op, op)
    px = _floats(x, "x")
    if out is None:
        out = torch.empty_like(x)
    if out.shape != x.shape:
        raise ValueError("out must have x's shape")
    _check(_lib.load_stft_library().fhip_unary_forward(int(op), _floats(out, "out"), px, x.numel(), _stream()), "fhip_unary_forward")
    return out
