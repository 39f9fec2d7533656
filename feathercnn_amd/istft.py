"""Python host-side mirror of include/feather_hip/feather_istft.h (``libfeather_istft.so``): ncnn's InverseSpectrogram (the inverse short-time
Fourier transform, its overlap-add a gather on the matrix pipe) on torch CUDA tensors.  Every device call goes through the C-ABI on the
current stream; there is no fallback path.
"""
from __future__ import annotations

import ctypes
import functools

import numpy as np

from . import _lib
from .booster import _stream

NET_ROUTE = 119  # FHIP_ISTFT_NET_ROUTE
MAX_NFFT, TILE_Q, TILE_R, CHUNK, TAPS = 4096, 128, 64, 16, 4  # FHIP_ISTFT_MAX_NFFT, _TILE_Q, _TILE_R, _CHUNK, _TAPS

_check = _lib.checker(_lib.load_istft_library, "fhip_istft_last_error")


def route_rule(n_fft: int, hoplen: int) -> str:
    """The rule of fhip_istft_route restated for a call the library accepts: there is one kernel."""
    return "fhip::istft_mfma_kernel"


def istft_route(n_fft: int, hoplen: int) -> str:
    """The kernel a call would launch (fhip_istft_route)."""
    name = ctypes.create_string_buffer(128)
    _check(_lib.load_istft_library().fhip_istft_route(int(n_fft), int(hoplen), name, 128), "fhip_istft_route")
    return name.value.decode()


def _hop(n_fft, hoplen):
    return n_fft // 4 if hoplen is None else hoplen


def output_length(frames: int, n_fft: int, hoplen=None, center: bool = True) -> int:
    """out_len of inverse_spectrogram()'s rows (fhip_istft_output_dim)."""
    out = ctypes.c_int()
    _check(_lib.load_istft_library().fhip_istft_output_dim(int(frames), int(n_fft), int(_hop(n_fft, hoplen)), int(bool(center)), ctypes.byref(out)), "fhip_istft_output_dim")
    return out.value


def basis(n_fft: int, winlen=None, window_type: int = 0, normalized: int = 0, onesided: bool = True) -> np.ndarray:
    """The host basis [n_fft][2 freqs] in float32 (fhip_istft_basis): no device call."""
    freqs = n_fft // 2 + 1 if onesided else n_fft
    out = np.empty((max(n_fft, 1), 2 * max(freqs, 1)), np.float32)
    _check(_lib.load_istft_library().fhip_istft_basis(int(n_fft), int(n_fft if winlen is None else winlen), int(window_type), int(normalized), int(bool(onesided)),
                                                      out.ctypes.data_as(ctypes.c_void_p), out.size), "fhip_istft_basis")
    return out


def envelope(frames: int, n_fft: int, hoplen=None, winlen=None, window_type: int = 0, center: bool = True) -> np.ndarray:
    """The host inverse envelope [out_len] in float32 (fhip_istft_envelope): no device call.  Refuses a kept envelope sample below 1e-11."""
    hop = _hop(n_fft, hoplen)
    out = np.empty(output_length(frames, n_fft, hop, center), np.float32)
    _check(_lib.load_istft_library().fhip_istft_envelope(int(frames), int(n_fft), int(hop), int(n_fft if winlen is None else winlen), int(window_type), int(bool(center)),
                                                         out.ctypes.data_as(ctypes.c_void_p), out.size), "fhip_istft_envelope")
    return out


@functools.lru_cache(maxsize=8)
def _device_basis(device, *key):
    import torch
    return torch.from_numpy(basis(*key)).to(device)


@functools.lru_cache(maxsize=8)
def _device_envelope(device, *key):
    import torch
    return torch.from_numpy(envelope(*key)).to(device)


def _floats(t, what, dim=None):
    import torch
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous() or (dim is not None and t.dim() != dim):
        raise ValueError(f"{what} must be a contiguous float32 CUDA tensor" + (f" of rank {dim}" if dim else ""))
    return ctypes.c_void_p(t.data_ptr())


def inverse_spectrogram(x, n_fft: int, hoplen=None, winlen=None, window_type: int = 0, center: bool = True, normalized: int = 0, onesided: bool = True,
                        device_basis=None, device_envelope=None, out=None):
    """ncnn's InverseSpectrogram of x [n][freqs][frames][2] -> [n][out_len] (fhip_istft_forward).  device_basis, device_envelope: the device
    copies of basis(...) and envelope(...) for the same arguments; made and kept (the last eight) where they are not given."""
    import torch
    px = _floats(x, "x", 4)
    n, freqs, frames, two = x.shape
    if two != 2 or freqs != (n_fft // 2 + 1 if onesided else n_fft):
        raise ValueError("x must be [n][freqs][frames][2] with freqs = n_fft // 2 + 1 (onesided) or n_fft")
    hop = _hop(n_fft, hoplen)
    out_len = output_length(frames, n_fft, hop, center)
    win = None if winlen is None else int(winlen)
    if device_basis is None:
        device_basis = _device_basis(x.device, int(n_fft), win, int(window_type), int(normalized), bool(onesided))
    if device_envelope is None:
        device_envelope = _device_envelope(x.device, int(frames), int(n_fft), int(hop), win, int(window_type), bool(center))
    if out is None:
        out = torch.empty((n, out_len), device=x.device, dtype=torch.float32)
    if tuple(out.shape) != (n, out_len):
        raise ValueError(f"out must be {(n, out_len)}")
    _check(_lib.load_istft_library().fhip_istft_forward(n, frames, int(n_fft), int(hop), int(bool(center)), int(bool(onesided)), px, _floats(device_basis, "device_basis", 2),
                                                        _floats(device_envelope, "device_envelope", 1), _floats(out, "out"), out_len, _stream()), "fhip_istft_forward")
    return out
