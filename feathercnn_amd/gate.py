"""Python host-side mirror of include/feather_hip/feather_gate.h (``libfeather_gate.so``): squeeze-and-excitation channel gating, Swish and
HardSigmoid on torch CUDA tensors.  Every call goes through the C-ABI on the current stream; there is no fallback path.
"""
from __future__ import annotations

import ctypes

from . import _lib
from .booster import _ptr, _stream

ACT_NONE, ACT_RELU = 0, 1
SWISH, HARDSIGMOID = 0, 1
KINDS = {"swish": SWISH, "hard_sigmoid": HARDSIGMOID}
MACTS = {None: 0, "none": 0, "relu": 1, "swish": 2}
GACTS = {"sigmoid": 0, "hard_sigmoid": 1}
OP_APPLY, OP_SQUEEZE, OP_EXCITE, OP_ACTIVATION = range(4)
OPS = {"apply": OP_APPLY, "squeeze": OP_SQUEEZE, "excite": OP_EXCITE, "activation": OP_ACTIVATION}


_check = _lib.checker(_lib.load_gate_library, "fhip_gate_last_error")


def _f32(t, what, dims=None):
    import torch
    if t.dtype != torch.float32 or not t.is_contiguous() or (dims is not None and t.dim() != dims):
        raise ValueError(f"{what} must be a contiguous float32 tensor" + (f" of {dims} dimensions" if dims else ""))


def channel_gate(x, gate, residual=None, relu: bool = False, out=None):
    """out = act(x * gate[n][c] [+ residual]) for a contiguous float32 [N][C][H][W] CUDA tensor and a gate of N * C values; the product
    and the sum are rounded separately.  out may be x or residual."""
    import torch
    _f32(x, "x", 4)
    _f32(gate, "gate")
    n, c, h, w = x.shape
    if gate.numel() != n * c:
        raise ValueError("gate must hold one value per (n, c) plane")
    if residual is not None:
        _f32(residual, "residual", 4)
        if residual.shape != x.shape:
            raise ValueError("residual must have x's shape")
    if out is None:
        out = torch.empty_like(x)
    _check(_lib.load_gate_library().fhip_channel_gate_forward(n, c, h, w, _ptr(out), _ptr(x), _ptr(gate), _ptr(residual), int(bool(relu)), _stream()),
           "fhip_channel_gate_forward")
    return out


def squeeze_scratch_bytes(shape) -> int:
    """Bytes of scratch squeeze needs for an [N][C][H][W] tensor (0 unless the plane takes the split route)."""
    n, c, h, w = shape
    b = ctypes.c_size_t()
    _check(_lib.load_gate_library().fhip_squeeze_get_buffer_size(n, c, h, w, ctypes.byref(b)), "fhip_squeeze_get_buffer_size")
    return b.value


def squeeze(x, out=None, scratch=None):
    """mean[n][c] of a contiguous float32 [N][C][H][W] CUDA tensor, as [N][C][1][1]; `scratch` is allocated here when the shape needs one
    and none is given."""
    import torch
    _f32(x, "x", 4)
    n, c, h, w = x.shape
    if out is None:
        out = torch.empty((n, c, 1, 1), dtype=torch.float32, device=x.device)
    need = squeeze_scratch_bytes(x.shape)
    if need and scratch is None:
        scratch = torch.empty(need // 4, dtype=torch.float32, device=x.device)
    if need and (scratch.dtype != torch.float32 or not scratch.is_contiguous() or scratch.numel() * 4 < need):
        raise ValueError(f"scratch must be a contiguous float32 tensor of at least {need} bytes")
    _check(_lib.load_gate_library().fhip_squeeze_forward(n, c, h, w, _ptr(out), _ptr(x), _ptr(scratch) if need else None, _stream()),
           "fhip_squeeze_forward")
    return out


def excite(mean, w1, b1, w2, b2, mact="relu", gact="sigmoid", alpha: float = 0.2, beta: float = 0.5, out=None, slices=None):
    """gate = gact(W2 . mact(W1 . mean + b1) + b2) per image: mean holds N * C values, w1 is [R][C], w2 [C][R], b1 / b2 [R] / [C] or None.
    Returns [N][C][1][1].  `slices` deals the output channels of an image out to that many blocks (fhip_excite_forward_slices)."""
    import torch
    for t, what in ((mean, "mean"), (w1, "w1"), (w2, "w2")):
        _f32(t, what)
    r, c = w1.shape[0], w1.numel() // w1.shape[0]
    n = mean.numel() // c
    if mean.numel() != n * c or w2.numel() != c * r or w2.shape[0] != c:
        raise ValueError("mean must be [N][C], w1 [R][C] and w2 [C][R]")
    for b, k, what in ((b1, r, "b1"), (b2, c, "b2")):
        if b is not None:
            _f32(b, what)
            if b.numel() != k:
                raise ValueError(f"{what} has the wrong size")
    if out is None:
        out = torch.empty((n, c, 1, 1), dtype=torch.float32, device=mean.device)
    lib = _lib.load_gate_library()
    args = (n, c, r, _ptr(out), _ptr(mean), _ptr(w1), _ptr(b1), _ptr(w2), _ptr(b2), MACTS[mact], GACTS[gact], float(alpha), float(beta), _stream())
    if slices is None:
        _check(lib.fhip_excite_forward(*args), "fhip_excite_forward")
    else:
        _check(lib.fhip_excite_forward_slices(int(slices), *args), "fhip_excite_forward_slices")
    return out


def gate_activation(x, kind, alpha: float = 0.2, beta: float = 0.5, out=None):
    """Element-wise "swish" or "hard_sigmoid" (alpha, beta) of a contiguous float32 [N][C][...] CUDA tensor; out may be x."""
    import torch
    if x.dim() < 2:
        raise ValueError("gate_activation needs a contiguous float32 [N][C][...] tensor")
    _f32(x, "x")
    k = KINDS[kind] if isinstance(kind, str) else int(kind)
    n, c = x.shape[:2]
    hw = x.numel() // (n * c) if x.numel() else 0
    if out is None:
        out = torch.empty_like(x)
    _check(_lib.load_gate_library().fhip_gate_activation_forward(k, _ptr(out), _ptr(x), n, c, hw, float(alpha), float(beta), _stream()),
           "fhip_gate_activation_forward")
    return out


def gate_route(op, x, out=None, residual=None) -> str:
    """The kernel instantiation the entry `op` ("apply", "squeeze", "excite", "activation") launches for these tensors (fhip_gate_route)."""
    n, c = x.shape[:2]
    h, w = (x.shape[2], x.shape[3]) if x.dim() == 4 else (x.numel() // (n * c), 1)
    name = ctypes.create_string_buffer(96)
    _check(_lib.load_gate_library().fhip_gate_route(OPS[op], n, c, h, w, _ptr(x if out is None else out), _ptr(x), _ptr(residual), name, len(name)),
           "fhip_gate_route")
    return name.value.decode()
