"""Python host-side mirror of include/feather_hip/feather_rnn.h (``libfeather_rnn.so``): the recurrent core of ncnn's LSTM, GRU and RNN layers
on torch CUDA tensors.  Every device call goes through the C-ABI on the current stream; there is no fallback path.
"""
from __future__ import annotations

import ctypes

from . import _lib
from .booster import _stream

NET_ROUTE = 114  # FHIP_RNN_NET_ROUTE
LSTM, GRU, RNN = range(3)  # FHIP_RNN_LSTM, FHIP_RNN_GRU, FHIP_RNN_RNN
GATES = {LSTM: 4, GRU: 3, RNN: 1}
ROUTE_AUTO, ROUTE_STEP, ROUTE_SEQUENCE = range(3)  # FHIP_RNN_ROUTE_*
UNIT_TILE, SEQ_TILE, MFMA_MULTIPLE, SEQUENCE_TILE = 32, 32, 4, 4  # FHIP_RNN_UNIT_TILE, _SEQ_TILE, _MFMA_MULTIPLE, _SEQUENCE_TILE
SEQUENCE_LDS_FLOATS = 40960  # FHIP_RNN_SEQUENCE_LDS_FLOATS
SEQUENCE_MAX_H = {LSTM: 100, GRU: 115, RNN: 198}  # FHIP_RNN_SEQUENCE_MAX_H_LSTM, _GRU, _RNN
SEQUENCE_MAX_N = 256  # FHIP_RNN_SEQUENCE_MAX_N

_check = _lib.checker(_lib.load_rnn_library, "fhip_rnn_last_error")


def _f32(t, what, shape=None):
    import torch
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32:
        raise ValueError(f"{what} must be a float32 CUDA tensor")
    if shape is not None and (tuple(t.shape) != tuple(shape) or not t.is_contiguous()):
        raise ValueError(f"{what} must be a contiguous tensor of shape {tuple(shape)}")


def _rows(t, what):
    """(n, T, width, row stride) of a [n][T][width] tensor with unit column stride and equally spaced rows."""
    _f32(t, what)
    if t.dim() != 3 or t.stride(2) != 1 or (t.shape[0] > 1 and t.stride(0) != t.shape[1] * t.stride(1)):
        raise ValueError(f"{what} must be [n][T][width] with unit column stride and equally spaced rows")
    return t.shape[0], t.shape[1], t.shape[2], t.stride(1)


def recurrent(cell: int, xp, wh, direction: int = 0, bn=None, h0=None, c0=None, out=None, states: bool = False, route: int = ROUTE_AUTO):
    """The recurrence of an LSTM, GRU or RNN over the input projections xp [n][T][nd * G * H] (bias added; may be a view with a larger row
    stride) with the recurrent weights wh [nd][G * H][H] (fhip_rnn_forward_route).  bn [nd][H]: the GRU's BN bias row.  h0, c0: None or
    [n][nd][H].  -> out [n][T][nd * H], or (out, hn, cn) with states (cn None unless LSTM)."""
    import torch
    n, t, width, xs = _rows(xp, "xp")
    _f32(wh, "wh")
    if wh.dim() != 3 or not wh.is_contiguous():
        raise ValueError("wh must be a contiguous [nd][G * H][H] tensor")
    nd, h = wh.shape[0], wh.shape[2]
    if cell not in GATES or nd != (2 if direction == 2 else 1) or wh.shape[1] != GATES[cell] * h or width != nd * GATES[cell] * h:
        raise ValueError("cell, direction, xp and wh do not fit each other")
    if cell == GRU:
        _f32(bn, "bn", (nd, h))
    for s, what in ((h0, "h0"), (c0, "c0")):
        if s is not None:
            _f32(s, what, (n, nd, h))
    if out is None:
        out = torch.empty((n, t, nd * h), device=xp.device, dtype=torch.float32)
    _, _, ow, os_ = _rows(out, "out")
    if tuple(out.shape[:2]) != (n, t) or ow != nd * h:
        raise ValueError("out must be [n][T][nd * H]")
    hn = torch.empty((n, nd, h), device=xp.device, dtype=torch.float32) if states else None
    cn = torch.empty((n, nd, h), device=xp.device, dtype=torch.float32) if states and cell == LSTM else None
    scratch = torch.empty((nd, n, h), device=xp.device, dtype=torch.float32) if cell == LSTM else None
    at = lambda x: None if x is None else ctypes.c_void_p(x.data_ptr())  # (views: _rows has checked their strides)
    _check(_lib.load_rnn_library().fhip_rnn_forward_route(int(cell), int(direction), n, t, h, at(xp), xs, at(wh), at(bn) if cell == GRU else None, at(h0),
                                                          at(c0) if cell == LSTM else None, at(out), os_, at(hn), at(cn), at(scratch), _stream(), int(route)),
           "fhip_rnn_forward")
    return (out, hn, cn) if states else out


def sequence_fits(cell: int, h: int) -> bool:
    """Whether Wh and the state of the sequence route fit the chip's LDS (fhip_rnn_sequence_fits)."""
    return bool(_lib.load_rnn_library().fhip_rnn_sequence_fits(int(cell), int(h)))


def rnn_route(cell: int, h: int, n: int = 1, t: int = 1, route: int = ROUTE_AUTO) -> str:
    """The kernel instantiation a call would launch (fhip_rnn_route), T times on the step route."""
    name = ctypes.create_string_buffer(128)
    _check(_lib.load_rnn_library().fhip_rnn_route(int(cell), int(h), int(n), int(t), int(route), name, 128), "fhip_rnn_route")
    return name.value.decode()
