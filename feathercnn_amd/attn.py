"""Python host-side mirror of include/feather_hip/feather_attn.h (``libfeather_attn.so``): the layers of a Vision Transformer encoder -- the
attention core of ncnn's MultiHeadAttention, LayerNorm, GELU and the element-wise BinaryOp -- on torch CUDA tensors.  Every device call goes
through the C-ABI on the current stream; there is no fallback path.
"""
from __future__ import annotations

import ctypes

from . import _lib
from .booster import _ptr, _stream

NET_ROUTE = 113  # FHIP_ATTN_NET_ROUTE
MFMA_MAX_D, DIRECT_MAX_D, QUERY_TILE, KEY_TILE, LN_WAVE_MAX = 128, 4096, 64, 32, 256  # FHIP_ATTN_*
ADD, SUB, MUL, DIV, MAX, MIN = range(6)  # the binary ops (ncnn's BinaryOp 0=)
SCALAR, TENSOR, BROADCAST = range(3)  # the operand forms of fhip_binary_forward
ATTENTION, LAYER_NORM, GELU, BINARY = range(4)  # fhip_attn_op

_check = _lib.checker(_lib.load_attn_library, "fhip_attn_last_error")


def _f32(t, what):
    import torch
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32:
        raise ValueError(f"{what} must be a float32 CUDA tensor")


def _rows(t, what):
    """(n, T, E, row stride) of a [n][T][E] tensor whose rows are contiguous and equally spaced over (n, T): a dense tensor or a column
    slice of a fused [n][T][3E] projection."""
    _f32(t, what)
    if t.dim() != 3 or t.stride(2) != 1 or (t.shape[0] > 1 and t.stride(0) != t.shape[1] * t.stride(1)):
        raise ValueError(f"{what} must be [n][T][E] with unit column stride and equally spaced rows")
    return t.shape[0], t.shape[1], t.shape[2], t.stride(1)


def attention(q, k, v, heads: int, out=None):
    """softmax over the keys of q k^T, times v, per image and head (fhip_attention_forward).  q [n][Tq][E], k and v [n][Tk][E]; each may be a
    column slice of a fused projection (its row stride is passed on).  The caller has scaled q.  -> [n][Tq][E], dense."""
    import torch
    n, tq, e, qs = _rows(q, "q")
    nk, tk, ek, ks = _rows(k, "k")
    nv, tv, ev, vs = _rows(v, "v")
    if (nk, ek) != (n, e) or (nv, tv, ev) != (n, tk, e):
        raise ValueError("q, k and v must agree in batch and width, k and v in length")
    if out is None:
        out = torch.empty((n, tq, e), device=q.device, dtype=torch.float32)
    _f32(out, "out")
    if not out.is_contiguous() or tuple(out.shape) != (n, tq, e):
        raise ValueError("out must be a contiguous [n][Tq][E] tensor")
    at = lambda t: ctypes.c_void_p(t.data_ptr())  # (a column slice is no dense tensor: _rows has checked its strides)
    _check(_lib.load_attn_library().fhip_attention_forward(n, int(heads), tq, tk, e, at(q), qs, at(k), ks, at(v), vs, _ptr(out), _stream()),
           "fhip_attention_forward")
    return out


def _affine(t, l, what):
    if t is None:
        return None
    _f32(t, what)
    if not t.is_contiguous() or t.numel() != l:
        raise ValueError(f"{what} must hold one float per column")
    return _ptr(t)


def layer_norm(x, gamma=None, beta=None, eps: float = 1e-3, out=None):
    """LayerNorm over the last dimension of a contiguous float32 CUDA tensor (fhip_layer_norm_forward)."""
    import torch
    _f32(x, "x")
    if not x.is_contiguous():
        raise ValueError("x must be contiguous")
    l = x.shape[-1]
    out = torch.empty_like(x) if out is None else out
    _check(_lib.load_attn_library().fhip_layer_norm_forward(x.numel() // l, l, _affine(gamma, l, "gamma"), _affine(beta, l, "beta"), float(eps), _ptr(out), _ptr(x),
                                                            _stream()), "fhip_layer_norm_forward")
    return out


def add_layer_norm(a, b, gamma=None, beta=None, eps: float = 1e-3):
    """-> (a + b, LayerNorm(a + b)) in one launch (fhip_add_layer_norm_forward): bit for bit binary(ADD) then layer_norm."""
    import torch
    _f32(a, "a")
    _f32(b, "b")
    if not a.is_contiguous() or not b.is_contiguous() or a.shape != b.shape:
        raise ValueError("a and b must be contiguous and of one shape")
    l = a.shape[-1]
    s, y = torch.empty_like(a), torch.empty_like(a)
    _check(_lib.load_attn_library().fhip_add_layer_norm_forward(a.numel() // l, l, _affine(gamma, l, "gamma"), _affine(beta, l, "beta"), float(eps), _ptr(s), _ptr(y),
                                                                _ptr(a), _ptr(b), _stream()), "fhip_add_layer_norm_forward")
    return s, y


def gelu(x, fast: bool = False, out=None):
    """ncnn's GELU (0=fast_gelu) of a contiguous float32 CUDA tensor (fhip_gelu_forward)."""
    import torch
    _f32(x, "x")
    if not x.is_contiguous():
        raise ValueError("x must be contiguous")
    out = torch.empty_like(x) if out is None else out
    _check(_lib.load_attn_library().fhip_gelu_forward(int(bool(fast)), _ptr(out), _ptr(x), x.numel(), _stream()), "fhip_gelu_forward")
    return out


def binary(op: int, a, b, swap: bool = False, out=None):
    """ncnn's BinaryOp 0=op (ADD .. MIN) of a contiguous float32 CUDA tensor `a` and `b`: a Python number, a tensor of a's shape, or a tensor of
    one image's worth of a's elements, broadcast over the batch (fhip_binary_forward).  swap computes b op a."""
    import torch
    _f32(a, "a")
    if not a.is_contiguous():
        raise ValueError("a must be contiguous")
    out = torch.empty_like(a) if out is None else out
    if isinstance(b, (int, float)):
        form, pb, scalar, per = SCALAR, None, float(b), 0
    else:
        _f32(b, "b")
        if not b.is_contiguous():
            raise ValueError("b must be contiguous")
        form, pb, scalar, per = (TENSOR if b.numel() == a.numel() else BROADCAST), _ptr(b), 0.0, b.numel()
    _check(_lib.load_attn_library().fhip_binary_forward(int(op), form, int(bool(swap)), _ptr(out), _ptr(a), pb, scalar, a.numel(), per, _stream()),
           "fhip_binary_forward")
    return out


def attn_route(what: int, a: int = 0, b: int = 0) -> str:
    """The kernel instantiation a call would launch (fhip_attn_route): ATTENTION (a = E, b = heads), LAYER_NORM (a = L, b = with the add), GELU
    (a = fast, b = 16-byte aligned) or BINARY (a = form, b = 16-byte aligned)."""
    name = ctypes.create_string_buffer(128)
    _check(_lib.load_attn_library().fhip_attn_route(int(what), int(a), int(b), name, 128), "fhip_attn_route")
    return name.value.decode()
