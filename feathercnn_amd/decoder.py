"""Python host-side mirror of include/feather_hip/feather_decoder.h (``libfeather_decoder.so``): the layers of a decoder-only language model
-- masked scaled dot-product attention with grouped-query heads, a key/value cache and a split-KV route, key/value concatenation, RMSNorm,
rotary embedding and token embedding -- on torch CUDA tensors.  Every device call goes through the C-ABI on the current stream; there is no
fallback path.
"""
from __future__ import annotations

import ctypes
import math

from . import _lib
from .booster import _stream

NET_ROUTE = 120  # FHIP_DECODER_NET_ROUTE
MAX_D, KEY_TILE, ROW_TILES, MAX_SPLITS, RMS_WAVE_MAX = 128, 32, (32, 64, 128), 256, 256  # FHIP_DECODER_*
SPLIT_BLOCKS, SPLIT_TARGET, SPLIT_MIN_TILES = 128, 512, 2  # the auto rule of fhip_sdpa_get_buffer_size
SDPA, COMBINE, KV_CONCAT, RMS_NORM, ROTARY, EMBED = range(6)  # fhip_decoder_op

_check = _lib.checker(_lib.load_decoder_library, "fhip_decoder_last_error")

_INTS = ("n heads kv_heads tq tk d q_image_stride q_head_stride q_row_stride k_image_stride k_head_stride k_row_stride v_image_stride v_head_stride "
         "v_row_stride out_image_stride out_head_stride out_row_stride mask_image_stride mask_head_stride causal splits row_tile").split()


class SdpaDesc(ctypes.Structure):
    """fhip_sdpa_desc, field for field."""
    _fields_ = [(name, ctypes.c_int) for name in _INTS] + [("scale", ctypes.c_float)]


def route_rule(what: int, a: int = 0, b: int = 0, c: int = 0) -> str:
    """The rule of fhip_decoder_route restated for a call the library accepts."""
    if what == SDPA:
        tile = c or next(t for t in ROW_TILES if b <= t or t == ROW_TILES[-1])
        return "fhip::sdpa_kernel<%d, %d>" % ((a + 31) // 32, tile // 32)
    return {COMBINE: "fhip::sdpa_combine_kernel", KV_CONCAT: "fhip::kv_concat_kernel<%d>" % bool(a), RMS_NORM: "fhip::rms_norm_kernel<%d>" % (a > RMS_WAVE_MAX),
            ROTARY: "fhip::rotary_kernel<%d>" % a, EMBED: "fhip::embed_kernel"}[what]


def decoder_route(what: int, a: int = 0, b: int = 0, c: int = 0) -> str:
    """The kernel instantiation a call would launch (fhip_decoder_route): SDPA (a = d, b = group * tq, c = row_tile), COMBINE, KV_CONCAT
    (a = 16-byte accesses), RMS_NORM (a = L), ROTARY (a = interleaved) or EMBED."""
    name = ctypes.create_string_buffer(128)
    _check(_lib.load_decoder_library().fhip_decoder_route(int(what), int(a), int(b), int(c), name, 128), "fhip_decoder_route")
    return name.value.decode()


def sdpa_plan(desc: SdpaDesc):
    """-> (scratch bytes, splits) of a description (fhip_sdpa_get_buffer_size): no device call."""
    size, splits = ctypes.c_size_t(), ctypes.c_int()
    _check(_lib.load_decoder_library().fhip_sdpa_get_buffer_size(ctypes.byref(desc), ctypes.byref(size), ctypes.byref(splits)), "fhip_sdpa_get_buffer_size")
    return size.value, splits.value


def _f32(t, what, dim=None):
    import torch
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or (dim is not None and t.dim() != dim):
        raise ValueError(f"{what} must be a float32 CUDA tensor" + (f" of rank {dim}" if dim else ""))
    return ctypes.c_void_p(t.data_ptr())


def _dense(t, what, dim=None):
    p = _f32(t, what, dim)
    if not t.is_contiguous():
        raise ValueError(f"{what} must be contiguous")
    return p


def _strides(t, what):
    """(image, head, row) strides of a [n][heads][T][d] view with contiguous columns: a dense blob, a transposed view of a token-major
    projection buffer, a slice of a cache."""
    _f32(t, what, 4)
    if t.shape[3] > 1 and t.stride(3) != 1:
        raise ValueError(f"{what} must be [n][heads][T][d] with unit column stride")
    return t.stride(0) if t.shape[0] > 1 else 0, t.stride(1) if t.shape[1] > 1 else 0, t.stride(2) if t.shape[2] > 1 else t.shape[3]


def prepare_sdpa(q, k, v, mask=None, causal: bool = False, scale=None, splits: int = 0, row_tile: int = 0, out=None, scratch=None):
    """Everything of sdpa() but the launch -> (run, out): run() makes the C-ABI call on the tensors as they then are, on the current
    stream, and nothing else (what a decoding loop or a benchmark repeats)."""
    import torch
    n, heads, tq, d = q.shape
    nk, kv_heads, tk, dk = k.shape
    if (nk, dk) != (n, d) or tuple(v.shape) != tuple(k.shape):
        raise ValueError("q, k and v must agree in batch and width, k and v in shape")
    if out is None:
        out = torch.empty((n, heads, tq, d), device=q.device, dtype=torch.float32)
    if tuple(out.shape) != (n, heads, tq, d):
        raise ValueError("out must be [n][heads][Tq][d]")
    desc = SdpaDesc(n=n, heads=heads, kv_heads=kv_heads, tq=tq, tk=tk, d=d, causal=int(bool(causal)), splits=int(splits), row_tile=int(row_tile),
                    scale=float(1.0 / math.sqrt(d) if scale is None else scale))
    for name, t in (("q", q), ("k", k), ("v", v), ("out", out)):
        for part, stride in zip(("image", "head", "row"), _strides(t, name)):
            setattr(desc, f"{name}_{part}_stride", stride)
    pm = None
    if mask is not None:
        pm = _dense(mask, "mask")
        m4 = mask.reshape((1,) * (4 - mask.dim()) + tuple(mask.shape))
        if m4.shape[2:] != (tq, tk) or m4.shape[0] not in (1, n) or m4.shape[1] not in (1, heads):
            raise ValueError("mask must be [Tq][Tk], [heads or 1][Tq][Tk] or [n or 1][heads or 1][Tq][Tk]")
        desc.mask_image_stride = m4.stride(0) if m4.shape[0] > 1 else 0
        desc.mask_head_stride = m4.stride(1) if m4.shape[1] > 1 else 0
    size, _ = sdpa_plan(desc)
    if size and scratch is None:
        scratch = torch.empty(((size + 3) // 4,), device=q.device, dtype=torch.float32)
    if size and (scratch.numel() * 4 < size):
        raise ValueError(f"scratch must hold {size} bytes")
    fn, keep = _lib.load_decoder_library().fhip_sdpa_forward, (q, k, v, mask, out, scratch)  # the tensors live as long as the call does
    args = (ctypes.byref(desc), _f32(q, "q"), _f32(k, "k"), _f32(v, "v"), pm, _f32(out, "out"), _dense(scratch, "scratch") if size else None)

    def run(_keep=keep):
        _check(fn(*args, _stream()), "fhip_sdpa_forward")
    return run, out


def sdpa(q, k, v, mask=None, causal: bool = False, scale=None, splits: int = 0, row_tile: int = 0, out=None, scratch=None):
    """Scaled dot-product attention (fhip_sdpa_forward).  q [n][heads][Tq][d], k and v [n][kv_heads][Tk][d], each any view with contiguous
    columns; mask: None or additive float32 [Tq][Tk], [heads or 1][Tq][Tk] or [n or 1][heads or 1][Tq][Tk], dense; scale: 1 / sqrt(d) where
    None.  A row that sees no key gives zeros.  scratch: a float32 CUDA tensor of sdpa_plan()'s bytes; made where the call needs one and none
    is given.  -> out [n][heads][Tq][d] (dense where made here)."""
    run, out = prepare_sdpa(q, k, v, mask, causal, scale, splits, row_tile, out, scratch)
    run()
    return out


def kv_concat(past, fresh, out=None):
    """present = past followed by fresh along the tokens (fhip_kv_concat_forward): [n][kv_heads][Tp][d] (or None) and [n][kv_heads][Tn][d]
    -> [n][kv_heads][Tp + Tn][d], a bit copy."""
    import torch
    pf = _dense(fresh, "fresh", 4)
    n, kvh, tn, d = fresh.shape
    tp = 0 if past is None else past.shape[2]
    if past is not None and (tuple(past.shape[:2]) + (past.shape[3],)) != (n, kvh, d):
        raise ValueError("past and fresh must agree in batch, heads and width")
    if out is None:
        out = torch.empty((n, kvh, tp + tn, d), device=fresh.device, dtype=torch.float32)
    if tuple(out.shape) != (n, kvh, tp + tn, d):
        raise ValueError("out must be [n][kv_heads][Tp + Tn][d]")
    _check(_lib.load_decoder_library().fhip_kv_concat_forward(n, kvh, tp, tn, d, _dense(past, "past", 4) if tp else None, pf, _dense(out, "out"), _stream()),
           "fhip_kv_concat_forward")
    return out


def rms_norm(x, gamma=None, eps: float = 1e-6, out=None):
    """RMSNorm over the last dimension of a contiguous float32 CUDA tensor (fhip_rms_norm_forward)."""
    import torch
    px = _dense(x, "x")
    l = x.shape[-1]
    if gamma is not None and gamma.numel() != l:
        raise ValueError("gamma must hold one float per column")
    out = torch.empty_like(x) if out is None else out
    _check(_lib.load_decoder_library().fhip_rms_norm_forward(x.numel() // l, l, None if gamma is None else _dense(gamma, "gamma"), float(eps), _dense(out, "out"), px,
                                                             _stream()), "fhip_rms_norm_forward")
    return out


def rotary(x, cos, sin, interleaved: bool = False, out=None):
    """Rotary embedding of x [n][heads][T][d] with cos and sin [T][d / 2] (shared) or [n][T][d / 2] (fhip_rotary_forward); out may be x."""
    import torch
    px = _dense(x, "x", 4)
    n, heads, t, d = x.shape
    pc, ps = _dense(cos, "cos"), _dense(sin, "sin")
    if cos.shape != sin.shape or tuple(cos.shape) not in ((t, d // 2), (n, t, d // 2)):
        raise ValueError("cos and sin must be [T][d / 2] or [n][T][d / 2]")
    out = torch.empty_like(x) if out is None else out
    _check(_lib.load_decoder_library().fhip_rotary_forward(n, heads, t, d, int(bool(interleaved)), pc, ps, t * (d // 2) if cos.dim() == 3 else 0, _dense(out, "out"), px,
                                                           _stream()), "fhip_rotary_forward")
    return out


def embed(ids, weight, bias=None, out=None):
    """out[..., E] = weight[clamp(ids, 0, vocab - 1)] (+ bias) for int32 CUDA ids (fhip_embed_forward)."""
    import torch
    if not isinstance(ids, torch.Tensor) or not ids.is_cuda or ids.dtype != torch.int32 or not ids.is_contiguous():
        raise ValueError("ids must be a contiguous int32 CUDA tensor")
    pw = _dense(weight, "weight", 2)
    vocab, e = weight.shape
    if out is None:
        out = torch.empty(tuple(ids.shape) + (e,), device=weight.device, dtype=torch.float32)
    _check(_lib.load_decoder_library().fhip_embed_forward(ids.numel(), e, vocab, ctypes.c_void_p(ids.data_ptr()), pw, None if bias is None else _dense(bias, "bias"),
                                                          _dense(out, "out"), _stream()), "fhip_embed_forward")
    return out
