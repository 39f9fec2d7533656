"""Python host-side mirror of include/feather_hip/feather_detect.h (``libfeather_detect.so``): the layers of an SSD detection head --
Permute, Normalize, a softmax along any axis, PriorBox (on the host) and DetectionOutput -- on torch CUDA tensors.  Every device call goes
through the C-ABI on the current stream; there is no fallback path.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from .booster import _ptr, _stream

NET_ROUTE = 109  # FHIP_DETECT_NET_ROUTE
MAX_PRIORS, MAX_CLASSES, MAX_TOP_K, CHUNK, PERMUTE_CONCAT_MAX = 1 << 22, 256, 1024, 1024, 8
PERMUTE, NORMALIZE, SOFTMAX, SELECT, MERGE, PERMUTE_CONCAT = range(6)  # fhip_detect_op

_check = _lib.checker(_lib.load_detect_library, "fhip_detect_last_error")


def _f32(t, what):
    import torch
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise ValueError(f"{what} must be a contiguous float32 tensor")


def permute_output_dim(order_type: int, dims: int, c: int, h: int, w: int):
    """(c, h, w) of Permute's output for an input (c, h, w) of rank `dims` (fhip_permute_output_dim)."""
    o = [ctypes.c_int() for _ in range(3)]
    _check(_lib.load_detect_library().fhip_permute_output_dim(int(order_type), int(dims), c, h, w, *[ctypes.byref(v) for v in o]), "fhip_permute_output_dim")
    return tuple(v.value for v in o)


def permute(x, order_type: int, out=None):
    """ncnn's Permute of a contiguous float32 CUDA tensor [N][C][H][W] (rank 3) or [N][H][W] (rank 2), image by image (fhip_permute_forward)."""
    import torch
    _f32(x, "x")
    if x.dim() not in (3, 4):
        raise ValueError("x must be [N][C][H][W] or [N][H][W]")
    dims = x.dim() - 1
    n, (c, h, w) = x.shape[0], ((1,) + tuple(x.shape[1:]) if dims == 2 else tuple(x.shape[1:]))
    oc, oh, ow = permute_output_dim(order_type, dims, c, h, w)
    shape = (n, oc, oh, ow) if dims == 3 else (n, oh, ow)
    if out is None:
        out = torch.empty(shape, device=x.device, dtype=torch.float32)
    _check(_lib.load_detect_library().fhip_permute_forward(int(order_type), dims, n, c, h, w, _ptr(out), _ptr(x), _stream()), "fhip_permute_forward")
    return out


def permute_concat(xs, out=None):
    """Concat of Flatten of Permute(order 3) of up to 8 contiguous float32 [N][C][H][W] CUDA tensors, in one launch: [N][sum of C*H*W]
    (fhip_permute_concat_forward)."""
    import torch
    for x in xs:
        _f32(x, "a source")
    n = xs[0].shape[0]
    k = len(xs)
    c = (ctypes.c_int * k)(*[x.shape[1] for x in xs])
    hw = (ctypes.c_int * k)(*[x.shape[2] * x.shape[3] for x in xs])
    ptrs = (ctypes.c_void_p * k)(*[x.data_ptr() for x in xs])
    if out is None:
        out = torch.empty((n, sum(x[0].numel() for x in xs)), device=xs[0].device, dtype=torch.float32)
    _check(_lib.load_detect_library().fhip_permute_concat_forward(k, c, hw, n, _ptr(out), ptrs, _stream()), "fhip_permute_concat_forward")
    return out


def normalize(x, scale, eps: float = 1e-10, channel_shared: bool = False, out=None):
    """ncnn's Normalize in its SSD form (across channels, per pixel) of a contiguous float32 [N][C][H][W] CUDA tensor; `scale`: C floats, or one
    with channel_shared (fhip_normalize_forward)."""
    import torch
    _f32(x, "x")
    _f32(scale, "scale")
    n, c, h, w = x.shape
    if scale.numel() != (1 if channel_shared else c):
        raise ValueError("scale must hold one value per channel (one value with channel_shared)")
    if out is None:
        out = torch.empty_like(x)
    _check(_lib.load_detect_library().fhip_normalize_forward(n, c, h, w, int(bool(channel_shared)), float(eps), _ptr(out), _ptr(x), _ptr(scale), _stream()),
           "fhip_normalize_forward")
    return out


def axis_softmax(x, axis: int, out=None):
    """Softmax of a contiguous float32 CUDA tensor along `axis` (fhip_axis_softmax_forward)."""
    import torch
    _f32(x, "x")
    axis = axis + x.dim() if axis < 0 else axis
    outer = int(np.prod(x.shape[:axis], dtype=np.int64))
    inner = int(np.prod(x.shape[axis + 1:], dtype=np.int64))
    if out is None:
        out = torch.empty_like(x)
    _check(_lib.load_detect_library().fhip_axis_softmax_forward(outer, x.shape[axis], inner, _ptr(out), _ptr(x), _stream()), "fhip_axis_softmax_forward")
    return out


def priorbox(h: int, w: int, image_w: int, image_h: int, min_sizes, max_sizes=(), aspect_ratios=(), variances=(0.1, 0.1, 0.2, 0.2), flip: bool = True,
             clip: bool = False, step_w: float = 0.0, step_h: float = 0.0, offset: float = 0.5) -> np.ndarray:
    """ncnn's PriorBox for a feature map of h x w cells, on the host: a float32 array [2][4 * h * w * num_prior] (fhip_priorbox_fill; needs no
    device).  step <= 0: image extent / feature extent."""
    def arr(v):
        a = np.ascontiguousarray(np.asarray(v, dtype=np.float32).reshape(-1))
        return a, (a.ctypes.data_as(ctypes.POINTER(ctypes.c_float)) if a.size else None)
    mn, mnp = arr(min_sizes)
    mx, mxp = arr(max_sizes)
    ar, arp = arr(aspect_ratios)
    va, vap = arr(variances)
    if va.size != 4:
        raise ValueError("four variances")
    lib = _lib.load_detect_library()
    per = ctypes.c_int()
    args = (int(h), int(w), int(image_w), int(image_h), mnp, mn.size, mxp, mx.size, arp, ar.size, vap, int(bool(flip)), int(bool(clip)), float(step_w),
            float(step_h), float(offset), ctypes.byref(per))
    _check(lib.fhip_priorbox_fill(*args, None, 0), "fhip_priorbox_fill")
    out = np.empty((2, 4 * h * w * per.value), dtype=np.float32)
    _check(lib.fhip_priorbox_fill(*args, out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), out.size), "fhip_priorbox_fill")
    return out


def detection_output(location, confidence, prior, num_class: int, nms_threshold: float = 0.45, nms_top_k: int = 400, keep_top_k: int = 200,
                     confidence_threshold: float = 0.01, out=None):
    """ncnn's DetectionOutput with a batch: location [N][4P], confidence [N][P * num_class], prior [1 or N][2][4P], contiguous float32 CUDA
    tensors -> [N][keep_top_k][6] rows (label, score, xmin, ymin, xmax, ymax), zero rows past an image's count (fhip_detection_output_forward)."""
    import torch
    for t, what in ((location, "location"), (confidence, "confidence"), (prior, "prior")):
        _f32(t, what)
    n, p = location.shape[0], location.shape[1] // 4
    if location.dim() != 2 or location.shape[1] != 4 * p or tuple(confidence.shape) != (n, p * num_class) or tuple(prior.shape[1:]) != (2, 4 * p):
        raise ValueError("location [N][4P], confidence [N][P * num_class], prior [1 or N][2][4P]")
    lib = _lib.load_detect_library()
    nbytes = ctypes.c_size_t()
    _check(lib.fhip_detection_output_get_buffer_size(n, p, int(num_class), int(nms_top_k), int(keep_top_k), ctypes.byref(nbytes)),
           "fhip_detection_output_get_buffer_size")
    scratch = torch.empty((nbytes.value + 7) // 8, device=location.device, dtype=torch.int64)
    if out is None:
        out = torch.empty((n, int(keep_top_k), 6), device=location.device, dtype=torch.float32)
    _check(lib.fhip_detection_output_forward(n, p, int(num_class), float(nms_threshold), int(nms_top_k), int(keep_top_k), float(confidence_threshold),
                                             prior.shape[0], _ptr(out), _ptr(location), _ptr(confidence), _ptr(prior), _ptr(scratch), _stream()),
           "fhip_detection_output_forward")
    return out


def detect_route(what: int, a: int = 0, b: int = 0, c: int = 1, h: int = 1, w: int = 1, out=None, x=None) -> str:
    """The kernel instantiation a call would launch (fhip_detect_route): what = PERMUTE (a = order_type, b = rank), NORMALIZE, SOFTMAX, SELECT,
    MERGE or PERMUTE_CONCAT."""
    name = ctypes.create_string_buffer(128)
    _check(_lib.load_detect_library().fhip_detect_route(int(what), int(a), int(b), int(c), int(h), int(w), _ptr(out) if out is not None else None,
                                                        _ptr(x) if x is not None else None, name, 128), "fhip_detect_route")
    return name.value.decode()
