"""Python host-side mirror of include/feather_hip/feather_yolo.h (``libfeather_yolo.so``): the layers of a YOLO detection head -- Reorg,
YoloDetectionOutput (YOLOv2) and Yolov3DetectionOutput -- on torch CUDA tensors.  Every device call goes through the C-ABI on the current
stream; there is no fallback path.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from .booster import _ptr, _stream

NET_ROUTE = 110  # FHIP_YOLO_NET_ROUTE
MAX_SCALES, MAX_BOXES, MAX_CLASSES, MAX_CELLS, MAX_ROWS, CHUNK, REORG_TILE = 4, 16, 256, 1 << 22, 1024, 1024, 4096
REORG, SCORE, SELECT = range(3)  # fhip_yolo_op

_check = _lib.checker(_lib.load_yolo_library, "fhip_yolo_last_error")


def _f32(t, what):
    import torch
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous() or t.dim() != 4:
        raise ValueError(f"{what} must be a contiguous float32 CUDA tensor [N][C][H][W]")


def reorg_output_dim(stride: int, c: int, h: int, w: int):
    """(c, h, w) of Reorg's output for an input (c, h, w) (fhip_reorg_output_dim)."""
    o = [ctypes.c_int() for _ in range(3)]
    _check(_lib.load_yolo_library().fhip_reorg_output_dim(int(stride), int(c), int(h), int(w), *[ctypes.byref(v) for v in o]), "fhip_reorg_output_dim")
    return tuple(v.value for v in o)


def reorg(x, stride: int, mode: int = 0, out=None):
    """ncnn's Reorg of a contiguous float32 CUDA tensor [N][C][H][W]: [N][C * stride^2][H / stride][W / stride] (fhip_reorg_forward)."""
    import torch
    _f32(x, "x")
    n, c, h, w = x.shape
    oc, oh, ow = reorg_output_dim(stride, c, h, w)
    if out is None:
        out = torch.empty((n, oc, oh, ow), device=x.device, dtype=torch.float32)
    elif not out.is_cuda or out.dtype != torch.float32 or not out.is_contiguous() or out.numel() != n * oc * oh * ow:
        raise ValueError("out must be a contiguous float32 CUDA tensor of the output's size")
    _check(_lib.load_yolo_library().fhip_reorg_forward(int(stride), int(mode), n, c, h, w, _ptr(out), _ptr(x), _stream()), "fhip_reorg_forward")
    return out


def _floats(v):
    a = np.ascontiguousarray(np.asarray(v, dtype=np.float32).reshape(-1))
    return a, (a.ctypes.data_as(ctypes.POINTER(ctypes.c_float)) if a.size else None)


def _ints(v):
    a = np.ascontiguousarray(np.asarray(v, dtype=np.int32).reshape(-1))
    return a, (a.ctypes.data_as(ctypes.POINTER(ctypes.c_int)) if a.size else None)


def yolo_detection(bottoms, num_class: int, num_box: int, biases, confidence_threshold: float = 0.01, nms_threshold: float = 0.45, rows: int = 256,
                   mask=None, anchors_scale=None, out=None):
    """ncnn's YoloDetectionOutput -- or, with `mask` and `anchors_scale`, Yolov3DetectionOutput -- of 1 .. 4 contiguous float32 CUDA tensors
    [N][num_box * (5 + num_class)][H_i][W_i] -> [N][rows][6] rows (label + 1, score, xmin, ymin, xmax, ymax), zero rows past an image's count
    (fhip_yolo_detection_forward)."""
    import torch
    for t in bottoms:
        _f32(t, "a bottom")
    version = 2 if mask is None else 3
    k, n = len(bottoms), bottoms[0].shape[0]
    for t in bottoms:
        if t.shape[0] != n or t.shape[1] != num_box * (5 + num_class):
            raise ValueError("every bottom must be [N][num_box * (5 + num_class)][H][W] with the same N")
    h, hp = _ints([t.shape[2] for t in bottoms])
    w, wp = _ints([t.shape[3] for t in bottoms])
    b, bp = _floats(biases)
    m, mp = _ints(mask if mask is not None else [])
    s, sp = _floats(anchors_scale if anchors_scale is not None else [])
    if version == 3 and (m.size != k * num_box or s.size != k):
        raise ValueError("mask must hold num_box entries per bottom and anchors_scale one")
    lib = _lib.load_yolo_library()
    nbytes = ctypes.c_size_t()
    _check(lib.fhip_yolo_get_buffer_size(n, k, int(num_box), int(num_class), hp, wp, ctypes.byref(nbytes)), "fhip_yolo_get_buffer_size")
    scratch = torch.empty(max((nbytes.value + 7) // 8, 1), device=bottoms[0].device, dtype=torch.int64)
    if out is None:
        out = torch.empty((n, int(rows), 6), device=bottoms[0].device, dtype=torch.float32)
    elif not out.is_cuda or out.dtype != torch.float32 or not out.is_contiguous() or out.numel() != n * int(rows) * 6:
        raise ValueError("out must be a contiguous float32 CUDA tensor [N][rows][6]")
    ptrs = (ctypes.c_void_p * k)(*[t.data_ptr() for t in bottoms])
    _check(lib.fhip_yolo_detection_forward(version, n, k, int(num_box), int(num_class), hp, wp, float(confidence_threshold), float(nms_threshold), bp, b.size, mp,
                                           sp, int(rows), _ptr(out), ptrs, _ptr(scratch), _stream()), "fhip_yolo_detection_forward")
    return out


def yolo_route(what: int, a: int = 0, b: int = 0) -> str:
    """The kernel instantiation a call would launch (fhip_yolo_route): what = REORG (a = stride, b = w), SCORE (a = version) or SELECT."""
    name = ctypes.create_string_buffer(128)
    _check(_lib.load_yolo_library().fhip_yolo_route(int(what), int(a), int(b), name, 128), "fhip_yolo_route")
    return name.value.decode()
