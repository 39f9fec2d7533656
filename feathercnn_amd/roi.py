"""Python host-side mirror of include/feather_hip/feather_roi.h (``libfeather_roi.so``): the layers of a two-stage detector -- Proposal,
ROIPooling, ROIAlign and PSROIPooling -- on torch CUDA tensors.  Every device call goes through the C-ABI on the current stream; there is
no fallback path.  generate_anchors is a host function and needs no device.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from .booster import _ptr, _stream

NET_ROUTE = 111  # FHIP_ROI_NET_ROUTE
MAX_ANCHORS, MAX_CELLS, MAX_ROIS, MAX_POOLED, MAX_GRID, CHUNK = 32, 1 << 24, 2048, 64, 4096, 1024
KEYS, SELECT, POOL, ALIGN, PSROI = range(1, 6)  # fhip_roi_op
RATIOS, SCALES = (0.5, 1.0, 2.0), (8.0, 16.0, 32.0)  # ncnn's Proposal

_check = _lib.checker(_lib.load_roi_library, "fhip_roi_last_error")


def _f32(t, what, dims=4):
    import torch
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous() or t.dim() != dims:
        raise ValueError(f"{what} must be a contiguous float32 CUDA tensor of rank {dims}")


def _floats(v):
    a = np.ascontiguousarray(np.asarray(v, dtype=np.float32).reshape(-1))
    return a, (a.ctypes.data_as(ctypes.POINTER(ctypes.c_float)) if a.size else None)


def generate_anchors(base_size: int = 16, ratios=RATIOS, scales=SCALES) -> np.ndarray:
    """ncnn's generate_anchors: [len(ratios) * len(scales)][4] float32, row ratio_index * len(scales) + scale_index (fhip_roi_generate_anchors)."""
    r, rp = _floats(ratios)
    s, sp = _floats(scales)
    out = np.zeros((max(r.size * s.size, 1), 4), np.float32)
    _check(_lib.load_roi_library().fhip_roi_generate_anchors(int(base_size), rp, r.size, sp, s.size, out.ctypes.data_as(ctypes.POINTER(ctypes.c_float))),
           "fhip_roi_generate_anchors")
    return out[:r.size * s.size]


def proposal(score, bbox, im_info, anchors=None, feat_stride: int = 16, pre_nms_topN: int = 6000, after_nms_topN: int = 300, nms_thresh: float = 0.7,
             min_size: float = 16, with_scores: bool = False):
    """ncnn's Proposal of score [N][2A][H][W], bbox [N][4A][H][W] and im_info [N][3] -> rois [N][after_nms_topN][4], rows (x1, y1, x2, y2), the
    sentinel (0, 0, -1, -1) past an image's count; with_scores: (rois, scores [N][after_nms_topN]).  anchors: [A][4], default
    generate_anchors() (fhip_proposal_forward)."""
    import torch
    _f32(score, "score")
    _f32(bbox, "bbox")
    _f32(im_info, "im_info", 2)
    a, ap = _floats(generate_anchors() if anchors is None else anchors)
    A = a.size // 4
    n, _, h, w = score.shape
    if a.size != 4 * A or score.shape[1] != 2 * A or tuple(bbox.shape) != (n, 4 * A, h, w) or tuple(im_info.shape) != (n, 3):
        raise ValueError("score must be [N][2A][H][W], bbox [N][4A][H][W] and im_info [N][3] for anchors [A][4]")
    lib = _lib.load_roi_library()
    nbytes = ctypes.c_size_t()
    _check(lib.fhip_proposal_get_buffer_size(n, A, h, w, ctypes.byref(nbytes)), "fhip_proposal_get_buffer_size")
    scratch = torch.empty(max((nbytes.value + 7) // 8, 1), device=score.device, dtype=torch.int64)
    rois = torch.empty((n, int(after_nms_topN), 4), device=score.device, dtype=torch.float32)
    scores = torch.empty((n, int(after_nms_topN)), device=score.device, dtype=torch.float32) if with_scores else None
    _check(lib.fhip_proposal_forward(n, A, h, w, int(feat_stride), int(pre_nms_topN), int(after_nms_topN), float(nms_thresh), float(min_size), ap, _ptr(rois),
                                     _ptr(scores) if with_scores else None, _ptr(score), _ptr(bbox), _ptr(im_info), _ptr(scratch), _stream()),
           "fhip_proposal_forward")
    return (rois, scores) if with_scores else rois


def _pooled(x, rois, channels, pooled):
    import torch
    _f32(x, "x")
    _f32(rois, "rois", 3)
    n, c, h, w = x.shape
    if rois.shape[0] != n or rois.shape[2] != 4:
        raise ValueError("rois must be [N][R][4] with the features' N")
    pw, ph = (pooled, pooled) if isinstance(pooled, int) else pooled
    out = torch.empty((n * rois.shape[1], channels, ph, pw), device=x.device, dtype=torch.float32)
    return out, (n, c, h, w, int(rois.shape[1]), int(pw), int(ph))


def roi_pool(x, rois, pooled=7, spatial_scale: float = 0.0625):
    """ncnn's ROIPooling of features [N][C][H][W] over rois [N][R][4] -> [N * R][C][pooled_h][pooled_w]; pooled: one extent or (width, height)
    (fhip_roi_pool_forward)."""
    out, dims = _pooled(x, rois, x.shape[1], pooled)
    _check(_lib.load_roi_library().fhip_roi_pool_forward(*dims, float(spatial_scale), _ptr(out), _ptr(x), _ptr(rois), _stream()), "fhip_roi_pool_forward")
    return out


def roi_align(x, rois, pooled=7, spatial_scale: float = 0.0625, sampling_ratio: int = 0, aligned: bool = False, version: int = 0):
    """ncnn's ROIAlign, version 0 (ncnn's original) or 1 (detectron2 / torchvision) (fhip_roi_align_forward)."""
    out, dims = _pooled(x, rois, x.shape[1], pooled)
    _check(_lib.load_roi_library().fhip_roi_align_forward(*dims, float(spatial_scale), int(sampling_ratio), int(bool(aligned)), int(version), _ptr(out), _ptr(x),
                                                          _ptr(rois), _stream()), "fhip_roi_align_forward")
    return out


def psroi_pool(x, rois, output_dim: int, pooled=7, spatial_scale: float = 0.0625):
    """ncnn's PSROIPooling of features [N][output_dim * pooled_h * pooled_w][H][W] -> [N * R][output_dim][pooled_h][pooled_w]
    (fhip_psroi_pool_forward)."""
    out, dims = _pooled(x, rois, int(output_dim), pooled)
    _check(_lib.load_roi_library().fhip_psroi_pool_forward(*dims, float(spatial_scale), int(output_dim), _ptr(out), _ptr(x), _ptr(rois), _stream()),
           "fhip_psroi_pool_forward")
    return out


def roi_route(what: int, a: int = 0, b: int = 0) -> str:
    """The kernel a call would launch (fhip_roi_route): what = KEYS, SELECT, POOL, ALIGN (a = version) or PSROI."""
    name = ctypes.create_string_buffer(128)
    _check(_lib.load_roi_library().fhip_roi_route(int(what), int(a), int(b), name, 128), "fhip_roi_route")
    return name.value.decode()
