"""One way to run the entry points of libfeather_roi.so on the device with every tensor between guards (tests/guarded.py): proposal() and the
three ROI layers, which tests/test_roi_gpu.py compares with tests/roi_ref.py, and sweep(), which walks them so that every instantiation of
tests/roi_cases.targets() is launched -- tests/roi_trace_child.py runs it under the kernel trace."""
import ctypes

import numpy as np

import roi_cases as C
import roi_ref as R
import side_contract
from guarded import Guarded, describe

F = np.float32
V = ctypes.c_void_p


def route(lib, what, a=0, b=0):
    name = ctypes.create_string_buffer(128)
    assert lib.fhip_roi_route(what, a, b, name, 128) == 0, lib.fhip_roi_last_error()
    return name.value.decode()


def _finish(buffers, outs):
    import torch
    torch.cuda.synchronize()
    for g in buffers:
        assert g.guards_intact() is None, describe(g.guards_intact())
    for out in outs:
        assert out.unwritten() == 0, out.unwritten()
    return [out.values() for out in outs]


def proposal(lib, score, bbox, im_info, anchors=None, feat_stride=16, pre_nms_topN=6000, after_nms_topN=300, nms_thresh=0.7, min_size=16, offset=0, with_scores=True):
    """-> (rois [n][R][4], scores [n][R] or None); the bottoms, the outputs (poison) and the scratch (poison) lie between guards."""
    a = np.ascontiguousarray(R.generate_anchors() if anchors is None else anchors, F)
    n, _, h, w = score.shape
    A, rows = len(a), after_nms_topN
    nbytes = ctypes.c_size_t()
    assert lib.fhip_proposal_get_buffer_size(n, A, h, w, ctypes.byref(nbytes)) == 0, lib.fhip_roi_last_error()
    ins = [Guarded(x.size, x, offset) for x in (score, bbox, np.asarray(im_info, F).reshape(n, 3))]
    rois, scratch = Guarded(n * rows * 4, "poison", offset), Guarded((nbytes.value + 3) // 4, "poison", 0)
    scores = Guarded(n * rows, "poison", offset) if with_scores else None
    rc = lib.fhip_proposal_forward(n, A, h, w, feat_stride, pre_nms_topN, rows, nms_thresh, float(min_size), a.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                   V(rois.ptr), V(scores.ptr) if with_scores else None, V(ins[0].ptr), V(ins[1].ptr), V(ins[2].ptr), V(scratch.ptr),
                                   side_contract.stream())
    assert rc == 0, lib.fhip_roi_last_error()
    outs = _finish(ins + [rois, scratch] + ([scores] if with_scores else []), [rois, scratch] + ([scores] if with_scores else []))
    return outs[0].reshape(n, rows, 4), (outs[2].reshape(n, rows) if with_scores else None)


def _pooled(lib, call, x, rois, channels, pw, ph, offset):
    n, c, h, w = x.shape
    r = np.ascontiguousarray(rois, F).reshape(n, -1, 4)
    src, boxes, out = Guarded(x.size, x, offset), Guarded(r.size, r, offset), Guarded(n * r.shape[1] * channels * ph * pw, "poison", offset)
    rc = call((n, c, h, w, r.shape[1], pw, ph), V(out.ptr), V(src.ptr), V(boxes.ptr))
    assert rc == 0, lib.fhip_roi_last_error()
    return _finish([src, boxes, out], [out])[0].reshape(n * r.shape[1], channels, ph, pw)


def roi_pool(lib, x, rois, pw, ph, scale, offset=0):
    return _pooled(lib, lambda d, o, i, r: lib.fhip_roi_pool_forward(*d, scale, o, i, r, side_contract.stream()), x, rois, x.shape[1], pw, ph, offset)


def roi_align(lib, x, rois, pw, ph, scale, sampling, aligned, version, offset=0):
    return _pooled(lib, lambda d, o, i, r: lib.fhip_roi_align_forward(*d, scale, sampling, aligned, version, o, i, r, side_contract.stream()), x, rois, x.shape[1], pw,
                   ph, offset)


def psroi_pool(lib, x, rois, output_dim, pw, ph, scale, offset=0):
    return _pooled(lib, lambda d, o, i, r: lib.fhip_psroi_pool_forward(*d, scale, output_dim, o, i, r, side_contract.stream()), x, rois, output_dim, pw, ph, offset)


def sweep(lib, seen):
    """Launches every instantiation once on small data, compared with the restatement as it goes; seen(route name) for each launch, in launch
    order."""
    inputs, args, want64, want32, _ = C.case(C.CASES[0])
    rois, scores = proposal(lib, *inputs, **args)
    assert np.array_equal(scores, want32[1]) and R.counts(rois) == R.counts(want32[0])
    seen(route(lib, C.KEYS))
    seen(route(lib, C.SELECT))
    cfg = C.POOLED[1]
    x, r, want = C.pool_case(cfg)
    assert np.array_equal(roi_pool(lib, x, r, *cfg), want)
    seen(route(lib, C.POOL))
    for version in (0, 1):
        cfg = (version, 0, 2) + C.POOLED[1]
        x, r, want = C.align_case(cfg)
        got = roi_align(lib, x, r, cfg[3], cfg[4], cfg[5], cfg[2], cfg[1], cfg[0])
        assert np.array_equal(got, want)
        seen(route(lib, C.ALIGN, version))
    cfg = C.PS_CASES[1]
    x, r, want = C.psroi_case(cfg)
    assert np.array_equal(psroi_pool(lib, x, r, 2, *cfg), want)
    seen(route(lib, C.PSROI))
