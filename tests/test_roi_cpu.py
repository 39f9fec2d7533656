"""The two-stage detection layers without a GPU: the restatement against itself in float64 and against hand-computed examples, the committed
seeds against the margins, the anchors against the published ones, the Net switch (fhip_net_set_roi) and what LoadParam answers, every
entry's host checks, the route names and the zoo nets."""
import ctypes
import re

import numpy as np
import pytest

import roi_cases as C
import roi_ref as R
import side_contract as SC
from test_resample_cpu import HOSTILE_VALUES

F = np.float32
NEW_TYPES = ("Proposal", "ROIPooling", "ROIAlign", "PSROIPooling")
GOOD = {  # type -> (params that load, bottoms, tops)
    "Proposal": ("0=16 1=16 2=6000 3=300 4=0.7 5=16", 3, 1),
    "ROIPooling": ("0=7 1=7 2=0.0625", 2, 1),
    "ROIAlign": ("0=7 1=7 2=0.0625 3=2 4=1 5=1", 2, 1),
    "PSROIPooling": ("0=3 1=3 2=0.0625 3=2", 2, 1),
}


def _net(param, roi=None, detection=False, extended=False, yolo=None):
    from feathercnn_amd.net import Net
    net = Net()
    if roi is not None:
        net.SetRoi(roi)
    if detection:
        net.SetDetection(True)
    if extended:
        net.SetExtendedLayers(True)
    if yolo is not None:
        net.SetYolo(yolo)
    net.LoadParam(param)
    return net


def _refused(param, code, *words, **kw):
    from feathercnn_amd import FeatherHipError
    with pytest.raises(FeatherHipError) as e:
        _net(param, **kw)
    assert f"code {code}" in str(e.value) and all(w in str(e.value) for w in words), str(e.value)
    return str(e.value)


def _one(type_, params="", bottoms=1, tops=1):
    """A .param of an 8-channel 6x6 input (split for the layers that read several bottoms) and one layer `l` of `type_`."""
    ins = " ".join(f"s_{i}" for i in range(bottoms))
    outs = " ".join(["l"] + [f"l_{i}" for i in range(1, tops)])
    lines = ["Input data 0 1 data 0=6 1=6 2=8", f"Split s 1 {bottoms} data " + ins, f"{type_} l {bottoms} {tops} {ins} {outs} {params}".strip()]
    return ("7767517\n%d %d\n" % (len(lines), 1 + bottoms + tops) + "\n".join(lines) + "\n").encode()


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", C.CASES, ids=C.case_id)
def test_committed_seeds_pass_the_margins_and_float32_agrees_with_float64(c):
    inputs, args, want64, want32, m = C.case(c)
    assert C.stable(m), m  # the generator's own check, on the committed seed: nothing is skipped on the GPU
    assert C.first_stable_seed(c, start=C.SEEDS.get(c, 0))[0] == C.SEEDS.get(c, 0)
    assert R.counts(want32[0]) == R.counts(want64[0]) and np.array_equal(want32[1], want64[1]), "counts, rows or order"  # scores are distinct: they name the rows
    tol, e32 = C.tolerance(want64, want32, inputs[2])
    assert e32 <= 2.0 ** -20, e32  # a handful of float32 roundings
    counts = R.counts(want64[0])
    assert min(counts) >= 1 and all((img[k:] == (0, 0, -1, -1)).all() and not s[k:].any() for img, s, k in zip(want64[0], want64[1], counts))
    score = inputs[0][:, 9:].reshape(c[1], -1)
    assert all(len(np.unique(s)) == s.size for s in score)  # distinct scores: the order is exact
    if c[0] != "3x5":
        assert score.shape[1] > (2 * C.CHUNK if c[0] == "24x32" else C.CHUNK)  # past a selection chunk; the large map past the selection buffer
    if c[3] == 16 and c[0] != "3x5":
        assert counts == [16] * c[1]  # after_nms_topN reached, long before the candidates end


def test_the_default_pre_nms_topn_cuts_on_the_large_map():
    cut, full = C.case(C.CASES[7])[2][0], C.case(C.CASES[8])[2][0]
    a, b = R.counts(cut)[0], R.counts(full)[0]
    assert a < b < 300 and np.array_equal(cut[0, :a], full[0, :a])  # the late boxes behind candidate 6000 are missing, nothing else


def test_proposal_by_hand():
    """One cell, nine anchors, only anchor 3 -- (-56, -56, 72, 72): 128 px around (8, 8) -- and anchor 4 decode inside the image.  Anchor 3 with
    dx = dy = 0.25, dw = dh = ln(1/4): centre (40, 40), size 32: the box (24, 24, 56, 56).  Anchor 4 (256 px) with dx = dy = 0.125,
    dw = dh = ln(1/8): the same box, a lower score: IoU 1024 / (2 * 1089 - 1024) = 0.887, suppressed at 0.7, kept at 0.9."""
    score = np.zeros((1, 18, 1, 1), F)
    bbox = np.zeros((1, 36, 1, 1), F)
    bbox[0, 2::4] = bbox[0, 3::4] = -20  # every other anchor: a point, below min_size
    score[0, 9 + 3], score[0, 9 + 4] = 0.9, 0.8
    bbox[0, 12:16, 0, 0] = (0.25, 0.25, np.log(0.25), np.log(0.25))
    bbox[0, 16:20, 0, 0] = (0.125, 0.125, np.log(0.125), np.log(0.125))
    info = np.asarray([[100, 120, 1]], F)
    for dtype in (np.float32, np.float64):
        rois, scores = R.proposal(score, bbox, info, after_nms_topN=3, min_size=16, dtype=dtype)
        assert np.allclose(rois[0, 0], (24, 24, 56, 56), atol=1e-4) and scores[0, 0] == F(0.9) and R.counts(rois) == [1]
        assert (rois[0, 1:] == (0, 0, -1, -1)).all() and not scores[0, 1:].any()
        rois, scores = R.proposal(score, bbox, info, after_nms_topN=3, min_size=16, nms_thresh=0.9, dtype=dtype)
        assert R.counts(rois) == [2] and scores[0, 1] == F(0.8)
        rois, _ = R.proposal(score, bbox, np.asarray([[100, 120, 3]], F), after_nms_topN=3, min_size=16, dtype=dtype)  # 33 < 16 * 3
        assert R.counts(rois) == [0]
        rois, _ = R.proposal(score, bbox, np.asarray([[40, 50, 1]], F), after_nms_topN=3, min_size=10, dtype=dtype)  # clipped to the image
        assert np.allclose(rois[0, 0], (24, 24, 49, 39), atol=1e-4)


def test_roi_layers_by_hand():
    x = np.arange(2 * 4 * 4, dtype=F).reshape(1, 2, 4, 4)
    whole = np.asarray([[[0, 0, 3, 3]]], F)
    assert np.array_equal(R.roi_pool(x, whole, 2, 2, 1.0)[0, 0], [[5, 7], [13, 15]])  # the maximum of each quadrant
    assert np.array_equal(R.roi_pool(x, whole, 1, 1, 1.0)[0, :, 0, 0], [15, 31])
    assert np.array_equal(R.roi_pool(x, np.asarray([[[0, 0, -1, -1]]], F), 2, 2, 1.0)[0, 1], [[16, 16], [16, 16]])  # the sentinel: extents max(-1 - 0 + 1, 1) = 1, every bin is pixel (0, 0)
    assert R.roi_pool(x, np.asarray([[[9, 9, 12, 12]]], F), 2, 2, 1.0).any() == False  # outside: every bin is empty
    ps = np.arange(8 * 4 * 4, dtype=F).reshape(1, 8, 4, 4)
    y = R.psroi_pool(ps, whole, 2, 2, 2, 1.0)  # bins of 2 x 2 pixels; bin (d, p, q) reads channel (d * 2 + p) * 2 + q
    assert y.shape == (1, 2, 2, 2) and y[0, 0, 0, 0] == np.mean([0, 1, 4, 5]) and y[0, 1, 1, 1] == 7 * 16 + np.mean([10, 11, 14, 15])
    ramp = np.tile(np.arange(4, dtype=F), (1, 1, 4, 1))  # in[y][x] = x: bilinear interpolation is exact
    for version in (0, 1):
        y = R.roi_align(ramp, np.asarray([[[1, 1, 3, 3]]], F), 2, 2, 1.0, 2, 0, version)
        assert np.allclose(y[0, 0], [[1.5, 2.5], [1.5, 2.5]])  # samples at 1.25, 1.75 | 2.25, 2.75
    y = R.roi_align(ramp, np.asarray([[[1, 1, 3, 3]]], F), 2, 2, 1.0, 2, 1, 1)  # aligned: half a pixel to the left
    assert np.allclose(y[0, 0], [[1.0, 2.0], [1.0, 2.0]])


def test_the_restatement_in_float64_agrees_with_float32_on_the_roi_layers():
    for cfg in (C.ALIGN_CASES[0], C.ALIGN_CASES[-1]):
        x, r, want32 = C.align_case(cfg)
        v, a, s, pw, ph, scale = cfg
        assert np.abs(R.roi_align(x, r, pw, ph, scale, s, a, v, dtype=np.float64) - want32).max() < 1e-5
    x, r, want32 = C.psroi_case(C.PS_CASES[0])
    assert np.abs(R.psroi_pool(x, r, 2, 3, 3, C.PS_CASES[0][2], dtype=np.float64) - want32).max() < 1e-5
    x, r, want32 = C.pool_case(C.POOLED[1])
    assert np.array_equal(R.roi_pool(x, r, *C.POOLED[1], dtype=np.float64), want32)  # values are moved


def test_generate_anchors_gives_the_published_anchors_shifted_by_ncnns_centring():
    """py-faster-rcnn's generate_anchors(16) centres on 7.5 and counts x2 - x1 + 1 as the width; ncnn centres on 8 and takes x2 - x1: the same x1 and
    y1, x2 and y2 one larger.  The shift is (0, 0, +1, +1)."""
    from feathercnn_amd import generate_anchors
    published = np.asarray([(-84, -40, 99, 55), (-176, -88, 191, 103), (-360, -184, 375, 199), (-56, -56, 71, 71), (-120, -120, 135, 135),
                            (-248, -248, 263, 263), (-36, -80, 51, 95), (-80, -168, 95, 183), (-168, -344, 183, 359)], F)
    got = generate_anchors(16)
    assert got.dtype == F and np.array_equal(got, published + np.asarray((0, 0, 1, 1), F))
    assert np.array_equal(got[-1], (-168, -344, 184, 360)) and np.array_equal(got, R.generate_anchors(16))
    for base in (1, 2, 4, 7, 32):
        assert np.array_equal(generate_anchors(base), R.generate_anchors(base)), base
    assert np.array_equal(generate_anchors(8, (1.0, 3.0), (2.0,)), R.generate_anchors(8, (1.0, 3.0), (2.0,)))


# ---- the switch --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("type_", NEW_TYPES)
def test_default_net_refuses_the_new_types(type_):
    params, bottoms, tops = GOOD[type_]
    p = _one(type_, params, bottoms, tops)
    msg = _refused(p, -200, type_)
    assert msg.rstrip().endswith("(fhip_net_set_roi lifts this)"), msg
    for other in (dict(detection=True), dict(extended=True), dict(yolo=8), dict(detection=True, extended=True, yolo=8)):  # the other switches lift nothing here
        assert "fhip_net_set_roi lifts this" in _refused(p, -200, type_, **other)
    assert (type_, "l", "ROI") in _net(p, roi=True).layers()
    assert (type_, "l", "ROI") in _net(p, roi=True, detection=True, extended=True, yolo=8).layers()


def test_on_then_off_equals_the_default_and_the_switch_is_refused_after_loadparam():
    from feathercnn_amd import FeatherHipError
    from feathercnn_amd.net import Net
    net = Net()
    net.SetRoi()
    net.SetRoi(False)
    with pytest.raises(FeatherHipError, match="code -200") as e:
        net.LoadParam(_one("ROIPooling", GOOD["ROIPooling"][0], 2))
    assert "fhip_net_set_roi lifts this" in str(e.value)
    net = _net(_one("ReLU"))
    with pytest.raises(FeatherHipError, match="before LoadParam") as e:
        net.SetRoi()
    assert "code -2" in str(e.value)


@pytest.mark.parametrize("type_", ["PixelShuffle", "Padding", "Reorg"])
def test_other_types_stay_refused_with_the_switch_on(type_):
    msg = _refused(_one(type_, "0=2"), -200, type_, roi=True)
    assert "fhip_net_set_roi" not in msg


def test_the_route_code_and_the_bindings():
    import feathercnn_amd
    from feathercnn_amd import _lib, net, roi
    header = open(SC.INCLUDE + "/feather_hip/feather_roi.h").read()
    code = int(re.search(r"#define\s+FHIP_ROI_NET_ROUTE\s+(\d+)", header).group(1))
    assert code == net.ROI_ROUTE == roi.NET_ROUTE == feathercnn_amd.ROI_NET_ROUTE == 111 and net.ROUTE_NAMES[code] == "ROI"
    assert list(net.ROUTE_NAMES.values()).count("ROI") == 1 and list(_lib.OPEN_LIBRARIES) == ["yolo", "roi"]
    for macro, value in (("FHIP_ROI_MAX_ANCHORS", roi.MAX_ANCHORS), ("FHIP_ROI_MAX_CELLS", roi.MAX_CELLS), ("FHIP_ROI_MAX_ROIS", roi.MAX_ROIS),
                         ("FHIP_ROI_MAX_POOLED", roi.MAX_POOLED), ("FHIP_ROI_MAX_GRID", roi.MAX_GRID), ("FHIP_ROI_CHUNK", roi.CHUNK)):
        assert eval(re.search(r"#define\s+%s\s+(.+)" % macro, header).group(1)) == value, macro
    assert roi.CHUNK == C.CHUNK and roi.MAX_GRID == R.MAX_GRID and (roi.KEYS, roi.SELECT, roi.POOL, roi.ALIGN, roi.PSROI) == (C.KEYS, C.SELECT, C.POOL, C.ALIGN, C.PSROI)
    text = open(SC.INCLUDE + "/feather_hip/feather_net.h").read()
    cxx = open(SC.INCLUDE + "/feather/net.h").read()
    assert "fhip_net_set_roi" in text and "fhip_net_set_roi" in _lib.SIGNATURES and "SetRoi(bool on = true)" in cxx and "ExtractProposals" in cxx
    assert callable(net.Net.SetRoi) and callable(net.Net.ExtractProposals)
    assert all(callable(getattr(feathercnn_amd, f)) for f in ("generate_anchors", "proposal", "roi_pool", "roi_align", "psroi_pool", "roi_route"))
    seen = {roi.roi_route(roi.KEYS), roi.roi_route(roi.SELECT), roi.roi_route(roi.POOL), roi.roi_route(roi.ALIGN, 0), roi.roi_route(roi.ALIGN, 1), roi.roi_route(roi.PSROI)}
    assert seen == C.targets()


# ---- hostile values ------------------------------------------------------------------------------------------------------------------------
IDS = {"Proposal": (0, 1, 2, 3, 4, 5), "ROIPooling": (0, 1, 2), "ROIAlign": (0, 1, 2, 3, 4, 5), "PSROIPooling": (0, 1, 2, 3)}


@pytest.mark.parametrize("type_", NEW_TYPES)
def test_hostile_param_values_load_or_are_minus_100_naming_the_id(type_):
    from feathercnn_amd import FeatherHipError
    params, bottoms, tops = GOOD[type_]
    answers = set()
    for pid in IDS[type_]:
        for v in HOSTILE_VALUES:
            kept = [kv for kv in params.split() if not kv.startswith(f"{pid}=")]
            try:
                _net(_one(type_, " ".join(kept + [f"{pid}={v}"]), bottoms, tops), roi=True)
                answers.add("ok")
            except FeatherHipError as e:
                assert "code -100" in str(e) and "layer l" in str(e) and f"({pid}=" in str(e), (type_, pid, v, str(e))
                answers.add("refused")
    assert answers == {"ok", "refused"}


def test_wrong_bottom_and_top_counts_are_refused():
    _refused(_one("Proposal", GOOD["Proposal"][0], 2), -100, "layer l", roi=True)
    _refused(_one("Proposal", GOOD["Proposal"][0], 3, 3), -100, "layer l", roi=True)
    _net(_one("Proposal", GOOD["Proposal"][0], 3, 2), roi=True)  # rois and scores
    for type_ in ("ROIPooling", "ROIAlign", "PSROIPooling"):
        _refused(_one(type_, GOOD[type_][0], 1), -100, "layer l", roi=True)
        _refused(_one(type_, GOOD[type_][0], 3), -100, "layer l", roi=True)
        _refused(_one(type_, GOOD[type_][0], 2, 2), -100, "layer l", roi=True)
    _refused(_one("PSROIPooling", "0=3 1=3 2=0.0625", 2), -100, "layer l", "(3=", roi=True)  # no output_dim


# ---- the C-ABI's host checks: none of these calls needs (or reaches) a GPU -------------------------------------------------------------------
V = ctypes.c_void_p
ANCHORS = (ctypes.c_float * 36)(*R.generate_anchors().reshape(-1))


def _proposal(lib, n=1, A=9, h=2, w=2, stride=16, pre=6000, after=4, nms=0.7, min_size=16.0, anchors=ANCHORS, rois=0x1000, scores=0x2000, score=0x3000,
              bbox=0x4000, info=0x5000, scratch=0x6000):
    return lib.fhip_proposal_forward(n, A, h, w, stride, pre, after, nms, min_size, anchors, V(rois), V(scores), V(score), V(bbox), V(info), V(scratch), None)


def test_every_entry_refuses_bad_arguments_on_the_host():
    lib = SC.library("roi")
    bad = SC.BADARG
    out = (ctypes.c_float * 128)()
    r3, s3 = (ctypes.c_float * 3)(0.5, 1, 2), (ctypes.c_float * 3)(8, 16, 32)
    assert lib.fhip_roi_generate_anchors(16, r3, 3, s3, 3, out) == 0 and list(out[:4]) == [-84, -40, 100, 56]
    for args in ((0, r3, 3, s3, 3, out), (16, r3, 0, s3, 3, out), (16, r3, 3, s3, 0, out), (16, None, 3, s3, 3, out), (16, r3, 3, None, 3, out),
                 (16, r3, 3, s3, 3, None), (16, (ctypes.c_float * 3)(0.5, 0, 2), 3, s3, 3, out), (16, r3, 3, (ctypes.c_float * 3)(8, float("nan"), 32), 3, out),
                 (16, (ctypes.c_float * 3)(0.5, float("inf"), 2), 3, s3, 3, out), (16, (ctypes.c_float * 11)(*[1.0] * 11), 11, s3, 3, out)):
        assert lib.fhip_roi_generate_anchors(*args) == bad, args[0:1] + args[2:3] + args[4:5]
    size = ctypes.c_size_t()
    assert lib.fhip_proposal_get_buffer_size(2, 9, 38, 50, ctypes.byref(size)) == 0 and size.value == 2 * 9 * 38 * 50 * 8
    for args in ((0, 9, 2, 2), (65536, 9, 2, 2), (1, 0, 2, 2), (1, 33, 2, 2), (1, 9, 0, 2), (1, 9, 2, 0), (1, 9, 4097, 4096), (1, 9, 2048, 1024), (60, 9, 2048, 512)):
        assert lib.fhip_proposal_get_buffer_size(*args, ctypes.byref(size)) == bad, args
    assert lib.fhip_proposal_get_buffer_size(1, 9, 2, 2, None) == bad
    # the Proposal: a call that passes every check but the one named (no stream is ever touched: each is refused first)
    nan, inf = float("nan"), float("inf")
    hostile = (ctypes.c_float * 36)(*([1.0] * 35 + [nan]))
    for what, kw in (("n", dict(n=0)), ("anchors", dict(A=33)), ("extent", dict(h=0)), ("stride", dict(stride=0)), ("stride overflow", dict(stride=1 << 30)),
                     ("after 0", dict(after=0)), ("after", dict(after=2049)), ("nan thresh", dict(nms=nan)), ("inf thresh", dict(nms=inf)), ("nan min_size", dict(min_size=nan)),
                     ("no anchors", dict(anchors=None)), ("nan anchor", dict(anchors=hostile)), ("null rois", dict(rois=None)), ("null score", dict(score=None)),
                     ("null bbox", dict(bbox=None)), ("null info", dict(info=None)), ("null scratch", dict(scratch=None)), ("misaligned rois", dict(rois=0x1002)),
                     ("misaligned scores", dict(scores=0x2002)), ("misaligned score", dict(score=0x3001)), ("misaligned bbox", dict(bbox=0x4002)),
                     ("misaligned info", dict(info=0x5003)), ("misaligned scratch", dict(scratch=0x6004)), ("rois over score", dict(rois=0x3000 + 16)),
                     ("rois over bbox", dict(rois=0x4000 + 64)), ("rois over info", dict(rois=0x5000 - 8)), ("scores over bbox", dict(scores=0x4000 + 8)),
                     ("scratch over score", dict(scratch=0x3000 + 8)), ("rois over scratch", dict(rois=0x6000 + 8)), ("scores over rois", dict(scores=0x1000 + 32)),
                     ("scores over scratch", dict(scores=0x6000 + 16))):
        assert _proposal(lib, **kw) == bad, what
        assert lib.fhip_roi_last_error() != b"", what
    # the ROI layers: (n, c, h, w, R, pooled_w, pooled_h, scale)
    good = (1, 18, 6, 6, 4, 3, 3, 0.25)
    ptrs = (V(0x1000), V(0x10000), V(0x20000), None)
    calls = {"pool": lambda a, p=ptrs: lib.fhip_roi_pool_forward(*a, *p), "align": lambda a, p=ptrs: lib.fhip_roi_align_forward(*a, 2, 0, 1, *p),
             "psroi": lambda a, p=ptrs: lib.fhip_psroi_pool_forward(*a, 2, *p)}
    for name, call in calls.items():
        for k, v in ((0, 0), (1, 0), (2, 0), (3, 0), (4, 0), (5, 0), (6, 0), (5, 65), (6, 65), (7, nan), (7, inf), (0, 1 << 30), (4, 1 << 30)):
            a = list(good)
            a[k] = v
            assert call(a) == bad, (name, k, v)
        for p in ((None, V(0x10000), V(0x20000), None), (V(0x1000), None, V(0x20000), None), (V(0x1000), V(0x10000), None, None), (V(0x1002), V(0x10000), V(0x20000), None),
                  (V(0x1000), V(0x10001), V(0x20000), None), (V(0x1000), V(0x10000), V(0x20002), None), (V(0x10000 + 64), V(0x10000), V(0x20000), None),
                  (V(0x20000 + 16), V(0x10000), V(0x20000), None)):
            assert call(good, p) == bad, (name, p)
    for extra in ((2, 0, 2), (2, 2, 0), (2, -1, 1), (-1, 0, 1), (4097, 0, 1)):  # (sampling_ratio, aligned, version)
        assert lib.fhip_roi_align_forward(*good, *extra, *ptrs) == bad, extra
    assert lib.fhip_psroi_pool_forward(*good, 3, *ptrs) == bad and b"output_dim" in lib.fhip_roi_last_error()  # 3 * 9 != 18
    assert lib.fhip_psroi_pool_forward(*good, 0, *ptrs) == bad
    name = ctypes.create_string_buffer(64)
    for args in ((0, 0, 0), (6, 0, 0), (-1, 0, 0), (4, 2, 0), (4, -1, 0)):
        assert lib.fhip_roi_route(*args, name, 64) == bad, args
    assert lib.fhip_roi_route(1, 0, 0, None, 64) == bad and lib.fhip_roi_route(1, 0, 0, name, 0) == bad
    seen = set()
    for args in ((1, 0, 0), (2, 0, 0), (3, 0, 0), (4, 0, 0), (4, 1, 0), (5, 0, 0)):
        assert lib.fhip_roi_route(*args, name, 64) == 0
        seen.add(name.value.decode())
    assert seen == C.targets()


def test_the_python_mirror_refuses_tensors_that_are_not_on_the_device():
    import torch
    from feathercnn_amd import roi
    with pytest.raises(ValueError, match="CUDA"):
        roi.roi_pool(torch.zeros(1, 1, 4, 4), torch.zeros(1, 1, 4))
    with pytest.raises(ValueError, match="CUDA"):
        roi.roi_align(np.zeros((1, 1, 4, 4), F), np.zeros((1, 1, 4), F))
    with pytest.raises(ValueError, match="CUDA"):
        roi.psroi_pool(torch.zeros(1, 18, 4, 4), torch.zeros(1, 1, 4), 2, 3)
    with pytest.raises(ValueError, match="CUDA"):
        roi.proposal(torch.zeros(1, 18, 2, 2), torch.zeros(1, 36, 2, 2), torch.zeros(1, 3))


# ---- the zoo -------------------------------------------------------------------------------------------------------------------------------
def _load(name, p, **off):
    kw = dict(roi=True, detection=True)
    kw.update(off)
    from feathercnn_amd.net import Net
    net = Net()
    net.SetRoi(kw["roi"])
    net.SetDetection(kw["detection"])
    net.SetDilated(name == "rfcn_resnet50" and not off.get("no_dilated"))
    net.LoadParam(p)
    return net


def test_zoo_nets_build_and_load_with_their_switches():
    from feathercnn_amd import FeatherHipError, model_zoo
    assert model_zoo.ROI_NETS == ("tiny_faster_rcnn", "tiny_rfcn", "faster_rcnn_vgg16", "rfcn_resnet50") and all(n in model_zoo.MODELS for n in model_zoo.ROI_NETS)
    for name, roi_layers in zip(model_zoo.ROI_NETS, (2, 2, 2, 3)):
        p, nbytes, i, o = model_zoo.MODELS[name](dry=True)
        types = [t for t, *_ in R.parse_param(p)]
        assert types.count("Input") == 2 and types.count("Proposal") == 1 and (i, o) == ("data", "cls_score" if name == "tiny_rfcn" else "cls_prob")
        net = _load(name, p)
        assert sum(a == "ROI" for _, _, a in net.layers()) == roi_layers
        for off in (dict(roi=False), dict(detection=False)) + ((dict(no_dilated=True),) if name == "rfcn_resnet50" else ()):
            with pytest.raises(FeatherHipError):
                _load(name, p, **off)
    p, nbytes, _, _ = model_zoo.faster_rcnn_vgg16(dry=True)
    layers = {nm: (t, pd) for t, nm, _, _, pd in R.parse_param(p)}
    assert layers["rois"][1] == {0: 16, 1: 16, 2: 6000, 3: 300, 4: 0.7, 5: 16} and layers["roi_pool5"] == ("ROIPooling", {0: 7, 1: 7, 2: 0.0625})
    assert layers["fc6"][1][2] == 512 * 49 * 4096 and layers["cls_score"][1][0] == 21 and layers["bbox_pred"][1][0] == 84 and "pool5" not in layers
    assert 136.6e6 < nbytes / 4 < 137.5e6  # VGG-16 Faster R-CNN has 137 M parameters
    p, nbytes, _, _ = model_zoo.rfcn_resnet50(dry=True)
    layers = {nm: (t, pd) for t, nm, _, _, pd in R.parse_param(p)}
    assert layers["psroipooled_cls_rois"] == ("PSROIPooling", {0: 7, 1: 7, 2: 0.0625, 3: 21}) and layers["psroipooled_loc_rois"][1][3] == 8
    assert layers["rfcn_cls"][1][0] == 21 * 49 and layers["res5a_branch2b"][1][2] == 2 and layers["res5a_branch2a"][1][3] == 1  # conv5: dilation 2, stride 1


def test_tiny_zoo_nets():
    from feathercnn_amd import model_zoo
    for name in sorted(C.NETS):
        (p, b, i, o), trace = C.net_model(name)
        assert model_zoo.MODELS[name](dry=True) == (p, len(b), i, o)  # the dry builder writes the same .param and counts the same bytes
        (score, bbox, info), tops, args = C.proposal_args(p)
        assert tops == ["rois"] and info == "im_info" and args["after_nms_topN"] == C.NET_ROIS
        x, im_info, blobs, m = C.net_input(name)
        assert C.stable(m) and m["order"] >= 1e-5 and m["round"] >= 1e-3, m
        assert blobs[score].shape == (3, 18, 12, 16) and blobs[bbox].shape == (3, 36, 12, 16) and blobs["rois"].shape == (3, C.NET_ROIS, 1, 4)
        assert np.allclose(blobs[score][:, :9] + blobs[score][:, 9:], 1, atol=1e-6)  # the two-way softmax
        assert blobs[o].shape == (3 * C.NET_ROIS, 5, 1, 1)
    types = [t for t, *_ in R.parse_param(C.net_model("tiny_faster_rcnn")[0][0])]
    assert types.count("Reshape") == 2 and "ROIPooling" in types and types.count("InnerProduct") == 4
    types = [t for t, *_ in R.parse_param(C.net_model("tiny_rfcn")[0][0])]
    assert "PSROIPooling" in types and types[-1] == "Pooling"
