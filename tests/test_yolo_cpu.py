"""The YOLO layers without a GPU: the restatement against itself in float64 and against hand-computed examples, the committed seeds against
the margins, the Net switch (fhip_net_set_yolo) and what LoadParam answers, every entry's host checks, and the zoo nets' shapes."""
import ctypes
import math

import numpy as np
import pytest

import side_contract as SC
import yolo_cases as C
import yolo_ref as R
from test_resample_cpu import HOSTILE_VALUES

F = np.float32
NEW_TYPES = ("Reorg", "YoloDetectionOutput", "Yolov3DetectionOutput")
GOOD = {  # type -> (params that load, bottoms)
    "Reorg": ("0=2", 1),
    "YoloDetectionOutput": ("0=3 1=1 2=0.25 3=0.45 -23304=2,1.0,2.0", 1),
    "Yolov3DetectionOutput": ("0=3 1=1 2=0.25 3=0.45 -23304=4,1.0,2.0,3.0,4.0 -23305=2,1.0,0.0 -23306=2,32.0,16.0", 2),
}


def _net(param, yolo=None, detection=False, extended=False, load_weights=False):
    from feathercnn_amd.net import Net
    net = Net()
    if yolo is not None:
        net.SetYolo(yolo)
    if detection:
        net.SetDetection(True)
    if extended:
        net.SetExtendedLayers(True)
    net.LoadParam(param)
    if load_weights:
        net.LoadWeights(b"")
    return net


def _refused(param, code, *words, **kw):
    from feathercnn_amd import FeatherHipError
    with pytest.raises(FeatherHipError) as e:
        _net(param, **kw)
    assert f"code {code}" in str(e.value) and all(w in str(e.value) for w in words), str(e.value)
    return str(e.value)


def _one(type_, params="", bottoms=1):
    """A .param of an 8-channel 6x6 input (split for the layers that read several bottoms) and one layer `l` of `type_`."""
    ins = " ".join(f"s_{i}" for i in range(bottoms))
    lines = ["Input data 0 1 data 0=6 1=6 2=8", f"Split s 1 {bottoms} data " + ins, f"{type_} l {bottoms} 1 {ins} l {params}".strip()]
    return ("7767517\n%d %d\n" % (len(lines), 2 + bottoms) + "\n".join(lines) + "\n").encode()


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", C.case_ids(), ids=lambda c: "v%d-%s-n%d-c%d" % c)
def test_committed_seeds_pass_the_margins_and_float32_agrees_with_float64(cid):
    bottoms, args, want64, want32, m = C.case(*cid)
    assert C.stable(m), m  # the generator's own check, on the committed seed: nothing is skipped on the GPU
    assert C.first_stable_seed(*cid, start=C.SEEDS.get(cid, 0))[0] == C.SEEDS.get(cid, 0)
    assert np.array_equal(want32[:, :, 0], want64[:, :, 0]), "labels or row order"
    tol, e32 = C.tolerance(want64, want32)
    assert e32 <= 2.0 ** -20, e32  # a handful of float32 roundings
    counts = [len(d) for d in R.trim(want64)]
    assert min(counts) >= 1 and all(not img[k:].any() for img, k in zip(want64, counts))
    if cid[1] == "three_past_a_chunk":  # more candidates than one selection round takes, fewer survivors than rows
        conf, _, _ = R.scores(bottoms, args["version"], args["num_class"], args["num_box"], np.float64)
        assert (conf >= args["confidence_threshold"]).sum(axis=1).min() > C.CHUNK and max(counts) < args["rows"]
    if cid[1] == "two_past_the_buffer":  # more candidates than the selection buffer holds: it is cut, in each of the first rounds
        conf, _, _ = R.scores(bottoms, args["version"], args["num_class"], args["num_box"], np.float64)
        assert (conf >= args["confidence_threshold"]).sum(axis=1).min() > 3 * C.CHUNK and max(counts) < args["rows"]


def _head(boxes, classes):
    """A 1 x 1-cell bottom [1][len(boxes) * (5 + classes)][1][1] from rows (x, y, w, h, objectness, scores...)."""
    return np.asarray(boxes, F).reshape(1, -1, 1, 1)


def test_version_2_by_hand():
    """One cell, two boxes, two classes.  Box 0: objectness 0 (sigmoid 1/2), scores (0, ln 3): softmax (1/4, 3/4), class 1, confidence 3/8.
    x = y = 0: the centre (1/2, 1/2); w = ln 2 with bias 0.25: bw = 1/2; h = 0 with bias 0.5: bh = 1/2: the box (1/4, 1/4, 3/4, 3/4).
    Box 1: objectness -30: confidence below any threshold."""
    x = _head([[0, 0, math.log(2), 0, 0, 0, math.log(3)], [0, 0, 0, 0, -30, 1, 0]], 2)
    for dtype in (np.float32, np.float64):
        out = R.detection([x], 2, 2, 2, [0.25, 0.5, 1, 1], 0.25, 0.45, 4, dtype=dtype)
        assert out.shape == (1, 4, 6) and not out[0, 1:].any()
        assert np.allclose(out[0, 0], [2, 0.375, 0.25, 0.25, 0.75, 0.75], rtol=1e-6, atol=0)
    assert not R.detection([x], 2, 2, 2, [0.25, 0.5, 1, 1], 0.5, 0.45, 4).any()  # 3/8 is below 1/2: no candidate


def test_version_3_by_hand():
    """One cell, one box per bottom, two bottoms.  Bottom 0: objectness ln 3 (sigmoid 3/4), raw scores (-9, ln 3): class 1, confidence 9/16; mask 1:
    the anchor (8, 16), stride 32: bw = e^0 * 8 / 32 = 1/4, bh = 16 / 32 = 1/2: the box (3/8, 1/4, 5/8, 3/4).  Bottom 1: the same values and
    mask 0, the anchor (4, 4), stride 16: a box (3/8, 3/8, 5/8, 5/8) of equal confidence -- the later index -- inside the first, IoU 1/2."""
    x = _head([[0, 0, 0, 0, math.log(3), -9, math.log(3)]], 2)
    args = dict(version=3, num_class=2, num_box=1, biases=[4, 4, 8, 16], mask=[1, 0], anchors_scale=[32, 16], confidence_threshold=0.5, rows=3)
    for dtype in (np.float32, np.float64):
        out = R.detection([x, x], nms_threshold=0.6, dtype=dtype, **args)
        assert np.allclose(out[0, 0], [2, 0.5625, 0.375, 0.25, 0.625, 0.75], rtol=1e-6) and np.allclose(out[0, 1], [2, 0.5625, 0.375, 0.375, 0.625, 0.625], rtol=1e-6)
        assert not out[0, 2].any()
        out = R.detection([x, x], nms_threshold=0.4, dtype=dtype, **args)  # IoU 1/2 > 0.4: the second is suppressed
        assert out[0, 0, 0] == 2 and not out[0, 1:].any()


def test_reorg_by_hand():
    x = np.arange(2 * 4 * 6, dtype=F).reshape(1, 2, 4, 6)
    y = R.reorg(x, 2)
    assert y.shape == (1, 8, 2, 3) and np.array_equal(y[0, 0], [[0, 2, 4], [12, 14, 16]]) and np.array_equal(y[0, 3], [[7, 9, 11], [19, 21, 23]])
    assert np.array_equal(y[0, 4], 24 + y[0, 0]) and np.array_equal(R.reorg(x, 2, 1)[0, 1], y[0, 4])  # mode 1: channel (sh * s + sw) * c + q
    assert R.reorg(np.zeros((1, 1, 7, 9), F), 2).shape == (1, 4, 3, 4)  # rounded down


# ---- the switch --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("type_", NEW_TYPES)
def test_default_net_refuses_the_new_types(type_):
    params, bottoms = GOOD[type_]
    p = _one(type_, params, bottoms)
    msg = _refused(p, -200, type_)
    assert msg.rstrip().endswith("(fhip_net_set_yolo lifts this)"), msg
    for other in (dict(detection=True), dict(extended=True), dict(detection=True, extended=True)):  # the other switches alone lift nothing here
        assert "fhip_net_set_yolo lifts this" in _refused(p, -200, type_, **other)
    net = _net(p, yolo=8)
    assert (type_, "l", "YOLO") in net.layers()
    assert (type_, "l", "YOLO") in _net(p, yolo=8, detection=True, extended=True).layers()


def test_on_then_off_equals_the_default_and_the_switch_is_refused_after_loadparam():
    from feathercnn_amd import FeatherHipError
    from feathercnn_amd.net import Net
    net = Net()
    net.SetYolo()
    net.SetYolo(0)
    with pytest.raises(FeatherHipError, match="code -200") as e:
        net.LoadParam(_one("Reorg", "0=2"))
    assert "fhip_net_set_yolo lifts this" in str(e.value)
    net = _net(_one("ReLU"))
    with pytest.raises(FeatherHipError, match="before LoadParam") as e:
        net.SetYolo()
    assert "code -2" in str(e.value)
    for rows in (-1, 1025):
        with pytest.raises(FeatherHipError, match="code -2"):
            Net().SetYolo(rows)
    Net().SetYolo(1024)


@pytest.mark.parametrize("type_", ["PixelShuffle", "Padding"])
def test_types_out_of_scope_stay_unknown_with_the_switch_on(type_):
    assert "lifts this" not in _refused(_one(type_), -200, type_, yolo=8)
    assert "lifts this" not in _refused(_one(type_), -200, type_, yolo=8, detection=True, extended=True)


# ---- hostile values ------------------------------------------------------------------------------------------------------------------------
IDS = {"Reorg": (0, 1), "YoloDetectionOutput": (0, 1, 2, 3), "Yolov3DetectionOutput": (0, 1, 2, 3)}


@pytest.mark.parametrize("type_", NEW_TYPES)
def test_hostile_param_values_load_or_are_minus_100_naming_the_id(type_):
    from feathercnn_amd import FeatherHipError
    params, bottoms = GOOD[type_]
    answers = set()
    for pid in IDS[type_]:
        for v in HOSTILE_VALUES:
            kept = [kv for kv in params.split() if not kv.startswith(f"{pid}=")]
            try:
                _net(_one(type_, " ".join(kept + [f"{pid}={v}"]), bottoms), yolo=8)
                answers.add("ok")
            except FeatherHipError as e:
                # (a num_box that no longer matches the arrays is refused at the array: the message then names that id)
                assert "code -100" in str(e) and "layer l" in str(e) and (f"({pid}=" in str(e) or (pid == 1 and "(-2330" in str(e))), (type_, pid, v, str(e))
                answers.add("refused")
    assert answers == {"ok", "refused"}


@pytest.mark.parametrize("arrays,word", [
    ("", "-23304"), ("-23304=0", "-23304"), ("-23304=3,1.0,2.0,3.0", "-23304"), ("-23304=2,1.0,nan", "-23304"), ("-23304=2,inf,1.0", "-23304"),
    ("-23304=130," + ",".join(["1.0"] * 130), "-23304")])
def test_hostile_biases(arrays, word):
    for type_ in ("YoloDetectionOutput", "Yolov3DetectionOutput"):
        rest = " ".join(kv for kv in GOOD[type_][0].split() if not kv.startswith("-23304"))
        _refused(_one(type_, rest + " " + arrays, GOOD[type_][1]), -100, "layer l", word, yolo=8)
    _refused(_one("YoloDetectionOutput", "0=3 1=2 -23304=2,1.0,2.0"), -100, "layer l", "-23304", yolo=8)  # fewer pairs than boxes


@pytest.mark.parametrize("arrays,word", [
    ("-23306=2,32.0,16.0", "-23305"), ("-23305=1,0.0 -23306=2,32.0,16.0", "-23305"), ("-23305=2,0.0,2.0 -23306=2,32.0,16.0", "-23305"),
    ("-23305=2,0.0,-1.0 -23306=2,32.0,16.0", "-23305"), ("-23305=2,0.0,0.5 -23306=2,32.0,16.0", "-23305"), ("-23305=2,0.0,nan -23306=2,32.0,16.0", "-23305"),
    ("-23305=2,1.0,0.0", "-23306"), ("-23305=2,1.0,0.0 -23306=1,32.0", "-23306"), ("-23305=2,1.0,0.0 -23306=2,32.0,0.0", "-23306"),
    ("-23305=2,1.0,0.0 -23306=2,32.0,inf", "-23306"), ("-23305=2,1.0,0.0 -23306=2,-1.0,16.0", "-23306")])
def test_hostile_masks_and_anchor_scales(arrays, word):
    _refused(_one("Yolov3DetectionOutput", "0=3 1=1 2=0.25 3=0.45 -23304=4,1.0,2.0,3.0,4.0 " + arrays, 2), -100, "layer l", word, yolo=8)


def test_wrong_bottom_and_top_counts_are_refused():
    _refused(_one("Reorg", "0=2", 2), -100, "layer l", yolo=8)
    _refused(_one("YoloDetectionOutput", GOOD["YoloDetectionOutput"][0], 5), -100, "layer l", yolo=8)


# ---- the C-ABI's host checks: none of these calls needs (or reaches) a GPU -------------------------------------------------------------------
def _ints(*v):
    return (ctypes.c_int * len(v))(*v)


def _floats(*v):
    return (ctypes.c_float * len(v))(*v)


def _detect(lib, version=2, n=1, scales=1, num_box=1, num_class=1, h=(2,), w=(2,), conf=0.5, nms=0.45, biases=(1.0, 1.0), mask=(0,), scale=(1.0,), rows=4,
            out=4096, bottoms=(8192,), scratch=16384, num_biases=None):
    V = ctypes.c_void_p
    return lib.fhip_yolo_detection_forward(version, n, scales, num_box, num_class, _ints(*h), _ints(*w), conf, nms, _floats(*biases) if biases else None,
                                           len(biases) if num_biases is None else num_biases, _ints(*mask) if mask else None, _floats(*scale) if scale else None,
                                           rows, V(out), (V * len(bottoms))(*bottoms), V(scratch), None)


def test_every_entry_refuses_bad_arguments_on_the_host():
    lib = SC.library("yolo")
    bad = SC.BADARG
    o = [ctypes.c_int() for _ in range(3)]
    refs = [ctypes.byref(v) for v in o]
    assert lib.fhip_reorg_output_dim(2, 3, 7, 9, *refs) == 0 and [v.value for v in o] == [12, 3, 4]
    for args in ((0, 1, 4, 4), (2, 0, 4, 4), (2, 1, 1, 4), (2, 1, 4, 1), (-1, 1, 4, 4), (1 << 15, 2, 1 << 15, 1 << 15)):
        assert lib.fhip_reorg_output_dim(*args, *refs) == bad, args
    assert lib.fhip_reorg_output_dim(2, 1, 4, 4, None, None, None) == bad
    assert lib.fhip_reorg_forward(2, 0, 1, 1, 4, 4, None, None, None) == bad  # NULL pointers
    assert lib.fhip_reorg_forward(2, 2, 1, 1, 4, 4, 4096, 8192, None) == bad and b"mode" in lib.fhip_yolo_last_error()
    assert lib.fhip_reorg_forward(2, 0, 0, 1, 4, 4, 4096, 8192, None) == bad  # n < 1
    assert lib.fhip_reorg_forward(2, 0, 1, 1 << 16, 1 << 8, 1 << 8, 4096, 1 << 40, None) == bad  # 2^32 elements
    assert lib.fhip_reorg_forward(2, 0, 1, 1, 4, 4, 4098, 8192, None) == bad  # misaligned
    assert lib.fhip_reorg_forward(2, 0, 1, 1, 4, 4, 4096, 4096 + 32, None) == bad  # overlapping
    size = ctypes.c_size_t()
    assert lib.fhip_yolo_get_buffer_size(2, 2, 3, 20, _ints(11, 22), _ints(11, 22), ctypes.byref(size)) == 0 and size.value == 2 * 3 * (121 + 484) * 8
    for args in ((0, 1, 1, 1), (65536, 1, 1, 1), (1, 0, 1, 1), (1, 5, 1, 1), (1, 1, 0, 1), (1, 1, 17, 1), (1, 1, 1, 0), (1, 1, 1, 257)):
        assert lib.fhip_yolo_get_buffer_size(*args, _ints(2, 2, 2, 2, 2), _ints(2, 2, 2, 2, 2), ctypes.byref(size)) == bad, args
    assert lib.fhip_yolo_get_buffer_size(1, 1, 1, 1, _ints(0), _ints(2), ctypes.byref(size)) == bad
    assert lib.fhip_yolo_get_buffer_size(1, 1, 1, 1, _ints(2049), _ints(2048), ctypes.byref(size)) == bad  # more than 2^22 boxes
    assert lib.fhip_yolo_get_buffer_size(1, 1, 16, 1, _ints(512), _ints(513), ctypes.byref(size)) == bad
    assert lib.fhip_yolo_get_buffer_size(600, 1, 1, 250, _ints(128), _ints(128), ctypes.byref(size)) == bad  # a bottom of 2^31 elements
    assert lib.fhip_yolo_get_buffer_size(1, 1, 1, 1, None, None, ctypes.byref(size)) == bad and lib.fhip_yolo_get_buffer_size(1, 1, 1, 1, _ints(2), _ints(2), None) == bad
    # the detection: a call that passes every check but the one named (no stream is ever touched: each is refused first)
    for what, kw in (("version", dict(version=4)), ("rows 0", dict(rows=0)), ("rows", dict(rows=1025)), ("nan threshold", dict(conf=float("nan"))),
                     ("inf threshold", dict(nms=float("inf"))), ("no biases", dict(biases=None, num_biases=2)), ("odd biases", dict(biases=(1.0, 1.0, 1.0))),
                     ("short biases", dict(num_box=2)), ("nan bias", dict(biases=(1.0, float("nan")))), ("too many biases", dict(biases=(1.0,) * 130)),
                     ("no mask", dict(version=3, mask=None)), ("no scale", dict(version=3, scale=None)), ("mask outside", dict(version=3, mask=(1,))),
                     ("negative mask", dict(version=3, mask=(-1,))), ("scale 0", dict(version=3, scale=(0.0,))), ("scale nan", dict(version=3, scale=(float("nan"),))),
                     ("null out", dict(out=None)), ("null bottom", dict(bottoms=(None,))), ("null scratch", dict(scratch=None)), ("misaligned out", dict(out=4098)),
                     ("misaligned bottom", dict(bottoms=(8194,))), ("misaligned scratch", dict(scratch=16388)), ("out over bottom", dict(out=8192 + 16)),
                     ("scratch over bottom", dict(scratch=8192 + 16)), ("out over scratch", dict(out=16384 + 8)), ("n", dict(n=0)), ("scales", dict(scales=5)),
                     ("classes", dict(num_class=257)), ("boxes", dict(num_box=17)), ("extent", dict(h=(0,)))):
        assert _detect(lib, **kw) == bad, what
        assert lib.fhip_yolo_last_error() != b"", what
    name = ctypes.create_string_buffer(64)
    for args in ((0, 0, 4), (0, 2, 0), (1, 4, 0), (1, 0, 0), (9, 0, 0)):
        assert lib.fhip_yolo_route(*args, name, 64) == bad, args
    assert lib.fhip_yolo_route(2, 0, 0, None, 64) == bad and lib.fhip_yolo_route(2, 0, 0, name, 0) == bad
    seen = set()
    for args in ((0, 2, 26), (0, 1, 26), (0, 2, 4096), (1, 2, 0), (1, 3, 0), (2, 0, 0)):
        assert lib.fhip_yolo_route(*args, name, 64) == 0
        seen.add(name.value.decode())
    assert seen == C.targets()


def test_the_python_mirror_holds_the_header_limits():
    import re
    from feathercnn_amd import yolo
    text = open(SC.INCLUDE + "/feather_hip/feather_yolo.h").read()
    for macro, value in (("FHIP_YOLO_MAX_SCALES", yolo.MAX_SCALES), ("FHIP_YOLO_MAX_BOXES", yolo.MAX_BOXES), ("FHIP_YOLO_MAX_CLASSES", yolo.MAX_CLASSES),
                         ("FHIP_YOLO_MAX_CELLS", yolo.MAX_CELLS), ("FHIP_YOLO_MAX_ROWS", yolo.MAX_ROWS), ("FHIP_YOLO_CHUNK", yolo.CHUNK),
                         ("FHIP_REORG_TILE", yolo.REORG_TILE), ("FHIP_YOLO_NET_ROUTE", yolo.NET_ROUTE)):
        assert eval(re.search(r"#define\s+%s\s+(.+)" % macro, text).group(1)) == value, macro
    assert yolo.CHUNK == C.CHUNK and (yolo.REORG, yolo.SCORE, yolo.SELECT) == (0, 1, 2)
    assert yolo.reorg_output_dim(2, 64, 26, 26) == (256, 13, 13) and yolo.yolo_route(yolo.REORG, 2, 26) == "fhip::reorg_tile_kernel"


def test_the_python_mirror_refuses_tensors_that_are_not_on_the_device():
    import torch
    from feathercnn_amd import yolo
    with pytest.raises(ValueError, match="CUDA"):
        yolo.reorg(torch.zeros(1, 1, 4, 4), 2)
    with pytest.raises(ValueError, match="CUDA"):
        yolo.yolo_detection([torch.zeros(1, 6, 2, 2)], 1, 1, [1.0, 1.0])
    with pytest.raises(ValueError, match="CUDA"):
        yolo.reorg(np.zeros((1, 1, 4, 4), F), 2)


# ---- the zoo -------------------------------------------------------------------------------------------------------------------------------
def test_zoo_nets_have_the_published_shapes():
    from feathercnn_amd import model_zoo
    assert model_zoo.YOLO_NETS == ("tiny_yolov2", "tiny_yolov3", "yolov2_tiny_voc", "mobilenetv2_yolov3") and all(n in model_zoo.MODELS for n in model_zoo.YOLO_NETS)
    p, nbytes, i, o = model_zoo.yolov2_tiny_voc(dry=True)
    s = R.shapes(p)
    heads, args = C.head_args(p)
    assert [s[h] for h in heads] == [(125, 13, 13)] and args["num_box"] == 5 and args["num_class"] == 20 and len(args["biases"]) == 10
    assert 15.8e6 < nbytes / 4 < 15.95e6  # tiny-yolo-voc has 15.87 M parameters
    p, nbytes, i, o = model_zoo.mobilenetv2_yolov3(dry=True)
    s = R.shapes(p)
    heads, args = C.head_args(p)
    assert [s[h] for h in heads] == [(3 * (5 + 20), 11, 11), (3 * (5 + 20), 22, 22)]
    assert args["version"] == 3 and args["mask"] == [3, 4, 5, 0, 1, 2] and args["anchors_scale"] == [32.0, 16.0] and len(args["biases"]) == 12
    for name in model_zoo.YOLO_NETS:  # every one loads with its switches, and not without
        p, _, _, _ = model_zoo.MODELS[name](dry=True)
        net = _net(p, yolo=64, extended=name == "tiny_yolov3")
        assert sum(a == "YOLO" for _, _, a in net.layers()) == (2 if name == "tiny_yolov2" else 1)
        _refused(p, -200, "lifts this")


def test_tiny_zoo_nets():
    from feathercnn_amd import model_zoo
    for name, extents in (("tiny_yolov2", [(16, 6, 10)]), ("tiny_yolov3", [(16, 4, 6), (16, 8, 12)])):
        (p, b, i, o), trace = C.net_model(name)
        assert model_zoo.MODELS[name](dry=True) == (p, len(b), i, o)  # the dry builder writes the same .param and counts the same bytes
        heads, args = C.head_args(p)
        assert list(heads) == list(C.NETS[name]["heads"]) and [R.shapes(p)[h] for h in heads] == extents
        x, blobs, want64, m = C.net_input(name)
        assert C.stable(m), m
        assert [blobs[h].shape[1:] for h in heads] == extents
    types = [t for t, *_ in R.parse_param(C.net_model("tiny_yolov2")[0][0])]
    assert "Reorg" in types and "Concat" in types and types[-1] == "YoloDetectionOutput"
    types = [t for t, *_ in R.parse_param(C.net_model("tiny_yolov3")[0][0])]
    assert "Interp" in types and "Concat" in types and types[-1] == "Yolov3DetectionOutput"
    # numpy_forward's Reorg is the restatement's
    x = np.random.default_rng(1).uniform(-1, 1, (2, 3, 7, 9)).astype(F)
    for mode in (0, 1):
        assert np.array_equal(model_zoo.numpy_forward([("reorg", "r", "x", "r", dict(stride=2, mode=mode))], "x", x)["r"], R.reorg(x, 2, mode))
