"""The detection head without a GPU: the Net switch and what it lifts, the param readers of the new layer types under hostile values,
fhip_priorbox_fill (a host function) against the restatement, the restatement (tests/detect_ref.py) against cases computed by hand, the
fused layer lists of tiny_ssd, and the restatement on tiny_ssd end to end.  What the library shares with the other run-time libraries is in
tests/test_detect_contract_cpu.py."""
import numpy as np
import pytest

import detect_cases as DC
import detect_ref as R
from test_resample_cpu import HOSTILE_VALUES

F = np.float32
NEW_TYPES = ("Permute", "Flatten", "Reshape", "Normalize", "PriorBox", "DetectionOutput")


def _net(param, weights=b"", detection=None, extended=False, level=1, load_weights=True):
    from feathercnn_amd.net import Net
    net = Net(fusion=level)
    if detection is not None:
        net.SetDetection(detection)
    if extended:
        net.SetExtendedLayers(True)
    net.LoadParam(param)
    if load_weights:
        net.LoadWeights(weights)
    return net


def _refused(param, code, *words, **kw):
    from feathercnn_amd import FeatherHipError
    with pytest.raises(FeatherHipError) as e:
        _net(param, **kw)
    assert f"code {code}" in str(e.value) and all(w in str(e.value) for w in words), str(e.value)
    return str(e.value)


def _one(type_, params="", bottoms=1, tops=1, extra=""):
    """A .param of an 8-channel 6x6 input (split for the layers that read several bottoms) and one layer `l` of `type_`."""
    ins = " ".join(f"s_{i}" for i in range(bottoms))
    outs = " ".join(["l"] + [f"l{i}" for i in range(1, tops)])
    lines = ["Input data 0 1 data 0=6 1=6 2=8", f"Split s 1 {max(bottoms, 1)} data " + " ".join(f"s_{i}" for i in range(max(bottoms, 1))),
             f"{type_} l {bottoms} {tops} {ins} {outs} {params}".strip()] + ([extra] if extra else [])
    blobs = 1 + max(bottoms, 1) + tops + (1 if extra else 0)
    return ("7767517\n%d %d\n" % (len(lines), blobs) + "\n".join(lines) + "\n").encode()


GOOD = {  # type -> (params that load, bottoms)
    "Permute": ("0=3", 1), "Flatten": ("", 1), "Reshape": ("0=-1 1=8", 1), "Normalize": ("0=0 1=0 2=1e-10 3=8 4=1", 1),
    "PriorBox": ("-23300=1,2.0 -23301=1,3.0 -23302=1,2.0 3=0.1 4=0.1 5=0.2 6=0.2 7=1 8=0 9=-233 10=-233 11=-233.0 12=-233.0 13=0.5", 2),
    "DetectionOutput": ("0=3 1=0.45 2=10 3=5 4=0.5", 3),
}


# ---- the switch ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("type_", NEW_TYPES)
def test_default_net_refuses_the_new_types(type_):
    params, bottoms = GOOD[type_]
    p = _one(type_, params, bottoms)
    msg = _refused(p, -200, type_, "fhip_net_set_detection lifts this")
    assert "fhip_net_set_extended_layers" not in msg
    assert "fhip_net_set_extended_layers" not in _refused(p, -200, type_, extended=True)  # the other switch alone lifts nothing here
    assert "fhip_net_set_detection lifts this" in _refused(p, -200, type_, detection=False)  # on then off is the default
    net = _net(p, detection=True, load_weights=False)
    assert ("%s" % type_, "l", "DETECT") in net.layers()


def test_on_then_off_equals_the_default_and_the_switch_is_refused_after_loadparam():
    from feathercnn_amd import FeatherHipError
    from feathercnn_amd.net import Net
    p = _one("Permute", "0=3")
    net = Net()
    net.SetDetection(True)
    net.SetDetection(False)
    with pytest.raises(FeatherHipError, match="code -200"):
        net.LoadParam(p)
    net = _net(_one("ReLU"))
    with pytest.raises(FeatherHipError, match="before LoadParam") as e:
        net.SetDetection(True)
    assert "code -2" in str(e.value)


@pytest.mark.parametrize("type_", ["PixelShuffle", "Padding"])
def test_types_out_of_scope_stay_unknown_with_the_switch_on(type_):
    msg = _refused(_one(type_), -200, type_, detection=True)
    assert "lifts this" not in msg
    assert "lifts this" not in _refused(_one(type_), -200, type_)


def test_default_net_keeps_concat_and_softmax_as_they_were():
    _refused(_one("Concat", "0=1", 2), -100, "only concat at axis = 0")
    _refused(_one("Concat", "0=1", 2), -100, "only concat at axis = 0", extended=True)
    for params in ("", "0=1", "0=2 1=0", "0=7 1=1"):  # a default Softmax ignores its params
        assert ("Softmax", "l", None) in _net(_one("Softmax", params)).layers()


def test_existing_types_load_as_before_with_the_switch_on():
    for type_, params, bottoms in (("Concat", "0=0", 2), ("Concat", "", 2), ("Softmax", "", 1), ("ReLU", "", 1), ("Concat", "0=2", 2), ("Softmax", "0=1 1=1", 1)):
        layers = _net(_one(type_, params, bottoms), detection=True).layers()
        assert (type_, "l", "DETECT" if type_ != "ReLU" else None) in layers, layers
    _refused(_one("Softmax", "0=1"), -100, "too old", "l", detection=True)  # an axis without fixbug0
    _refused(_one("Softmax", "0=1 1=0"), -100, "too old", detection=True)


# ---- hostile values ------------------------------------------------------------------------------------------------------------------------
IDS = {"Permute": (0,), "Flatten": (), "Reshape": (0, 1, 2, 3), "Normalize": (0, 1, 2, 3, 4, 9), "PriorBox": tuple(range(3, 14)), "DetectionOutput": (0, 1, 2, 3, 4),
       "Concat": (0,), "Softmax": (0, 1)}


@pytest.mark.parametrize("type_", sorted(IDS))
def test_hostile_param_values_are_accepted_or_minus_100(type_):
    """Every id of every type with each of HOSTILE_VALUES in place of its good value: the layer loads, or LoadParam answers -100 and names it."""
    from feathercnn_amd import FeatherHipError
    params, bottoms = GOOD.get(type_, ("0=0", 2 if type_ == "Concat" else 1))
    answers = set()
    for pid in IDS[type_]:
        for v in HOSTILE_VALUES:
            kept = [kv for kv in params.split() if not kv.startswith(f"{pid}=")]
            try:
                _net(_one(type_, " ".join(kept + [f"{pid}={v}"]), bottoms), detection=True, load_weights=False)
                answers.add("ok")
            except FeatherHipError as e:
                assert "code -100" in str(e) and "layer l" in str(e), (type_, pid, v, str(e))
                answers.add("refused")
    assert not IDS[type_] or "ok" in answers
    if type_ in ("Permute", "Reshape", "Normalize", "PriorBox", "DetectionOutput", "Softmax"):
        assert "refused" in answers


@pytest.mark.parametrize("array", ["-23300=0", "-23300=1,0.0", "-23300=1,-2.0", "-23300=1,nan", "-23300=1,inf", "-23300=1,1e39", "-23300=1,2.0 -23301=2,3.0,4.0",
                                   "-23300=1,2.0 -23302=1,0.0", "-23300=1,2.0 -23302=1,-1.0", "-23300=65," + ",".join(["2.0"] * 65)])
def test_hostile_priorbox_arrays(array):
    rest = " ".join(kv for kv in GOOD["PriorBox"][0].split() if not kv.startswith("-233"))
    _refused(_one("PriorBox", array + " " + rest, 2), -100, "layer l", detection=True, load_weights=False)


@pytest.mark.parametrize("type_", NEW_TYPES + ("Softmax",))
def test_wrong_bottom_and_top_counts_are_refused(type_):
    params, bottoms = GOOD.get(type_, ("", 1))
    for b, t in ((bottoms + 1, 1), (bottoms, 2)) + (((bottoms - 1, 1),) if bottoms > 1 else ()):
        _refused(_one(type_, params, b, t), -100, "layer l", detection=True, load_weights=False)


def test_limits_are_refused_by_name():
    _refused(_one("DetectionOutput", "0=257 1=0.45 2=10 3=5 4=0.5", 3), -100, "num_class", detection=True)
    _refused(_one("DetectionOutput", "0=1 1=0.45 2=10 3=5 4=0.5", 3), -100, "num_class", detection=True)
    _refused(_one("DetectionOutput", "0=3 1=0.45 2=1025 3=5 4=0.5", 3), -100, "nms_top_k", detection=True)
    _refused(_one("DetectionOutput", "0=3 1=0.45 2=10 3=0 4=0.5", 3), -100, "keep_top_k", detection=True)
    _refused(_one("Normalize", "0=1 1=0 2=1e-10 3=8 4=1"), -100, "across_spatial", detection=True)
    _refused(_one("Normalize", "0=0 1=0 2=1e-10 3=8 4=0"), -100, "across_channel", detection=True)
    _refused(_one("Normalize", "0=0 1=0 2=1e-10 3=8 4=1 9=1"), -100, "eps_mode", detection=True)
    _refused(_one("Normalize", "0=0 1=0 2=-1.0 3=8 4=1"), -100, "eps", detection=True)
    _refused(_one("Reshape", "0=-1 1=-1"), -100, "at most one", detection=True)
    _refused(_one("Reshape", "0=4 3=1"), -100, "permute", detection=True)


@pytest.mark.parametrize("params", DC.BAD_RESHAPES)
def test_bad_reshapes_load_and_are_left_to_reshape(params):
    """Every extent is a legal value on its own, so LoadParam accepts them; the element count is known at Reshape, behind a fed input, which
    takes a device: tests/test_detect_gpu.py::test_reshape_that_changes_the_element_count_is_minus_300 feeds these nets."""
    net = _net(DC.reshape_of_four(params), detection=True)
    assert ("Reshape", "l", "DETECT") in net.layers()


def test_a_fused_head_never_joins_a_channel_map():
    """Level 2: a ShuffleChannel or a Slice behind a collapsed head.  The head keeps the type string "Concat" and is no ConcatLayer; the
    channel-map pass must ask the object, not the string, and leave both layers as they are."""
    from feathercnn_amd import model_zoo
    for tail in ("shuffle", "slice"):
        g = model_zoo.GraphBuilder(3)
        a, b = g.split("split", g.input("data", 4, 5, 5), 2)
        fa = g.flatten("flat_a", g.permute("perm_a", g.relu("relu_a", a), 3))
        fb = g.flatten("flat_b", g.permute("perm_b", g.conv("conv_b", b, 4, 6, 1), 3))
        cat = g.concat("cat", [fa, fb], 0)
        if tail == "shuffle":
            g.shuffle("tail", cat, 1)
        else:
            g.slice("tail", cat, [-233])
        p, w = g.finish()
        for _ in range(20):  # what lies behind a 128-byte object differs from load to load
            got = _fused_layers(p, w, 2)
            assert got[-2:] == [("Concat", "cat", "DETECT"), ("ShuffleChannel" if tail == "shuffle" else "Slice", "tail", "SHUFFLE")], got
        assert [nm for _, nm, _ in got] == ["data", "split", "relu_a", "conv_b", "cat", "tail"]


# ---- PriorBox, a host function ---------------------------------------------------------------------------------------------------------
PRIORBOX_CASES = [
    dict(h=3, w=3, image_w=30, image_h=30, min_sizes=[6.0]),                                                           # no max sizes, no ratios
    dict(h=5, w=7, image_w=28, image_h=20, min_sizes=[8.0], max_sizes=[12.0], aspect_ratios=[2.0, 3.0], clip=True),    # a non-square map, clip
    dict(h=4, w=4, image_w=33, image_h=31, min_sizes=[4.0, 9.0], max_sizes=[9.0, 14.0], aspect_ratios=[2.0], flip=False),
    dict(h=2, w=3, image_w=300, image_h=300, min_sizes=[60.0], aspect_ratios=[2.0], step_w=64.0, step_h=100.0, offset=0.25),  # explicit steps
    dict(h=1, w=1, image_w=300, image_h=300, min_sizes=[285.0], max_sizes=[300.0], aspect_ratios=[2.0, 3.0], variances=(0.3, 0.4, 0.5, 0.6)),  # a 1x1 map
    dict(h=19, w=19, image_w=300, image_h=300, min_sizes=[60.0], aspect_ratios=[2.0]),                                 # step 300 / 19 is no fp32 number
]


@pytest.mark.parametrize("case", PRIORBOX_CASES, ids=[f"{c['h']}x{c['w']}" for c in PRIORBOX_CASES])
def test_priorbox_fill_equals_the_restatement(case):
    from feathercnn_amd import priorbox
    got, want = priorbox(**case), R.priorbox(**case)
    per = R.num_prior(len(case["min_sizes"]), len(case.get("max_sizes", ())), len(case.get("aspect_ratios", ())), case.get("flip", True))
    assert got.shape == want.shape == (2, 4 * case["h"] * case["w"] * per) and got.dtype == np.float32
    assert np.array_equal(got, want)
    assert np.array_equal(got[1].reshape(-1, 4), np.tile(np.asarray(case.get("variances", (0.1, 0.1, 0.2, 0.2)), F), (got.shape[1] // 4, 1)))
    if case.get("clip"):
        assert got[0].min() >= 0 and got[0].max() <= 1 and (got[0] == 0).any()


def test_priorbox_by_hand():
    """One cell of a 2 x 2 map on a 20 x 20 image, min 4, max 9, ratio 4 with its flip: centre (5, 5), boxes 4 x 4, 6 x 6, 8 x 2 and 2 x 8."""
    got = R.priorbox(2, 2, 20, 20, [4.0], [9.0], [4.0])[0].reshape(2, 2, 4, 4)[0, 0]
    want = np.array([[3, 3, 7, 7], [2, 2, 8, 8], [1, 4, 9, 6], [4, 1, 6, 9]], np.float64) / 20
    assert np.allclose(got, want, rtol=0, atol=1e-7)
    assert np.allclose(R.priorbox(2, 2, 20, 20, [4.0], [9.0], [4.0])[0].reshape(2, 2, 4, 4)[1, 0, 0], np.array([3, 13, 7, 17]) / 20, rtol=0, atol=1e-7)  # rows outer


def test_priorbox_refusals():
    from feathercnn_amd import FeatherHipError, priorbox
    for bad in (dict(h=0), dict(min_sizes=[]), dict(min_sizes=[-1.0]), dict(max_sizes=[3.0, 4.0]), dict(aspect_ratios=[0.0]), dict(offset=float("nan")),
                dict(variances=(0.1, 0.1, float("inf"), 0.2)), dict(image_w=0)):
        with pytest.raises(FeatherHipError, match="code -2"):
            priorbox(**{**PRIORBOX_CASES[1], **bad})


# ---- the restatement by hand -------------------------------------------------------------------------------------------------------------
def _boxes(*xyxy):
    """Priors that decode to themselves (location 0): -> (loc [1][4P], prior [1][2][4P])."""
    b = np.asarray(xyxy, F).reshape(-1)
    return np.zeros((1, b.size), F), np.stack([b, np.tile(F([0.1, 0.1, 0.2, 0.2]), b.size // 4)])[None]


def _conf(*rows):
    return np.asarray(rows, F).reshape(1, -1)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_detection_output_by_hand(dtype):
    # two boxes [0, 0, 2, 2] and [1, 0, 3, 2]: intersection 2, union 6, IoU 1/3 -- on either side of the threshold
    loc, prior = _boxes([0, 0, 2, 2], [1, 0, 3, 2])
    conf = _conf([0.1, 0.9], [0.2, 0.8])
    kept = R.trim(R.detection_output(loc, conf, prior, 2, 0.34, 10, 10, 0.5, dtype))[0]
    assert kept[:, :2].tolist() == [[1, F(0.9)], [1, F(0.8)]] and kept[1, 2:].tolist() == [1, 0, 3, 2]
    m = {}
    dropped = R.trim(R.detection_output(loc, conf, prior, 2, 0.33, 10, 10, 0.5, dtype, m))[0]
    assert dropped[:, :2].tolist() == [[1, F(0.9)]] and abs(m["iou"] - (1 / 3 - float(F(0.33)))) < 1e-6 and abs(m["threshold"] - 0.3) < 1e-6
    # equal scores: the lower prior index goes first and suppresses the other
    tie = R.trim(R.detection_output(loc, _conf([0, 0.7], [0, 0.7]), prior, 2, 0.2, 10, 10, 0.5, dtype))[0]
    assert tie[:, 2:].tolist() == [[0, 0, 2, 2]]
    # equal scores across classes: the lower class goes first
    loc3, prior3 = _boxes([0, 0, 1, 1], [5, 5, 6, 6])
    rows = R.trim(R.detection_output(loc3, _conf([0, 0.6, 0.7], [0, 0.7, 0.6]), prior3, 3, 0.5, 10, 10, 0.5, dtype))[0]
    assert rows[:, 0].tolist() == [1, 2, 1, 2] and rows[:, 1].tolist() == [F(0.7), F(0.7), F(0.6), F(0.6)] and rows[0, 2:].tolist() == [5, 5, 6, 6]
    # no candidate: all rows zero; a score equal to the threshold is none
    none = R.detection_output(loc, _conf([0.9, 0.5], [0.9, 0.1]), prior, 2, 0.45, 10, 4, 0.5, dtype)
    assert none.shape == (1, 4, 6) and not none.any()
    # keep_top_k cuts the merged list; nms_top_k cuts the candidates before the NMS
    cut = R.trim(R.detection_output(loc3, _conf([0, 0.6, 0.7], [0, 0.7, 0.6]), prior3, 3, 0.5, 10, 3, 0.5, dtype))[0]
    assert cut[:, 0].tolist() == [1, 2, 1]
    first = R.trim(R.detection_output(loc3, _conf([0, 0.6, 0.7], [0, 0.7, 0.6]), prior3, 3, 0.5, 1, 10, 0.5, dtype))[0]
    assert first[:, 0].tolist() == [1, 2] and first[:, 1].tolist() == [F(0.7), F(0.7)]
    # the decode: a prior [0, 0, 2, 4] moved by (0.1 * 5 * 2, 0.1 * -5 * 4) and scaled by exp(0.2 * ln 2 / 0.2) = 2 in w
    prior1 = np.stack([F([0, 0, 2, 4]), F([0.1, 0.1, 0.2, 0.2])])[None]
    moved = R.trim(R.detection_output(F([[5, -5, np.log(2) / 0.2, 0]]), _conf([0, 1]), prior1, 2, 0.45, 1, 1, 0.5, dtype))[0]
    assert np.allclose(moved[0, 2:], [2 - 2, 0 - 2, 2 + 2, 0 + 2], rtol=0, atol=1e-5)


def test_permute_normalize_softmax_by_hand():
    x = np.arange(24, dtype=F).reshape(1, 2, 3, 4)
    assert R.permute(x, 3).shape == (1, 3, 4, 2) and R.permute(x, 3)[0, 1, 2].tolist() == [x[0, 0, 1, 2], x[0, 1, 1, 2]]  # NCHW -> NHWC
    for order, shape in enumerate([(2, 3, 4), (2, 4, 3), (3, 2, 4), (3, 4, 2), (4, 2, 3), (4, 3, 2)]):
        assert R.permute(x, order).shape == (1,) + shape and sorted(R.permute(x, order).reshape(-1)) == sorted(x.reshape(-1))
    assert np.array_equal(R.permute(x, 5)[0], x[0].transpose(2, 1, 0)) and np.array_equal(R.permute(x, 0), x)
    y = R.normalize(F([[[[3.0]], [[4.0]]]]), F([2.0, 10.0]), 1e-10)
    assert np.allclose(y.reshape(-1), [1.2, 8.0], rtol=1e-6) and y.dtype == np.float32
    assert np.allclose(R.normalize(F([[[[3.0]], [[4.0]]]]), F([2.0]), 1e-10, True).reshape(-1), [1.2, 1.6], rtol=1e-6)
    assert np.allclose(R.softmax(F([[0.0, np.log(3.0)]]), 1), [[0.25, 0.75]])


# ---- tiny_ssd ----------------------------------------------------------------------------------------------------------------------------
def _fused_layers(param, weights, level):
    from feathercnn_amd import FeatherHipError
    net = _net(param, weights, detection=True, level=level)
    with pytest.raises(FeatherHipError, match="has not been fed"):
        net.Forward()
    return net.layers()


def test_zoo_nets():
    from feathercnn_amd import model_zoo
    assert model_zoo.DETECTION_NETS == ("tiny_ssd", "mobilenet_ssd", "vgg16_ssd300") and all(n in model_zoo.MODELS for n in model_zoo.DETECTION_NETS)
    p, b, i, o = model_zoo.tiny_ssd()
    assert model_zoo.tiny_ssd(dry=True) == (p, len(b), i, o) and R.Net(p, b).read == len(b)
    for name, priors in (("mobilenet_ssd", 1917), ("vgg16_ssd300", 8732)):
        p, nbytes, i, o = model_zoo.MODELS[name](dry=True)
        layers = R.parse_param(p)
        assert (i, o) == ("data", "detection_out") and sum(t == "PriorBox" for t, *_ in layers) == 6 and sum(t == "Permute" for t, *_ in layers) == 12
        assert [nm for t, nm, *_ in layers if t in ("Reshape", "Softmax", "DetectionOutput")] == ["mbox_conf_reshape", "mbox_conf_softmax", "detection_out"]
        net = _net(p, detection=True, load_weights=False) if name == "mobilenet_ssd" else None
        assert net is None or sum(a == "DETECT" for _, _, a in net.layers()) == 12 * 2 + 6 + 3 + 4
    assert "vgg16_ssd300" in model_zoo.DILATED_LAYERS
    p = model_zoo.vgg16_ssd300(dry=True)[0]
    _refused(p, -200, detection=True, load_weights=False)  # it needs SetDilated too
    from feathercnn_amd.net import Net
    net = Net()
    net.SetDetection(True)
    net.SetDilated(True)
    net.LoadParam(p)
    routes = [a for _, _, a in net.layers()]
    assert routes.count("DETECT") == 12 * 2 + 6 + 3 + 4 + 1 and ("Normalize", "conv4_3_norm", "DETECT") in net.layers()  # + the Normalize


def test_fused_layer_lists_of_tiny_ssd():
    p, b, _, _ = DC.tiny_ssd_model()
    every = [nm for _, nm, *_ in R.parse_param(p)]
    heads = [f"{s}_mbox_{k}_{f}" for s in ("conv2_norm", "conv3", "conv4") for k in ("loc", "conf") for f in ("perm", "flat")]
    for level in (0, 1):
        got = _fused_layers(p, b, level)
        names = [nm for _, nm, _ in got]
        assert set(heads) <= set(names) and (level == 1 or names == every)
        routes = {nm: (t, a) for t, nm, a in got}
        assert routes["mbox_loc"] == routes["mbox_conf"] == routes["mbox_priorbox"] == ("Concat", "DETECT") and routes["conv2_norm"] == ("Normalize", "DETECT")
        assert ("relu1" in names) == (level == 0)  # a convolution keeps its own fusions
    got = _fused_layers(p, b, 2)
    names = [nm for _, nm, _ in got]
    assert not set(heads) & set(names) and names == [nm for nm in every if nm in names]
    routes = {nm: (t, a) for t, nm, a in got}
    assert routes["mbox_loc"] == routes["mbox_conf"] == routes["mbox_priorbox"] == ("Concat", "DETECT")
    assert {"conv2_norm", "mbox_conf_reshape", "mbox_conf_softmax", "mbox_conf_flatten", "detection_out", "conv3_mbox_priorbox"} <= set(names)
    assert [nm for t, nm, _ in got if t in ("Permute", "Flatten")] == ["mbox_conf_flatten"]  # twelve layers fewer, two launches for twelve


def test_a_concat_with_a_multi_consumer_link_stays_as_written():
    from feathercnn_amd import model_zoo
    g = model_zoo.GraphBuilder(3)
    a, b = g.split("split", g.input("data", 4, 5, 5), 2)
    pa = g.permute("perm_a", g.relu("relu_a", a), 3)
    pa, also = g.split("again", pa, 2)  # the permuted blob has a second consumer (through the Split)
    fa, fb = g.flatten("flat_a", pa), g.flatten("flat_b", g.permute("perm_b", g.conv("conv_b", b, 4, 6, 1), 3))
    g.concat("cat", [fa, fb], 0)
    g.relu("other", also)
    p, w = g.finish()
    names = [nm for _, nm, _ in _fused_layers(p, w, 2)]
    assert {"perm_a", "flat_a", "perm_b", "flat_b", "cat"} <= set(names)
    g = model_zoo.GraphBuilder(3)  # the same without the second consumer: one layer
    a, b = g.split("split", g.input("data", 4, 5, 5), 2)
    fa = g.flatten("flat_a", g.permute("perm_a", g.relu("relu_a", a), 3))
    fb = g.flatten("flat_b", g.permute("perm_b", g.conv("conv_b", b, 4, 6, 1), 3))
    g.concat("cat", [fa, fb], 0)
    p, w = g.finish()
    got = _fused_layers(p, w, 2)
    assert [nm for _, nm, _ in got] == ["data", "split", "relu_a", "conv_b", "cat"] and got[-1] == ("Concat", "cat", "DETECT")
    g = model_zoo.GraphBuilder(3)  # another order than 3 is no head
    x = g.input("data", 4, 5, 5)
    g.concat("cat", [g.flatten("flat", g.permute("perm", x, 4))], 0)
    p, w = g.finish()
    assert [nm for _, nm, _ in _fused_layers(p, w, 2)] == ["data", "perm", "flat", "cat"]


def test_the_mobilenet_ssd_input_is_stable():
    """The input of tests/test_detect_gpu.py::test_mobilenet_ssd_from_pixels: the float64 restatement of the whole net meets the margins (the
    builder asserts it and searches seeds; here the figures are held too)."""
    px, blobs, margins = DC.mobilenet_ssd_input()
    assert px.shape == (2, 300, 300, 3) and px.dtype == np.uint8 and min(margins.values()) >= DC.MARGIN, margins
    assert blobs["mbox_priorbox"].shape == (1, 1, 2, 4 * 1917) and blobs["detection_out"].shape == (2, 1, 100, 6)
    assert [len(d) for d in R.trim(blobs["detection_out"][:, 0])] == [7, 7]


def test_the_restatement_runs_tiny_ssd():
    x, blobs, margins = DC.tiny_ssd_input()
    p, b, i, o = DC.tiny_ssd_model()
    assert min(margins.values()) >= DC.MARGIN
    shapes = {k: v.shape for k, v in blobs.items()}
    assert shapes["conv2_norm"] == (3, 24, 10, 14) and shapes["conv3_mbox_loc_perm"] == (3, 5, 7, 24) and shapes["conv4_mbox_conf_flat"] == (3, 1, 1, 3 * 4 * 12)
    assert shapes["mbox_loc"] == (3, 1, 1, 4 * 678) and shapes["mbox_conf_reshape"] == (3, 1, 678, 3) and shapes["mbox_priorbox"] == (1, 1, 2, 4 * 678)
    assert shapes[o] == (3, 1, 20, 6)
    net = R.Net(p, b)
    net.run(i, x, o)
    assert net.ranks["mbox_loc"] == 1 and net.ranks["mbox_conf_reshape"] == 2 and net.ranks["mbox_priorbox"] == 2 and net.ranks[o] == 2 and net.ranks["conv2_norm"] == 3
    conf = blobs["mbox_conf_flatten"].reshape(3, 678, 3)
    assert np.allclose(conf.sum(axis=2), 1, atol=1e-6)
    assert np.percentile(conf[:, :, 1:], 5) < 0.1 and np.percentile(conf[:, :, 1:], 95) > 0.7  # the scores spread over (0, 1)
    # the layers under test from their inputs
    assert np.array_equal(blobs["conv3_mbox_loc_perm"], blobs["conv3_mbox_loc"].transpose(0, 2, 3, 1))
    assert np.array_equal(blobs["mbox_loc"].reshape(3, -1), R.permute_concat([blobs[f"{s}_mbox_loc"] for s in ("conv2_norm", "conv3", "conv4")]))
    norms = np.sqrt((blobs["conv2_norm"].astype(np.float64) ** 2 / (np.asarray(R.Net(p, b).w["conv2_norm"], np.float64) ** 2)[None, :, None, None]).sum(axis=1))
    live = (blobs["split2_0"] ** 2).sum(axis=1) > 1e-6
    assert np.allclose(norms[live], 1, atol=1e-5)
    dets = R.trim(blobs[o][:, 0])
    assert all(1 <= len(d) <= 20 for d in dets) and all((np.diff(d[:, 1]) <= 0).all() and set(d[:, 0]) <= {1.0, 2.0} for d in dets)
    # float32 and float64 select the same rows on a stable input
    assert np.array_equal(net.run(i, x, o)[:, 0, :, 0], blobs[o][:, 0, :, 0])
