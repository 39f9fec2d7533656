"""feather::Net with int8 activations between int8 layers (Net.SetRequantized, libfeather_q8.so) on the MI355X: tiny_requant equals its twin
run on the device and the numpy restatement (tests/q8_ref.net_forward) bit for bit, at every fusion level that loads it, with and without
graph mode, after re-planning, with a reader whose scale differs; and what cannot read a q8 blob is refused with NET_E_TOPOLOGY (-300)."""
import numpy as np
import pytest

import q8_ref as Q

pytestmark = pytest.mark.gpu
F = np.float32
FP32_BLOBS = ("relu_pw", "side", "pool", "fc")  # what every level keeps of the fp32 blobs
_REF = {}


def _x(n=3, size=16, seed=41):
    return np.random.default_rng(seed).uniform(-1, 1, (n, 3, size, size)).astype(F)


def _want(bn, level, mismatch=None):
    """The restatement's blobs for the seeded batch-3 input, computed once per model and level."""
    key = (bn, level, mismatch)
    if key not in _REF:
        from feathercnn_amd import model_zoo
        _REF[key] = Q.net_forward(model_zoo.tiny_requant(bn=bn, mismatch=mismatch), _x(), level)
    return _REF[key]


def _net(model, level, graph=False, requantized=True):
    from feathercnn_amd.net import Net
    net = Net(fusion=level, graph=graph)
    net.SetQuantized(True)
    if requantized:
        net.SetRequantized(True)
    net.LoadParam(model[0])
    net.LoadWeights(model[1])
    return net


def _run(net, x, names=FP32_BLOBS, forwards=1):
    net.FeedInput("data", x)
    for _ in range(forwards):
        net.Forward()
    return {k: net.Extract(k) for k in names}


@pytest.mark.parametrize("bn,level", [(True, 2), (True, 3), (False, 0), (False, 1), (False, 2), (False, 3)])
@pytest.mark.parametrize("graph", [False, True], ids=["plain", "graph"])
def test_tiny_requant_equals_its_twin_and_the_restatement(cuda, bn, level, graph):
    from feathercnn_amd import model_zoo
    x = _x()
    want = _want(bn, min(level, 2))
    net = _net(model_zoo.tiny_requant(bn=bn), level, graph)
    got = _run(net, x, forwards=2 if graph else 1)  # the second Forward replays the captured graph
    twin = _run(_net(model_zoo.tiny_requant(bn=bn, twin=True), level, graph, requantized=False), x)
    routed = [nm for _, nm, a in net.layers() if a == "QCONV"]
    assert routed == list(model_zoo.QUANT_LAYERS["tiny_requant"])
    if level >= 2 and bn:
        assert not {"BatchNorm", "Scale"} & {t for t, _, _ in net.layers()}  # they exist only folded
    for k in FP32_BLOBS:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (k, int((got[k] != want[k]).sum()))
        assert np.array_equal(got[k], twin[k]), k
    net.close()


@pytest.mark.parametrize("level", [0, 1])
def test_an_unfused_batchnorm_behind_a_requantised_layer_is_refused(cuda, level):
    from feathercnn_amd import FeatherHipError, model_zoo
    net = _net(model_zoo.tiny_requant(), level)
    net.FeedInput("data", _x())
    with pytest.raises(FeatherHipError) as e:
        net.Forward()
    assert "code -300" in str(e.value) and "conv3" in str(e.value) and "conv3_bn" in str(e.value) and "fhip_net_set_" not in str(e.value), str(e.value)


def test_re_planning_to_another_batch_and_size_equals_a_fresh_net(cuda):
    from feathercnn_amd import model_zoo
    model = model_zoo.tiny_requant(fc=False)  # an InnerProduct would pin the input size
    net = _net(model, 2, graph=True)
    for n, size in ((3, 16), (5, 16), (2, 24), (3, 16)):
        x = _x(n, size, seed=n + size)
        got = _run(net, x, names=("relu_pw", "side", "pool"))
        fresh = _net(model, 2)
        ref = _run(fresh, x, names=("relu_pw", "side", "pool"))
        for k in got:
            assert np.array_equal(got[k], ref[k]), (n, size, k)
        if n != 5:
            want = Q.net_forward(model, x, 2)
            assert all(np.array_equal(got[k], want[k]) for k in got), (n, size)
        fresh.close()
    net.close()


@pytest.mark.parametrize("reader", ["conv2", "dw", "side"])
def test_a_reader_with_its_own_scale_equals_the_restatement(cuda, reader):
    from feathercnn_amd import model_zoo
    got = _run(_net(model_zoo.tiny_requant(mismatch=reader), 2), _x())
    want = _want(True, 2, reader)
    assert all(np.array_equal(got[k], want[k]) for k in FP32_BLOBS)
    assert not np.array_equal(got["fc"], _want(True, 2)["fc"])


def test_a_q8_blob_cannot_be_extracted(cuda):
    from feathercnn_amd import FeatherHipError, model_zoo
    net = _net(model_zoo.tiny_requant(), 2)
    _run(net, _x())
    for blob in ("relu1", "pool2", "split_1"):
        with pytest.raises(FeatherHipError) as e:
            net.Extract(blob)
        assert "code -300" in str(e.value) and blob in str(e.value), str(e.value)


def _reader_net(tail):
    """data -> c1 (int8, requantised, 16 channels) -> `tail`: the lines of the layers behind it and their weights."""
    from feathercnn_amd import model_zoo
    g = model_zoo.GraphBuilder(3, quant={})
    x = g.conv("c1", g.input("data", 3, 8, 8), 3, 16, 3, 1, 1, requant=20.0)
    tail(g, x)
    return g.finish()


READERS = {
    "average_pooling": (lambda g, x: g.pool("r", x, 2, 2, avg=True), "Pooling"),
    "eltwise": (lambda g, x: g.eltwise("r", *g.split("s", x)), "Eltwise"),
    "concat": (lambda g, x: g.concat("r", g.split("s", x)), "Concat"),
    "inner_product": (lambda g, x: g.fc("r", x, 16 * 64, 4), "InnerProduct"),
    "fp32_convolution": (lambda g, x: g.conv("r", x, 16, 8, 1, quant=False), "Convolution"),
    "softmax": (lambda g, x: g.softmax("r", x), "Softmax"),
}


@pytest.mark.parametrize("name", sorted(READERS))
def test_a_layer_that_cannot_read_a_q8_blob_is_refused(cuda, name):
    from feathercnn_amd import FeatherHipError
    tail, type_ = READERS[name]
    net = _net(_reader_net(tail), 2)
    net.FeedInput("data", _x(2, 8))
    with pytest.raises(FeatherHipError) as e:
        net.Forward()
    msg = str(e.value)
    assert "code -300" in msg and "layer c1" in msg and type_ + " layer r" in msg and "fhip_net_set_" not in msg and "Requantized" not in msg, msg


@pytest.mark.parametrize("name,size", [("vgg16", 32), ("resnet50", 64), ("mobilenet_v1", 64)])
def test_a_requantised_zoo_net_equals_its_int8_build(cuda, name, size):
    """The _int8_rq builds (every output scale its readers' input scale) at a small input, batch 2, fusion level 2, graph mode: the class
    scores equal those of the _int8 build bit for bit, and no fewer layers report QCONV."""
    from feathercnn_amd import model_zoo
    x = _x(2, size, seed=size)
    out = {}
    for which in ("_int8", "_int8_rq"):
        model = model_zoo.MODELS[name + which](size=size, classes=10)
        net = _net(model, 2, graph=True, requantized=which == "_int8_rq")
        net.FeedInput(model[2], x)
        net.Forward()
        out[which] = (net.Extract(model[3]), sum(a == "QCONV" for _, _, a in net.layers()))
        net.close()
    assert out["_int8"][1] == out["_int8_rq"][1] > 10
    assert np.isfinite(out["_int8"][0]).all() and np.array_equal(out["_int8"][0], out["_int8_rq"][0])


@pytest.mark.parametrize("level", [0, 2])
def test_a_relu_on_a_shared_q8_blob_leaves_the_other_reader_its_bytes(cuda, level):
    """c1 (requantised) -> Split -> {ReLU -> ra, rb} -> sum: the ReLU of a q8 blob runs in place only where it alone reads the blob; here rb
    reads the same bytes, so the ReLU writes a top of its own and rb still sees the negative values."""
    from feathercnn_amd import model_zoo
    g = model_zoo.GraphBuilder(7, quant={})
    x = g.conv("c1", g.input("data", 3, 8, 8), 3, 16, 3, 1, 1, requant=40.0)
    a, b = g.split("s", x)
    a = g.conv("ra", g.relu("relu_a", a), 16, 8, 1, quant=40.0)
    b = g.conv("rb", b, 16, 8, 1, quant=40.0)
    g.eltwise("sum", a, b)
    model = g.finish()
    xin = _x(2, 8, seed=3)
    want = Q.net_forward(model, xin, level)
    assert (want["s_1"].q < 0).mean() > 0.2  # there are negative values to lose
    got = _run(_net(model, level, graph=True), xin, names=("ra", "rb", "sum"), forwards=2)
    for k in got:
        assert np.array_equal(got[k], want[k]), (level, k)
