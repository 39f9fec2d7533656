"""The 1-D layers without a device: the switch and the refusals of the Net runtime, the route rule and its Python mirror over the case
table, and the room float32 leaves every case of tests/conv1d_cases.py."""
import numpy as np
import pytest

import conv1d_cases as C

CONV = "0=4 1=3 5=1 6=60"  # 5 input channels, 4 outputs, 3 taps
TYPES = {"Convolution1D": CONV, "ConvolutionDepthWise1D": "0=5 1=3 5=1 6=15 7=5", "Pooling1D": "0=0 1=2 2=2"}


def _one(type_, params, c=1, h=5, w=20):
    lines = [f"Input in0 0 1 in0 0={w} 1={h} 2={c}", f"{type_} l 1 1 in0 top {params}"]
    return ("7767517\n2 2\n" + "\n".join(lines) + "\n").encode()


def _net(param, conv1d=True, detection=True):
    from feathercnn_amd.net import Net
    net = Net()
    if conv1d:
        net.SetConv1d()
    if detection:
        net.SetDetection(True)
    net.LoadParam(param)
    return net


def _refused(param, code, word, **kw):
    from feathercnn_amd import FeatherHipError
    with pytest.raises(FeatherHipError, match=f"code {code}") as e:
        _net(param, **kw)
    assert word in str(e.value), str(e.value)
    return str(e.value)


@pytest.mark.parametrize("type_", sorted(TYPES))
def test_the_switch(type_):
    from feathercnn_amd import FeatherHipError
    from feathercnn_amd.net import Net
    p = _one(type_, TYPES[type_])
    assert "(fhip_net_set_conv1d lifts this)" in _refused(p, -200, type_, conv1d=False)
    msg = _refused(p, -200, "fhip_net_set_detection", detection=False)
    assert type_ in msg and "set both" in msg
    net = _net(p)
    assert (type_, "l", "CONV1D") in net.layers()
    with pytest.raises(FeatherHipError, match="before LoadParam"):
        net.SetConv1d(False)
    net = Net()
    net.SetConv1d()
    net.SetConv1d(False)  # on-then-off equals the default
    net.SetDetection(True)
    with pytest.raises(FeatherHipError, match="code -200"):
        net.LoadParam(p)


@pytest.mark.parametrize("type_,params,word", [
    ("Convolution1D", CONV + " 19=1", "19=1"), ("Convolution1D", CONV + " 8=1", "8=1"), ("Convolution1D", "0=0 1=3 6=60", "0=0"), ("Convolution1D", "0=4 1=0 6=60", "1=0"),
    ("Convolution1D", CONV + " 3=0", "3=0"), ("Convolution1D", CONV + " 2=0", "2=0"), ("Convolution1D", "0=4 1=3 6=61", "6=61"), ("Convolution1D", CONV + " 9=7", "9=7"),
    ("Convolution1D", CONV + " 4=-2", "4=-2"), ("Convolution1D", "0=65536 1=32768 6=60", "2^31"),
    ("ConvolutionDepthWise1D", "0=4 1=3 6=60 7=3", "7=3"), ("ConvolutionDepthWise1D", "0=4 1=3 6=18 7=2", "6=18"),  # three input channels, which 2 does not divide
    ("Pooling1D", "0=2 1=2", "0=2"), ("Pooling1D", "0=0 1=0", "1=0"), ("Pooling1D", "0=0 1=2 2=0", "2=0"), ("Pooling1D", "0=0 1=2 5=4", "5=4"), ("Pooling1D", "0=0 7=1 8=0", "8=0"),
], ids=lambda v: str(v).replace(" ", "_"))
def test_loadparam_refusals_name_the_layer_and_the_param(type_, params, word):
    msg = _refused(_one(type_, params), -100, word)
    assert "layer l" in msg and type_ in msg


def test_the_zoo_nets_load_and_the_route_rule_is_the_tables():
    from feathercnn_amd import conv1d as M, model_zoo
    p = model_zoo.quartznet_5x5(dry=True)[0]
    layers = _net(p).layers()
    assert len(layers) == 57 and {a for t, _, a in layers[1:]} == {"CONV1D"}
    seen = {C.POOL}
    for case in C.CONV_CASES:
        _, c, _, k, kw, s, d, _, _, _, group = case[:11]
        assert M.conv1d_route(c, k, kw, d, s, group) == M.route_rule(c, k, kw, d, s, group) == case[-1], case
        seen.add(case[-1])
    assert seen == C.targets()
    assert M.route_rule(512, 512, 87, 2, 1, 512) == C.DW and M.route_rule(64, 256, 33, 1, 2) == C.LARGE and M.route_rule(512, 1024, 1) == C.SMALL


@pytest.mark.parametrize("case", C.CONV_CASES, ids=C.case_id)
def test_every_case_leaves_float32_room(case):
    t = C.conv_case(case)
    y32 = C.conv_float(case, t["x"], t["w"], t["bias"], np.float32)
    assert y32.shape == t["y"].shape and np.abs(y32 - t["y"]).max() / np.abs(t["y"]).max() <= C.TOL / 10
