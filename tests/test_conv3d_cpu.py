"""The 3-D layers without a device: tests/conv3d_ref.py against torch's conv3d, max_pool3d and avg_pool3d in float64 on explicitly padded
volumes (SAME pads, pad_value and ncnn's divisors have no torch counterpart), the switch and the refusals of the Net runtime, and the
route rule with its Python mirror over the case table."""
import numpy as np
import pytest

import conv3d_cases as C
import conv3d_ref as R

CONV = "0=4 1=3 5=1 6=324"  # 3 input channels, 4 outputs, 3 x 3 x 3 taps
TYPES = {"Convolution3D": CONV, "ConvolutionDepthWise3D": "0=3 1=3 5=1 6=81 7=3", "Pooling3D": "0=0 1=2 2=2"}
BOUND = 1e-12  # float64 against float64: the two sum in different orders


@pytest.mark.parametrize("case", C.CONV_CASES, ids=C.case_id)
def test_the_convolution_restatement_is_torchs_on_the_padded_volume(case):
    import torch
    import torch.nn.functional as tf
    _, _, dhw, _, kernel, stride, dilation, pads, pad_value, group, act, (a0, a1) = case[:12]
    t = C.conv_case(case)
    axes = [R.conv_axis(e, k, d, s, lo, hi) for e, k, d, s, lo, hi in zip(dhw, R.three(kernel), R.three(dilation), R.three(stride), *R.six(pads))]
    x = tf.pad(torch.from_numpy(np.array(t["x"])).double(), [p for a in reversed(axes) for p in a[:2]], value=float(pad_value))
    bias = None if t["bias"] is None else torch.from_numpy(np.array(t["bias"])).double()
    y = tf.conv3d(x, torch.from_numpy(np.array(t["w"])).double(), bias, R.three(stride), 0, R.three(dilation), group).numpy()
    y = R.activate(y, act, np.float64(C.F(a0)), np.float64(C.F(a1)))
    assert y.shape == t["y"].shape and np.abs(y - t["y"]).max() / np.abs(y).max() <= BOUND


@pytest.mark.parametrize("case", C.POOL_CASES, ids=C.case_id)
def test_the_pooling_restatement_is_torchs_on_the_padded_volume(case):
    import torch
    import torch.nn.functional as tf
    _, _, dhw, kernel, stride, pads, mode, avg, include, global_, out_dhw, _ = case
    host, want = C.pool_case(case)
    x = torch.from_numpy(np.array(host)).double()
    if global_ or out_dhw is not None:
        y = (tf.adaptive_avg_pool3d if avg else tf.adaptive_max_pool3d)(x, (1, 1, 1) if global_ else out_dhw).numpy()
    else:
        kern, st = R.three(kernel), R.three(stride)
        axes = [R.pool_axis(e, k, s, lo, hi, mode) for e, k, s, lo, hi in zip(dhw, kern, st, *R.six(pads))]
        # the pads, and behind them the tail a window of full mode hangs over: cells that hold nothing and never count
        widths = [(lo, max(hi, (out - 1) * s + k - e - lo)) for (lo, hi, out), e, k, s in zip(axes, dhw, kern, st)]
        flat = [p for w in reversed(widths) for p in w]
        if not avg:
            y = tf.max_pool3d(tf.pad(x, flat, value=float("-inf")), kern, st).numpy()
        else:
            counted = torch.ones_like(x)
            if include:  # the cells of the padded volume count, the tail does not
                counted = tf.pad(counted, [p for a in reversed(axes) for p in a[:2]], value=1.0)
                flat = [p - q for p, q in zip(flat, [p for a in reversed(axes) for p in a[:2]])]
                x = tf.pad(x, [p for a in reversed(axes) for p in a[:2]])
            total, cells = tf.avg_pool3d(tf.pad(x, flat), kern, st), tf.avg_pool3d(tf.pad(counted, flat), kern, st)
            y = torch.where(cells > 0, total / cells.clamp(min=1e-300), torch.zeros_like(total)).numpy()
    assert y.shape == want.shape and (np.abs(y - want).max() / np.abs(y).max() <= BOUND if avg else np.array_equal(y.astype(np.float32), want))


def _one(type_, params):
    return ("7767517\n2 2\nInput in0 0 1 in0 0=8 1=8 11=4 2=3\n%s l 1 1 in0 top %s\n" % (type_, params)).encode()


def _net(param, conv3d=True, detection=True):
    from feathercnn_amd.net import Net
    net = Net()
    if conv3d:
        net.SetConv3d()
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
    assert "(fhip_net_set_conv3d lifts this)" in _refused(p, -200, type_, conv3d=False)  # a default net: what the parent commit answers too
    msg = _refused(p, -200, "fhip_net_set_detection", detection=False)
    assert type_ in msg and "set both" in msg
    net = _net(p)
    assert (type_, "l", "CONV3D") in net.layers()
    with pytest.raises(FeatherHipError, match="before LoadParam"):
        net.SetConv3d(False)
    net = Net()
    net.SetConv3d()
    net.SetConv3d(False)  # on-then-off equals the default
    net.SetDetection(True)
    with pytest.raises(FeatherHipError, match="code -200"):
        net.LoadParam(p)


@pytest.mark.parametrize("type_,params,word", [
    ("Convolution3D", CONV + " 19=1", "19=1"), ("Convolution3D", CONV + " 8=1", "8=1"), ("Convolution3D", "0=0 1=3 6=324", "0=0"), ("Convolution3D", "0=4 1=3 21=0 6=324", "21=0"),
    ("Convolution3D", CONV + " 13=0", "13=0"), ("Convolution3D", CONV + " 22=0", "22=0"), ("Convolution3D", "0=4 1=3 6=325", "6=325"), ("Convolution3D", CONV + " 9=7", "9=7"),
    ("Convolution3D", CONV + " 24=-1", "24=-1"), ("Convolution3D", CONV + " 16=-2", "16=-2"), ("Convolution3D", "0=65536 1=1024 11=1024 21=64 6=324", "2^31"),
    ("ConvolutionDepthWise3D", "0=4 1=3 6=324 7=3", "7=3"), ("ConvolutionDepthWise3D", "0=4 1=3 6=162 7=2", "6=162"),  # three input channels, which 2 does not divide
    ("Pooling3D", "0=2 1=2", "0=2"), ("Pooling3D", "0=0 1=2 21=0", "21=0"), ("Pooling3D", "0=0 1=2 12=0", "12=0"), ("Pooling3D", "0=0 1=2 5=4", "5=4"),
    ("Pooling3D", "0=0 1=2 23=-1", "23=-1"), ("Pooling3D", "0=0 7=1 8=2 28=0", "28=0"),
], ids=lambda v: str(v).replace(" ", "_"))
def test_loadparam_refusals_name_the_layer_and_the_param(type_, params, word):
    msg = _refused(_one(type_, params), -100, word)
    assert "layer l" in msg and type_ in msg


def test_the_zoo_nets_load_and_the_route_rule_is_the_tables():
    from feathercnn_amd import conv3d as M, model_zoo
    for name, count in (("tiny_c3d", 14), ("c3d", 13), ("r3d_18", 21)):
        layers = _net(getattr(model_zoo, name)(dry=True)[0]).layers()
        assert sum(a == "CONV3D" for _, _, a in layers) == count, (name, layers)
    seen = {C.POOL, C.PACK}
    for case in C.CONV_CASES:
        _, c, _, k, kernel, stride, dilation, _, _, group, _, _, _, _, direct, name = case
        assert M.conv3d_route(c, k, kernel, dilation, stride, group, direct) == M.route_rule(c, k, kernel, dilation, stride, group, direct) == name, case
        seen.add(name)
    assert seen == C.targets()
    assert M.route_rule(64, 128, 3) == C.M128 and M.route_rule(3, 64, (3, 7, 7), 1, (1, 2, 2)) == C.DIRECT and M.route_rule(128, 256, 3, 1, 2) == C.M128
