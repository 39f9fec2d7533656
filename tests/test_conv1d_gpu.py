"""The 1-D layers on the device: libfeather_conv1d.so through feathercnn_amd.conv1d on strided, offset buffers against tests/conv1d_ref.py
(convolutions within TOL = 1e-4 of float64, the project's bound for convolutions; pooling bit for bit), and tiny_tcn through feather::Net
against model_zoo.numpy_forward."""
import numpy as np
import pytest

import conv1d_cases as C

pytestmark = pytest.mark.gpu
F = np.float32
SENTINEL = F(12345.0)


def _strided(a, slack, offset):
    """A device copy of a [n][C][L] whose rows are `slack` floats apart and which starts `offset` floats past a 16-byte boundary, in a buffer
    full of SENTINEL -> (view, buffer)."""
    import torch
    n, c, l = a.shape
    buf = torch.full((offset + n * c * (l + slack) + 4,), float(SENTINEL), device="cuda", dtype=torch.float32)
    view = buf.as_strided((n, c, l), (c * (l + slack), l + slack, 1), offset)
    view.copy_(torch.from_numpy(np.array(a)))
    return view, buf


def _untouched(buf, view_shape, slack, offset):
    """Every float of the buffer outside the rows still holds SENTINEL."""
    n, c, l = view_shape
    host = buf.cpu().numpy()
    rows = host[offset:offset + n * c * (l + slack)].reshape(n * c, l + slack)
    return (host[:offset] == SENTINEL).all() and (rows[:, l:] == SENTINEL).all() and (host[offset + n * c * (l + slack):] == SENTINEL).all()


def _error(got, want):
    return float(np.abs(got.astype(np.float64) - want).max() / np.abs(want).max())


@pytest.mark.parametrize("case", C.CONV_CASES, ids=C.case_id)
def test_convolution_equals_the_float64_restatement(cuda, case):
    import torch
    from feathercnn_amd import conv1d as M
    n, c, l, k, kw, s, d, pl, pr, pad_value, group, act, (a0, a1), bias, slack, offset, kernel = case
    t = C.conv_case(case)
    assert M.conv1d_route(c, k, kw, d, s, group) == kernel == M.route_rule(c, k, kw, d, s, group)
    x, _ = _strided(t["x"], slack, offset)
    y, ybuf = _strided(np.full(t["y"].shape, SENTINEL, F), slack, offset)
    dev = lambda a: None if a is None else torch.from_numpy(np.array(a)).cuda()
    M.conv1d(x, dev(t["w"]), dev(t["bias"]), s, d, pl, pr, pad_value, group, act, a0, a1, out=y)
    got = y.cpu().numpy()
    err = _error(got, t["y"])
    print(f"{C.case_id(case)}: error {err:.3g} (bound {C.TOL:g})")
    assert np.isfinite(got).all() and err <= C.TOL, (case, err)
    assert _untouched(ybuf, got.shape, slack, offset)


@pytest.mark.parametrize("case", C.POOL_CASES, ids=C.case_id)
def test_pooling_is_the_restatement_bit_for_bit(cuda, case):
    from feathercnn_amd import conv1d as M
    n, c, l, kw, s, pl, pr, mode, avg, include, global_, out_w, slack, offset = case
    host, want = C.pool_case(case)
    x, _ = _strided(host, slack, offset)
    y, ybuf = _strided(np.full(want.shape, SENTINEL, F), slack, offset)
    M.pool1d(x, kw, s, pl, pr, mode, bool(avg), bool(include), bool(global_), out_w, out=y)
    assert np.array_equal(y.cpu().numpy(), want), case
    assert _untouched(ybuf, want.shape, slack, offset) and M.conv1d_route(c, c, 0) == C.POOL


@pytest.mark.parametrize("level", [0, 2])
def test_tiny_tcn_every_blob_and_a_second_length(cuda, level):
    from feathercnn_amd.net import Net
    p, b, i, o = C.net_model()[0]
    net = Net(fusion=level)
    for switch in (net.SetConv1d, net.SetRecurrent, net.SetTransformer):
        switch()
    net.SetDetection(True)
    net.LoadParam(p)
    net.LoadWeights(b)
    assert [a for t, _, a in net.layers() if t.endswith("1D")] == ["CONV1D"] * 5
    for length in (40, 52, 40):  # re-planned at a second length and back
        x, want = C.net_input(3, length)
        net.FeedInput(i, x)
        net.Forward()
        for name, chw in C.net_shapes(length).items():
            got = net.Extract(name)
            assert got.shape == (3,) + chw == want[name].shape, (name, length)
            assert _error(got, want[name].astype(np.float64)) <= C.TOL, (name, length)


def _switched(param, weights=None):
    from feathercnn_amd.net import Net
    net = Net()
    net.SetConv1d()
    net.SetDetection(True)
    net.LoadParam(param)
    if weights is not None:
        net.LoadWeights(weights)
    return net


@pytest.mark.parametrize("c,h,w,layer,word", [
    (2, 5, 20, "Convolution1D l 1 1 in0 top 0=4 1=3 5=1 6=60", "rank 3"),  # a blob with channels is no 1-D blob
    (1, 6, 20, "Convolution1D l 1 1 in0 top 0=4 1=3 5=1 6=60", "5 input channels"),  # weights for 5 channels, a blob of 6
    (1, 5, 20, "Convolution1D l 1 1 in0 top 0=4 1=25 4=2 5=1 6=500", "shorter than the dilated kernel"),  # Lo < 1
    (1, 5, 3, "Pooling1D l 1 1 in0 top 0=0 1=4 5=1", "shorter than the window"),
], ids=["rank3", "channels", "lo", "pool_lo"])
def test_what_only_reshape_can_refuse(cuda, c, h, w, layer, word):
    from feathercnn_amd import FeatherHipError
    net = _switched(f"7767517\n2 2\nInput in0 0 1 in0 0={w} 1={h} 2={c}\n{layer}\n".encode(), _zero_weights(layer))
    with pytest.raises(FeatherHipError, match="code -100") as e:
        net.FeedInput("in0", np.zeros((1, c, h, w), F))
        net.Forward()
    assert "layer l" in str(e.value) and "in0" in str(e.value) and word in str(e.value), str(e.value)


def _zero_weights(layer):
    """The .bin of the one layer: a zero tag, zero weights and a zero bias (6= and 0= of its line); nothing for a pooling."""
    p = dict(kv.split("=") for kv in layer.split()[6:])
    return (b"\0" * (4 + 4 * int(p["6"]) + 4 * int(p["0"]))) if "6" in p else b""


def test_global_pooling_gives_a_blob_of_rank_1_that_innerproduct_takes(cuda):
    from feathercnn_amd import model_zoo
    g, trace = model_zoo.GraphBuilder(89), []
    g.trace = trace
    g.fc("fc", g.pool1d("gap", g.input("data", 1, 4, 20), avg=True, global_=True), 4, 3)
    p, b = g.finish()
    net = _switched(p, b)
    x = np.random.default_rng(15000).uniform(-1, 1, (3, 1, 4, 20)).astype(F)
    want = model_zoo.numpy_forward(trace, "data", x)
    net.FeedInput("data", x)
    net.Forward()
    assert net.Extract("gap").shape == (3, 1, 1, 4) == want["gap"].shape and net.Extract("fc").shape == (3, 3, 1, 1)
    assert _error(net.Extract("gap"), want["gap"].astype(np.float64)) <= C.TOL and _error(net.Extract("fc"), want["fc"].astype(np.float64)) <= C.TOL
