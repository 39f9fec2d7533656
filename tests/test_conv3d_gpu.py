"""The 3-D layers on the device: libfeather_conv3d.so through feathercnn_amd.conv3d on offset buffers against tests/conv3d_ref.py
(convolutions and average pooling within TOL = 1e-4 of float64, the project's bound; max pooling bit for bit), and tiny_c3d, r3d_18 and c3d
through feather::Net against model_zoo.numpy_forward."""
import numpy as np
import pytest

import conv3d_cases as C

pytestmark = pytest.mark.gpu
F = np.float32
SENTINEL = F(12345.0)


def _offset(a, offset):
    """A dense device copy of `a` that starts `offset` floats past a 16-byte boundary, in a buffer full of SENTINEL -> (view, buffer)."""
    import torch
    buf = torch.full((offset + a.size + 4,), float(SENTINEL), device="cuda", dtype=torch.float32)
    view = buf[offset:offset + a.size].view(a.shape)
    view.copy_(torch.from_numpy(np.array(a)))
    return view, buf


def _untouched(buf, size, offset):
    host = buf.cpu().numpy()
    return (host[:offset] == SENTINEL).all() and (host[offset + size:] == SENTINEL).all()


def _error(got, want):
    return float(np.abs(got.astype(np.float64) - want).max() / np.abs(want).max())


def _conv(case):
    import torch
    from feathercnn_amd import conv3d as M
    n, c, dhw, k, kernel, stride, dilation, pads, pad_value, group, act, (a0, a1), bias, offset, direct, kernel_name = case
    t = C.conv_case(case)
    assert M.conv3d_route(c, k, kernel, dilation, stride, group, direct) == kernel_name
    x, _ = _offset(t["x"], offset)
    y, ybuf = _offset(np.full(t["y"].shape, SENTINEL, F), offset)
    dev = lambda a: None if a is None else torch.from_numpy(np.array(a)).cuda()
    M.conv3d(x, dev(t["w"]), dev(t["bias"]), stride, dilation, pads, pad_value, group, act, a0, a1, direct=bool(direct), out=y)
    got = y.cpu().numpy()
    assert _untouched(ybuf, got.size, offset)
    return got, t["y"]


@pytest.mark.parametrize("case", C.CONV_CASES, ids=C.case_id)
def test_convolution_equals_the_float64_restatement(cuda, case):
    got, want = _conv(case)
    err = _error(got, want)
    print(f"{C.case_id(case)}: error {err:.3g} (bound {C.TOL:g})")
    assert np.isfinite(got).all() and err <= C.TOL, (case, err)


def test_the_matrix_and_the_direct_kernel_agree(cuda):
    (mfma, want), (direct, _) = _conv(C.CONV_CASES[0]), _conv(C.CONV_CASES[1])
    assert C.CONV_CASES[0][:14] == C.CONV_CASES[1][:14] and _error(mfma, direct.astype(np.float64)) <= C.TOL


@pytest.mark.parametrize("case", C.POOL_CASES, ids=C.case_id)
def test_pooling_equals_the_restatement_and_max_bit_for_bit(cuda, case):
    from feathercnn_amd import conv3d as M
    n, c, dhw, kernel, stride, pads, mode, avg, include, global_, out_dhw, offset = case
    host, want = C.pool_case(case)
    x, _ = _offset(host, offset)
    y, ybuf = _offset(np.full(want.shape, SENTINEL, F), offset)
    M.pool3d(x, kernel, stride, pads, mode, bool(avg), bool(include), bool(global_), out_dhw, out=y)
    got = y.cpu().numpy()
    assert (_error(got, want) <= C.TOL) if avg else np.array_equal(got, want), case
    assert _untouched(ybuf, want.size, offset) and M.conv3d_route(c, 0) == C.POOL


def _net(name, level=2, graph=False, **kw):
    from feathercnn_amd.net import Net
    p, b, i, o = C.net_model(name)[0]
    net = Net(fusion=level, graph=graph, **kw)
    net.SetConv3d()
    net.SetDetection(True)
    net.LoadParam(p)
    net.LoadWeights(b)
    return net, i, o


@pytest.mark.parametrize("level,graph", [(0, False), (1, False), (2, True), (3, False), (3, True)])
def test_tiny_c3d_every_blob(cuda, level, graph):
    net, i, _ = _net("tiny_c3d", level, graph)
    assert [a for t, _, a in net.layers() if t.endswith("3D")] == ["CONV3D"] * 14
    for batch in (1, 2, 2):  # re-planned at a second batch; the last forward replays the graph
        x, want = C.net_input("tiny_c3d", batch)
        net.FeedInput(i, x)
        net.Forward()
        for name, ref in want.items():
            got = net.Extract(name)
            assert got.shape == ref.shape, (name, got.shape, ref.shape)
            assert _error(got, ref.astype(np.float64)) <= C.TOL, (name, batch)


@pytest.mark.parametrize("name,batch", [("r3d_18", 2), ("c3d", 1)])
def test_the_video_nets_equal_the_numpy_forward(cuda, name, batch):
    net, i, o = _net(name)
    x, want = C.net_input(name, batch)
    net.FeedInput(i, x)
    net.Forward()
    got = net.Extract(o)
    assert got.shape == want[o].shape and _error(got, want[o].astype(np.float64)) <= C.TOL


def test_a_volume_is_refused_where_it_cannot_be_read(cuda):
    from feathercnn_amd import FeatherHipError
    from feathercnn_amd.net import Net
    conv = "Convolution3D conv 1 1 data conv 0=4 1=3 5=1 6=324"
    param = ("7767517\n3 3\nInput data 0 1 data\n%s\nBatchNorm bn 1 1 conv bn 0=4\n" % conv).encode()
    weights = b"\0" * (4 + 4 * 324 + 4 * 4 + 4 * 16)
    x = np.zeros((1, 3, 4, 6, 6), F)

    def net(sub_batches=1):
        n = Net(sub_batches=sub_batches)
        n.SetConv3d()
        n.SetDetection(True)
        n.LoadParam(param)
        n.LoadWeights(weights)
        return n

    n = net()
    n.FeedInput("data", x)
    with pytest.raises(FeatherHipError, match="code -300") as e:  # a BatchNorm behind a volume
        n.Forward()
    assert "layer conv" in str(e.value) and "BatchNorm layer bn" in str(e.value)
    with pytest.raises(FeatherHipError, match="fhip_net_extract_volume"):  # the image entry never returns four extents of five
        n.ExtractDevice("data")
    assert n.Extract("data").shape == x.shape
    with pytest.raises(FeatherHipError, match="sub-batch"):
        net(2).FeedInput("data", x)
