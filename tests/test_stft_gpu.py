"""The audio front end on the device: libfeather_stft.so through feathercnn_amd.stft against tests/stft_ref.py (float64) within TOL = 1e-4,
the project's bound on the normalised error, and tiny_audio and quartznet_5x5_wave through feather::Net against model_zoo.numpy_forward."""
import numpy as np
import pytest

import stft_cases as C

pytestmark = pytest.mark.gpu
F = np.float32
SENTINEL = F(12345.0)


def _error(got, want):
    return float(np.abs(got.astype(np.float64) - want).max() / np.abs(want).max())


def _at_offset(a, offset):
    """A device copy of `a` that starts `offset` floats past a 16-byte boundary, in a buffer full of SENTINEL -> (view, buffer)."""
    import torch
    buf = torch.full((offset + a.size + 4,), float(SENTINEL), device="cuda", dtype=torch.float32)
    view = buf[offset:offset + a.size].view(a.shape)
    view.copy_(torch.from_numpy(np.array(a)))
    return view, buf


@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_spectrogram_equals_the_float64_restatement(cuda, case):
    from feathercnn_amd import stft as M
    host, want = C.spectrogram_case(case)
    x, _ = _at_offset(host, case[-1])
    y, ybuf = _at_offset(np.full(want.shape, SENTINEL, F), case[-1])
    M.spectrogram(x, out=y, **C.case_kwargs(case))
    got, whole = y.cpu().numpy(), ybuf.cpu().numpy()
    err = _error(got, want)
    print(f"{C.case_id(case)}: error {err:.3g} (bound {C.TOL:g})")
    assert np.isfinite(got).all() and err <= C.TOL, (case, err)
    assert (whole[:case[-1]] == SENTINEL).all() and (whole[case[-1] + got.size:] == SENTINEL).all()


@pytest.mark.parametrize("offset", [0, 1, 2, 3])
@pytest.mark.parametrize("power", [0, 1, 2])
def test_every_power_at_every_offset_of_the_waveform(cuda, power, offset):
    from feathercnn_amd import stft as M
    import stft_ref as R
    host = C.spectrogram_case(C.CASES[2])[0]
    kw = dict(C.case_kwargs(C.CASES[2]), power=power)
    x, _ = _at_offset(host, offset)
    assert _error(M.spectrogram(x, **kw).cpu().numpy(), R.spectrogram(host, **kw)) <= C.TOL


@pytest.mark.parametrize("power", [1, 2])
def test_a_silent_input_gives_exactly_zero(cuda, power):
    import torch
    from feathercnn_amd import stft as M
    y = M.spectrogram(torch.zeros((2, 800), device="cuda"), 400, power, 160, 400, 1)
    assert y.shape == (2, 201, 6) and not y.cpu().numpy().any()


@pytest.mark.parametrize("count", C.UNARY_COUNTS)
@pytest.mark.parametrize("op", C.UNARY_OPS)
def test_unary_in_place_and_out_of_place(cuda, op, count):
    from feathercnn_amd import stft as M
    host, want = C.unary_case(op, count)
    assert np.isfinite(want).all()
    for offset, kernel in ((0, C.VECTOR), (1, C.SCALAR)):
        x, buf = _at_offset(host, offset)
        assert M.stft_route(1, op, offset == 0) == kernel
        out = M.unary(op, x).cpu().numpy()
        assert M.unary(op, x, out=x) is x  # in place
        whole = buf.cpu().numpy()
        assert np.array_equal(whole[offset:offset + count], out) and (whole[:offset] == SENTINEL).all() and (whole[offset + count:] == SENTINEL).all()
        assert _error(out, want) <= C.TOL, (op, count, offset)


def _net(level=2, graph=False, replicas=1, conv1d=False):
    from feathercnn_amd.net import Net
    net = Net(fusion=level, graph=graph, sub_batches=replicas)
    for switch in (net.SetAudio, net.SetTransformer) + ((net.SetConv1d,) if conv1d else ()):
        switch()
    net.SetDetection(True)
    return net


@pytest.mark.parametrize("level,graph,replicas,batch", [(0, False, 1, 3), (1, False, 1, 1), (2, False, 2, 3), (3, False, 1, 3), (0, True, 1, 1), (2, True, 1, 3), (3, True, 2, 3),
                                                        (1, False, 2, 1)])
def test_tiny_audio_every_blob(cuda, level, graph, replicas, batch):
    (p, b, i, o), _ = C.net_model()
    net = _net(level, graph, replicas)
    net.LoadParam(p)
    net.LoadWeights(b)
    x, want = C.net_input(batch)
    net.FeedInput(i, x)
    net.Forward()
    first = {name: net.Extract(name) for name in C.NET_SHAPES}
    if graph:  # replay the captured graph, twice
        for _ in range(2):
            net.Forward()
            assert all(np.array_equal(net.Extract(name), first[name]) for name in C.NET_SHAPES)
    assert [a for t, _, a in net.layers() if t in ("Spectrogram", "UnaryOp")] == ["STFT"] * 6  # nothing fuses into these layers
    for name, chw in C.NET_SHAPES.items():
        assert first[name].shape == (batch,) + chw == want[name].shape, name
        assert _error(first[name], want[name].astype(np.float64)) <= C.TOL, name


def test_quartznet_from_a_short_waveform(cuda):
    from feathercnn_amd import model_zoo
    trace = []
    p, b, i, o = model_zoo.quartznet_5x5_wave(samples=1600, trace=trace)
    net = _net(conv1d=True)
    net.LoadParam(p)
    net.LoadWeights(b)
    x = np.random.default_rng(18000).uniform(-1, 1, (1, 1, 1, 1600)).astype(F)
    want = model_zoo.numpy_forward(trace, i, x)
    net.FeedInput(i, x)
    net.Forward()
    for name, shape in (("stft", (1, 1, 257, 11)), ("log", (1, 1, 64, 11)), (o, (1, 1, 29, 6))):
        got = net.Extract(name)
        assert got.shape == shape == want[name].shape and _error(got, want[name].astype(np.float64)) <= C.TOL, name


@pytest.mark.parametrize("type_,params", [("Spectrogram", {0: 4}), ("UnaryOp", {0: 0})])
def test_a_q8_bottom_is_refused(cuda, type_, params):
    from feathercnn_amd import FeatherHipError, model_zoo
    g = model_zoo.GraphBuilder(3, quant={})
    g.layer(type_, "r", [g.conv("c1", g.input("data", 3, 8, 8), 3, 16, 3, 1, 1, requant=20.0)], ["r"], params)
    p, b = g.finish()
    net = _net()
    net.SetQuantized(True)
    net.SetRequantized(True)
    net.LoadParam(p)
    net.LoadWeights(b)
    net.FeedInput("data", np.random.default_rng(2).uniform(-1, 1, (2, 3, 8, 8)).astype(F))
    with pytest.raises(FeatherHipError) as e:
        net.Forward()
    msg = str(e.value)
    assert "code -300" in msg and "layer c1" in msg and type_ + " layer r" in msg and "blob c1" in msg, msg
