"""InverseSpectrogram on the device: libfeather_istft.so through feathercnn_amd.istft against tests/istft_ref.py (float64) within TOL = 1e-4,
the project's bound on the normalised error, and tiny_resynth through feather::Net against model_zoo.numpy_forward."""
import numpy as np
import pytest

import istft_cases as C

pytestmark = pytest.mark.gpu
SENTINEL = C.F(12345.0)


def _error(got, want):
    return float(np.abs(got.astype(np.float64) - want).max() / np.abs(want).max())


def _at_offset(a, offset):  # a device copy of `a` that starts `offset` floats past a 16-byte boundary, in a buffer full of SENTINEL -> (view, buffer)
    import torch
    buf = torch.full((offset + a.size + 4,), float(SENTINEL), device="cuda", dtype=torch.float32)
    view = buf[offset:offset + a.size].view(a.shape)
    view.copy_(torch.from_numpy(np.array(a)))
    return view, buf


@pytest.mark.parametrize("case,offset", [(c, 0) for c in C.CASES] + [(C.CASES[3], 1)], ids=lambda v: C.case_id(v) if isinstance(v, tuple) else f"off{v}")
def test_inverse_spectrogram_equals_the_float64_restatement(cuda, case, offset):  # offset 1: x and y 4-byte but not 8-byte aligned (the loader's scalar form)
    from feathercnn_amd import istft as M
    host, want = C.case_data(case)
    x = _at_offset(host, offset)[0]
    y, ybuf = _at_offset(np.full(want.shape, SENTINEL, C.F), offset)
    M.inverse_spectrogram(x, out=y, **C.case_kwargs(case))
    got, whole = y.cpu().numpy(), ybuf.cpu().numpy()
    err = _error(got, want)
    print(f"{C.case_id(case)} offset {offset}: error {err:.3g} (bound {C.TOL:g})")
    assert np.isfinite(got).all() and err <= C.TOL, (case, err)
    assert (whole[:offset] == SENTINEL).all() and (whole[offset + got.size:] == SENTINEL).all()


def test_a_silent_input_gives_exactly_zero(cuda):
    import torch
    from feathercnn_amd import istft as M
    y = M.inverse_spectrogram(torch.zeros((2, 201, 6, 2), device="cuda"), 400, 160, 400, 1)
    assert y.shape == (2, 800) and not y.cpu().numpy().any()


def _net(graph=False):
    from feathercnn_amd import model_zoo
    from feathercnn_amd.net import Net
    trace = []
    p, b, i, o = model_zoo.tiny_resynth(trace=trace)
    net = Net(fusion=2, graph=graph)
    net.SetAudio()
    net.SetDetection(True)
    net.LoadParam(p)
    net.LoadWeights(b)
    return net, trace, i


def _run(net, i, x):
    net.FeedInput(i, x)
    net.Forward()
    return {name: net.Extract(name) for name in ("stft", "wave", "neg")}


@pytest.mark.parametrize("graph", [False, True])
def test_tiny_resynth_and_re_planning(cuda, graph):
    from feathercnn_amd import model_zoo
    long, short = (np.random.default_rng(19200 + l).uniform(-1, 1, (3, 1, 1, l)).astype(C.F) for l in (70, 45))
    net, trace, i = _net(graph)
    first = _run(net, i, long)
    want = model_zoo.numpy_forward(trace, i, long)
    assert first["wave"].shape == (3, 1, 1, 68) == want["wave"].shape and [a for _, _, a in net.layers()][1:] == ["STFT", "ISTFT", "STFT"]
    for name in first:
        assert _error(first[name], want[name].astype(np.float64)) <= C.TOL, name
    assert _error(first["neg"], -long[..., :68].astype(np.float64)) <= C.TOL  # the waveform comes back
    if graph:  # replay the captured graph, twice
        for _ in range(2):
            net.Forward()
            assert np.array_equal(net.Extract("neg"), first["neg"])
    again = _run(net, i, short)  # another input length: the envelope is re-made at Init
    fresh = _run(_net(graph)[0], i, short)
    assert again["neg"].shape == (3, 1, 1, 44) and all(np.array_equal(again[name], fresh[name]) for name in again)
    assert _error(again["neg"], -short[..., :44].astype(np.float64)) <= C.TOL
