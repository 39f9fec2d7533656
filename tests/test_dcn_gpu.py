"""Deformable convolution on the device: libfeather_dcn.so through feathercnn_amd.dcn on offset buffers against tests/dcn_ref.py in float64
(within TOL = 1e-4, the project's bound for convolutions), its two degenerate forms against the plain convolution, and tiny_dcn through
feather::Net against model_zoo.numpy_forward."""
import numpy as np
import pytest

import dcn_cases as C
import dcn_ref as R

pytestmark = pytest.mark.gpu
F = np.float32
SENTINEL = F(12345.0)


def _offset(a, off):
    """A device copy of `a` that starts `off` floats past a 16-byte boundary, in a buffer full of SENTINEL -> (view, buffer)."""
    import torch
    buf = torch.full((off + a.size + 4,), float(SENTINEL), device="cuda", dtype=torch.float32)
    view = buf[off:off + a.size].view(a.shape)
    view.copy_(torch.from_numpy(np.array(a)))
    return view, buf


def _error(got, want):
    return float(np.abs(got.astype(np.float64) - want).max() / np.abs(want).max())


@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_forward_equals_the_float64_restatement(cuda, case):
    from feathercnn_amd import dcn as M
    n, c, h, w, k, (kh, kw), stride, dilation, pads, g, _, act, (a0, a1), _, off, _, kernel = case
    t = C.case(case)
    assert M.dcn_route(c, k, kh, kw, g) == kernel == M.route_rule(c, k, kh, kw, g)
    dev = {name: None if a is None else _offset(a, off)[0] for name, a in t.items() if name != "y"}
    y, ybuf = _offset(np.full(t["y"].shape, SENTINEL, F), off)
    M.deform_conv2d(dev["x"], dev["offset"], dev["mask"], dev["w"].contiguous(), dev["bias"], stride, dilation, pads, g, act, a0, a1, out=y)
    got, host = y.cpu().numpy(), ybuf.cpu().numpy()
    err = _error(got, t["y"])
    print(f"{C.case_id(case)}: error {err:.3g} (bound {C.TOL:g})")
    assert np.isfinite(got).all() and err <= C.TOL, (case, err)
    assert (host[:off] == SENTINEL).all() and (host[off + got.size:] == SENTINEL).all()


@pytest.mark.parametrize("shift", [(0, 0), (1, -2), (-3, 2)], ids=str)
def test_whole_offsets_are_the_plain_convolution_of_a_shifted_input(cuda, shift):
    """Zero offsets and no mask: the plain convolution.  The same whole offset on every tap: the plain convolution, without pads, of the
    zero-padded input shifted by it."""
    import torch
    from feathercnn_amd import dcn as M
    n, c, h, w, k, kernel, stride, dilation, pads = 2, 5, 9, 11, 7, (3, 3), (2, 1), (1, 2), (1, 2, 2, 1)
    rng = np.random.default_rng(16500)
    x, wt = rng.uniform(-1, 1, (n, c, h, w)).astype(F), rng.uniform(-0.3, 0.3, (k, c) + kernel).astype(F)
    ho, wo = R.output_dim(h, w, kernel, dilation, stride, pads)
    offset = np.tile(np.array(shift, F)[None, :, None, None], (n, 9, ho, wo))
    padded = np.zeros((n, c, h + pads[0] + pads[1], w + pads[2] + pads[3]))
    for yy in range(padded.shape[2]):  # padded[yy][xx] = x[yy - top + dy][xx - left + dx], 0 outside the plane
        for xx in range(padded.shape[3]):
            sy, sx = yy - pads[0] + shift[0], xx - pads[2] + shift[1]
            if 0 <= sy < h and 0 <= sx < w:
                padded[:, :, yy, xx] = x[:, :, sy, sx]
    want = R.conv2d(padded, wt, None, stride, dilation)
    if shift == (0, 0):
        assert np.array_equal(want, R.conv2d(x, wt, None, stride, dilation, pads))
    got = M.deform_conv2d(*(torch.from_numpy(a).cuda() for a in (x, offset)), None, torch.from_numpy(wt).cuda(), None, stride, dilation, pads).cpu().numpy()
    assert got.shape == want.shape and _error(got, want) <= C.TOL


def _switched(param, weights=None, level=1, deformable=True):
    from feathercnn_amd.net import Net
    net = Net(fusion=level)
    if deformable:
        net.SetDeformable()
    net.LoadParam(param)
    if weights is not None:
        net.LoadWeights(weights)
    return net


@pytest.mark.parametrize("level", [0, 2])
def test_tiny_dcn_every_blob_and_a_second_size(cuda, level):
    from feathercnn_amd import FeatherHipError
    p, b, i, o = C.net_model()[0]
    net = _switched(p, b, level)
    assert ("DeformableConv2D", "dcn", "DCN") in net.layers()
    for size in ((10, 12), (8, 14), (10, 12)):  # re-planned at a second size and back
        x, want = C.net_input(3, size)
        net.FeedInput(i, x)
        net.Forward()
        seen = set()
        for name, ref in want.items():
            try:
                got = net.Extract(name)
            except FeatherHipError:  # a blob a fusion of level 2 absorbed into its consumer
                assert level == 2, name
                continue
            seen.add(name)
            assert got.shape == ref.shape and _error(got, ref.astype(np.float64)) <= C.TOL, (name, size, level)
        assert {"om_slice_0", "mask", "dcn", "fc"} <= seen and (level or seen == set(want)), seen


@pytest.mark.parametrize("shapes,word", [
    ({"off": 16}, "an offset blob of (18, 8, 8), blob off"),  # the wrong channel count
    ({"msk_h": 7}, "a mask blob of (9, 8, 8), blob msk"),  # a mask of another plane
    ({"in0": 6}, "5 input channels, blob in0 has 6"),  # weights for 5 channels
], ids=["offset", "mask", "channels"])
def test_what_only_reshape_can_refuse(cuda, shapes, word):
    from feathercnn_amd import FeatherHipError
    cin, coff, mh = shapes.get("in0", 5), shapes.get("off", 18), shapes.get("msk_h", 8)
    param = (f"7767517\n4 4\nInput in0 0 1 in0 0=8 1=8 2={cin}\nInput off 0 1 off 0=8 1=8 2={coff}\nInput msk 0 1 msk 0=8 1={mh} 2=9\n"
             "DeformableConv2D l 3 1 in0 off msk top 0=4 1=3 4=1 5=1 6=180\n").encode()
    weights = b"\0" * (4 + 4 * 180 + 4 * 4)
    with pytest.raises(FeatherHipError, match="code -200"):
        _switched(param, deformable=False)
    net = _switched(param, weights)
    with pytest.raises(FeatherHipError, match="code -100") as e:
        for name, shape in (("in0", (1, cin, 8, 8)), ("off", (1, coff, 8, 8)), ("msk", (1, 9, mh, 8))):
            net.FeedInput(name, np.zeros(shape, F))
        net.Forward()
    assert "layer l" in str(e.value) and word in str(e.value), str(e.value)
