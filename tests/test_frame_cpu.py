"""libfeather_frame.so and the framing layers of the Net runtime (Padding, Crop, PixelShuffle) without a device.

* tests/frame_ref.py, the restatement of feather_frame.h the GPU tests compare with, against oracles that are independent of it -- np.pad,
  torch.nn.functional.pad, torch.nn.functional.pixel_shuffle, plain slicing and tests/yolo_ref.reorg -- exactly (int32 views), on the very
  inputs of the GPU cases (tests/frame_cases.py).
* The Net switch (fhip_net_set_frame), what LoadParam and LoadWeights answer to every refusal of the issue, hostile values included.
* The fusion plans: which Paddings fusion level 2 folds into the convolution behind them, and the pads those convolutions then carry.
* The host refusals of the C-ABI: nothing reaches a device."""
import ctypes
import re
import struct

import numpy as np
import pytest

import frame_cases as C
import frame_ref as R
import side_contract as SC
import yolo_ref

F = np.float32
INT_MAX = 2 ** 31 - 1


def bits(a):
    return np.ascontiguousarray(a, F).view(np.int32)


# ---- the restatement against independent oracles -----------------------------------------------------------------------------------------
NP_MODE = {0: "constant", 1: "edge", 2: "reflect"}
TORCH_MODE = {0: "constant", 1: "replicate", 2: "reflect"}


def _independent_window(x, type_, value, per_channel, front, behind, top, bottom, left, right):
    """Slicing for the negative margins, then np.pad for the positive ones -- per channel where the constant differs by channel."""
    n, c, h, w = x.shape
    lo = [max(-m, 0) for m in (front, top, left)]
    hi = [dim - max(-m, 0) for dim, m in zip((c, h, w), (behind, bottom, right))]
    pads = [(max(a, 0), max(b, 0)) for a, b in ((front, behind), (top, bottom), (left, right))]
    u = x.view(np.uint32)
    fill = int(np.asarray(value, F).view(np.uint32))
    if type_ != 0:
        # a crop on one side and a border on the other: the border reads the UNcropped plane, so pad first (by the positive margins), slice after
        full = np.pad(u, [(0, 0), (0, 0), pads[1], pads[2]], mode=NP_MODE[type_])
        return full[:, lo[0]:hi[0], lo[1]:full.shape[2] - max(-bottom, 0), lo[2]:full.shape[3] - max(-right, 0)].view(F)
    planes = []
    for q in range(lo[0], hi[0]):
        k = fill if per_channel is None else int(np.asarray(per_channel, F).view(np.uint32)[q])
        planes.append(np.pad(u[:, q, lo[1]:hi[1], lo[2]:hi[2]], [(0, 0), pads[1], pads[2]], mode="constant", constant_values=k))
    body = np.stack(planes, axis=1)
    return np.pad(body, [(0, 0), pads[0], (0, 0), (0, 0)], mode="constant", constant_values=fill).view(F)


@pytest.mark.parametrize("name", sorted(C.WINDOWS))
def test_the_window_restatement_equals_numpy_pad_and_slicing(name):
    x, kw, want = C.window_case(name)
    other = _independent_window(x, kw["type_"], kw["value"], kw.get("per_channel"), kw["front"], kw["behind"], kw["top"], kw["bottom"], kw["left"], kw["right"])
    assert other.shape == want.shape and np.array_equal(bits(other), bits(want)), name
    (h, w), _, (f, b, t, bo, l, r), _, _ = C.WINDOWS[name]
    assert want.shape == (2, 3 + f + b, h + t + bo, w + l + r)


def test_every_window_target_has_a_case_and_the_planted_values_are_there():
    seen = set()
    for name in C.WINDOWS:
        x, kw, want = C.window_case(name)
        seen.add(C.window_target(kw["type_"], C.window_pads(name), want.shape[3]))
        u = x.view(np.uint32)
        assert (u == C.NAN_PAYLOAD).any() and (u == 0x80000000).any() and np.isinf(x).any()
    assert seen == {t for t in C.targets() if "window" in t}
    lefts = {C.WINDOWS[n][2][4] for n in C.WINDOWS}
    assert {0, 1, 4} <= lefts
    assert any(C.WINDOWS[n][3] == C.NAN_PAYLOAD for n in C.WINDOWS) and any(C.WINDOWS[n][3] == C.MINUS_ZERO for n in C.WINDOWS)


@pytest.mark.parametrize("type_", [0, 1, 2])
def test_padding_equals_torch_pad(type_):
    import torch
    x = np.random.default_rng(type_).uniform(-1, 1, (2, 3, 7, 9)).astype(F)
    for t, bo, l, r in ((1, 2, 3, 0), (0, 0, 4, 1), (6, 6, 8, 8) if type_ != 0 else (9, 9, 11, 11), (0, 1, 0, 1)):
        kw = dict(mode=TORCH_MODE[type_]) if type_ else dict(mode="constant", value=0.25)
        want = torch.nn.functional.pad(torch.from_numpy(x), (l, r, t, bo), **kw).numpy()
        got = R.pad(x, t, bo, l, r, type_, 0.25)
        assert np.array_equal(bits(got), bits(want)), (type_, t, bo, l, r)
    want = np.pad(x, [(0, 0), (1, 2), (0, 0), (0, 0)], constant_values=0.5)
    assert np.array_equal(bits(R.pad(x, value=0.5, front=1, behind=2)), bits(want))


def test_crop_equals_slicing():
    x = C.planted((2, 5, 7, 9), 7)
    assert np.array_equal(bits(R.crop(x, 2, 1, 1, 4, 3, 2)), bits(x[:, 1:3, 1:4, 2:6]))
    assert np.array_equal(bits(R.crop(x, 2, 1, woffset2=3, hoffset2=2, coffset2=4)), bits(x[:, :1, 1:5, 2:6]))
    like = np.zeros((2, 3, 4, 5), F)
    assert np.array_equal(bits(R.crop(x, 1, 2, 1, like=like)), bits(x[:, 1:4, 2:6, 1:6]))
    assert np.array_equal(bits(R.crop(x)), bits(x))
    for bad in (dict(woffset=9), dict(outw=10), dict(hoffset=3, outh=5), dict(coffset=-1), dict(woffset=5, woffset2=4)):
        with pytest.raises(ValueError):
            R.crop(x, **bad)


@pytest.mark.parametrize("case", C.SHUFFLES, ids=C.shuffle_id)
def test_the_pixel_shuffle_restatement_equals_torch_and_inverts_reorg(case):
    import torch
    r, Cq, mode, (h, w) = case
    x = C.shuffle_input(case)
    got = R.pixel_shuffle(x, r, mode)
    assert got.shape == (2, Cq, h * r, w * r)
    if mode == 0:
        want = torch.nn.functional.pixel_shuffle(torch.from_numpy(x.view(np.int32).copy()), r).numpy()  # on the words: nothing may touch a NaN
        assert np.array_equal(bits(got), want)
    back = yolo_ref.reorg(got, r, mode)  # PixelShuffle mode m inverts Reorg mode m
    assert np.array_equal(bits(back), bits(x))
    assert C.shuffle_target(r, w, h) in C.targets()


def test_the_shuffle_cases_reach_both_kernels_on_both_sides_of_the_tile():
    rw = sorted({r * w for r, _, _, (h, w) in C.SHUFFLES if r > 1})
    assert C.TILE in rw and any(C.TILE - 4 < v < C.TILE for v in rw) and any(C.TILE < v <= C.TILE + 4 for v in rw)
    assert {C.shuffle_target(r, w, h) for r, _, _, (h, w) in C.SHUFFLES} == {t for t in C.targets() if "shuffle" in t}
    tiled = [(r, h, w) for r, _, _, (h, w) in C.SHUFFLES if "tile" in C.shuffle_target(r, w, h)]
    assert (4, 8, 8) in tiled and (2, 8, 8) not in tiled  # a block of the tile kernel moves TILE_MIN elements or more: 32 x 32 does, 16 x 16 does not
    assert all(min(h * r, C.TILE // (r * w)) * r * w >= C.TILE_MIN for r, h, w in tiled)


def test_the_activation_of_the_restatement():
    x = np.asarray([1.5, -2.0, 0.0, -0.0, np.nan, np.inf, -np.inf], F)
    got = R.activation(x, R.RELU_SLOPE, 0.2)
    assert np.array_equal(got[[0, 1, 2, 5, 6]], np.asarray([1.5, F(-2.0) * F(0.2), 0.0, np.inf, -np.inf], F)) and np.isnan(got[4]) and np.signbit(got[3])
    zero = R.activation(x, R.RELU_SLOPE, 0.0)
    assert np.signbit(zero[1]) and zero[1] == 0 and np.isnan(zero[4])  # one product: a negative x gives -0.0, a NaN stays
    plain = R.activation(x, R.RELU_PLAIN)
    assert np.array_equal(bits(plain), bits(np.asarray([1.5, 0, 0, 0, 0, np.inf, 0], F)))
    assert R.activation(x, R.RELU_NONE) is x or np.array_equal(bits(R.activation(x)), bits(x))


# ---- the switch --------------------------------------------------------------------------------------------------------------------------
GOOD = {"Padding": ("0=1 1=1 2=1 3=1", 1), "Crop": ("0=1 1=1", 1), "PixelShuffle": ("0=2", 1)}


def _one(type_, params="", bottoms=1, tops=1, c=4, h=6, w=8):
    """A net of `bottoms` Inputs in0 .. and one layer `l` of `type_` that reads them all."""
    lines = [f"Input in{k} 0 1 in{k} 0={w} 1={h} 2={c}" for k in range(bottoms)]
    lines.append(f"{type_} l {bottoms} {tops} " + " ".join(f"in{k}" for k in range(bottoms)) + " " + " ".join("t%d" % k for k in range(tops)) + " " + params)
    return ("7767517\n%d %d\n" % (len(lines), bottoms + tops) + "\n".join(lines) + "\n").encode()


def _net(param, weights=None, frame=False, level=1, **switches):
    from feathercnn_amd.net import Net
    net = Net(fusion=level)
    if frame:
        net.SetFrame()
    if switches.get("detection"):
        net.SetDetection(True)
    if switches.get("extended"):
        net.SetExtendedLayers(True)
    if switches.get("yolo"):
        net.SetYolo(switches["yolo"])
    if switches.get("roi"):
        net.SetRoi()
    if switches.get("dilated"):
        net.SetDilated(True)
    if switches.get("quantized"):
        net.SetQuantized(True)
    net.LoadParam(param)
    if weights is not None:
        net.LoadWeights(weights)
    return net


def _refused(param, code, word, **kw):
    from feathercnn_amd import FeatherHipError
    with pytest.raises(FeatherHipError, match=f"code {code}") as e:
        _net(param, **kw)
    assert word in str(e.value), str(e.value)
    return str(e.value)


@pytest.mark.parametrize("type_", sorted(GOOD))
def test_default_net_refuses_the_new_types(type_):
    p = _one(type_, *GOOD[type_])
    for other in ({}, dict(detection=True), dict(extended=True), dict(yolo=8), dict(roi=True), dict(detection=True, extended=True, yolo=8, roi=True)):
        msg = _refused(p, -200, type_, **other)
        assert "lifts this" not in msg and "fhip_net_set_extended_layers" not in msg and "(fhip_net_set_frame enables it)" in msg
    assert (type_, "l", "FRAME") in _net(p, frame=True).layers()
    assert (type_, "l", "FRAME") in _net(p, frame=True, detection=True, extended=True, yolo=8, roi=True).layers()


def test_on_then_off_equals_the_default_and_the_switch_is_refused_after_loadparam():
    from feathercnn_amd import FeatherHipError
    from feathercnn_amd.net import Net
    net = Net()
    net.SetFrame()
    net.SetFrame(False)
    with pytest.raises(FeatherHipError, match="code -200") as e:
        net.LoadParam(_one("PixelShuffle", "0=2"))
    assert "PixelShuffle" in str(e.value) and "lifts this" not in str(e.value)
    net = _net(_one("ReLU"))
    with pytest.raises(FeatherHipError, match="before LoadParam") as e:
        net.SetFrame()
    assert "code -2" in str(e.value)


def test_the_route_code_and_the_bindings():
    import feathercnn_amd
    from feathercnn_amd import _lib, frame, net
    header = open(SC.INCLUDE + "/feather_hip/feather_frame.h").read()
    code = int(re.search(r"#define\s+FHIP_FRAME_NET_ROUTE\s+(\d+)", header).group(1))
    assert code == net.FRAME_ROUTE == frame.NET_ROUTE == feathercnn_amd.FRAME_NET_ROUTE == R.NET_ROUTE == 112 and net.ROUTE_NAMES[112] == "FRAME"
    assert list(net.ROUTE_NAMES.values()).count("FRAME") == 1 and list(_lib.STANDALONE_LIBRARIES) == ["frame"]
    assert int(re.search(r"#define\s+FHIP_FRAME_TILE\s+(\d+)", header).group(1)) == frame.TILE == C.TILE
    text = open(SC.INCLUDE + "/feather_hip/feather_net.h").read()
    assert "FHIP_FRAME_NET_ROUTE" not in re.sub(r"/\*.*?\*/", "", text, flags=re.S)  # the set of FHIP_NET_ROUTE_* there is pinned: the code lives in its own header
    cxx = open(SC.INCLUDE + "/feather/net.h").read()
    assert "fhip_net_set_frame" in text and "fhip_net_set_frame" in _lib.SIGNATURES and "SetFrame(bool on = true)" in cxx and callable(net.Net.SetFrame)
    for f in ("pad", "crop", "window", "window_output_dim", "pixel_shuffle", "pixel_shuffle_output_dim", "frame_route"):
        assert callable(getattr(feathercnn_amd, f)) and f in feathercnn_amd.__all__, f
    seen = {frame.frame_route(frame.WINDOW, t, 0, pad, ow, al) for t in range(3) for pad in (0, 1) for ow in (8, 9) for al in (0, 1)}
    shuffles = {(r, w, h): frame.frame_route(frame.SHUFFLE, r, w, h) for r, w, h in ((1, 8, 8), (2, 8, 8), (4, 8, 8), (2, C.TILE // 2, 1), (2, C.TILE // 2 + 1, 1))}
    assert all(name == C.shuffle_target(*k) for k, name in shuffles.items()) and "tile" in shuffles[(4, 8, 8)] and "direct" in shuffles[(2, 8, 8)]
    assert seen | set(shuffles.values()) == C.targets()
    header_min = int(re.search(r"#define\s+FHIP_FRAME_TILE_MIN\s+(\d+)", header).group(1))
    assert header_min == frame.TILE_MIN == C.TILE_MIN
    assert frame.frame_route(frame.WINDOW, 2, 0, 1, 8, 0) == "fhip::window_kernel<2, 0>" and frame.frame_route(frame.WINDOW, 2, 0, 0, 8, 1) == "fhip::window_kernel<3, 1>"
    assert frame.window_output_dim(3, 5, 7, 1, 2, -1, 3, 0, -2) == (6, 7, 5) == R.window_output_dim(3, 5, 7, 1, 2, -1, 3, 0, -2)
    assert frame.pixel_shuffle_output_dim(3, 18, 5, 7) == (2, 15, 21) == R.pixel_shuffle_output_dim(3, 18, 5, 7)


# ---- refusals at LoadParam (-100) ------------------------------------------------------------------------------------------------------
LOADPARAM_REFUSALS = [
    ("Padding", "0=-1", 1, "0=-1"), ("Padding", "3=-7", 1, "3=-7"), ("Padding", "0=-233", 1, "dynamic"), ("Padding", "2=-233", 1, "dynamic"),
    ("Padding", "0=1", 2, "dynamic"), ("Padding", "0=1 4=3", 1, "type"), ("Padding", "0=1 4=-1", 1, "type"), ("Padding", "4=1 6=4", 1, "type 0"),
    ("Padding", "4=2 7=1", 1, "type 0"), ("Padding", "4=1 8=2", 1, "type 0"), ("Padding", "7=-1", 1, "7=-1"), ("Padding", "6=-4", 1, "6=-4"),
    ("Padding", f"0={-INT_MAX}", 1, "must be >= 0"),
    ("Crop", "-23309=1,2", 1, "starts"), ("Crop", "-23310=1,4", 1, "starts"), ("Crop", "-23311=1,0", 1, "starts"), ("Crop", "0=-1", 1, "0=-1"),
    ("Crop", "7=-2", 1, "7=-2"), ("Crop", "0=1", 3, "one or two bottoms"), ("Crop", "3=0", 1, "3=0"), ("Crop", f"5={-INT_MAX}", 1, "5="),
    ("PixelShuffle", "0=0", 1, "0=0"), ("PixelShuffle", "0=-2", 1, "0=-2"), ("PixelShuffle", "0=2 1=2", 1, "1=2"), ("PixelShuffle", "0=2 1=-1", 1, "1=-1"),
    ("PixelShuffle", "0=2", 2, "one bottom"),
]


@pytest.mark.parametrize("type_,params,bottoms,word", LOADPARAM_REFUSALS, ids=lambda v: str(v).replace(" ", "_"))
def test_loadparam_refusals(type_, params, bottoms, word):
    msg = _refused(_one(type_, params, bottoms), -100, word, frame=True)
    assert "layer l" in msg


def test_ids_outside_a_layers_list_are_out_of_range():
    for type_ in GOOD:
        _refused(_one(type_, GOOD[type_][0] + " 40=1.0"), -2, "out of range", frame=True)


def test_good_forms_load():
    for params in ("0=0 1=1 2=0 3=1", "0=3 1=3 2=3 3=3 4=2", "0=1 1=2 4=1", "5=0.5 7=1 8=2", "0=1 6=4", f"0={INT_MAX} 2={INT_MAX}", ""):
        _net(_one("Padding", params), frame=True)
    for params, bottoms in (("0=1 1=2 2=1 3=4 4=2 5=2", 1), ("6=1 7=1 8=1", 1), ("0=1 1=1", 2), ("3=-233 4=-233 5=-233", 1), (f"0={INT_MAX}", 1), ("", 1)):
        _net(_one("Crop", params, bottoms), frame=True)
    for params in ("0=2", "0=1", "0=2 1=1", "0=46341", ""):
        _net(_one("PixelShuffle", params), frame=True)


def test_a_per_channel_size_that_overruns_the_bin_fails_loadweights_naming_the_layer():
    from feathercnn_amd import FeatherHipError
    for size, data in ((4, b"\0" * 12), (INT_MAX, b"\0" * 64), (4, b"")):
        net = _net(_one("Padding", f"0=1 6={size}"), frame=True)
        with pytest.raises(FeatherHipError) as e:
            net.LoadWeights(data)
        assert "Layer l loading weights failed" in str(e.value), str(e.value)
    net = _net(_one("Padding", "0=1 6=4"), frame=True)
    net.LoadWeights(struct.pack("<4f", 1, 2, 3, 4))
    from feathercnn_amd import FeatherHipError as E
    net = _net(_one("Padding", "0=1 6=4"), frame=True)  # a layer with per-channel values needs a weight file, the others do not
    with pytest.raises(E, match="weights have not been loaded"):
        net.Forward()


# ---- the fusion plans --------------------------------------------------------------------------------------------------------------------
def _fused(param, weights, level, **switches):
    """The net after the fusion pass: Forward runs it first and then stops at the input that has not been fed."""
    from feathercnn_amd import FeatherHipError
    net = _net(param, weights, frame=True, level=level, **switches)
    with pytest.raises(FeatherHipError, match="has not been fed"):
        net.Forward()
    return net


def _pads(net, name):
    i = [nm for _, nm, _ in net.layers()].index(name)
    p = net.conv_params()[i][0]
    return p.pad_top, p.pad_bottom, p.pad_left, p.pad_right


@pytest.mark.parametrize("name", ["tiny_frame", "mobilenet_v1_tf"])
def test_fusion_2_folds_the_zero_paddings_and_only_those(name):
    from feathercnn_amd import model_zoo
    kw = dict(classes=10) if name == "mobilenet_v1_tf" else {}
    p, b, i, o = model_zoo.MODELS[name](**kw)
    assert model_zoo.MODELS[name](dry=True, **kw) == (p, len(b), i, o)  # the dry builder writes the same .param and counts the same bytes
    folded, kept = model_zoo.ZERO_PADDINGS[name]
    written = [(t, nm) for t, nm, *_ in R.parse_param(p)]
    assert {nm for t, nm in written if t == "Padding"} == set(folded) | set(kept)
    for level in (0, 1):
        net = _fused(p, b, level)
        names = [nm for _, nm, _ in net.layers()]
        assert set(folded) | set(kept) <= set(names)
        if level == 0:
            assert [(t, nm) for t, nm, _ in net.layers()] == written
    net = _fused(p, b, 2)
    layers = net.layers()
    names = [nm for _, nm, _ in layers]
    assert not set(folded) & set(names) and set(kept) <= set(names)
    conv_behind = {pad: [l[1] for l in R.parse_param(p) if pad in l[2]][0] for pad in folded}
    for pad, conv in conv_behind.items():
        assert _pads(net, conv) == (0, 1, 0, 1), (pad, conv)  # the convolution's own pad 0 plus the Padding's (0, 1, 0, 1)
        assert _pads(_fused(p, b, 1), conv) == (0, 0, 0, 0)
    if name == "tiny_frame":
        assert ("PixelShuffle", "ps0", "FRAME") in layers and "relu_ps" not in names and "relu_ps" in [nm for _, nm, _ in _fused(p, b, 1).layers()]
        assert _pads(net, "out") == (1, 1, 1, 1) and _pads(net, "conv1") == (0, 0, 0, 0)
    assert all(a == "FRAME" for t, _, a in layers if t in ("Padding", "Crop", "PixelShuffle"))


def _pad_conv(pad_params, conv_params, extra=(), weights=8 * 4 * 9 + 8):
    """Input -> Padding pad -> Convolution conv (4 -> 8, 3x3) [+ extra lines]; -> (param, bin)."""
    lines = ["Input data 0 1 data 0=8 1=8 2=4", f"Padding pad 1 1 data pad {pad_params}", f"Convolution conv 1 1 pad conv 0=8 1=3 5=1 6=288 {conv_params}"] + list(extra)
    blobs = 3 + sum(int(l.split()[3]) for l in extra)
    param = ("7767517\n%d %d\n" % (len(lines), blobs) + "\n".join(lines) + "\n").encode()
    return param, struct.pack("<I", 0) + np.zeros(weights, F).tobytes()


def test_what_folds_and_what_stays():
    def names(param, weights, **sw):
        return [nm for _, nm, _ in _fused(param, weights, 2, **sw).layers()]

    p, b = _pad_conv("0=0 1=1 2=0 3=1", "3=2")
    net = _fused(p, b, 2)
    assert [nm for _, nm, _ in net.layers()] == ["data", "conv"] and _pads(net, "conv") == (0, 1, 0, 1)
    p, b = _pad_conv("0=2 1=1 2=3 3=0", "4=1")  # onto pads the convolution has: the sums
    net = _fused(p, b, 2)
    assert _pads(net, "conv") == (3, 2, 4, 1) and "pad" not in [nm for _, nm, _ in net.layers()]
    assert "pad" in names(*_pad_conv("0=1 1=1 2=1 3=1 5=0.5", ""))           # a value other than 0
    assert "pad" in names(*_pad_conv("0=1 1=1 2=1 3=1 5=-0.0", ""))          # -0.0 is not the convolution's +0.0 either
    assert "pad" in names(*_pad_conv("0=1 1=1 2=1 3=1 4=1", ""))             # replicate
    assert "pad" in names(*_pad_conv("0=1 1=1 2=1 3=1 4=2", ""))             # reflect
    p, b = _pad_conv("0=1 6=4", "")
    assert "pad" in names(p, np.zeros(4, F).tobytes() + b)                   # per-channel values (they precede the convolution's in the .bin)
    assert "pad" in names(*_pad_conv("0=1 1=1 2=1 3=1", "", extra=["ReLU second 1 1 pad second"]))  # two readers
    assert "pad" in names(*_pad_conv("0=1 1=1 2=1 3=1", "4=-233"))           # automatic pads are no pads to add to
    assert "pad" in names(*_pad_conv("0=1 1=1 2=1 3=1", "2=2"), dilated=True)  # a dilated layer
    p, _ = _pad_conv("0=1 1=1 2=1 3=1", "8=1")                              # an int8 layer
    q = struct.pack("<I", 0x000D4B38) + bytes(288) + np.zeros(8, F).tobytes() + np.ones(8, F).tobytes() + np.ones(1, F).tobytes()
    assert "pad" in names(p, q, quantized=True)
    lines = ["Input data 0 1 data 0=8 1=8 2=4", "Padding pad 1 1 data pad 0=1 1=1 2=1 3=1 7=1", "Convolution conv 1 1 pad conv 0=8 1=3 5=1 6=360"]
    p = ("7767517\n3 3\n" + "\n".join(lines) + "\n").encode()
    assert "pad" in names(p, struct.pack("<I", 0) + np.zeros(360 + 8, F).tobytes())  # a channel margin
    # a depthwise layer folds too
    lines = ["Input data 0 1 data 0=8 1=8 2=4", "Padding pad 1 1 data pad 0=0 1=1 2=0 3=1", "ConvolutionDepthWise conv 1 1 pad conv 0=4 1=3 3=2 6=36 7=4"]
    p = ("7767517\n3 3\n" + "\n".join(lines) + "\n").encode()
    net = _fused(p, struct.pack("<I", 0) + np.zeros(36, F).tobytes(), 2)
    assert [nm for _, nm, _ in net.layers()] == ["data", "conv"] and _pads(net, "conv") == (0, 1, 0, 1)


# ---- the host refusals of the C-ABI ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    return SC.library("frame")


def _bad(lib, rc, word=""):
    assert rc == SC.BADARG, rc
    msg = lib.fhip_frame_last_error().decode()
    assert word in msg, msg


A, B = 0x10000000, 0x20000000  # addresses that are never touched: every call below is refused on the host


def _window(lib, type_=0, per_channel=None, n=1, c=3, h=4, w=5, m=(0, 0, 1, 1, 1, 1), out=A, in_=B, value=0.0):
    return lib.fhip_frame_window_forward(type_, ctypes.c_float(value), per_channel, n, c, h, w, *m, ctypes.c_void_p(out), ctypes.c_void_p(in_), None)


def _shuffle(lib, r=2, mode=0, relu=0, n=1, c=8, h=4, w=5, out=A, in_=B):
    return lib.fhip_pixel_shuffle_forward(r, mode, relu, ctypes.c_float(0), n, c, h, w, ctypes.c_void_p(out), ctypes.c_void_p(in_), None)


def test_the_window_refuses_on_the_host(lib):
    _bad(lib, _window(lib, out=0), "null")
    _bad(lib, _window(lib, in_=0), "null")
    _bad(lib, _window(lib, out=A + 2), "aligned")
    _bad(lib, _window(lib, in_=B + 1), "aligned")
    _bad(lib, _window(lib, per_channel=ctypes.c_void_p(B + 2)), "aligned")
    _bad(lib, _window(lib, out=B + 16), "overlap")
    _bad(lib, _window(lib, in_=A + 4 * 3 * 6 * 7 - 4), "overlap")
    for dims in (dict(n=0), dict(c=0), dict(h=0), dict(w=-1)):
        _bad(lib, _window(lib, **dims), "< 1")
    for m in ((0, 0, -2, -2, 0, 0), (0, 0, 0, 0, -5, 0), (-1, -2, 0, 0, 0, 0), (0, 0, -INT_MAX, 0, 0, 0)):
        _bad(lib, _window(lib, m=m), "output dimension")
    _bad(lib, _window(lib, n=1 << 16, c=1 << 10, h=8, w=4, m=(0,) * 6), "2^31")
    _bad(lib, _window(lib, n=4, c=4, h=4, w=4, m=(0, 0, 1 << 14, 0, 1 << 14, 0)), "2^31")
    _bad(lib, _window(lib, m=(0, 0, INT_MAX, 0, 0, 0)), "2^31")
    _bad(lib, _window(lib, m=(INT_MAX, INT_MAX, INT_MAX, INT_MAX, INT_MAX, INT_MAX)), "2^31")
    for t in (-1, 3, INT_MAX):
        _bad(lib, _window(lib, type_=t), "type")
    for m in ((0, 0, 4, 0, 0, 0), (0, 0, 0, 4, 0, 0), (0, 0, 0, 0, 5, 0), (0, 0, 0, 0, 0, 9)):
        _bad(lib, _window(lib, type_=2, m=m), "reflect")
    for t in (1, 2):
        _bad(lib, _window(lib, type_=t, m=(1, 0, 0, 0, 0, 0)), "type 0")
        _bad(lib, _window(lib, type_=t, m=(0, 2, 0, 0, 0, 0)), "type 0")
        _bad(lib, _window(lib, type_=t, per_channel=ctypes.c_void_p(B + 4096)), "type 0")
    o = [ctypes.c_int() for _ in range(3)]
    _bad(lib, lib.fhip_frame_window_output_dim(3, 4, 5, 0, 0, 0, 0, 0, 0, None, ctypes.byref(o[1]), ctypes.byref(o[2])), "null")
    _bad(lib, lib.fhip_frame_window_output_dim(3, 4, 5, 0, 0, -4, 0, 0, 0, *[ctypes.byref(v) for v in o]), "output dimension")
    assert lib.fhip_frame_window_output_dim(3, 4, 5, 1, 2, -1, 3, 0, -2, *[ctypes.byref(v) for v in o]) == 0 and [v.value for v in o] == [6, 6, 3]


def test_pixel_shuffle_refuses_on_the_host(lib):
    _bad(lib, _shuffle(lib, out=0), "null")
    _bad(lib, _shuffle(lib, in_=0), "null")
    _bad(lib, _shuffle(lib, out=A + 1), "aligned")
    _bad(lib, _shuffle(lib, in_=B + 2), "aligned")
    _bad(lib, _shuffle(lib, out=B + 4 * 8 * 4 * 5 - 4), "overlap")
    for r in (0, -1):
        _bad(lib, _shuffle(lib, r=r), "upscale_factor")
    _bad(lib, _shuffle(lib, r=46341, c=INT_MAX), "multiple")  # r * r passes 2^31
    _bad(lib, _shuffle(lib, r=3, c=8), "multiple")
    _bad(lib, _shuffle(lib, r=2, c=2), "multiple")
    for mode in (-1, 2):
        _bad(lib, _shuffle(lib, mode=mode), "mode")
    for relu in (-1, 3):
        _bad(lib, _shuffle(lib, relu=relu), "relu")
    for dims in (dict(n=0), dict(c=0), dict(h=0), dict(w=0)):
        _bad(lib, _shuffle(lib, **dims))
    _bad(lib, _shuffle(lib, n=1 << 12, c=1 << 10, h=1 << 5, w=1 << 4), "2^31")
    o = [ctypes.c_int() for _ in range(3)]
    _bad(lib, lib.fhip_pixel_shuffle_output_dim(2, 8, 4, 5, ctypes.byref(o[0]), None, ctypes.byref(o[2])), "null")
    _bad(lib, lib.fhip_pixel_shuffle_output_dim(2, 8, 1 << 30, 5, *[ctypes.byref(v) for v in o]), "2^31")


def test_the_route_refuses(lib):
    name = ctypes.create_string_buffer(64)
    _bad(lib, lib.fhip_frame_route(0, 0, 0, 0, 0, 0, None, 0), "null")
    _bad(lib, lib.fhip_frame_route(0, 0, 0, 1, 8, 1, name, 0), "null")
    _bad(lib, lib.fhip_frame_route(2, 0, 0, 0, 8, 1, name, 64), "unknown")
    _bad(lib, lib.fhip_frame_route(C.WINDOW, 3, 0, 1, 8, 1, name, 64), "type")
    _bad(lib, lib.fhip_frame_route(C.WINDOW, 0, 0, 1, 0, 1, name, 64), "out_w")
    _bad(lib, lib.fhip_frame_route(C.SHUFFLE, 0, 8, 8, 0, 0, name, 64), "< 1")
    _bad(lib, lib.fhip_frame_route(C.SHUFFLE, 2, 0, 8, 0, 0, name, 64), "< 1")
    _bad(lib, lib.fhip_frame_route(C.SHUFFLE, 2, 8, 0, 0, 0, name, 64), "< 1")
