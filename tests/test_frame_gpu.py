"""libfeather_frame.so and the framing layers of the Net runtime on the device, against tests/frame_ref.py.

* The window (Padding and Crop) and PixelShuffle equal the restatement bit for bit (int32 views: NaN payloads and -0.0 count), from 16-byte
  aligned and from misaligned guarded buffers (tests/guarded.py): an element written outside `out`, or one left unwritten, fails.
* One kernel trace: the sweep launches what fhip_frame_route names, and that is every instantiation of the library.
* tiny_frame through the Net at batch 3: fusion 0, 1, 2, the graph on and off, 1 and 2 sub-batch replicas.  Every framing layer's top is
  the restatement of its own bottom, bit for bit; the outputs are within the project's net-level bound (normalised max error <= 1e-4,
  tests/test_net_gpu.py; tests/helpers.py holds no number of its own) of the fp64 restatement and of fusion level 0; the fused
  PixelShuffle + ReLU equals the two layers bit for bit.
* What only a Reshape can refuse (-100; a q8 bottom: -300, and a zero Padding in front of a requantised convolution stays), re-planning across input sizes, and FeedPixels -> espcn_x3 -> ExtractPixels end to end."""
import numpy as np
import pytest

import frame_cases as C
import frame_ref as R
import frame_sweep as SW
import kernel_instances as KI
import ktrace
import side_contract

pytestmark = pytest.mark.gpu
F = np.float32
TOL = 1e-4  # the project's net-level bound (tests/test_net_gpu.py)


@pytest.fixture(scope="module")
def lib(cuda):
    return side_contract.library("frame")


# ---- the C-ABI: exact --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(C.WINDOWS))
def test_the_window_is_a_bit_copy(lib, name):
    x, kw, want = C.window_case(name)
    for offset in (0, 1):
        got = SW.window(lib, x, offset=offset, **kw)
        assert SW.same_bits(got, want), (name, offset, int((got.view(np.uint32) != want.view(np.uint32)).sum()))
        assert SW.route(lib, C.WINDOW, kw["type_"], 0, int(C.window_pads(name)), want.shape[3], 1 - offset) == C.window_target(kw["type_"], C.window_pads(name),
                                                                                                                  want.shape[3], not offset)


@pytest.mark.parametrize("case", C.SHUFFLES, ids=C.shuffle_id)
def test_pixel_shuffle_is_exact(lib, case):
    r, _, mode, (h, w) = case
    x = C.shuffle_input(case)
    for k, (relu, slope) in enumerate(C.RELUS):
        got = SW.pixel_shuffle(lib, x, r, mode, relu, slope, offset=(C.SHUFFLES.index(case) + k) % 2)  # aligned and misaligned buffers in turn
        want = R.pixel_shuffle(x, r, mode, relu, slope)
        if relu == R.RELU_PLAIN:  # the device maximum: a zero's sign is its own (feather_frame.h), everything else is exact
            assert got.shape == want.shape and np.array_equal(got, want) and not np.isnan(got).any(), (case, relu)
        else:
            assert SW.same_bits(got, want), (case, relu, slope, int((got.view(np.uint32) != want.view(np.uint32)).sum()))
    assert SW.route(lib, C.SHUFFLE, r, w, h) == C.shuffle_target(r, w, h)


def test_the_python_mirror(cuda):
    import torch
    from feathercnn_amd import frame
    x, kw, want = C.window_case("const_channels_per_channel")
    t = torch.from_numpy(x).cuda()
    got = frame.window(t, kw["type_"], float(kw["value"]), torch.from_numpy(kw["per_channel"]).cuda(), kw["front"], kw["behind"], kw["top"], kw["bottom"], kw["left"],
                       kw["right"])
    assert SW.same_bits(got.cpu().numpy(), want)
    x, kw, want = C.window_case("ref_7x9_left1")
    assert SW.same_bits(frame.pad(torch.from_numpy(x).cuda(), kw["top"], kw["bottom"], kw["left"], kw["right"], frame.REFLECT).cpu().numpy(), want)
    assert SW.same_bits(frame.crop(torch.from_numpy(x).cuda(), 2, 1, 1, 4, 3, 2).cpu().numpy(), R.crop(x, 2, 1, 1, 4, 3, 2))
    case = C.SHUFFLES[7]
    x = C.shuffle_input(case)
    got = frame.pixel_shuffle(torch.from_numpy(x).cuda(), case[0], case[2], frame.RELU_SLOPE, 0.2)
    assert SW.same_bits(got.cpu().numpy(), R.pixel_shuffle(x, case[0], case[2], R.RELU_SLOPE, 0.2))
    mode0 = [c for c in C.SHUFFLES if c[2] == 0 and c[3] == (8, 8)][0]
    x = np.random.default_rng(1).uniform(-1, 1, C.shuffle_input(mode0).shape).astype(F)
    t = torch.from_numpy(x).cuda()
    assert torch.equal(frame.pixel_shuffle(t, mode0[0]), torch.nn.functional.pixel_shuffle(t, mode0[0]))


def test_the_sweep_launches_what_the_route_names(cuda, tmp_path):
    """One child under rocprofv3 --kernel-trace (tests/frame_trace_child.py): the library's kernels in the trace are, launch for launch, the
    routes fhip_frame_route named, and together every instantiation tests/frame_cases.targets() names -- which is every instantiation the
    library holds (tests/test_frame_contract_cpu.py)."""
    text, rows, _ = ktrace.trace("frame_trace_child.py", [], tmp_path, 240)
    named = [ln[len("route "):] for ln in text.splitlines() if ln.startswith("route ")]
    launched = [KI.normalise(name) for _, name, *_ in rows]
    launched = [nm for nm in launched if nm in C.targets()]
    assert launched == named, (launched, named)
    assert set(launched) == C.targets()


# ---- the net -----------------------------------------------------------------------------------------------------------------------------
def _nerr(got, want):
    return float(np.abs(got.astype(np.float64) - want).max() / max(np.abs(want).max(), 1e-30))


def _net(level=2, graph=False, replicas=1, model=None):
    from feathercnn_amd.net import Net
    p, b, i, o = model or C.net_model()[0]
    net = Net(fusion=level, graph=graph, sub_batches=replicas)
    net.SetFrame()
    net.LoadParam(p)
    net.LoadWeights(b)
    return net


def _own_restatement(net, blobs_of, layer):
    """The restatement of one framing layer of tiny_frame applied to the bottoms the net itself holds."""
    type_, name, bottoms, tops, pd = layer
    v = [blobs_of(b) for b in bottoms]
    if type_ == "Padding":
        pc = None
        if pd.get(6, 0):
            pc = dict((nm, a) for kind, nm, _, _, a in C.net_model()[1] if kind == "padding")[name]["per_channel"]
        return R.pad(v[0], pd.get(0, 0), pd.get(1, 0), pd.get(2, 0), pd.get(3, 0), pd.get(4, 0), F(pd.get(5, 0.0)), pc, pd.get(7, 0), pd.get(8, 0))
    if type_ == "Crop":
        return R.crop(v[0], pd.get(0, 0), pd.get(1, 0), pd.get(2, 0), pd.get(3, -233), pd.get(4, -233), pd.get(5, -233), pd.get(6, 0), pd.get(7, 0), pd.get(8, 0),
                      like=v[1] if len(v) > 1 else None)
    return R.pixel_shuffle(v[0], pd[0], pd.get(1, 0))


def _run(net, batch=3):
    (p, b, i, o), _ = C.net_model()
    x, want = C.net_input(batch)
    net.FeedInput(i, x)
    net.Forward()
    return x, want, net.Extract(o)


def test_tiny_frame_at_level_0_every_framing_top_is_the_restatement_of_its_bottom(cuda):
    (p, b, i, o), _ = C.net_model()
    net = _net(0)
    x, want, out = _run(net)
    assert SW.same_bits(net.Extract("pad_reflect"), want["pad_reflect"])  # straight behind the input: numpy_forward's blob, bit for bit
    cache = {}

    def blob(name):
        if name not in cache:
            cache[name] = net.Extract(name)
        return cache[name]

    layers = [l for l in R.parse_param(p) if l[0] in ("Padding", "Crop", "PixelShuffle")]
    assert [l[1] for l in layers] == list(C.FRAME_TOPS)
    for layer in layers:
        got = blob(layer[3][0])
        assert got.shape == want[layer[1]].shape and SW.same_bits(got, _own_restatement(net, blob, layer)), layer[1]
        assert _nerr(got, want[layer[1]]) <= TOL, (layer[1], _nerr(got, want[layer[1]]))
    assert out.shape == want[o].shape == (3, 3, 10, 12) and _nerr(out, want[o]) <= TOL, _nerr(out, want[o])
    assert sum(a == "FRAME" for _, _, a in net.layers()) == len(C.FRAME_TOPS)


def test_tiny_frame_at_every_setting(cuda):
    (p, b, i, o), _ = C.net_model()
    _, want, level0 = _run(_net(0))
    relu0 = None
    for level, graph, replicas in ((0, False, 1), (1, False, 1), (2, False, 1), (2, True, 1), (2, False, 2), (1, True, 2), (0, True, 2)):
        net = _net(level, graph, replicas)
        _, _, out = _run(net)
        if graph:  # replay the captured graph
            net.Forward()
            assert np.array_equal(net.Extract(o), out)
        err, drift = _nerr(out, want[o]), _nerr(out, level0.astype(np.float64))
        print(f"tiny_frame level {level} graph {graph} replicas {replicas}: error {err:.3g} against fp64, {drift:.3g} against level 0 (bound {TOL:g})")
        assert out.shape == level0.shape and err <= TOL and drift <= TOL, (level, graph, replicas, err, drift)
        names = [nm for _, nm, _ in net.layers()]
        top = net.Extract("relu_ps")
        if level == 0:  # the graph and the replicas change nothing: the same kernels on the same data
            assert np.array_equal(out, level0), (level, graph, replicas)
            relu0 = top if relu0 is None else relu0
            assert SW.same_bits(top, relu0)
        if level == 2:  # the zero Padding is folded and PixelShuffle has absorbed the ReLU: its top is the activation of its own bottom
            assert "relu_ps" not in names and "pad_same" not in names
            assert np.array_equal(top, R.pixel_shuffle(net.Extract("conv_up"), 2, 0, R.RELU_PLAIN))
        else:
            assert "relu_ps" in names and "pad_same" in names


def _shuffle_relu(slope):
    lines = ["Input data 0 1 data 0=6 1=5 2=8", "PixelShuffle ps 1 1 data ps 0=2", "ReLU relu 1 1 ps relu" + ("" if slope is None else f" 0={slope}")]
    return ("7767517\n3 3\n" + "\n".join(lines) + "\n").encode(), b"", "data", "relu"


@pytest.mark.parametrize("slope", [None, 0.2])
def test_pixel_shuffle_and_relu_fused_equal_the_two_layers_bit_for_bit(cuda, slope):
    x = C.planted((3, 8, 5, 6), 11)
    tops = []
    for level in (0, 2):
        net = _net(level, model=_shuffle_relu(slope))
        net.FeedInput("data", x)
        net.Forward()
        tops.append(net.Extract("relu"))
        assert ("relu" in [nm for _, nm, _ in net.layers()]) == (level == 0)
    assert tops[0].shape == (3, 2, 10, 12) and SW.same_bits(tops[0], tops[1])
    if slope is not None:
        assert SW.same_bits(tops[1], R.pixel_shuffle(x, 2, 0, R.RELU_SLOPE, slope))


def _single(type_, params, c=4, h=6, w=8, bottoms=1):
    lines = [f"Input in{k} 0 1 in{k} 0={w} 1={h} 2={c}" for k in range(bottoms)]
    lines.append(f"{type_} l {bottoms} 1 " + " ".join(f"in{k}" for k in range(bottoms)) + f" top {params}")
    return ("7767517\n%d %d\n" % (len(lines), bottoms + 1) + "\n".join(lines) + "\n").encode()


def test_no_op_layers_alias_their_bottom_and_launch_nothing(cuda):
    from feathercnn_amd.net import Net
    x = C.planted((2, 4, 6, 8), 5)
    for type_, params in (("Padding", "0=0 1=0 2=0 3=0 4=2"), ("Crop", "0=0 1=0 2=0 3=8 4=6 5=4"), ("Crop", ""), ("PixelShuffle", "0=1")):
        net = Net()
        net.SetFrame()
        net.LoadParam(_single(type_, params))
        net.LoadWeights(b"")
        net.FeedInput("in0", x)
        net.Forward()
        assert SW.same_bits(net.Extract("top"), x), (type_, params)
        assert net.ExtractDevice("top")[0] == net.ExtractDevice("in0")[0], (type_, params)  # the same storage, as a Split top


def test_shapes_that_do_not_fit_are_minus_100_at_reshape(cuda):
    from feathercnn_amd import FeatherHipError
    from feathercnn_amd.net import Net

    def run(param, feeds, weights=b"", **switches):
        net = Net()
        net.SetFrame()
        if switches.get("detection"):
            net.SetDetection(True)
        net.LoadParam(param)
        net.LoadWeights(weights)
        for k, v in feeds.items():
            net.FeedInput(k, v)
        net.Forward()
        return net

    x = np.zeros((2, 4, 6, 8), F)
    run(_single("Padding", "0=5 1=5 2=7 3=7 4=2"), dict(in0=x))  # dim - 1: the largest reflect pad
    run(_single("Padding", "0=1 6=4"), dict(in0=x), np.zeros(4, F).tobytes())
    run(_single("Crop", "0=7 1=5 2=3"), dict(in0=x))  # down to 1 x 1 x 1
    cases = [("reflect pad = h", _single("Padding", "0=6 4=2"), dict(in0=x), b""), ("reflect pad = w", _single("Padding", "3=8 4=2"), dict(in0=x), b""),
             ("per-channel size", _single("Padding", "0=1 6=5"), dict(in0=x), np.zeros(5, F).tobytes()),
             ("2^31 elements", _single("Padding", "0=20000 2=20000"), dict(in0=x), b""),
             ("INT_MAX margins", _single("Padding", "0=2147483647 1=2147483647"), dict(in0=x), b""),
             ("crop leaves w", _single("Crop", "0=3 3=6"), dict(in0=x), b""), ("crop leaves h", _single("Crop", "1=6"), dict(in0=x), b""),
             ("crop leaves c", _single("Crop", "2=2 8=2"), dict(in0=x), b""), ("crop offsets of INT_MAX", _single("Crop", "0=2147483647 6=2147483647"), dict(in0=x), b""),
             ("reference larger than the blob", _single("Crop", "", bottoms=2), dict(in0=x, in1=np.zeros((2, 4, 7, 8), F)), b""),
             ("reference of another batch", _single("Crop", "", bottoms=2), dict(in0=x, in1=np.zeros((1, 4, 6, 8), F)), b""),
             ("c % r^2", _single("PixelShuffle", "0=3"), dict(in0=x), b""), ("r of 46341", _single("PixelShuffle", "0=46341"), dict(in0=x), b"")]
    for what, param, feeds, weights in cases:
        with pytest.raises(FeatherHipError, match="code -100") as e:
            run(param, feeds, weights)
        assert "layer l" in str(e.value), (what, str(e.value))
    # under SetDetection a blob knows its rank: a flattened blob is refused
    lines = ["Input in0 0 1 in0 0=8 1=6 2=4", "Flatten flat 1 1 in0 flat", "Padding l 1 1 flat top 0=1"]
    with pytest.raises(FeatherHipError, match="code -100") as e:
        run(("7767517\n3 3\n" + "\n".join(lines) + "\n").encode(), dict(in0=x), detection=True)
    assert "rank" in str(e.value)
    got = run(_single("Crop", "0=1 1=2", bottoms=2), dict(in0=C.planted((2, 4, 6, 8), 3), in1=np.zeros((2, 2, 3, 5), F)))
    assert SW.same_bits(got.Extract("top"), C.planted((2, 4, 6, 8), 3)[:, :2, 2:5, 1:6])


# ---- q8 blobs (the int8 activation behind a requantised convolution, Net.SetRequantized) ---------------------------------------------------
def _behind_requantised(tail):
    """data -> c1 (int8 weights, requantised int8 output 8=101, 16 channels) -> `tail`."""
    from feathercnn_amd import model_zoo
    g = model_zoo.GraphBuilder(3, quant={})
    tail(g, g.conv("c1", g.input("data", 3, 8, 8), 3, 16, 3, 1, 1, requant=20.0))
    return g.finish()


def _q8_net(model, level):
    from feathercnn_amd.net import Net
    net = Net(fusion=level)
    net.SetFrame()
    net.SetQuantized(True)
    net.SetRequantized(True)
    net.LoadParam(model[0])
    net.LoadWeights(model[1])
    return net


Q8_READERS = {"Padding": lambda g, x: g.padding("r", x, 1, 1, 1, 1), "Padding_reflect": lambda g, x: g.padding("r", x, 1, 1, 1, 1, type_=2),
              "Crop": lambda g, x: g.crop("r", x, 1, 1), "PixelShuffle": lambda g, x: g.pixel_shuffle("r", x, 2)}


@pytest.mark.parametrize("name", sorted(Q8_READERS))
@pytest.mark.parametrize("level", [0, 2])
def test_a_framing_layer_cannot_read_a_q8_blob(cuda, name, level):
    """A q8 bottom is refused at Reshape by the check every layer that cannot read one meets: NET_E_TOPOLOGY (-300), naming the producer and
    the layer."""
    from feathercnn_amd import FeatherHipError
    type_ = name.split("_")[0]
    net = _q8_net(_behind_requantised(Q8_READERS[name]), level)
    net.FeedInput("data", np.random.default_rng(2).uniform(-1, 1, (2, 3, 8, 8)).astype(F))
    with pytest.raises(FeatherHipError) as e:
        net.Forward()
    msg = str(e.value)
    assert "code -300" in msg and "layer c1" in msg and type_ + " layer r" in msg and "blob c1" in msg, msg


def test_a_zero_padding_in_front_of_a_requantised_convolution_stays(cuda):
    """Padding (0, 1, 0, 1) -> int8 Convolution 8=101 (stride 2, pad 0) -> int8 Convolution: the fold leaves the int8 routes alone, so the
    Padding runs at level 2 as at level 0 and the two levels give the same bits."""
    from feathercnn_amd import model_zoo
    g = model_zoo.GraphBuilder(7, quant={})
    x = g.padding("pad", g.input("data", 3, 8, 8), 0, 1, 0, 1)
    x = g.conv("c1", x, 3, 16, 3, 2, 0, requant=20.0)
    g.conv("c2", x, 16, 8, 1)
    model = g.finish()
    x = np.random.default_rng(3).uniform(-1, 1, (2, 3, 8, 8)).astype(F)
    outs = []
    for level in (0, 2):
        net = _q8_net(model, level)
        net.FeedInput("data", x)
        net.Forward()
        names = [nm for _, nm, _ in net.layers()]
        assert names == ["data", "pad", "c1", "c2"], (level, names)
        p = net.conv_params()[names.index("c1")][0]
        assert (p.pad_top, p.pad_bottom, p.pad_left, p.pad_right) == (0, 0, 0, 0)
        assert SW.same_bits(net.Extract("pad"), R.pad(x, 0, 1, 0, 1))
        outs.append(net.Extract("c2"))
    assert outs[0].shape == (2, 8, 4, 4) and np.array_equal(outs[0], outs[1]) and outs[0].std() > 0


def _espcn(size):
    from feathercnn_amd import model_zoo
    return model_zoo.espcn_x3(seed=5, size=size, channels=3)


def test_replanning_across_input_sizes_equals_a_fresh_net(cuda):
    """The same net fed a second input size (and the first again): what a fresh net at that size gives, bit for bit."""
    rng = np.random.default_rng(9)
    xs = {size: rng.uniform(-1, 1, (2, 3) + size).astype(F) for size in ((8, 12), (11, 7))}
    for level, graph in ((2, True), (0, False)):
        net = _net(level, graph, model=_espcn((8, 12)))
        seen = {}
        for size in ((8, 12), (11, 7), (8, 12)):
            net.FeedInput("data", xs[size])
            net.Forward()
            out = net.Extract("out")
            assert out.shape == (2, 3, 3 * size[0], 3 * size[1])
            fresh = _net(level, graph, model=_espcn(size))
            fresh.FeedInput("data", xs[size])
            fresh.Forward()
            assert np.array_equal(out, fresh.Extract("out")), (level, graph, size)
            assert np.array_equal(out, seen.setdefault(size, out))
    # and a window layer whose output follows the input: a reflect Padding and a Crop by second offsets
    lines = ["Input data 0 1 data 0=8 1=6 2=3", "Padding pad 1 1 data pad 0=2 1=1 2=3 3=0 4=2", "Crop crop 1 1 pad crop 0=1 6=1 7=2"]
    param = ("7767517\n3 3\n" + "\n".join(lines) + "\n").encode()
    net = _net(2, True, model=(param, b"", "data", "crop"))
    for shape in ((2, 3, 6, 8), (3, 3, 9, 5), (2, 3, 6, 8)):
        x = C.planted(shape, sum(shape))
        net.FeedInput("data", x)
        net.Forward()
        assert SW.same_bits(net.Extract("crop"), R.crop(R.pad(x, 2, 1, 3, 0, R.REFLECT), 1, woffset2=1, hoffset2=2)), shape


def test_feed_pixels_espcn_extract_pixels_end_to_end(cuda):
    """uint8 frames in, a 3x larger uint8 image out, nothing on the host in between -- and the same bytes when the two ends and the sub-pixel
    layer are run one by one through the C-ABI on the net's own convolution output (the convolutions and TanH between them are the Net's: they
    are held to their own references in tests/test_net_gpu.py and tests/test_inorm_gpu.py)."""
    import torch
    from feathercnn_amd import PIXEL_RGB, float_to_pixels, frame, pixels_to_float
    frames = np.random.default_rng(21).integers(0, 256, (2, 16, 20, 3), dtype=np.uint8)
    norm = [1 / 255.0] * 3
    net = _net(2, model=_espcn((16, 20)))
    net.FeedPixels("data", frames, PIXEL_RGB, norm=norm)
    net.Forward()
    image = net.ExtractPixels("out", PIXEL_RGB, norm=[255.0] * 3)
    assert image.shape == (2, 48, 60, 3) and image.dtype == np.uint8 and image.std() > 0
    x = pixels_to_float(torch.from_numpy(frames).cuda(), PIXEL_RGB, norm=norm)
    assert np.array_equal(x.cpu().numpy(), net.Extract("data"))
    up = frame.pixel_shuffle(torch.from_numpy(net.Extract("conv3")).cuda(), 3)
    assert np.array_equal(up.cpu().numpy(), net.Extract("out"))
    by_hand = float_to_pixels(up, PIXEL_RGB, norm=[255.0] * 3)
    assert np.array_equal(by_hand.cpu().numpy(), image)
