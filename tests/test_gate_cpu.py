"""libfeather_gate.so (squeeze-and-excitation channel gating, Swish, HardSigmoid) without a GPU.

Checks of the yardstick, which need no library: the fp64 restatement the GPU tests compare against (tests/gate_ref.py) equals what torch
computes on the CPU (tests/golden/se_golden.npz, written by tests/golden/make_se_golden.py), and it runs tiny_se.

Checks of the feature (they fail on the parent commit, where BinaryOp answers -200 and the library does not exist): fhip_gate_route names
the kernels tests/gate_cases.py states; bad arguments are refused on the host
with their word; feather::Net loads every new line with route GATE and refuses what the definition leaves out; fusion level 2 collapses
the blocks of tiny_se that match and leaves the one that does not; the zoo nets load at every level and the restatement reads every
weight byte.  What the library shares with the other run-time libraries -- its exports, the instantiations it holds, its route code, the build
of its application, its last-error state -- is in tests/test_side_contract_cpu.py."""
import ctypes
import os

import numpy as np
import pytest

import gate_cases as GC
import gate_ref as R
import side_contract

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "se_golden.npz")
BADARG = -2
NEW_MODELS = ["tiny_se", "se_resnet50", "efficientnet_b0"]


lib = side_contract.fixture("gate")


# ---- the definition ------------------------------------------------------------------------------------------------------------------
def test_restatement_against_golden():
    g = np.load(GOLDEN)
    worst = 0.0
    for tag, mact, gact in (("relu_sigmoid", "relu", "sigmoid"), ("swish_hsig", "swish", "hard_sigmoid"), ("none_sigmoid", None, "sigmoid")):
        t = lambda k: g[f"{tag}.{k}"]
        mean = R.squeeze(t("x"))
        gate = R.excite(mean, t("w1"), t("b1"), t("w2"), t("b2"), mact, gact, alpha=1.0 / 6, beta=0.5)
        # alpha = 1 / 6 is handed to the library as a float32: the restatement follows it, torch divides by 6 in float64
        tol = 1e-12 if gact == "sigmoid" else 4e-8
        for got, want, bound in ((mean, t("mean"), 1e-12), (gate, t("gate"), tol), (R.channel_gate(t("x"), t("gate")), t("y"), 1e-12),
                                 (R.channel_gate(t("x"), t("gate"), t("res")), t("y_res"), 1e-12),
                                 (R.channel_gate(t("x"), t("gate"), t("res"), relu=True), t("y_res_relu"), 1e-12)):
            e = float(np.abs(got - want).max())
            worst = max(worst, e)
            assert got.shape == want.shape and e <= bound, (tag, e)
    hs = g["swish_hsig.gate"]
    assert (hs == 0).any() and (hs == 1).any() and ((hs > 0) & (hs < 1)).any()  # the golden block reaches both clamps
    assert np.abs(R.swish(g["act.x"]) - g["act.swish"]).max() <= 1e-12
    assert np.abs(R.hard_sigmoid(g["act.x"], 1.0 / 6, 0.5) - g["act.hardsigmoid"]).max() <= 1e-12
    assert np.array_equal(R.hard_sigmoid(np.float32([-3, -2.5, 0, 2.5, 3]), 0.2, 0.5, np.float32), np.float32([0, 0, 0.5, 1, 1]))
    print(f"gate_ref vs torch (fp64): worst absolute difference {worst:.2e}")


def test_restatement_runs_tiny_se():
    from feathercnn_amd import model_zoo
    p, b, i, o = model_zoo.tiny_se()
    ref = R.Net(p, b)
    assert ref.read == len(b)
    x = np.random.default_rng(3).uniform(-1, 1, (2, 3, 24, 24)).astype(np.float32)
    blobs = ref.run(i, x, o, keep=True)
    shapes = {k: v.shape for k, v in blobs.items()}
    assert shapes["a_scale"] == (2, 16, 24, 24) and shapes["b_mul"] == (2, 24, 12, 12) and shapes["c_mul"] == (2, 20, 5, 5) and shapes["d_scale"] == (2, 20, 5, 5)
    assert shapes["a_sigmoid"] == (2, 16, 1, 1) and shapes["aux"] == (2, 4, 1, 1)
    assert np.allclose(blobs["prob"].reshape(2, -1).sum(axis=1), 1.0, atol=1e-5)
    # the layers under test, from their inputs: the gate first among c_mul's bottoms, second among b_mul's
    assert np.array_equal(blobs["b_mul"], R.channel_gate(blobs["b_split_0"], blobs["b_sigmoid"], dtype=np.float32))
    assert np.array_equal(blobs["c_mul"], R.channel_gate(blobs["c_split_0"], blobs["c_hsigmoid"], dtype=np.float32))
    assert 0 < blobs["c_hsigmoid"].min() and blobs["c_hsigmoid"].max() <= 1


# ---- the library ---------------------------------------------------------------------------------------------------------------------
def test_instantiations_and_route_names(lib):
    name = ctypes.create_string_buffer(96)
    v = ctypes.c_void_p
    seen = set()
    for h, w in GC.APPLY_PLANES:
        for off in GC.OFFSETS:
            for which in range(3):  # the misaligned pointer: out, in, residual
                ptrs = [v(0x10000 + (4 * off if which == k else 0)) for k in range(3)]
                assert lib.fhip_gate_route(0, 2, 3, h, w, *ptrs, name, 96) == 0
                want = f"fhip::gate_apply_kernel<{'true' if (h * w) % 4 == 0 and off == 0 else 'false'}>"
                assert name.value.decode() == want, (h, w, off, which)
                seen.add(want)
    for h, w in GC.SQUEEZE_PLANES:
        for off in (0, 1):
            assert lib.fhip_gate_route(1, 2, 3, h, w, None, v(0x10000 + 4 * off), None, name, 96) == 0
            assert name.value.decode() == GC.squeeze_route(h, w, off == 0), (h, w, off)
            seen.add(name.value.decode())
        sb = ctypes.c_size_t(1)
        assert lib.fhip_squeeze_get_buffer_size(2, 3, h, w, ctypes.byref(sb)) == 0
        assert sb.value == (2 * 3 * -(-h * w // GC.SPLIT_CHUNK) * 4 if h * w > GC.SPLIT_CHUNK else 0), (h, w)
    assert lib.fhip_gate_route(2, 2, 3, 1, 1, None, None, None, name, 96) == 0 and name.value.decode() == "fhip::excite_kernel"
    seen.add(name.value.decode())
    for count, off in ((8, 0), (8, 1), (7, 0)):
        assert lib.fhip_gate_route(3, 1, 1, count, 1, v(0x10000 + 4 * off), v(0x20000), None, name, 96) == 0
        seen.add(name.value.decode())
    assert seen | {"fhip::squeeze_merge_kernel"} == GC.targets()  # the tables' shapes reach every instantiation
    assert lib.fhip_gate_route(4, 2, 3, 7, 7, None, None, None, name, 96) == BADARG and "unknown" in lib.fhip_gate_last_error().decode()


def test_refusals_come_before_any_device_call(lib):
    err = lambda: lib.fhip_gate_last_error().decode()
    v = lambda p: ctypes.c_void_p(p) if p else None
    nan, inf = float("nan"), float("inf")

    def apply(n=2, c=3, h=8, w=8, out=0x1000, x=0x2000, gate=0x3000, res=0x4000, act=0):
        return lib.fhip_channel_gate_forward(n, c, h, w, v(out), v(x), v(gate), v(res), act, None)
    for kw, word in (({"n": 0}, "dimension"), ({"c": 0}, "dimension"), ({"h": -1}, "dimension"), ({"w": 0}, "dimension"),
                     ({"n": 1 << 15, "c": 1 << 10, "h": 8, "w": 8}, "2^31"), ({"out": None}, "null"), ({"x": None}, "null"), ({"gate": None}, "null"),
                     ({"out": 0x1002}, "aligned"), ({"x": 0x2001}, "aligned"), ({"gate": 0x3002}, "aligned"), ({"res": 0x4003}, "aligned"),
                     ({"act": 2}, "unknown"), ({"act": -1}, "unknown")):
        assert apply(**kw) == BADARG and word in err(), (kw, err())

    def squeeze(n=2, c=3, h=8, w=8, mean=0x1000, x=0x2000, scratch=None):
        return lib.fhip_squeeze_forward(n, c, h, w, v(mean), v(x), v(scratch), None)
    for kw, word in (({"n": 0}, "dimension"), ({"h": 0}, "dimension"), ({"n": 1 << 15, "c": 1 << 10, "h": 8, "w": 8}, "2^31"), ({"mean": None}, "null"),
                     ({"x": None}, "null"), ({"x": 0x2002}, "aligned"), ({"mean": 0x1001}, "aligned"), ({"h": 132, "w": 132}, "scratch"),
                     ({"h": 132, "w": 132, "scratch": 0x5002}, "aligned")):
        assert squeeze(**kw) == BADARG and word in err(), (kw, err())
    sb = ctypes.c_size_t()
    assert lib.fhip_squeeze_get_buffer_size(2, 3, 8, 8, None) == BADARG and "null" in err()
    assert lib.fhip_squeeze_get_buffer_size(0, 3, 8, 8, ctypes.byref(sb)) == BADARG and "dimension" in err()

    def excite(n=2, c=8, r=2, gate=0x1000, mean=0x2000, w1=0x3000, b1=0x4000, w2=0x5000, b2=0x6000, mact=1, gact=0, alpha=0.2, beta=0.5, slices=None):
        args = (n, c, r, v(gate), v(mean), v(w1), v(b1), v(w2), v(b2), mact, gact, alpha, beta, None)
        return lib.fhip_excite_forward(*args) if slices is None else lib.fhip_excite_forward_slices(slices, *args)
    for kw, word in (({"n": 0}, "dimension"), ({"c": 0}, "dimension"), ({"r": 0}, "dimension"), ({"c": 1 << 16, "r": 1 << 15}, "2^31"),
                     ({"gate": None}, "null"), ({"mean": None}, "null"), ({"w1": None}, "null"), ({"w2": None}, "null"), ({"w1": 0x3002}, "aligned"),
                     ({"b2": 0x6001}, "aligned"), ({"mact": 3}, "unknown"), ({"gact": 2}, "unknown"), ({"gact": 1, "alpha": nan}, "finite"),
                     ({"gact": 1, "beta": inf}, "finite"), ({"slices": 0}, "slices"), ({"slices": 1025}, "slices")):
        assert excite(**kw) == BADARG and word in err(), (kw, err())

    def act(kind=0, out=0x1000, x=0x2000, n=2, c=3, hw=8, alpha=0.2, beta=0.5):
        return lib.fhip_gate_activation_forward(kind, v(out), v(x), n, c, hw, alpha, beta, None)
    for kw, word in (({"kind": 2}, "unknown"), ({"kind": -1}, "unknown"), ({"out": None}, "null"), ({"x": None}, "null"), ({"x": 0x2002}, "aligned"),
                     ({"n": 0}, "dimension"), ({"hw": 0}, "dimension"), ({"n": 1 << 15, "c": 1 << 10, "hw": 64}, "2^31"), ({"kind": 1, "alpha": inf}, "finite"),
                     ({"kind": 1, "beta": nan}, "finite")):
        assert act(**kw) == BADARG and word in err(), (kw, err())


# ---- feather::Net --------------------------------------------------------------------------------------------------------------------
def _two(line, blobs=6):
    """An input [8][8][8], its global average and one more layer."""
    return f"7767517\n3 {blobs}\nInput data 0 1 data 0=8 1=8 2=8\nPooling gap 1 1 data gap 0=1 4=1\n{line}\n".encode()


def test_load_param_accepts_the_new_layers():
    """On the parent commit BinaryOp, Swish and HardSigmoid fail with code -200 (layer not registered) and Scale 0=-233 with -100."""
    from feathercnn_amd.net import Net
    for line, want in (("BinaryOp m 2 1 data gap m 0=2", ("BinaryOp", "m", "GATE")), ("BinaryOp m 2 1 gap data m 0=2", ("BinaryOp", "m", "GATE")),
                       ("BinaryOp m 2 1 data gap m 0=2 1=0", ("BinaryOp", "m", "GATE")), ("Scale m 2 1 data gap m 0=-233", ("Scale", "m", "GATE")),
                       ("Scale m 2 1 data gap m 0=-233 1=0", ("Scale", "m", "GATE")), ("Swish m 1 1 data m", ("Swish", "m", "GATE")),
                       ("HardSigmoid m 1 1 data m", ("HardSigmoid", "m", "GATE")), ("HardSigmoid m 1 1 data m 0=0.166667 1=0.5", ("HardSigmoid", "m", "GATE"))):
        net = Net()
        net.LoadParam(_two(line))
        assert net.layers()[2] == want, line
        net.LoadWeights(b"")  # none of them has weights
    net = Net()
    net.LoadParam(_two("Scale m 1 1 data m 0=8 1=1"))  # the one-bottom Scale is what it was
    assert net.layers()[2] == ("Scale", "m", None)


@pytest.mark.parametrize("line,code,word", [("BinaryOp m 2 1 data gap m 0=0", -100, "mul"), ("BinaryOp m 2 1 data gap m", -100, "mul"),
                                            ("BinaryOp m 2 1 data gap m 0=3", -100, "mul"), ("BinaryOp m 2 1 data gap m 0=2 1=1 2=0.5", -100, "scalar"),
                                            ("BinaryOp m 1 1 data m 0=2", -100, "two bottoms"), ("BinaryOp m 3 1 data gap gap m 0=2", -100, "two bottoms"),
                                            ("Scale m 2 1 data gap m 0=-233 1=1", -100, "bias"), ("Scale m 1 1 data m 0=-233", -100, "negative scale data size"),
                                            ("Scale m 1 1 data m 0=-5", -100, "negative scale data size"), ("HardSwish m 1 1 data m", -200, "HardSwish"),
                                            ("Interp m 1 1 data m 0=2", -200, "Interp"), ("PixelShuffle m 1 1 data m 0=2", -200, "PixelShuffle")])
def test_load_param_refuses_what_the_definition_leaves_out(line, code, word):
    from feathercnn_amd import FeatherHipError
    from feathercnn_amd.net import Net
    net = Net()
    with pytest.raises(FeatherHipError) as e:
        net.LoadParam(_two(line))
    assert f"code {code}" in str(e.value) and word in str(e.value), str(e.value)


def _fused_layers(param, weights, level):
    """The layer list after the fusion pass.  The pass is the first thing Forward does; without a device (or, with one, without an input)
    Forward then stops at the input that has not been fed, and the list it leaves is the fused one."""
    from feathercnn_amd import FeatherHipError
    from feathercnn_amd.net import Net
    net = Net(fusion=level)
    net.LoadParam(param)
    net.LoadWeights(weights)
    with pytest.raises(FeatherHipError, match="has not been fed"):
        net.Forward()
    return net.layers()


@pytest.mark.parametrize("name", NEW_MODELS)
def test_net_loads_the_se_nets(name):
    from feathercnn_amd import model_zoo
    from feathercnn_amd.net import Net
    p, b, i, o = model_zoo.MODELS[name]()
    layers = R.inorm_ref.gconv_ref.parse_param(p)
    assert R.Net(p, b).read == len(b)  # the restatement reads every weight byte ...
    gated = [nm for t, nm, bottoms, *_ in layers if t in ("BinaryOp", "Swish", "HardSigmoid") or (t == "Scale" and len(bottoms) == 2)]
    assert gated and any(t == "Pooling" for t, *_ in layers)
    assert model_zoo.MODELS[name](dry=True) == (p, len(b), i, o)  # the dry builder writes the same .param and counts the same bytes
    for level in (0, 1, 2, 3):
        net = Net(fusion=level)
        net.LoadParam(p)
        net.LoadWeights(b)  # ... and so does the runtime (a short read is an error)
        got = net.layers()
        assert [(t, nm) for t, nm, _ in got] == [(t, nm) for t, nm, *_ in layers]
        assert [nm for _, nm, a in got if a == "GATE"] == gated


def test_existing_builders_write_what_they_wrote():
    """GraphBuilder gained methods only: the .param text of nets that use none of them keeps its digest."""
    import hashlib
    from feathercnn_amd import model_zoo
    want = {"tiny_allsorts": "b910eddbebf3", "resnet50": "9346900569a1", "tiny_shuffle": "c8606d220268", "tiny_dilated": "a04e50b121f6", "tiny_generative": "89d183a43348"}
    got = {k: hashlib.sha256(model_zoo.MODELS[k](dry=True)[0]).hexdigest()[:12] for k in want}
    assert got == want, got


def test_fusion_2_collapses_the_blocks_of_tiny_se():
    from feathercnn_amd import model_zoo
    p, b, _, _ = model_zoo.tiny_se()
    every = [nm for _, nm, *_ in R.inorm_ref.gconv_ref.parse_param(p)]
    collapse, keep = model_zoo.SE_BLOCKS["tiny_se"]
    parts = {"a_gap": ("a_fc1", "a_relu", "a_fc2", "a_sigmoid", "a_scale", "res", "res_relu"), "b_gap": ("b_conv1", "b_swish", "b_conv2", "b_sigmoid", "b_mul"),
             "c_gap": ("c_conv1", "c_conv2", "c_hsigmoid", "c_mul")}
    for level in (0, 1):
        got = _fused_layers(p, b, level)
        routes = {nm: (t, a) for t, nm, a in got}
        for head in collapse + keep:
            assert routes[head] == ("Pooling", None), (level, head)
        assert routes["a_scale"] == ("Scale", "GATE") and routes["b_mul"] == ("BinaryOp", "GATE") and routes["c_mul"] == ("BinaryOp", "GATE")
        assert routes["d_scale"] == ("Scale", "GATE") and routes["conv3_swish"] == ("Swish", "GATE") and routes["c_hsigmoid"] == ("HardSigmoid", "GATE")
        assert ("a_relu" in routes) == (level == 0) and ("res_relu" in routes) == (level == 0)  # level 1: the pairwise pass took them
    for level in (2, 3):
        got = _fused_layers(p, b, level)
        names = [nm for _, nm, _ in got]
        routes = {nm: (t, a) for t, nm, a in got}
        for head in collapse:  # each block is one layer under its Pooling layer's type and name ...
            assert routes[head] == ("Pooling", "GATE"), (level, head, routes[head])
            assert not set(parts[head]) & set(names), (level, head)
        # ... that stands where the block's last layer stood: behind everything it reads
        assert names.index("a_gap") > names.index("a_split") and names.index("a_gap") < names.index("conv3")
        # the block whose gate has a second consumer stays layer by layer (its excite convolutions absorb their ReLU as anywhere else)
        assert routes["d_gap"] == ("Pooling", None) and routes["d_scale"] == ("Scale", "GATE") and routes["d_sigmoid"] == ("Sigmoid", None)
        assert {"d_conv1", "d_conv2", "d_gate_split", "aux"} <= set(names) and "d_relu" not in names
        assert routes["conv3_swish"] == ("Swish", "GATE")  # a Swish outside a block is a launch of its own
        assert names == [nm for nm in every if nm in names]  # nothing these blocks read is produced inside them: the file's order is kept
        assert sum(a == "GATE" for _, _, a in got) == 5


@pytest.mark.parametrize("change,why", [("Pooling a_gap 1 1 a_split_1 a_gap 0=0 1=1 2=1 3=0 4=1", "a max pooling"),
                                        ("Pooling a_gap 1 1 a_split_1 a_gap 0=1 1=1 2=1 3=0 4=0", "a pooling that is not global")])
def test_blocks_that_do_not_match_stay_layer_by_layer(change, why):
    from feathercnn_amd import model_zoo
    p, b, _, _ = model_zoo.tiny_se()
    old = "Pooling a_gap 1 1 a_split_1 a_gap 0=1 1=1 2=1 3=0 4=1"
    assert old.encode() in p
    got = _fused_layers(p.replace(old.encode(), change.encode()), b, 2)
    routes = {nm: (t, a) for t, nm, a in got}
    assert routes["a_gap"] == ("Pooling", None) and routes["a_scale"] == ("Scale", "GATE"), why
    assert routes["b_gap"] == ("Pooling", "GATE")


def test_a_grouped_or_strided_excite_convolution_is_no_block():
    from feathercnn_amd import model_zoo
    for kw, why in (({"group": 2}, "grouped"), ({"s": 2}, "strided"), ({"p": 1, "k": 3}, "padded 3x3")):
        g = model_zoo.GraphBuilder(5)
        x = g.relu("relu", g.conv("conv", g.input("data", 3, 8, 8), 3, 8, 3, 1, 1))
        keep, sq = g.split("split", x)
        m = g.pool("gap", sq, 1, 1, avg=True, global_=True)
        m = g.relu("r1", g.conv("e1", m, 8, 4, kw.get("k", 1), kw.get("s", 1), kw.get("p", 0), group=kw.get("group", 1), type_="Convolution"))
        m = g.sigmoid("sig", g.conv("e2", m, 4, 8, 1, type_="Convolution"))
        g.binary_mul("mul", keep, m)
        p, w = g.finish()
        routes = {nm: (t, a) for t, nm, a in _fused_layers(p, w, 2)}
        assert routes["gap"] == ("Pooling", None) and routes["mul"] == ("BinaryOp", "GATE"), why
    g = model_zoo.GraphBuilder(5)  # the same block as written: it collapses
    x = g.relu("relu", g.conv("conv", g.input("data", 3, 8, 8), 3, 8, 3, 1, 1))
    g.se_block("se", x, 8, 4, "converter")
    p, w = g.finish()
    got = _fused_layers(p, w, 2)
    assert [(t, nm) for t, nm, _ in got] == [("Input", "data"), ("Convolution", "conv"), ("Split", "se_split"), ("Pooling", "se_gap")]
    assert got[3][2] == "GATE"
