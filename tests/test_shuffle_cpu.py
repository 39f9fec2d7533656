"""libfeather_shuffle.so (ShuffleChannel, Slice and the channel map) without a GPU.

Checks of the yardstick, which need no library and pass on any tree: tests/shuffle_ref.py equals torch's channel_shuffle / split on the CPU,
`reverse` is the exact inverse, a composed table equals the three steps applied one by one, the restatement runs tiny_shuffle end to end.

Checks of the feature: fhip_channel_map_route names the instantiation of the case table for every kind, plane and offset; bad arguments are refused on the host with the documented codes; feather::Net loads
ShuffleChannel and Slice (the factory answered -200 before), reports route 103 from LoadParam on, refuses what the definition leaves out,
and at fusion level 2 reports the Concat / ShuffleChannel / Slice runs of tiny_shuffle and of a ShuffleNet v2 unit as one layer each.
Shapes: the runtime resolves a Slice through fhip_channel_slice_resolve, which is checked here against the restatement; the blob shapes
after Reshape need device memory and are checked in tests/test_shuffle_gpu.py.  What the library shares with the other run-time libraries -- its exports, the instantiations it holds, its route code, the build
of its application, its last-error state -- is in tests/test_side_contract_cpu.py."""
import ctypes

import numpy as np
import pytest

import shuffle_cases as SC
import shuffle_ref as R
import side_contract

BADARG = -2
NEW_MODELS = ["tiny_shuffle", "shufflenet_v2_x1_0", "shufflenet_v1_g3"]


lib = side_contract.fixture("shuffle")


# ---- the definition ------------------------------------------------------------------------------------------------------------------
def _torch_shuffle(t, group):
    import torch
    if hasattr(torch.nn.functional, "channel_shuffle"):
        return torch.nn.functional.channel_shuffle(t, group)
    n, c, h, w = t.shape
    return t.reshape(n, group, c // group, h, w).transpose(1, 2).reshape(n, c, h, w)


def test_restatement_against_torch():
    import torch
    rng = np.random.default_rng(1)
    for c, group in SC.SHUFFLES:
        x = rng.normal(0, 1, (2, c, 3, 5)).astype(np.float32)
        y = R.channel_shuffle(x, group)
        assert np.array_equal(y, _torch_shuffle(torch.from_numpy(x), group).numpy()), (c, group)
        # the header's formula, literally
        per = c // group
        for i in range(per):
            for k in range(group):
                assert np.array_equal(y[:, i * group + k], x[:, k * per + i])
        assert np.array_equal(R.channel_shuffle(y, group, reverse=True), x)  # reverse is the exact inverse ...
        assert np.array_equal(R.channel_shuffle(R.channel_shuffle(x, group, reverse=True), group), x)  # ... on either side
        assert np.array_equal(R.channel_shuffle(x, group, reverse=True), R.channel_shuffle(x, c // group))  # and the shuffle by C / group
    for c, sizes in SC.SLICES:
        x = rng.normal(0, 1, (2, c, 3, 5)).astype(np.float32)
        resolved = R.slice_sizes(c, sizes)
        parts = R.channel_slice(x, sizes)
        want = torch.split(torch.from_numpy(x)[:, :sum(resolved)], resolved, dim=1)
        assert len(parts) == len(want) and all(np.array_equal(p, w.numpy()) for p, w in zip(parts, want)), (c, sizes)
    assert R.slice_sizes(32, [5, -233, 14]) == [5, 13, 14] and R.slice_sizes(21, [4, -233, -233]) == [4, 8, 9]
    assert R.slice_sizes(116, [-233, -233]) == [58, 58] and R.slice_sizes(9, [-233, -233]) == [4, 5]
    for c, sizes in ((8, [5, 4]), (8, [8, -233]), (8, [0, 8]), (8, [])):
        with pytest.raises(ValueError):
            R.slice_sizes(c, sizes)
    with pytest.raises(ValueError):
        R.shuffle_order(10, 3)


def test_composed_table_equals_the_steps_one_by_one():
    rng = np.random.default_rng(2)
    for src_c, steps, outputs in (SC.THREE_SOURCES, SC.V2_BOUNDARY(58), SC.V2_BOUNDARY(3)):
        srcs = [rng.normal(0, 1, (3, c, 7, 7)).astype(np.float32) for c in src_c]
        blobs = {f"s{i}": s for i, s in enumerate(srcs)}
        for st in steps:
            if st[0] == "concat":
                blobs[st[2]] = np.concatenate([blobs[b] for b in st[1]], axis=1)
            elif st[0] == "shuffle":
                blobs[st[2]] = R.channel_shuffle(blobs[st[1]], st[3], st[4])
            else:
                blobs.update(zip(st[2], R.channel_slice(blobs[st[1]], st[3])))
        tables = R.compose(src_c, steps, outputs)
        got = R.apply_map(srcs, tables)
        assert all(np.array_equal(g, blobs[o]) for g, o in zip(got, outputs))
        assert {s for t in tables for s, _ in t} == set(range(len(src_c)))  # every source is read
    # ShuffleNet v2's boundary in closed form: the kept half is the even channels of the concatenation, the worked half the odd ones
    keep, work = R.compose(*SC.V2_BOUNDARY(4))
    assert keep == [(0, 0), (1, 0), (0, 1), (1, 1)] and work == [(0, 2), (1, 2), (0, 3), (1, 3)]


# ---- the library ---------------------------------------------------------------------------------------------------------------------
def test_instantiations_and_route_names(lib):
    name = ctypes.create_string_buffer(96)
    for kind in (0, 1, 2):
        for h, w in SC.PLANES:
            for off in SC.OFFSETS:
                ptrs = (ctypes.c_void_p * 3)(0x10000, 0x20000 + 4 * off, 0x30000)
                assert lib.fhip_channel_map_route(kind, h, w, ptrs, 3, name, 96) == 0
                assert name.value.decode() == SC.instance(kind, h, w, [off]), (kind, h, w, off)
    seen = {SC.instance(k, h, w, [o]) for k in (0, 1, 2) for h, w in SC.PLANES for o in SC.OFFSETS}
    assert seen == SC.targets()  # the GPU sweep's shapes reach every instantiation
    assert lib.fhip_channel_map_route(3, 7, 7, None, 0, name, 96) == BADARG


def test_slice_resolve_matches_the_restatement(lib):
    for c, sizes in SC.SLICES + [(464, [-233, -233]), (7, [-233, -233, -233])]:
        out = (ctypes.c_int * len(sizes))()
        assert lib.fhip_channel_slice_resolve(c, (ctypes.c_int * len(sizes))(*sizes), len(sizes), out) == 0
        assert list(out) == R.slice_sizes(c, sizes), (c, sizes)


def test_refusals_come_before_any_device_call(lib):
    err = lambda: lib.fhip_shuffle_last_error().decode()
    v = ctypes.c_void_p
    ints = lambda a: (ctypes.c_int * max(len(a), 1))(*a)

    def shuffle(c=12, group=3, n=2, h=7, w=7, out=0x1000, x=0x2000):
        return lib.fhip_channel_shuffle_forward(v(out) if out else None, v(x) if x else None, n, c, h, w, group, 0, None)
    for kw, word in (({"c": 10}, "divide"), ({"group": 0}, "group"), ({"group": -2}, "group"), ({"n": 0}, "dimension"), ({"h": 0}, "dimension"),
                     ({"n": 1 << 15, "c": 1 << 10, "group": 2, "h": 8, "w": 8}, "2^31"), ({"out": None}, "null"), ({"x": 0x2002}, "aligned")):
        assert shuffle(**kw) == BADARG and word in err(), (kw, err())

    def slice_(c=8, sizes=(4, 4), outs=(0x1000, 0x3000), x=0x2000):
        return lib.fhip_channel_slice_forward((v * max(len(outs), 1))(*outs), v(x) if x else None, 2, c, 7, 7, ints(sizes), len(sizes), None)
    for kw, word in (({"sizes": (5, 4)}, "more than"), ({"sizes": (8, -233)}, "without a channel"), ({"sizes": (0, 8)}, "positive"),
                     ({"sizes": ()}, "at least one"), ({"sizes": (1,) * 5, "outs": (0x1000,) * 5}, "too many"), ({"x": None}, "null"),
                     ({"outs": (0x1000, 0x3002)}, "aligned")):
        assert slice_(**kw) == BADARG and word in err(), (kw, err())
    out = ints([0, 0])
    assert lib.fhip_channel_slice_resolve(8, ints([5, 4]), 2, out) == BADARG and lib.fhip_channel_slice_resolve(8, None, 2, out) == BADARG

    m = ctypes.c_void_p()

    def create(src=(4, 4), outs=(8,), entries=tuple((i // 4, i % 4) for i in range(8))):
        flat = [x for e in entries for x in e]
        return lib.fhip_channel_map_create(ctypes.byref(m), ints(src), len(src), ints(outs), len(outs), ints(flat))
    for kw, word in (({"entries": ((0, 0),) * 7 + ((0, 4),)}, "names no channel"), ({"entries": ((2, 0),) * 8}, "names no channel"),
                     ({"entries": ((0, -1),) * 8}, "names no channel"), ({"src": (4, 0)}, "at least one channel"), ({"src": (1,) * 5}, "sources"),
                     ({"outs": (0,)}, "at least one channel")):
        assert create(**kw) == BADARG and word in err() and not m.value, (kw, err())
    assert lib.fhip_channel_map_forward(None, None, None, 1, 1, 1, None) == BADARG
    assert lib.fhip_channel_map_supported(1, 1, 1, 1) == 0 and lib.fhip_channel_map_supported(1, 0, 1, 1) == BADARG


# ---- feather::Net --------------------------------------------------------------------------------------------------------------------
def _one(line, c=8, blobs=2):
    return f"7767517\n2 {blobs}\nInput data 0 1 data 0=8 1=8 2={c}\n{line}\n".encode()


def test_load_param_accepts_the_new_layers():
    """On the parent commit both lines fail with code -200 (layer not registered)."""
    from feathercnn_amd.net import Net
    for line, want in (("ShuffleChannel s 1 1 data s 0=2", ("ShuffleChannel", "s", "SHUFFLE")), ("ShuffleChannel s 1 1 data s", ("ShuffleChannel", "s", "SHUFFLE")),
                       ("ShuffleChannel s 1 1 data s 0=4 1=1", ("ShuffleChannel", "s", "SHUFFLE")),
                       ("Slice s 1 2 data a b -23300=2,4,4", ("Slice", "s", "SHUFFLE")), ("Slice s 1 2 data a b -23300=2,-233,-233 1=0", ("Slice", "s", "SHUFFLE")),
                       ("Slice s 1 3 data a b c -23300=3,2,-233,3", ("Slice", "s", "SHUFFLE"))):
        net = Net()
        net.LoadParam(_one(line, blobs=4))
        assert net.layers()[1] == want, line
        net.LoadWeights(b"")  # neither layer has weights


@pytest.mark.parametrize("line,code", [("ShuffleChannel s 1 1 data s 0=0", -100), ("ShuffleChannel s 1 1 data s 0=-2", -100),
                                       ("Slice s 1 2 data a b -23300=2,4,4 1=1", -100), ("Slice s 1 2 data a b -23300=2,4,4 1=2", -100),
                                       ("Slice s 1 2 data a b -23300=3,2,2,4", -300), ("Slice s 1 3 data a b c -23300=2,4,4", -300),
                                       ("Slice s 1 2 data a b", -100), ("Slice s 1 2 data a b -23300=2,0,8", -100),
                                       ("Slice s 1 5 data a b c d e -23300=5,1,1,1,1,1", -100),
                                       ("Reshape s 1 1 data s 0=-1", -200), ("Permute s 1 1 data s 0=1", -200), ("PixelShuffle s 1 1 data s 0=2", -200)])
def test_load_param_refuses_what_the_definition_leaves_out(line, code):
    from feathercnn_amd import FeatherHipError
    from feathercnn_amd.net import Net
    net = Net()
    with pytest.raises(FeatherHipError) as e:
        net.LoadParam(_one(line, blobs=6))
    assert f"code {code}" in str(e.value), str(e.value)


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
def test_net_loads_the_shuffle_nets(name):
    from feathercnn_amd import model_zoo
    from feathercnn_amd.net import Net
    p, b, _, _ = model_zoo.MODELS[name]()
    layers = R.parse_param(p)
    assert R.Net(p, b).read == len(b)  # the restatement reads every weight byte ...
    moved = [nm for t, nm, *_ in layers if t in R.MAP_TYPES]
    assert moved and any(t == "ShuffleChannel" for t, *_ in layers)
    assert model_zoo.MODELS[name](dry=True) == (p, len(b), "data", "prob")  # the dry builder writes the same .param and counts the same bytes
    for level in (0, 1, 2, 3):
        net = Net(fusion=level)
        net.LoadParam(p)
        net.LoadWeights(b)  # ... and so does the runtime (a short read is an error)
        got = net.layers()
        assert [(t, nm) for t, nm, _ in got] == [(t, nm) for t, nm, *_ in layers]
        assert [nm for _, nm, a in got if a == "SHUFFLE"] == moved


def test_fusion_2_collapses_the_runs_of_tiny_shuffle():
    from feathercnn_amd import model_zoo
    p, b, _, _ = model_zoo.tiny_shuffle()
    every = [nm for _, nm, *_ in R.parse_param(p)]
    for level in (0, 1):
        got = _fused_layers(p, b, level)
        assert {nm for _, nm, _ in got} >= {"u1_concat", "u1_shuffle", "u2_slice", "u2_concat", "u2_shuffle", "three", "cat3", "unshuffle", "u3_slice",
                                            "u3_concat", "u3_shuffle", "v1a_shuffle", "v1b_shuffle", "v1b_concat"}
        routes = {nm: a for _, nm, a in got}
        assert routes["u1_concat"] is None and routes["v1b_concat"] is None  # a Concat of its own keeps its copies
        assert all(routes[nm] == "SHUFFLE" for nm in ("u1_shuffle", "u2_slice", "three", "unshuffle", "v1a_shuffle", "u3_slice"))
    for level in (2, 3):
        got = _fused_layers(p, b, level)
        names = [nm for _, nm, _ in got]
        routes = {nm: (t, a) for t, nm, a in got}
        # each run is one layer under its first layer's type and name ...
        for head, gone in (("u1_concat", ("u1_shuffle", "u2_slice")), ("u2_concat", ("u2_shuffle", "three")), ("cat3", ("unshuffle",)),
                           ("u3_concat", ("u3_shuffle",))):
            assert routes[head] == ("Concat", "SHUFFLE"), (level, head, routes[head])
            assert not set(gone) & set(names), (level, head)
        # ... a ShuffleChannel behind a grouped convolution and a Slice behind a ReLU stay launches of their own, a Concat that no shuffle
        # or slice follows keeps its copies, and the order of what is left is the file's
        assert routes["v1a_shuffle"] == ("ShuffleChannel", "SHUFFLE") and routes["v1b_shuffle"] == ("ShuffleChannel", "SHUFFLE")
        assert routes["u3_slice"] == ("Slice", "SHUFFLE") and routes["v1b_concat"] == ("Concat", None)
        assert names == [nm for nm in every if nm in names]
        assert sum(a == "SHUFFLE" for _, _, a in got) == 7


def test_fusion_2_collapses_a_v2_unit():
    """Concat(a, b) -> ShuffleChannel(2) -> Slice(2), the boundary between two ShuffleNet v2 units, alone in a net."""
    from feathercnn_amd import model_zoo
    g = model_zoo.GraphBuilder(3)
    x = g.input("data", 3, 8, 8)
    a, b = g.split("split", g.relu("relu", g.conv("conv", x, 3, 8, 1)))
    a = g.relu("relu_a", g.conv("conv_a", a, 8, 8, 1))
    keep, work = g.slice("slice", g.shuffle("shuffle", g.concat("concat", [a, b]), 2), [-233, -233])
    g.eltwise("sum", keep, work)
    p, w = g.finish()
    assert [(t, nm, a) for t, nm, a in _fused_layers(p, w, 0) if nm in ("concat", "shuffle", "slice")] == \
        [("Concat", "concat", None), ("ShuffleChannel", "shuffle", "SHUFFLE"), ("Slice", "slice", "SHUFFLE")]
    got = _fused_layers(p, w, 2)
    assert [(t, nm, a) for t, nm, a in got if nm in ("concat", "shuffle", "slice")] == [("Concat", "concat", "SHUFFLE")]
    assert [nm for _, nm, _ in got] == ["data", "conv", "split", "conv_a", "concat", "sum"]
    # a blob with two consumers ends the run: the Slice stays a layer of its own
    g = model_zoo.GraphBuilder(3)
    x = g.input("data", 8, 8, 8)
    s = g.shuffle("shuffle", g.concat("concat", [x, x]), 2)
    keep, work = g.slice("slice", s, [-233, -233])
    g.eltwise("sum", g.relu("relu", s), g.concat("again", [keep, work]))
    p, w = g.finish()
    assert [(t, nm, a) for t, nm, a in _fused_layers(p, w, 2)] == [("Input", "data", None), ("Concat", "concat", "SHUFFLE"), ("Slice", "slice", "SHUFFLE"),
                                                                   ("ReLU", "relu", None), ("Concat", "again", None), ("Eltwise", "sum", None)]


def test_every_zoo_builder_runs_dry():
    from feathercnn_amd import model_zoo
    for name, build in model_zoo.MODELS.items():
        p, nbytes, i, o = build(dry=True)
        assert isinstance(nbytes, int) and nbytes > 0 and p.startswith(b"7767517\n"), name
    p, nbytes, _, _ = model_zoo.shufflenet_v2_x1_0(dry=True)
    layers = R.parse_param(p)
    assert sum(t == "Slice" for t, *_ in layers) == 13 and sum(t == "ShuffleChannel" for t, *_ in layers) == 16
    assert 2.0e6 < nbytes / 4 < 2.6e6  # ShuffleNet v2 1.0x has 2.3 M parameters
    p, nbytes, _, _ = model_zoo.shufflenet_v1_g3(dry=True)
    assert sum(t == "ShuffleChannel" for t, *_ in R.parse_param(p)) == 16


def test_restatement_runs_tiny_shuffle():
    from feathercnn_amd import model_zoo
    p, b, i, o = model_zoo.tiny_shuffle()
    x = np.random.default_rng(3).uniform(-1, 1, (2, 3, 28, 28)).astype(np.float32)
    blobs = R.Net(p, b).run(i, x, o, keep=True)
    shapes = {k: v.shape for k, v in blobs.items()}
    assert shapes["u1_shuffle"] == (2, 32, 14, 14) and shapes["u2_slice_0"] == shapes["u2_slice_1"] == (2, 16, 14, 14)
    assert [shapes[f"three_{j}"][1] for j in range(3)] == [5, 13, 14]  # a three-way slice with one -233 share
    assert shapes["v1b_pool"] == shapes["v1b_g2_scale"][:1] + (24,) + shapes["v1b_g2_scale"][2:] == (2, 24, 7, 7)  # shortcut and branch agree
    assert shapes["u3_slice_0"] == (2, 30, 7, 7) and blobs["prob"].reshape(2, -1).shape == (2, 10)
    assert np.allclose(blobs["prob"].reshape(2, -1).sum(axis=1), 1.0, atol=1e-5)
    # the layers under test, bit for bit from their inputs
    cat = np.concatenate([blobs["u1_b1_pw_relu"], blobs["u1_b2_pw2_relu"]], axis=1)
    assert np.array_equal(blobs["u1_shuffle"], R.channel_shuffle(cat, 2))
    assert np.array_equal(blobs["u2_slice_1"], blobs["u1_shuffle"][:, 16:])
    assert np.array_equal(R.channel_shuffle(blobs["unshuffle"], 4), blobs["cat3"])
