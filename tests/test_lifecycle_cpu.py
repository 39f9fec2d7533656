"""The life-cycle table (tests/lifecycle_cases.py) without a GPU: the models parse, the float64 reference is finite and not constant on every
fed input, the walks are well-formed and together hold every step kind and every size class, the ids are unique.  Also where the cost of
the reference is measured (printed per input; the GPU tests share one evaluation per input)."""
import time

import numpy as np

import lifecycle_cases as LC
import seam_ref as R


def _fed(walk):
    return [(s[1], s[2] if len(s) > 2 else 0) for s in walk if s[0] == "feed"]


def test_models_parse_and_hold_every_plan_kind():
    param, weights, name, outputs = LC.model()
    net = R.Net(param, weights)
    types = [t for t, *_ in net.layers]
    for t in ("Input", "Convolution", "ConvolutionDepthWise", "ReLU", "Pooling", "Split", "Eltwise", "InnerProduct", "Sigmoid", "Scale", "InstanceNorm",
              "Dropout", "Softmax"):
        assert t in types, t
    by_name = {n: (t, b, tops, pd) for t, n, b, tops, pd in net.layers}
    assert by_name["conv0"][3][1] == 3 and by_name["conv0"][3][4] == 1 and by_name["conv0"][3][6] == 16 * 3 * 9  # the RGB 3x3 pad-1 first layer
    for n in LC.CONV3X3:
        assert by_name[n][3][1] == 3 and by_name[n][3].get(3, 1) == 1 and by_name[n][3][4] == 1, n
    assert by_name["sib_a"][3][0] > 64 and by_name["sib_b"][3][0] > 64 and by_name["sib_a"][3][1] == by_name["sib_b"][3][1] == 1
    assert by_name["dw"][3][7] == 128 and by_name["pw"][3][1] == 1 and 64 < by_name["pw"][3][0] < 160  # fhip_conv_can_fuse_dw_pw's range
    assert by_name["drop"][3][0] == 1.0 and by_name["se_scale"][3][0] == -233
    # at most 128 channels anywhere (the second model is the one exception, see lifecycle_cases)
    assert max(pd[0] for t, (_, _, _, pd) in ((by_name[n][0], by_name[n]) for n in by_name) if t in ("Convolution", "ConvolutionDepthWise")) <= 128
    assert len(weights) <= 1100 * 1024
    dparam, dweights, _, _ = LC.deep_model()
    assert [t for t, *_ in R.Net(dparam, dweights).layers] == ["Input", "Convolution", "ReLU"]


def test_reference_is_finite_and_no_blob_is_constant():
    """Every fed input of every walk; prints the cost of the float64 reference per input (one evaluation each, shared by the GPU tests)."""
    total, lines, floor = 0.0, [], (1.0, None)
    fed = sorted({f for w in LC.WALKS.values() for f in _fed(w)})
    for key, variant in fed:
        t0 = time.perf_counter()
        blobs = LC.reference(key, variant)
        dt = time.perf_counter() - t0
        total += dt
        lines.append(f"{key}/{variant} {LC.shape_of(key)}: {dt * 1e3:.0f} ms")
        for name, v in blobs.items():
            assert v.dtype == np.float32 and np.isfinite(v).all(), (key, variant, name)
            assert v.shape[0] == LC.shape_of(key)[0], (key, variant, name, v.shape)
            assert float(v.max()) > float(v.min()), (key, variant, name, "constant")
            if key in LC.SHAPES:  # what the calibration of the model is for (lifecycle_cases): no plane far below its tensor
                m = np.abs(v).max(axis=(2, 3))
                floor = min(floor, (float(m.min() / m.max()), name, key, variant))
                assert m.min() >= LC.PLANE_FLOOR * m.max(), (key, variant, name, float(m.min() / m.max()))
        outputs = LC.deep_model()[3] if key in LC.DEEP_SHAPES else LC.OUTPUTS
        for o in outputs:
            assert o in blobs
        if key in LC.SHAPES:
            # one-value planes are the ones plane_nerr cannot normalise: those behind the InnerProduct layers are bias (at least 0.05) + a sum
            # that stays below it -- a float32 sum of terms below 0.1 is off by some 1e-8, a millionth of the smallest value allowed here
            for name in ("se_fc1", "se_fc2", "fc"):
                assert float(blobs[name].min()) > 0.01, (key, variant, name, float(blobs[name].min()))
            for name in ("se_gap", "gap"):
                assert float(blobs[name].min()) >= 0.0, (key, variant, name)
    print(f"float64 reference: {len(fed)} inputs in {total:.2f} s; " + "; ".join(lines))
    print(f"smallest plane maximum relative to its tensor's: {floor}")
    # the walk with the most inputs must stay well inside "a few seconds" for one GPU test id even where it evaluates all of them itself
    assert total <= 5.0, total
    # a second variant of a shape is another input, not the same numbers
    assert not np.array_equal(LC.input("p14b4", 0), LC.input("p14b4", 1))


def test_walks_are_well_formed():
    kinds, classes = set(), set()
    for wname, walk in LC.WALKS.items():
        fed, forwards, last = False, 0, None
        for step in walk:
            assert step[0] in LC.STEP_KINDS, (wname, step)
            kinds.add(step[0])
            if step[0] == "feed":
                assert step[1] in (LC.DEEP_SHAPES if wname == "deep" else LC.SHAPES), (wname, step)
                assert len(step) in (2, 3)
                if step[1] in LC.CLASS:
                    classes.add(LC.CLASS[step[1]])
                fed = True
            elif step[0] == "forward":
                assert fed and isinstance(step[1], int) and step[1] >= 1, (wname, step)
                forwards += step[1]
            elif step[0] in ("set_tuned", "set_concurrency", "set_graph"):
                assert isinstance(step[1], bool), (wname, step)
            elif step[0] == "extract":
                assert last in ("forward", "extract") and step[2] in ("ok", "chained"), (wname, step)  # a blob is read behind a Forward
                assert step[1] in LC.reference("p3b1"), (wname, step)
            last = step[0]
        assert walk[-1][0] in ("forward", "extract") and forwards >= 5, wname
    assert kinds == set(LC.STEP_KINDS)
    assert classes == set(LC.CLASSES)
    assert set(LC.CLASS) == set(LC.SHAPES)


def test_required_walks():
    # (a) shrink -> grow -> return, three passes (the second and third are compared with the first)
    one = [s[1] for s in LC.WALK_CYCLE[:LC.PASS_ENDS[0]] if s[0] == "feed"]
    size = lambda k: int(np.prod(LC.SHAPES[k]))  # noqa: E731
    assert one[0] == one[3] and size(one[1]) < size(one[0]) < size(one[2])
    assert LC.WALK_CYCLE[:LC.PASS_ENDS[0]] * 3 == LC.WALK_CYCLE and all(LC.WALK_CYCLE[e - 1][0] == "forward" for e in LC.PASS_ENDS)
    # (b) every size class, entered from both directions: each class occurs at least twice, its neighbours in the walk differ
    order = [LC.CLASS[s[1]] for s in LC.WALK_ROUTES if s[0] == "feed"]
    for c in LC.CLASSES:
        at = [i for i, x in enumerate(order) if x == c]
        assert len(at) >= 2, c
        before = {order[i - 1] for i in at if i > 0 and order[i - 1] != c}
        assert len(before) >= 2 or c == order[0], (c, before)
    batches = {LC.SHAPES[s[1]][0] for w in LC.WALKS.values() for s in w if s[0] == "feed" and s[1] in LC.SHAPES}
    assert {1, 4, 5, 8} <= batches
    # (c) each of the four setters toggled between two Forwards at a fixed shape, and once with a feed in the same gap
    alone, with_feed = set(), set()
    gaps, gap = [], []
    for s in LC.WALK_SETTERS:
        if s[0] == "forward":
            gaps.append(gap)
            gap = []
        else:
            gap.append(s)
    for gap in gaps[1:]:
        setters = {s[0] for s in gap if s[0] in ("set_tuned", "set_concurrency", "set_graph", "stream")}
        (with_feed if any(s[0] == "feed" for s in gap) else alone).update(setters)
    assert alone == with_feed == {"set_tuned", "set_concurrency", "set_graph", "stream"}
    # (d) capture, two replays, new values at the same shape, a new shape, graph off, graph on
    g = LC.WALK_GRAPH
    assert g[:3] == [("feed", "p14b4"), ("forward", 1), ("forward", 2)] and g[3] == ("feed", "p14b4", 1)
    assert LC.SHAPES[g[5][1]] != LC.SHAPES["p14b4"] and ("set_graph", True) in g and g.index(("set_graph", False)) > g.index(("set_graph", True))
    # (e) 7 -> 2 -> 1 -> 7 images with three replicas, and a new size while two of them sit out
    r = [LC.SHAPES[s[1]] for s in LC.WALK_REPLICAS if s[0] == "feed"]
    assert [x[0] for x in r[:5]] == [7, 2, 1, 1, 7] and r[2][2:] != r[3][2:] and r[3][2:] == r[4][2:]


def test_ids_are_unique_and_settings_are_the_required_ones():
    rows = LC.table()
    ids = [LC.row_id(r) for r in rows]
    assert len(set(ids)) == len(ids), ids
    per = {}
    for w, lv, kw in rows:
        per.setdefault(w, []).append((lv, tuple(sorted(kw.items()))))
    want5 = [(lv, tuple(sorted(kw.items()))) for lv, kw in LC.LEVELS]
    assert per["cycle"] == per["routes"] == per["setters"] == want5
    assert per["graph"] == [(1, (("graph", True),)), (3, (("graph", True), ("tuned", True)))]
    assert sorted(per["replicas"]) == sorted([(2, (("sub_batches", 3),)), (2, (("graph", True), ("sub_batches", 3))),
                                              (3, (("sub_batches", 3), ("tuned", True))), (3, (("graph", True), ("sub_batches", 3), ("tuned", True)))])


def test_packed_layout_tells_apart_what_the_byte_count_does_not():
    """fhip_conv_packed_layout (host only): the 1024 -> 256 1x1 layer of the second model packs the same number of bytes on a 2x2 and on a 1x1
    plane but not the same bytes -- the key ConvLayer::Init keeps its packed weights under; a 3x3 layer changes between F(6,3) and F(4,3)."""
    import ctypes

    from feathercnn_amd import _lib
    from feathercnn_amd.booster import IM2COL, WINOGRADF63
    lib = _lib.load_library()

    def query(cin, cout, k, pad, h, w, algo):
        p = _lib.fhip_conv_param()
        p.input_channels, p.output_channels, p.input_h, p.input_w, p.kernel_h, p.kernel_w = cin, cout, h, w, k, k
        p.stride_h = p.stride_w = p.group = 1
        p.pad_left = p.pad_right = p.pad_top = p.pad_bottom = pad
        assert lib.fhip_conv_assign_output_dim(ctypes.byref(p)) == 0
        buf, packed, layout = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_int(-1)
        assert lib.fhip_conv_get_buffer_size(ctypes.byref(p), algo, 2, ctypes.byref(buf), ctypes.byref(packed)) == 0
        assert lib.fhip_conv_packed_layout(ctypes.byref(p), algo, ctypes.byref(layout)) == 0
        return packed.value, layout.value

    on = {key: query(1024, 256, 1, 0, shape[2], shape[3], IM2COL) for key, shape in LC.DEEP_SHAPES.items()}
    assert on["d2x2"][0] == on["d1x1"][0] and on["d2x2"][1] != on["d1x1"][1], on
    assert on["d3x1"][0] < on["d2x2"][0] and len({v[1] for v in on.values()}) == 3, on
    # the model's 1x1 layers never change their layout: its walks cannot show this fault, the second model's do
    assert len({query(64, 128, 1, 0, s, s, IM2COL) for s in (14, 8, 6, 3)}) == 1
    assert query(32, 32, 3, 1, 14, 14, WINOGRADF63)[1] == 64 and query(32, 32, 3, 1, 8, 8, WINOGRADF63)[1] == 36
    assert lib.fhip_conv_packed_layout(None, IM2COL, None) != 0


# ---- the model with int8 layers among fp32 ones ---------------------------------------------------------------------------------------
def test_mixed_model_and_its_walks():
    """LC.mixed_model(): 3 input channels, at most 128 anywhere, the seven int8 layers of its docstring among fp32 ones; its walks are
    well-formed and cover what they claim; on every fed input the evaluation fed its own blobs (tests/qseam_ref.py) is finite and the
    planes float64 is the yardstick of keep PLANE_FLOOR."""
    import qseam_ref as QR
    param, weights, name, outputs = LC.mixed_model()
    net = R.Net(param, weights)
    assert net.read == len(weights) and sorted(net.q) == sorted(LC.MIXED_INT8)
    by_name = {n: (t, pd) for t, n, _, _, pd in net.layers}
    assert by_name["conv0"][1][6] == 16 * 3 * 9 and not by_name["conv0"][1].get(8) and not by_name["fb"][1].get(8)
    assert max(pd[0] for t, pd in by_name.values() if t in ("Convolution", "ConvolutionDepthWise")) <= 128
    assert by_name["qdw"][0] == "ConvolutionDepthWise" and by_name["qdw"][1][7] == 32 and by_name["qpw"][1][1] == 1 and 64 < by_name["qpw"][1][0] < 160
    assert by_name["out"][0] == "InnerProduct" and by_name["out"][1][8] == 1
    order = [n for _, n, *_ in net.layers]
    assert order.index("qbn") + 3 == order.index("qbn_relu") and order.index("pool2") == order.index("q2") + 2  # BatchNorm, Scale, ReLU; ReLU, pooling
    # the walks
    for wname, walk in LC.MIXED_WALKS.items():
        fed = False
        for step in walk:
            assert step[0] in LC.STEP_KINDS and step[0] != "extract", (wname, step)
            if step[0] == "feed":
                assert step[1] in LC.MIXED_SHAPES, (wname, step)
                fed = True
            elif step[0] == "forward":
                assert fed and step[1] >= 1
        assert walk[-1][0] == "forward"
    feeds = [LC.MIXED_SHAPES[s[1]] for s in LC.WALK_MIXED if s[0] == "feed"]
    assert [f[0] for f in feeds[:4]] == [4, 5, 1, 4] and [f[2:] for f in feeds[3:7]] == [(16, 16), (12, 12), (13, 21), (16, 16)]
    kinds = [s[0] for s in LC.WALK_MIXED]
    assert {"set_tuned", "set_concurrency", "set_graph", "stream"} <= set(kinds)
    on = kinds.index("set_graph")
    assert LC.WALK_MIXED[on][1] is True and "feed" in kinds[on:kinds.index("set_graph", on + 1)]  # a new shape while the graph is on
    assert [LC.MIXED_SHAPES[s[1]][0] for s in LC.WALK_MIXED_REPLICAS if s[0] == "feed"][:3] == [7, 2, 1]
    rows = LC.mixed_table()
    ids = [LC.row_id(r) for r in rows]
    assert len(ids) == len(set(ids)) == 9 and not set(ids) & {LC.row_id(r) for r in LC.table()}
    assert all(r[2].get("sub_batches") == 3 for r in rows if r[0] == "mixed_replicas")
    # the evaluation
    floor = (1.0, None)
    for key, variant in sorted({f for w in LC.MIXED_WALKS.values() for f in _fed(w)}):
        x = LC.input(key, variant)
        for level in (0, 2):
            blobs = QR.own(net, x, level)
            assert all(o in blobs for o in outputs)
            for n, v in blobs.items():
                assert np.isfinite(v).all() and v.shape[0] == x.shape[0], (key, n)
            for n in LC.MIXED_FP32:
                if n in blobs:
                    m = np.abs(blobs[n]).max(axis=(2, 3))
                    floor = min(floor, (float(m.min() / m.max()), n, key, variant))
                    assert m.min() >= LC.PLANE_FLOOR * m.max(), (key, variant, n, float(m.min() / m.max()))
            assert float(blobs["gap"].min()) > 0.0  # a mean of values >= 0: no cancellation in the one-value planes
    print(f"mixed model: smallest plane maximum relative to its tensor's: {floor}")
