"""libfeather_yolo.so and the YOLO layers of the Net runtime on the device, against tests/yolo_ref.py.

* Reorg equals numpy exactly, both modes, from 16-byte aligned and from misaligned guarded buffers (tests/guarded.py).
* The detection on the cases of tests/yolo_cases.py, both versions: rows, labels and order equal the float32 restatement exactly; scores and
  coordinates are within max(8 x e32, 2^-20), relative, of the float64 restatement, e32 being the float32 restatement's own worst relative
  error against float64 on the same case.  Both figures are printed.
* The edge cases, one test each, and one kernel trace: the sweep launches what fhip_yolo_route names.
* tiny_yolov2 and tiny_yolov3 through FeedInput -> Forward -> ExtractDetections at fusion levels 0 and 2, in a captured graph, in 2 sub-batch
  replicas and re-planned across batch sizes.
"""
import numpy as np
import pytest

import kernel_instances as KI
import ktrace
import side_contract
import yolo_cases as C
import yolo_ref as R
import yolo_sweep as SW

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module")
def lib(cuda):
    return side_contract.library("yolo")


# ---- Reorg -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("shape", C.REORG_SHAPES + C.REORG_DIRECT, ids=lambda s: "x".join(map(str, s)))
def test_reorg_is_exact(lib, shape, mode):
    n, c, h, w, s = shape
    x = np.random.default_rng(sum(shape)).uniform(-1, 1, (n, c, h, w)).astype(F)
    for offset in (0, 1):
        got = SW.reorg(lib, x, s, mode, offset)
        assert got.shape == (n, c * s * s, h // s, w // s) and np.array_equal(got, R.reorg(x, s, mode)), (shape, mode, offset)
    assert SW.route(lib, 0, s, w) == ("fhip::reorg_direct_kernel" if shape in C.REORG_DIRECT else "fhip::reorg_tile_kernel")


# ---- the detection -------------------------------------------------------------------------------------------------------------------------
def _hold(got, want64, want32, what):
    """Rows, labels and order exactly; scores and coordinates at the tolerance of the case.  -> (e32, the device's worst relative error)."""
    assert np.array_equal(got[:, :, 0], want32[:, :, 0]) and np.array_equal(got[:, :, 0], want64[:, :, 0]), (what, "rows, labels or order")
    counts = [len(d) for d in R.trim(want64)]
    assert all(not img[k:].any() for img, k in zip(got, counts)), (what, "rows past the count are zero")
    tol, e32 = C.tolerance(want64, want32)
    err = R.worst_relative(got, want64)
    print(f"{what}: counts {counts}, e32 {e32:.3g}, device {err:.3g}, tolerance {tol:.3g}")
    assert err <= tol, (what, err, tol)
    return e32, err


@pytest.mark.parametrize("cid", C.case_ids(), ids=lambda c: "v%d-%s-n%d-c%d" % c)
def test_detection(lib, cid):
    bottoms, args, want64, want32, m = C.case(*cid)
    assert C.stable(m), m  # asserted where the table is built (tests/test_yolo_cpu.py); nothing is skipped here
    got = SW.detection(lib, bottoms, offset=C.case_ids().index(cid) % 2, **args)  # aligned and misaligned buffers in turn
    _hold(got, want64, want32, "v%d-%s-n%d-c%d" % cid)
    assert SW.route(lib, 1, cid[0]) == "fhip::yolo_score_kernel<%d>" % cid[0] and SW.route(lib, 2) == "fhip::yolo_select_kernel"


def _edge(version, n=1):
    """The bottoms and arguments of the two-scale case with 3 classes, as copies that a test may change."""
    bottoms, args, _, _, _ = C.case(version, "two_4x4_8x8", n, 3)
    return [b.copy() for b in bottoms], dict(args)


def _both(lib, bottoms, args, what):
    m = {}
    want64 = R.detection(bottoms, dtype=np.float64, margins=m, **args)
    want32 = R.detection(bottoms, dtype=np.float32, **args)
    assert C.stable(m), (what, m)
    got = SW.detection(lib, bottoms, **args)
    _hold(got, want64, want32, what)
    return got, want32


@pytest.mark.parametrize("version", [2, 3])
def test_an_image_without_candidates_gives_zero_rows(lib, version):
    bottoms, args = _edge(version)
    args["confidence_threshold"] = 0.95  # the grid ends at 0.9
    got, _ = _both(lib, bottoms, args, "no candidate")
    assert got.shape == (1, 64, 6) and not got.any()


@pytest.mark.parametrize("version", [2, 3])
def test_only_the_middle_image_detects(lib, version):
    bottoms, args = _edge(version, 3)
    for x in bottoms:
        v = x.reshape(3, args["num_box"], 5 + 3, *x.shape[2:])
        v[0, :, 4] = v[2, :, 4] = -20.0  # an objectness of sigmoid(-20) = 2e-9
    got, want32 = _both(lib, bottoms, args, "middle image")
    assert not got[0].any() and not got[2].any() and (got[1, :, 0] > 0).sum() >= 1
    alone = SW.detection(lib, [x[1:2] for x in bottoms], **args)
    assert np.array_equal(alone[0], got[1])  # an image's rows do not depend on its neighbours


@pytest.mark.parametrize("version", [2, 3])
def test_exact_ties_come_in_global_index_order(lib, version):
    """The raw values of one box -- objectness 6, so a confidence above every grid value -- copied into five boxes of both bottoms: five
    bitwise-equal confidences, ordered by bottom, then box, then row, then column.  The boxes are tiny and lie in different cells."""
    bottoms, args = _edge(version)
    nb = args["num_box"]
    v = [x.reshape(1, nb, 5 + 3, *x.shape[2:]) for x in bottoms]
    one = v[0][0, 0, :, 0, 0].copy()
    one[4] = 6.0
    one[2:4] = -6.0  # tiny whatever the anchor
    places = [(1, 1, 7, 0), (0, 1, 1, 1), (1, 0, 5, 5), (0, 0, 2, 3), (0, 0, 0, 0)]  # (bottom, box, row, column), not in order
    for b, pp, i, j in places:
        v[b][0, pp, :, i, j] = one
    got, want32 = _both(lib, bottoms, args, "ties")
    assert len(set(got[0, :5, 1].tolist())) == 1 and got[0, 5, 1] < got[0, 4, 1]  # five equal scores lead
    centres = [((j + 0.5) / bottoms[b].shape[3], (i + 0.5) / bottoms[b].shape[2]) for b, pp, i, j in sorted(places)]
    assert np.allclose((got[0, :5, 2] + got[0, :5, 4]) / 2, [c[0] for c in centres], atol=0.01) and np.allclose((got[0, :5, 3] + got[0, :5, 5]) / 2,
                                                                                                            [c[1] for c in centres], atol=0.01)


@pytest.mark.parametrize("version", [2, 3])
def test_nan_and_infinite_objectness(lib, version):
    """NaN is no candidate, -inf gives confidence 0 (below the threshold), +inf gives sigmoid 1: a candidate with its class factor as score."""
    bottoms, args = _edge(version)
    v = bottoms[1].reshape(1, args["num_box"], 5 + 3, 8, 8)
    top = np.argsort(-v[0, 0, 4].reshape(-1))[:3]  # the three most confident cells of box 0
    for cell, value in zip(top, (np.nan, -np.inf, np.inf)):
        v[0, 0, 4, cell // 8, cell % 8] = value
    got, want32 = _both(lib, bottoms, args, "nan and inf")
    assert np.isfinite(got).all() and (got[0, :, 0] > 0).sum() >= 1


@pytest.mark.parametrize("version", [2, 3])
def test_zero_area_boxes_suppress_nothing(lib, version):
    """Two candidates of one cell with w_raw = h_raw = -inf: boxes of zero area at the same point, IoU 0 / 0, and both are kept."""
    bottoms, args = _edge(version)
    v = bottoms[0].reshape(1, args["num_box"], 5 + 3, 4, 4)
    v[0, :, 4, 2, 1] = (7.0, 6.5)  # the two best confidences
    v[0, :, 0:2, 2, 1] = 0.25
    v[0, :, 2:4, 2, 1] = -np.inf
    got, want32 = _both(lib, bottoms, args, "zero area")
    assert (got[0, :2, 2] == got[0, :2, 4]).all() and (got[0, :2, 3] == got[0, :2, 5]).all() and got[0, 0, 2] == got[0, 1, 2]  # both kept, the same point


@pytest.mark.parametrize("version", [2, 3])
def test_the_output_is_a_prefix_whatever_rows_is(lib, version):
    bottoms, args, want64, want32, _ = C.case(version, "two_4x4_8x8", 3, 3)
    full = SW.detection(lib, bottoms, **args)
    for rows in (1, 5):
        got = SW.detection(lib, bottoms, **dict(args, rows=rows))
        assert np.array_equal(got, full[:, :rows]), rows


@pytest.mark.parametrize("version", [2, 3])
def test_more_rows_than_survivors(lib, version):
    """rows = 1024 where some 60 boxes survive: the same rows as at the case's own height, zeros behind them."""
    bottoms, args, want64, want32, _ = C.case(version, "two_4x4_8x8", 3, 3)
    full = SW.detection(lib, bottoms, **args)
    args = dict(args, rows=1024)
    more = SW.detection(lib, bottoms, **args)
    _hold(more, R.detection(bottoms, dtype=np.float64, **args), R.detection(bottoms, dtype=np.float32, **args), "rows 1024")
    counts = (more[:, :, 0] > 0).sum(axis=1)
    assert counts.max() < 1024 and all(np.array_equal(more[i, :min(k, 64)], full[i, :min(k, 64)]) and not more[i, k:].any() for i, k in enumerate(counts))


@pytest.mark.parametrize("version", [2, 3])
def test_rows_reached_in_a_later_round(lib, version):
    """The case with 3456 candidates per image at rows = 40: its survivors lie some 55 candidates apart, so row 40 is reached in the third
    selection round, behind two rounds that each sorted and cut the buffer; and the result is the prefix of the case's own."""
    bottoms, args, want64, want32, _ = C.case(version, "two_past_the_buffer", 1, 3)
    conf, _, _ = R.scores(bottoms, args["version"], args["num_class"], args["num_box"], np.float64)
    rank = (conf[0] > want64[0, 39, 1]).sum()  # candidates ordered before the 40th survivor
    assert (want64[0, :, 0] > 0).sum() > 40 and 2 * C.CHUNK < rank < 3 * C.CHUNK, rank
    got = SW.detection(lib, bottoms, **dict(args, rows=40))
    _hold(got, want64[:, :40], want32[:, :40], "rows reached in round 3")


@pytest.mark.parametrize("version", [2, 3])
def test_two_runs_are_bitwise_equal(lib, version):
    bottoms, args, _, _, _ = C.case(version, "three_past_a_chunk", 3, 3)
    a, b = SW.detection(lib, bottoms, **args), SW.detection(lib, bottoms, **args)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_the_sweep_launches_what_the_route_names(cuda, tmp_path):
    """One child under rocprofv3 --kernel-trace (tests/yolo_trace_child.py): the library's kernels in the trace are, launch for launch, the
    routes fhip_yolo_route named, and together every instantiation tests/yolo_cases.targets() names -- which is every instantiation the
    library holds (tests/test_open_contract_cpu.py)."""
    text, rows, _ = ktrace.trace("yolo_trace_child.py", [], tmp_path, 240)
    named = [ln[len("route "):] for ln in text.splitlines() if ln.startswith("route ")]
    launched = [KI.normalise(name) for _, name, *_ in rows]
    launched = [nm for nm in launched if nm in C.targets()]
    assert launched == named, (launched, named)
    assert set(launched) == C.targets()


# ---- the nets --------------------------------------------------------------------------------------------------------------------------------
ROWS = 16


def _nerr(got, want):
    return float(np.abs(got.astype(np.float64) - want).max() / max(np.abs(want).max(), 1e-30))


def _net(name, level=2, graph=False, replicas=1):
    from feathercnn_amd.net import Net
    (p, b, i, o), _ = C.net_model(name)
    net = Net(fusion=level, graph=graph, sub_batches=replicas)
    net.SetYolo(ROWS)
    if name == "tiny_yolov3":
        net.SetExtendedLayers(True)
    net.LoadParam(p)
    net.LoadWeights(b)
    return net


def _check_net(net, name, batch):
    """Feed the stable input of (name, batch), run, and hold the heads and the detections to the restatement; -> the detection top."""
    (p, b, i, o), _ = C.net_model(name)
    heads, args = C.head_args(p)
    x, want_heads, want64, m = C.net_input(name, batch, ROWS)
    assert C.stable(m), m  # the margins hold on this net's head input: checked on the CPU, before anything is compared
    net.FeedInput(i, x)
    net.Forward()
    got_heads = [net.Extract(h) for h in heads]
    for h, g in zip(heads, got_heads):  # behind device convolutions: the project's net-level bound
        assert g.shape == want_heads[h].shape and _nerr(g, want_heads[h]) <= 1e-4, (h, _nerr(g, want_heads[h]))
    top = net.Extract(o)
    assert top.shape == (batch, 1, ROWS, 6)
    got = top[:, 0]
    # the whole net against numpy_forward followed by the restatement: the same detections in the same order
    assert np.array_equal(got[:, :, 0], want64[:, :, 0]), "rows, labels or order"
    # the layer from its own inputs, at its own tolerance
    m2 = {}
    own64 = R.detection(got_heads, rows=ROWS, dtype=np.float64, margins=m2, **args)
    own32 = R.detection(got_heads, rows=ROWS, dtype=np.float32, **args)
    assert all(m2[k] >= C.MARGINS[k] / 2 for k in C.MARGINS), m2
    _hold(got, own64, own32, f"{name} at batch {batch}")
    dets = net.ExtractDetections(o)
    assert [d.shape for d in dets] == [d.shape for d in R.trim(got)] and all(np.array_equal(a, b) for a, b in zip(dets, R.trim(got)))
    assert min(len(d) for d in dets) >= 1
    routes = {nm: a for _, nm, a in net.layers()}
    assert routes[o] == "YOLO" and (name != "tiny_yolov2" or routes["reorg"] == "YOLO")
    return top


@pytest.mark.parametrize("name", sorted(C.NETS))
def test_tiny_nets_at_every_setting_equal_level_0_bit_for_bit(cuda, name):
    level0 = _check_net(_net(name, 0), name, 3)
    for level, graph, replicas in ((2, False, 1), (2, True, 1), (2, False, 2), (0, True, 2)):
        net = _net(name, level, graph, replicas)
        got = _check_net(net, name, 3)
        if graph:  # replay the captured graph
            net.Forward()
            assert np.array_equal(net.Extract("detection_out"), got)
        assert np.array_equal(got, level0), (level, graph, replicas)


@pytest.mark.parametrize("name", sorted(C.NETS))
def test_tiny_nets_replan_across_batch_sizes(cuda, name):
    for level, graph in ((2, True), (0, False)):
        net = _net(name, level, graph)
        first = _check_net(net, name, 3)
        _check_net(net, name, 2)
        _check_net(net, name, 5)
        again = _check_net(net, name, 3)
        assert np.array_equal(again, first)
