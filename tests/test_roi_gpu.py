"""libfeather_roi.so and the two-stage detection layers of the Net runtime on the device, against tests/roi_ref.py.

* ROIPooling, ROIAlign (both versions) and PSROIPooling equal the float32 restatement exactly, from 16-byte aligned and from misaligned
  guarded buffers (tests/guarded.py).
* Proposal on the cases of tests/roi_cases.py: rows, order, counts, sentinel rows and scores equal the float32 restatement exactly;
  coordinates are within max(8 x e32, 2^-20), relative to the larger image extent, of the float64 restatement, e32 being the float32
  restatement's own worst error against float64 on the same case.  Both figures are printed.
* The edge cases, one test each, and one kernel trace: the sweep launches what fhip_roi_route names.
* tiny_faster_rcnn and tiny_rfcn through FeedInput x2 -> Forward -> Extract / ExtractProposals at fusion levels 0 and 2, in a captured graph,
  in 2 sub-batch replicas and re-planned across batch sizes.
"""
import numpy as np
import pytest

import kernel_instances as KI
import ktrace
import roi_cases as C
import roi_ref as R
import roi_sweep as SW
import side_contract

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module")
def lib(cuda):
    return side_contract.library("roi")


# ---- the three ROI layers: exact ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", C.POOLED, ids=lambda c: "%dx%d-%g" % c)
def test_roi_pooling_is_exact(lib, cfg):
    x, r, want = C.pool_case(cfg)
    for offset in (0, 1):
        got = SW.roi_pool(lib, x, r, *cfg, offset=offset)
        assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (cfg, offset)
    assert SW.route(lib, C.POOL) == "fhip::roi_pool_kernel"


@pytest.mark.parametrize("cfg", C.ALIGN_CASES, ids=lambda c: "v%d-aligned%d-s%d-%dx%d-%g" % c)
def test_roi_align_is_exact(lib, cfg):
    version, aligned, sampling, pw, ph, scale = cfg
    x, r, want = C.align_case(cfg)
    for offset in (0, 1):
        got = SW.roi_align(lib, x, r, pw, ph, scale, sampling, aligned, version, offset=offset)
        assert got.shape == want.shape and np.array_equal(got, want), (cfg, offset, float(np.abs(got - want).max()))
    assert SW.route(lib, C.ALIGN, version) == "fhip::roi_align_kernel<%d>" % version


@pytest.mark.parametrize("cfg", C.PS_CASES, ids=lambda c: "%dx%d-%g" % c)
def test_psroi_pooling_is_exact(lib, cfg):
    x, r, want = C.psroi_case(cfg)
    for offset in (0, 1):
        got = SW.psroi_pool(lib, x, r, 2, *cfg, offset=offset)
        assert got.shape == want.shape and np.array_equal(got, want), (cfg, offset, float(np.abs(got - want).max()))
    assert SW.route(lib, C.PSROI) == "fhip::psroi_pool_kernel"


def test_single_roi_is_ncnns_layer(lib):
    """n = R = 1: ncnn's own shape."""
    x, r, _ = C.pool_case(C.POOLED[0])
    one = r[1:2, 20:21]
    assert np.array_equal(SW.roi_pool(lib, x[1:2], one, 7, 7, 0.0625), R.roi_pool(x[1:2], one, 7, 7, 0.0625))
    assert np.array_equal(SW.roi_align(lib, x[1:2], one, 7, 7, 0.0625, 0, 0, 0), R.roi_align(x[1:2], one, 7, 7, 0.0625, 0, 0, 0))


# ---- Proposal --------------------------------------------------------------------------------------------------------------------------------------
def _hold(got, want64, want32, im_info, what):
    """Rows, order, counts, sentinel rows and scores exactly; coordinates at the tolerance of the case.  -> (e32, the device's worst error)."""
    rois, scores = got
    counts = R.counts(want32[0])
    assert R.counts(rois) == counts == R.counts(want64[0]), (what, "counts", R.counts(rois), counts)
    if scores is not None:
        assert np.array_equal(scores.view(np.uint32), want32[1].view(np.uint32)) and np.array_equal(scores, want64[1]), (what, "scores, rows or order")
    assert all((img[k:] == (0, 0, -1, -1)).all() for img, k in zip(rois, counts)), (what, "sentinel rows")
    tol, e32 = C.tolerance(want64, want32, im_info)
    err = R.worst_coordinate_error(rois, want64[0], im_info)
    print(f"{what}: counts {counts}, e32 {e32:.3g}, device {err:.3g}, tolerance {tol:.3g}")
    assert err <= tol, (what, err, tol)
    return e32, err


@pytest.mark.parametrize("c", C.CASES, ids=C.case_id)
def test_proposal(lib, c):
    inputs, args, want64, want32, m = C.case(c)
    assert C.stable(m), m  # asserted where the table is built (tests/test_roi_cpu.py); nothing is skipped here
    got = SW.proposal(lib, *inputs, offset=C.CASES.index(c) % 2, **args)  # aligned and misaligned buffers in turn
    _hold(got, want64, want32, inputs[2], C.case_id(c))
    assert SW.route(lib, C.KEYS) == "fhip::proposal_key_kernel" and SW.route(lib, C.SELECT) == "fhip::proposal_select_kernel"


def _edge(shape="3x5", n=1, **changes):
    """The inputs and arguments of a case of that map with all candidates and 300 rows, as copies that a test may change."""
    c = (shape, n, 0, 300, 0, 1.0)
    score, bbox, info = C.draw(shape, n, 0)
    return [score.copy(), bbox.copy(), info.copy()], dict(C.args_of(c), **changes)


def _both(lib, inputs, args, what, with_scores=True):
    m = {}
    want64 = R.proposal(*inputs, dtype=np.float64, margins=m, **args)
    want32 = R.proposal(*inputs, dtype=np.float32, **args)
    assert C.stable(m), (what, m)
    got = SW.proposal(lib, *inputs, with_scores=with_scores, **args)
    _hold(got, want64, want32, inputs[2], what)
    return got, want32


def test_an_image_without_candidates_gives_only_sentinel_rows(lib):
    inputs, args = _edge(min_size=5000)
    (rois, scores), _ = _both(lib, inputs, args, "no candidate")
    assert rois.shape == (1, 300, 4) and (rois == (0, 0, -1, -1)).all() and not scores.any()


def test_only_the_middle_image_proposes(lib):
    inputs, args = _edge(n=3, min_size=16)
    inputs[2][0, 2] = inputs[2][2, 2] = 1000.0  # im_scale: a minimum box of 16000 px
    (rois, scores), _ = _both(lib, inputs, args, "middle image")
    assert R.counts(rois)[0] == R.counts(rois)[2] == 0 and R.counts(rois)[1] >= 1
    alone, alone_scores = SW.proposal(lib, *[x[1:2] for x in inputs], **args)
    assert np.array_equal(alone[0], rois[1]) and np.array_equal(alone_scores[0], scores[1])  # an image's rows do not depend on its neighbours


def test_bitwise_equal_scores_come_in_index_order(lib):
    """Five anchors of different cells get the same score above every other one and a 6-px box at their own cell's centre: five disjoint boxes
    with bitwise-equal scores, ordered by (q * h + i) * w + j."""
    inputs, args = _edge()
    score, bbox, info = inputs
    places = [(7, 2, 4), (0, 1, 1), (4, 0, 3), (0, 0, 2), (8, 2, 0)]  # (anchor, row, column), not in order
    a = R.generate_anchors().astype(np.float64)
    for q, i, j in places:
        aw, ah = a[q, 2] - a[q, 0], a[q, 3] - a[q, 1]
        score[0, 9 + q, i, j] = 2.0
        bbox[0, 4 * q:4 * q + 4, i, j] = (-(a[q, 0] + aw / 2 - 8) / aw, -(a[q, 1] + ah / 2 - 8) / ah, np.log(6 / aw), np.log(6 / ah))
    (rois, scores), _ = _both(lib, inputs, args, "ties")
    assert (scores[0, :5] == 2.0).all() and scores[0, 5] < 2.0
    centres = [(16 * j + 8, 16 * i + 8) for q, i, j in sorted(places)]
    assert np.allclose((rois[0, :5, 0] + rois[0, :5, 2]) / 2, [c[0] for c in centres], atol=0.01) and np.allclose((rois[0, :5, 1] + rois[0, :5, 3]) / 2,
                                                                                                               [c[1] for c in centres], atol=0.01)


def test_a_nan_score_and_a_nan_delta_are_no_candidates(lib):
    inputs, args = _edge()
    score, bbox, info = inputs
    fg = score[0, 9:].reshape(-1)
    first, second, third = np.argsort(-fg)[:3]
    q2, cell2 = divmod(int(second), 15)
    fg[first] = np.nan
    bbox[0, 4 * q2 + 2].reshape(-1)[cell2] = np.nan  # dw: a NaN width, NaN corners, a NaN extent
    want_best = float(fg[third])
    (rois, scores), _ = _both(lib, inputs, args, "nan")
    assert np.isfinite(rois).all() and np.isfinite(scores).all() and scores[0, 0] == want_best


def test_after_nms_topn_reached_mid_chunk_gives_a_prefix(lib):
    inputs, args, want64, want32, _ = C.case(C.CASES[3])  # 12x16, 1728 anchors, 207 survivors of 300 rows
    full, full_scores = SW.proposal(lib, *inputs, **args)
    for rows in (1, 5, 16, 100):
        got, got_scores = SW.proposal(lib, *inputs, **dict(args, after_nms_topN=rows))
        assert np.array_equal(got, full[:, :rows]) and np.array_equal(got_scores, full_scores[:, :rows]), rows
    rank = int((inputs[0][0, 9:] > full_scores[0, 15]).sum())  # candidates ordered before the 16th survivor
    assert 0 < rank % C.CHUNK < C.CHUNK - 1 and rank < C.CHUNK, rank  # inside the first selection round, not at its end


def test_without_the_score_top_and_two_runs_are_bitwise_equal(lib):
    inputs, args, want64, want32, _ = C.case(C.CASES[7])
    a, a_scores = SW.proposal(lib, *inputs, **args)
    b, none = SW.proposal(lib, *inputs, with_scores=False, **args)
    assert none is None and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_the_python_mirror(cuda):
    import torch
    from feathercnn_amd import roi
    inputs, args, want64, want32, _ = C.case(C.CASES[1])
    t = [torch.from_numpy(x).cuda() for x in inputs]
    rois, scores = roi.proposal(*t, with_scores=True, **args)
    assert np.array_equal(scores.cpu().numpy(), want32[1]) and R.counts(rois.cpu().numpy()) == R.counts(want32[0])
    x, r, want = C.pool_case(C.POOLED[1])
    assert np.array_equal(roi.roi_pool(torch.from_numpy(x).cuda(), torch.from_numpy(r).cuda(), (3, 2), 0.25).cpu().numpy(), want)
    cfg = C.ALIGN_CASES[-1]
    x, r, want = C.align_case(cfg)
    assert np.array_equal(roi.roi_align(torch.from_numpy(x).cuda(), torch.from_numpy(r).cuda(), (cfg[3], cfg[4]), cfg[5], cfg[2], cfg[1], cfg[0]).cpu().numpy(), want)
    x, r, want = C.psroi_case(C.PS_CASES[0])
    assert np.array_equal(roi.psroi_pool(torch.from_numpy(x).cuda(), torch.from_numpy(r).cuda(), 2, 3, C.PS_CASES[0][2]).cpu().numpy(), want)


def test_the_sweep_launches_what_the_route_names(cuda, tmp_path):
    """One child under rocprofv3 --kernel-trace (tests/roi_trace_child.py): the library's kernels in the trace are, launch for launch, the
    routes fhip_roi_route named, and together every instantiation tests/roi_cases.targets() names -- which is every instantiation the
    library holds (tests/test_open_contract_cpu.py)."""
    text, rows, _ = ktrace.trace("roi_trace_child.py", [], tmp_path, 240)
    named = [ln[len("route "):] for ln in text.splitlines() if ln.startswith("route ")]
    launched = [KI.normalise(name) for _, name, *_ in rows]
    launched = [nm for nm in launched if nm in C.targets()]
    assert launched == named, (launched, named)
    assert set(launched) == C.targets()


# ---- the nets --------------------------------------------------------------------------------------------------------------------------------
POOLED_BLOB = {"tiny_faster_rcnn": ("roi_pool", "feat_split_0"), "tiny_rfcn": ("psroi_cls", "rfcn_cls")}
OUTPUTS = {"tiny_faster_rcnn": ("cls_prob", "bbox_pred"), "tiny_rfcn": ("cls_score",)}


def _nerr(got, want):
    return float(np.abs(got.astype(np.float64) - want).max() / max(np.abs(want).max(), 1e-30))


def _net(name, level=2, graph=False, replicas=1):
    from feathercnn_amd.net import Net
    (p, b, i, o), _ = C.net_model(name)
    net = Net(fusion=level, graph=graph, sub_batches=replicas)
    net.SetDetection(True)
    net.SetRoi()
    net.LoadParam(p)
    net.LoadWeights(b)
    return net


def _check_net(net, name, batch):
    """Feed the stable input of (name, batch), run, and hold the RPN heads, the ROIs, the pooled rows and the outputs to the restatement; -> the
    ROI top."""
    (p, b, i, o), _ = C.net_model(name)
    (score, bbox, info_name), tops, args = C.proposal_args(p)
    x, info, blobs, m = C.net_input(name, batch)
    assert C.stable(m), m  # the margins hold on this net's head input: checked on the CPU, before anything is compared
    net.FeedInput(i, x)
    net.FeedInput(info_name, info)
    net.Forward()
    got_score, got_bbox = net.Extract(score), net.Extract(bbox)
    for nm, g in ((score, got_score), (bbox, got_bbox)):  # behind device convolutions: the project's net-level bound
        assert g.shape == blobs[nm].shape and _nerr(g, blobs[nm]) <= 1e-4, (nm, _nerr(g, blobs[nm]))
    top = net.Extract("rois")
    assert top.shape == (batch, C.NET_ROIS, 1, 4)
    # the whole net against numpy_forward: the same ROIs in the same order
    assert R.counts(top[:, :, 0]) == R.counts(blobs["rois"][:, :, 0]) and np.allclose(top, blobs["rois"], atol=1e-3), "rows or order"
    # the layer from its own inputs, at its own tolerance
    m2 = {}
    own64 = R.proposal(got_score, got_bbox, info, dtype=np.float64, margins=m2, **args)
    own32 = R.proposal(got_score, got_bbox, info, dtype=np.float32, **args)
    assert all(m2[k] >= C.MARGINS[k] / 2 for k in C.MARGINS) and m2["order"] > 0, m2
    _hold((top[:, :, 0], None), own64, own32, info, f"{name} at batch {batch}")
    rois = net.ExtractProposals("rois")
    assert all(np.array_equal(a, b) for a, b in zip(rois, R.trim(top[:, :, 0]))) and min(len(r) for r in rois) >= 2
    # the ROI layer from its own inputs: exact
    pooled_name, feat_name = POOLED_BLOB[name]
    pooled, feat = net.Extract(pooled_name), net.Extract(feat_name)
    want = R.roi_pool(feat, top, 3, 3, 0.25) if name == "tiny_faster_rcnn" else R.psroi_pool(feat, top, 5, 3, 3, 0.25)
    assert pooled.shape == want.shape == (batch * C.NET_ROIS,) + want.shape[1:] and np.array_equal(pooled, want)
    for out in OUTPUTS[name]:
        g = net.Extract(out)
        assert g.shape == blobs[out].shape and g.shape[0] == batch * C.NET_ROIS and _nerr(g, blobs[out]) <= 1e-4, (out, _nerr(g, blobs[out]))
    routes = {nm: a for _, nm, a in net.layers()}
    assert routes["rois"] == "ROI" and routes[pooled_name] == "ROI"
    return top


@pytest.mark.parametrize("name", sorted(C.NETS))
def test_tiny_nets_at_every_setting_equal_level_0_bit_for_bit(cuda, name):
    level0 = _check_net(_net(name, 0), name, 3)
    for level, graph, replicas in ((2, False, 1), (2, True, 1), (2, False, 2), (0, True, 2)):
        net = _net(name, level, graph, replicas)
        got = _check_net(net, name, 3)
        if graph:  # replay the captured graph
            net.Forward()
            assert np.array_equal(net.Extract("rois"), got)
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


def _roi_only(type_, params, c, h, w, rois):
    lines = [f"Input feat 0 1 feat 0={w} 1={h} 2={c}", f"Input rois 0 1 rois 0=4 1=1 2={rois}", f"{type_} pooled 2 1 feat rois pooled {params}"]
    return ("7767517\n3 3\n" + "\n".join(lines) + "\n").encode()


def test_a_user_fed_rois_input_gives_the_rows_proposal_gives(cuda):
    """The features and the ROIs of tiny_faster_rcnn fed into a net of two Inputs and one ROIPooling: the same pooled rows, bit for bit."""
    from feathercnn_amd.net import Net
    whole = _net("tiny_faster_rcnn")
    _check_net(whole, "tiny_faster_rcnn", 3)
    feat, rois, pooled = whole.Extract("feat_split_0"), whole.Extract("rois"), whole.Extract("roi_pool")
    for replicas in (1, 2):
        net = Net(fusion=2, sub_batches=replicas)
        net.SetRoi()
        net.LoadParam(_roi_only("ROIPooling", "0=3 1=3 2=0.25", 16, 12, 16, C.NET_ROIS))
        net.LoadWeights(b"")
        net.FeedInput("feat", feat)
        net.FeedInput("rois", rois)
        net.Forward()
        assert np.array_equal(net.Extract("pooled"), pooled), replicas
    x, r, want = C.align_case(C.ALIGN_CASES[5])  # the same route for ROIAlign, on the table's ROIs: sentinel and inverted ones included
    v, a, s, pw, ph, scale = C.ALIGN_CASES[5]
    net = Net()
    net.SetRoi()
    net.LoadParam(_roi_only("ROIAlign", f"0={pw} 1={ph} 2={scale} 3={s} 4={a} 5={v}", *x.shape[1:], C.ROIS))
    net.LoadWeights(b"")
    net.FeedInput("feat", x)
    net.FeedInput("rois", r.reshape(2, C.ROIS, 1, 4))
    net.Forward()
    assert np.array_equal(net.Extract("pooled"), want)


def test_shapes_that_do_not_fit_are_minus_100_at_reshape(cuda):
    from feathercnn_amd import FeatherHipError
    from feathercnn_amd.net import Net

    def run(param, feeds):
        net = Net()
        net.SetRoi()
        net.LoadParam(param)
        net.LoadWeights(b"")
        for k, v in feeds.items():
            net.FeedInput(k, v)
        net.Forward()

    feat, rois = np.zeros((2, 18, 6, 6), F), np.zeros((2, 4, 1, 4), F)
    run(_roi_only("PSROIPooling", "0=3 1=3 2=0.25 3=2", 18, 6, 6, 4), dict(feat=feat, rois=rois))
    for what, param, feeds in (("channels", _roi_only("PSROIPooling", "0=3 1=3 2=0.25 3=3", 18, 6, 6, 4), dict(feat=feat, rois=rois)),
                               ("rois of another batch", _roi_only("ROIPooling", "0=3 1=3", 18, 6, 6, 4), dict(feat=feat, rois=rois[:1])),
                               ("rois of 5 values", _roi_only("ROIAlign", "0=3 1=3", 18, 6, 6, 4), dict(feat=feat, rois=np.zeros((2, 4, 1, 5), F)))):
        with pytest.raises(FeatherHipError, match="code -100") as e:
            run(param, feeds)
        assert "layer pooled" in str(e.value), what
    lines = ["Input score 0 1 score 0=4 1=3 2=18", "Input bbox 0 1 bbox 0=4 1=3 2=36", "Input im_info 0 1 im_info 0=3 1=1 2=1", "Proposal rois 3 1 score bbox im_info rois 3=8"]
    param = ("7767517\n4 4\n" + "\n".join(lines) + "\n").encode()
    good = dict(score=np.zeros((2, 18, 3, 4), F), bbox=np.zeros((2, 36, 3, 4), F), im_info=np.tile(np.asarray([48, 64, 1], F), (2, 1, 1, 1)))
    run(param, good)
    for what, feeds in (("score channels", dict(good, score=np.zeros((2, 16, 3, 4), F))), ("bbox extent", dict(good, bbox=np.zeros((2, 36, 3, 5), F))),
                        ("im_info batch", dict(good, im_info=good["im_info"][:1])), ("im_info values", dict(good, im_info=np.zeros((2, 1, 1, 4), F)))):
        with pytest.raises(FeatherHipError, match="code -100") as e:
            run(param, feeds)
        assert "layer rois" in str(e.value), what
