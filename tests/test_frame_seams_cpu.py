"""The seams of Padding, Crop and PixelShuffle and the zero-Padding fold without a GPU (tests/frame_seam_cases.py and
tests/frame_fold_cases.py are the tables, tests/frame_seam_ref.py the float64 evaluator):

* the pair table builds the same bytes twice, the pairs that cannot exist are exactly the written list, and every new layer meets every
  listed neighbour on both sides that is not on that list -- no pair drops out silently;
* the evaluator agrees with feathercnn_amd.model_zoo.numpy_forward on tiny_frame: every framing top is, bit for bit, the restatement of
  numpy_forward's own bottoms (per-channel values read from the .bin where they stand), and the output agrees to float32 rounding;
* every case evaluates, reads its whole .bin, and no plane of an output or of P's top lies below 1e-3 of its tensor's maximum (the floor of tests/seam_cases.py's
  SALT rule), so that the per-plane metric of tests/test_frame_seams_gpu.py is defined everywhere;
* `expect` has a verdict for every pair on the side that holds a framing layer, and the verdicts hold on the fused layer list at levels 0, 2
  and 3 (the fusion pass runs without a device);
* the fold table claims own pads plus margins, and its folded / kept and absorbed-layer claims hold on the fused layer list."""
import numpy as np
import pytest

import frame_cases as FC
import frame_fold_cases as FF
import frame_ref
import frame_seam_cases as FS
import frame_seam_ref as R
import seam_cases as SC

ALIVE = 1e-3
_RESULTS = {}


def _evaluate(pname):
    if pname not in _RESULTS:
        rows = []
        for case in FS.cases_of(pname):
            net = R.Net(case.param, case.weights)
            rows.append((case, net, net.run("data", case.input(), keep=True)))
        _RESULTS[pname] = rows
    return _RESULTS[pname]


def _built():
    built, missing = {}, {}
    for pname, cname in FS.pairs():
        for plane in SC.PLANES:
            try:
                built[(pname, cname, plane)] = FS.build_case(pname, cname, plane)
            except SC.Incompatible:
                missing.setdefault((pname, cname), []).append(plane)
    return built, missing


def test_the_table_builds_deterministically_and_the_incompatible_pairs_are_the_written_list():
    built, missing = _built()
    again, _ = _built()
    assert built.keys() == again.keys()
    for key, case in built.items():
        assert case.param == again[key].param and case.weights == again[key].weights, key
    # a pair is missing on both planes or on none, and the missing ones are the list, each with a reason
    assert all(len(planes) == len(SC.PLANES) for planes in missing.values()), {k: v for k, v in missing.items() if len(v) != len(SC.PLANES)}
    assert set(missing) == set(FS.INCOMPATIBLE), (set(missing) ^ set(FS.INCOMPATIBLE))
    assert all(isinstance(why, str) and len(why) > 10 for why in FS.INCOMPATIBLE.values())
    assert len(FS.pairs()) == len(set(FS.pairs())) and len(built) == len(SC.PLANES) * (len(FS.pairs()) - len(FS.INCOMPATIBLE))
    # the tables of tests/seam_cases.py are as they were: this module extends copies
    assert not set(FS.NEW_UNARY) & set(SC.UNARY) and not set(FS.NEW_PRODUCERS) & set(SC.PRODUCERS) and "crop_like" not in SC.CONSUMERS


def test_every_new_layer_meets_every_neighbour_on_both_sides():
    pairs = set(FS.pairs())
    assert len(FS.OLD_PRODUCERS) == 19 and len(FS.OLD_CONSUMERS) == 25 and len(FS.NEW_UNARY) == 14
    for op in FS.NEW_UNARY:
        for p in FS.OLD_PRODUCERS + tuple(FS.NEW_PRODUCERS):  # op as the consumer
            assert (p, op) in pairs, (p, op)
        for c in FS.OLD_CONSUMERS + tuple(FS.NEW_CONSUMERS):  # op as the producer
            assert (op, c) in pairs, (op, c)
    for p in FS.OLD_PRODUCERS + tuple(FS.NEW_PRODUCERS):
        assert (p, "crop_like") in pairs
    built, _ = _built()
    for pname, cname in pairs:  # whatever is not on the list is built, on both planes, with the framing type where the table says it is
        if (pname, cname) in FS.INCOMPATIBLE:
            continue
        for plane in SC.PLANES:
            case = built[(pname, cname, plane)]
            if pname in FS.NEW_UNARY:
                assert case.p_types <= FS.FRAME_TYPES and case.p_types, (case.id, case.p_types)
            if cname in FS.NEW_CONSUMERS:
                assert case.c_types <= FS.FRAME_TYPES and case.c_types, (case.id, case.c_types)


def test_the_evaluator_agrees_with_numpy_forward_on_tiny_frame():
    (param, weights, i, o), _ = FC.net_model()
    x, want = FC.net_input(3)
    net = R.Net(param, weights)
    assert net.read == len(weights) and set(net.pc) == {"pad_pc"}
    blobs = net.run(i, x, keep=True)
    layers = [l for l in frame_ref.parse_param(param) if l[0] in R.FRAME_TYPES]
    assert [l[1] for l in layers] == list(FC.FRAME_TOPS)
    for layer in layers:
        top = layer[3][0]
        own = R.frame_layer(layer, [want[b] for b in layer[2]], net.pc.get(layer[1]))
        assert own.shape == want[top].shape and np.array_equal(own.view(np.uint32), np.asarray(want[top], np.float32).view(np.uint32)), layer[1]
        assert blobs[top].shape == want[top].shape
    assert np.array_equal(blobs["pad_reflect"].view(np.uint32), np.asarray(want["pad_reflect"], np.float32).view(np.uint32))  # straight behind the input
    # float32 against float64 rounded per blob: a sum of at most 9 * 24 products carries a few 2^-24 of the tensor's magnitude per layer
    err = float(np.abs(blobs[o].astype(np.float64) - want[o]).max() / np.abs(want[o]).max())
    assert blobs[o].shape == want[o].shape and err <= 1e-5, err


@pytest.mark.parametrize("pname", FS.row_names())
def test_every_case_evaluates_and_every_output_plane_is_alive(pname):
    rows = _evaluate(pname)
    assert len(rows) >= 10, (pname, len(rows))
    for case, net, blobs in rows:
        assert net.read == len(case.weights), case.id
        assert case.c_first in [l[1] for l in net.layers] and case.p_top in blobs, case.id
        for o in tuple(case.outputs) + (case.p_top,):  # the GPU test compares P's top too
            y = blobs[o].astype(np.float64)
            assert y.ndim == 4 and y.shape[0] == SC.BATCH and np.isfinite(y).all(), (case.id, o)
            peak = np.abs(y).max(axis=(2, 3))
            assert peak.min() >= ALIVE * peak.max(), (case.id, o, float(peak.min() / peak.max()))
        alone = net.run("data", case.input()[:1], keep=True)
        assert np.array_equal(alone[case.c_top], blobs[case.c_top][:1]), case.id
    for key in FS.SALT:  # every redraw is of a case that exists
        p, rest = key.split("->")
        assert (p, rest.split("@")[0]) in set(FS.pairs()) - set(FS.INCOMPATIBLE), key


def _net(case_or_model, level, tuned=False, dilated=False):
    from feathercnn_amd import FeatherHipError
    from feathercnn_amd.net import Net
    param, weights = case_or_model
    net = Net(fusion=level, tuned=tuned)
    net.SetFrame()
    if dilated:
        net.SetDilated(True)
    net.LoadParam(param)
    net.LoadWeights(weights)
    with pytest.raises(FeatherHipError, match="has not been fed"):
        net.Forward()  # the fusion pass runs first; the list it leaves is the fused one
    return net


def test_expect_has_a_verdict_wherever_a_framing_layer_stands():
    seen = set()
    for pname, cname in FS.pairs():
        for level, _ in FS.LEVELS:
            v = FS.expect(pname, cname, level)
            assert (v["p"] is not None) == (pname in FS.NEW_UNARY) and (v["c"] is not None) == (cname in FS.NEW_CONSUMERS), (pname, cname, level, v)
            assert v["p"] in (None, "folded", "absorbed", "alias", "kept") and v["c"] in (None, "alias", "kept")
            seen |= {v["p"], v["c"]}
            if level < 2:
                assert v["p"] not in ("folded", "absorbed")
    assert seen == {None, "folded", "absorbed", "alias", "kept"}
    # the rules, spot by spot: what folds, what only looks as if it could, what absorbs
    assert FS.expect("pad_same", "conv3x3s2", 2)["p"] == "folded" and FS.expect("pad_sym1", "gconv3", 3)["p"] == "folded" and FS.expect("pad_none", "dw3x3", 2)["p"] == "folded"
    for kept in (("pad_value", "conv3x3"), ("pad_rep", "conv3x3"), ("pad_reflect", "conv3x3"), ("pad_pc", "conv3x3"), ("pad_ch", "conv3x3"), ("pad_same", "dil3x3"),
                 ("pad_same", "deconv4"), ("pad_sym1", "maxpool2"), ("pad_sym1", "relu"), ("ps2", "prelu"), ("ps2", "conv3x3")):
        assert FS.expect(*kept, 2)["p"] == "kept", kept
    assert FS.expect("pad_none", "dil3x3", 2)["p"] == "alias" and FS.expect("pad_none", "conv3x3", 0)["p"] == "alias"
    assert FS.expect("ps2", "relu", 2)["p"] == FS.expect("ps2m1", "leaky", 3)["p"] == FS.expect("ps1", "relu", 2)["p"] == "absorbed"
    assert FS.expect("ps1", "relu", 0)["p"] == "alias" and FS.expect("conv3x3", "crop_none", 2)["c"] == "alias" and FS.expect("conv3x3", "crop_like", 2)["c"] == "kept"
    assert FS.folded_pads("pad_same", "conv3x3s2") == (1, 2, 1, 2) and FS.folded_pads("pad_sym1", "conv1x1") == (1, 1, 1, 1)


@pytest.mark.parametrize("pname", FS.row_names())
def test_the_claim_column_on_the_fused_layer_list(pname):
    verdicts = set()
    for case in FS.cases_of(pname, planes=SC.PLANES[:1]):  # the fusion pass does not look at the plane
        for level, kw in FS.LEVELS:
            net = _net((case.param, case.weights), level, dilated=case.dilated, **kw)
            v = FS.check_claim(case, level, net)
            verdicts |= {v["p"], v["c"]}
            net.close()
    if pname in FS.ZERO_PADS:
        assert "folded" in verdicts
    if pname in FS.SHUFFLES:
        assert "absorbed" in verdicts


def test_a_default_net_refuses_every_case():
    from feathercnn_amd import FeatherHipError
    from feathercnn_amd.net import Net
    case = FS.build_case("conv3x3", "pad_same", SC.PLANES[0])
    with pytest.raises(FeatherHipError, match="code -200"):
        Net().LoadParam(case.param)


def test_a_depthwise_layer_with_a_channel_multiplier_is_refused():
    """ps2 -> gconv3 (3 channels, group 3, 12 filters) loaded and ran as a depthwise layer with 3 output channels, nine of its twelve filters
    unread by the kernel: the pair is Incompatible now because LoadParam refuses the layer, and a plain depthwise layer still loads."""
    from feathercnn_amd import FeatherHipError, model_zoo
    from feathercnn_amd.net import Net
    for cout, refused in ((12, True), (3, False)):
        g = model_zoo.GraphBuilder(5)
        g.conv("dw", g.input("data", 3, 6, 6), 3, cout, 3, 1, 1, group=3)
        param, weights = g.finish()
        net = Net()
        if refused:
            with pytest.raises(FeatherHipError, match="code -200") as e:
                net.LoadParam(param)
            assert "layer dw" in str(e.value) and "channel multiplier" in str(e.value), str(e.value)
        else:
            net.LoadParam(param)
            net.LoadWeights(weights)
        net.close()
    assert ("ps2", "gconv3") in FS.INCOMPATIBLE and ("ps2m1", "gconv3") in FS.INCOMPATIBLE


# ---- the fold table ----------------------------------------------------------------------------------------------------------------------
def test_the_fold_table_claims_own_pads_plus_margins():
    ids = [n.id for n in FF.nets()]
    assert len(ids) == len(set(ids)) and len(FF.ROWS) >= 20
    used = {n.m for n in FF.nets()}
    assert set(FF.MARGINS) <= used and FF.LEFT_TAP in {n.m for row in ("dw3s1p1", "dw3s2p1") for n in FF.ROWS[row]}
    for n in FF.nets():
        assert n.exists(), n.id
        t, b, l, r = n.m
        for level, kw in FF.SETTINGS:
            c = n.claim(level, kw.get("tuned", False))
            assert c["folded"] == (n.folds and level >= 2), (n.id, level)
            assert c["pads"] == ((n.p + t, n.p + b, n.p + l, n.p + r) if c["folded"] else (n.p, n.p, n.p, n.p)), (n.id, level, c["pads"])
        # the convolution as written, behind the Padding, and the folded one give one output plane
        hp, wp = n.padded()
        assert n.out_plane() == (FF.conv_out(hp, n.k, n.s, n.p, n.p), FF.conv_out(wp, n.k, n.s, n.p, n.p)), n.id
    # every plan kind the rows exist for is claimed by some row at some setting, and declined by another
    claims = [(n, level, n.claim(level, kw.get("tuned", False))) for n in FF.nets() for level, kw in FF.SETTINGS]
    assert {c["algo"] for _, _, c in claims} == {"WINOGRADF63", "IM2COL", "DEPTHWISE", "GCONV"}
    assert {c["pool_fast"] for _, _, c in claims} == {None, True, False} and {c["residual"] for _, _, c in claims} == {0, 1, 2}
    assert {c["pair"] for _, _, c in claims} == {None, True, False}
    chains = {tuple(sorted(c["chain"].items())) for _, _, c in claims}
    assert chains == {(), (("a", (0, 1)), ("k", (1, 0))), (("b", (1, 0)), ("k", (0, 1))), (("b", (2, 0)), ("k", (0, 2)))}, chains
    assert any(n.tail == "pw72" and c["pair"] is None and level >= 2 for n, level, c in claims)  # the pair the fold takes away
    assert any(n.row == "first" and level == 3 and not c["chain"] for n, level, c in claims)  # the first layer the planner declines


@pytest.mark.parametrize("row", sorted(FF.ROWS))
def test_the_fold_rows_on_the_fused_layer_list_and_in_float64(row):
    for n in FF.ROWS[row]:
        param, weights, outputs = n.model()
        ref = R.Net(param, weights)
        assert ref.read == len(weights), n.id
        blobs = ref.run("data", n.input(max(FF.BATCHES)), keep=True)
        oh, ow = n.out_plane()
        assert blobs["k"].shape[2:] == (oh, ow), (n.id, blobs["k"].shape)
        for o in outputs:
            y = blobs[o].astype(np.float64)
            peak = np.abs(y).max(axis=(2, 3))
            assert np.isfinite(y).all() and peak.min() >= ALIVE * peak.max(), (n.id, o, float(peak.min() / peak.max()))
        for level, kw in FF.SETTINGS[:3]:
            net = _net((param, weights), level, kw.get("tuned", False))
            names = [nm for _, nm, _ in net.layers()]
            c = n.claim(level, kw.get("tuned", False))
            assert ("pad" not in names) == c["folded"] and "k" in names, (n.id, level, names)
            for gone in ("pool", "sum", "relu", "bn", "scale", "pw"):
                if gone in [l[1] for l in ref.layers]:
                    assert (gone not in names) == (gone in c["gone"]), (n.id, level, gone, names)
            net.close()
