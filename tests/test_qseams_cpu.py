"""The int8 seam table (tests/qseam_cases.py), its re-based evaluator (tests/qseam_ref.py) and the refusal nets (tests/qseam_refusals.py)
without a GPU: the per-layer `quant=` of GraphBuilder leaves every existing model byte for byte as it was (hashes taken from the builder
before the change); the table holds every int8 op on both sides, every producer and consumer of seam_cases or an Incompatible, and its
int8 layers reach all six kernels of qconv_cases by fhip_qconv_route; every compared plane of the float64 result keeps the floor; the
evaluator reproduces qconv_ref.net_forward on tiny_quant bit for bit at levels 0, 1 and 2; every twin differs from its int8 net in the
quantisation alone, and the host predicates accept the twins' shapes."""
import ctypes
import hashlib

import numpy as np
import pytest

import lifecycle_cases as LC
import qconv_cases as QK
import qconv_ref
import qseam_cases as QC
import qseam_ref as QR
import qseam_refusals as QF
import seam_cases as SC
import seam_ref as R
from feathercnn_amd import model_zoo

# sha256 (16 hex digits) over .param and .bin, taken with the GraphBuilder before it had a per-layer `quant=`, and over seam_cases before
# its Build had a channel count
BEFORE = {"tiny_quant": "6751d4ee387916f6", "tiny_allsorts": "b73e64d75441486b", "tiny_se": "6b187dcf7124eb49", "vgg16_int8 (dry)": "a6259756900af082",
          "seam_cases": (3480, "4f0dcdb9105ae43f")}
LIFECYCLE_BEFORE = ("36bd7ddd8c7b8841", 1008032)  # lifecycle_cases.model(): sha256 of the .param, bytes of the .bin


def _h(*parts, digits=16):
    m = hashlib.sha256()
    for p in parts:
        m.update(p if isinstance(p, (bytes, bytearray)) else repr(p).encode())
    return m.hexdigest()[:digits]


def test_existing_builds_are_byte_identical():
    assert _h(*model_zoo.tiny_quant()[:2]) == BEFORE["tiny_quant"]
    assert _h(*model_zoo.tiny_allsorts()[:2]) == BEFORE["tiny_allsorts"]
    assert _h(*model_zoo.tiny_se()[:2]) == BEFORE["tiny_se"]
    assert _h(*model_zoo.vgg16_int8(dry=True)[:2]) == BEFORE["vgg16_int8 (dry)"]
    # lifecycle_cases.model(): the .param, and the size of the .bin -- its calibration scales the filters by float64 statistics whose last
    # bits belong to the numpy build, so the bytes themselves are no constant
    param, weights, _, _ = LC.model()
    assert (_h(param), len(weights)) == LIFECYCLE_BEFORE
    # every case of seam_cases: id, files, input, outputs and the claim column
    m, n = hashlib.sha256(), 0
    for p in SC.PRODUCERS:
        for c in SC.cases_of(p):
            for part in (c.id, c.param, c.weights, c.input().tobytes(), c.outputs, c.p_top, [SC.expect(c.pname, c.cname, lv) for lv, _ in SC.LEVELS]):
                m.update(part if isinstance(part, bytes) else repr(part).encode())
            n += 1
    assert (n, m.hexdigest()[:16]) == BEFORE["seam_cases"]


def test_quant_keyword_writes_the_layer_of_the_whole_build_switch():
    """conv(quant=True) / fc(quant=True) in a fp32 build write what the same call writes in a quant={} build; quant=False in a quant={}
    build writes the fp32 layer; a number is the input scale."""
    def build(whole, per, scale=None):
        g = model_zoo.GraphBuilder(3, quant=whole)
        x = g.input("data", 16, 5, 5)
        x = g.conv("a", x, 16, 16, 3, 1, 1, quant=per)
        g.fc("b", x, 16 * 25, 7, quant=per if scale is None else scale)
        return g.finish()
    assert build(None, True) == build({}, None) and build({}, False) == build(None, None) == build(None, False)
    assert build(None, True, 8.0) == build({"b": 8.0}, None)
    p, w = build(None, True)
    assert p.count(b" 8=1") == 2
    for spelling, names in (("caffe", ("s_fc1", "s_fc2")), ("converter", ("s_conv1", "s_conv2"))):
        for sel in ((True, False), (False, True), (True, True)):
            g = model_zoo.GraphBuilder(3)
            g.se_block("s", g.input("data", 16, 4, 4), 16, 4, spelling, quant=sel)
            rows = {r.split()[1]: r for r in g.finish()[0].decode().splitlines()[2:]}
            assert [rows[n].endswith(" 8=1") for n in names] == list(sel), (spelling, sel)


# ---- the table --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def table():
    """[(case, seam_ref.Net, blobs of the evaluation at level 0)] for every case of the table: built and evaluated once."""
    out = []
    for row in QC.rows():
        for case in QC.cases_of(row):
            net = R.Net(case.param, case.weights)
            assert net.read == len(case.weights), case.id
            out.append((case, net, QR.own(net, case.input(), 0)))
    return out


def test_table_is_complete(table):
    built = {(c.pname, c.cname) for c, _, _ in table}
    rows = QC.rows()
    assert len(rows) == len(SC.PRODUCERS) + 2 * len(QC.QOPS) and all(any(True for _ in QC.cases_of(r)) for r in ("gconv4->q", "split_gconv4->q"))
    for op in QC.QOPS:  # every int8 op on both sides, behind an int8 op too, and with a second consumer
        assert ("conv3x3", op) in built and (op, "conv3x3") in built and ("split_" + op, "conv3x3") in built and ("q3x3", op) in built, op
    missing = []
    swap = lambda n: n.replace("gconv3", "gconv4")  # group 3 does not divide 16 channels: qseam_cases' stand-in
    assert set(QC.FP_PRODUCERS) == {swap(p) for p in SC.PRODUCERS} and set(QC.FP_CONSUMERS) == {swap(c) for c in SC.CONSUMERS}
    for p in QC.FP_PRODUCERS:
        for op in QC.QOPS:
            if (p, op) not in built:
                missing.append((p, op))
    for op in list(QC.QOPS) + ["split_" + o for o in QC.QOPS]:
        for c in QC.FP_CONSUMERS:
            if (op, c) not in built:
                missing.append((op, c))
    for p, c in missing:  # absent means Incompatible on both planes, nothing else
        for plane in QC.PLANES:
            with pytest.raises(QC.Incompatible):
                QC.build_case(p, c, plane)
    # no producer and no consumer drops out as a whole
    assert all(any((p, op) in built for op in QC.QOPS) for p in QC.FP_PRODUCERS) and all(any((op, c) in built for op in QC.QOPS) for c in QC.FP_CONSUMERS)
    ids = [c.id for c, _, _ in table]
    assert len(ids) == len(set(ids)) and all(k in ids for k in QC.SALT), [k for k in QC.SALT if k not in ids]
    for case, net, _ in table:  # both planes of every pair that exists on one... or Incompatible there
        assert len(QR.int8_indices(net)) == (case.pname.removeprefix("split_") in QC.QOPS) + (case.cname in QC.QOPS), case.id


def test_every_int8_kernel_is_reached(table):
    from feathercnn_amd import _lib
    lib = _lib.load_qconv_library()
    seen = {}
    for case, net, blobs in table:
        for i in QR.int8_indices(net):
            type_, name, bottoms, _, pd = net.layers[i]
            n, c, h, w = case.input().shape if bottoms[0] == "data" else blobs[bottoms[0]].shape
            if type_ == "InnerProduct":
                c, h, w, k, kk, s, p, group, bias = c * h * w, 1, 1, pd[0], 1, 1, 0, 1, pd.get(1, 0)
            else:
                k, kk, s, p, group, bias = pd[0], pd[1], pd.get(3, 1), pd.get(4, 0), pd.get(7, 1), pd.get(5, 0)
            q = _lib.fhip_qconv_param(output_channels=k, input_channels=c, input_h=h, input_w=w, kernel_h=kk, kernel_w=kk, stride_h=s, stride_w=s,
                                      pad_left=p, pad_right=p, pad_top=p, pad_bottom=p, group=group, bias_term=bias, activation=0, dilation_h=1,
                                      dilation_w=1, int8_scale_term=1)
            assert lib.fhip_qconv_assign_output_dim(ctypes.byref(q)) == 0
            assert lib.fhip_qconv_supported(ctypes.byref(q)) == 1, (case.id, name, lib.fhip_qconv_last_error())
            buf = ctypes.create_string_buffer(160)
            assert lib.fhip_qconv_route(ctypes.byref(q), buf, 160) == 0
            seen.setdefault(buf.value.decode(), case.id)
    assert set(seen) == {QK.MFMA128, QK.MFMA64, QK.GENERIC, QK.GENERIC16, QK.DW1, QK.DW2}, seen


def _floor(blobs, names):
    worst = (np.inf, None)
    for o in names:
        v = blobs.get(o)
        if v is None:  # inside an int8 layer's fusion at some level: not compared
            continue
        v = np.abs(v.astype(np.float64))
        worst = min(worst, (v.max(axis=(2, 3)).min() / v.max() / (QC.FLOOR_WIDE if v.shape[1] >= 72 else QC.FLOOR), o))
    return worst


def test_plane_floors(table):
    low = []
    for case, _, blobs in table:
        f, o = _floor(blobs, list(case.outputs) + [case.p_top])
        if not f >= 1.0:
            low.append((case.id, o, f))
    assert not low, (len(low), low[:20])
    for vs in QF.REFUSALS.values():
        for v in vs:
            f, o = _floor(QR.own(R.Net(*v.quant), v.input(), v.level), v.outputs)
            assert f >= 1.0, (v.tag, o, f)


def test_claims_cover_the_table(table):
    """The claim column agrees with the evaluator's own plan (qseam_ref.plan) for the layer behind an int8 P, at every level."""
    for case, net, _ in table:
        if case.pname.removeprefix("split_") not in QC.QOPS:
            assert QC.expect(case.pname, case.cname, 2) == ("kept", None)
            continue
        i = [j for j in QR.int8_indices(net) if net.layers[j][1] == "p"][0]
        first = [l[1] for l in net.layers].index(case.c_first)
        for level, _ in QC.LEVELS:
            verdict, _ = QC.expect(case.pname, case.cname, level)
            gone = QR.plan(net, i, level)
            assert (first in gone) == (verdict == "absorbed"), (case.id, level, verdict, gone)
            assert all(net.layers[j][1].startswith("c") for j in gone), (case.id, level, gone)


# ---- the evaluator ----------------------------------------------------------------------------------------------------------------------
class _Recorded:
    """A stand-in device: the blobs of qconv_ref.net_forward; the layer list that fusion `level` leaves by the rules of qseam_ref.plan."""

    def __init__(self, net, blobs, level):
        self.blobs = blobs
        gone = {j for i in QR.int8_indices(net) for j in QR.plan(net, i, level)}
        self.info = [(l[0], l[1], "QCONV" if R.is_int8(l) else None) for j, l in enumerate(net.layers) if j not in gone]

    def layers(self):
        return self.info

    def Extract(self, name):
        return self.blobs[name]


def test_evaluator_reproduces_net_forward_on_tiny_quant():
    model = model_zoo.tiny_quant()
    net = R.Net(model[0], model[1])
    assert net.read == len(model[1]) and sorted(net.q) == sorted(model_zoo.QUANT_LAYERS["tiny_quant"])
    x = np.random.default_rng(11).uniform(-1, 1, (3, 3, 16, 16)).astype(np.float32)
    for level in (0, 1, 2):
        want = qconv_ref.net_forward(model, x, level)
        # fed the recorded blobs: every int8 layer, with what the level absorbed, bit for bit (int8_layers asserts it); the fp32 layers
        # behind them within the float64 tolerance
        given = QR.int8_layers(net, x, _Recorded(net, want, level), level)
        assert sum(v is not None for v in given.values()) == 6
        blobs = net.run("data", x, keep=True, given=given)
        for name, v in want.items():
            if blobs.get(name) is not None:
                assert R.plane_nerr(blobs[name], v) <= 1e-4, (level, name)
        # fed its own blobs: bit for bit up to the first fp32 layer that rounds (BatchNorm / Scale, which level 2 folds away)
        mine = QR.own(net, x, level)
        exact = list(want) if level == 2 else ["data", "conv1", "relu1", "conv2", "relu2", "conv3"]
        for name in exact:
            if name in want and name in mine:
                assert np.array_equal(mine[name], want[name]), (level, name)
        # (the evaluator keeps no blob inside a fusion, net_forward keeps the ReLU fusions' -- they do not change a bit)
        assert level != 2 or (set(mine) <= set(want) and {"relu1", "relu2", "conv3_relu", "relu_dw", "relu_pw", "pool", "fc"} <= set(mine))


def test_evaluator_notices_one_wrong_value_and_one_wrong_plan():
    """The comparison can fail: one output of one int8 layer off by one float32 step, a ReLU the level does not absorb missing from the
    layer list, an int8 layer missing from it (adopted by a neighbour), an int8 layer on another route."""
    model = model_zoo.tiny_quant()
    net = R.Net(model[0], model[1])
    x = np.random.default_rng(12).uniform(-1, 1, (2, 3, 16, 16)).astype(np.float32)
    for level in (0, 2):
        want = qconv_ref.net_forward(model, x, level)
        dev = _Recorded(net, want, level)
        QR.int8_layers(net, x, dev, level)
        top = "relu_dw" if level else "dw"
        off = dict(want)
        off[top] = want[top].copy()
        at = np.unravel_index(np.argmax(off[top]), off[top].shape)
        off[top][at] = np.nextafter(off[top][at], np.float32(np.inf))
        with pytest.raises(AssertionError, match="1 of .* values differ"):
            QR.int8_layers(net, x, _Recorded(net, off, level), level)
        # a ReLU that level 0 keeps is gone; an int8 layer is gone (it then reads as absorbed by the int8 layer in front of it)
        for drop, message in ((("relu_dw", "absorbed"),) if level == 0 else ()) + (("pw", "absorbed|not a layer of its own"), ("conv1", "not a layer of its own")):
            wrong = _Recorded(net, want, level)
            wrong.info = [r for r in wrong.info if r[1] != drop]
            with pytest.raises(AssertionError, match=message):
                QR.int8_layers(net, x, wrong, level)
        wrong = _Recorded(net, want, level)
        wrong.info = [(t, n, "IM2COL" if n == "conv2" else a) for t, n, a in wrong.info]
        with pytest.raises(AssertionError):
            QR.int8_layers(net, x, wrong, level)


def test_given_blobs_leave_every_other_caller_as_it_was():
    case = SC.build_case("conv3x3", "relu", SC.PLANES[0])
    net, x = R.Net(case.param, case.weights), case.input()
    a = net.run("data", x, keep=True)
    b = net.run("data", x, keep=True, given={})
    assert all(np.array_equal(a[k], b[k]) for k in a) and not net.q
    marked = np.full_like(a["p"], 2.0)
    c = net.run("data", x, keep=True, given={"p": marked})  # P is skipped, C starts from the given blob
    assert np.array_equal(c["p"], marked) and np.array_equal(c["c"], marked)
    q = QC.build_case("conv3x3", "q3x3", QC.PLANES[0])
    with pytest.raises(RuntimeError, match="must be given"):
        R.Net(q.param, q.weights).run("data", q.input(), keep=True)


# ---- the refusals ---------------------------------------------------------------------------------------------------------------------
def test_twins_differ_in_the_quantisation_only():
    tags = []
    for name, variants in QF.REFUSALS.items():
        for v in variants:
            tags.append(v.tag)
            (qp, qw), (tp, tw) = v.quant, v.twin
            qrows, trows = qp.decode().splitlines(), tp.decode().splitlines()
            assert len(qrows) == len(trows)
            flagged = set()
            for a, b in zip(qrows, trows):
                if a != b:
                    assert a == b + " 8=1", (v.tag, a, b)
                    flagged.add(a.split()[1])
            assert flagged == set(v.qset), (v.tag, flagged)
            qn, tn = R.Net(qp, qw), R.Net(tp, tw)
            assert qn.read == len(qw) and tn.read == len(tw) and set(qn.q) == set(v.qset) and not tn.q
            for lname, w in tn.w.items():
                if lname not in qn.q:
                    assert all(np.array_equal(a, b) for a, b in zip(w, qn.w[lname]) if a is not None), (v.tag, lname)
                    continue
                q = qn.q[lname]  # the same filters, quantised by the one rule; the same bias; the default input scale
                wq, s_w = model_zoo.quantize_weights(w[0], w[0].shape[0])
                assert np.array_equal(wq.reshape(q["wq"].shape), q["wq"]) and np.array_equal(s_w, q["s_w"]), (v.tag, lname)
                assert np.array_equal(w[1], q["b"]) and q["s_in"] == model_zoo.QUANT_DEFAULT_SCALE, (v.tag, lname)
    assert len(tags) == len(set(tags)) and set(QF.REFUSALS) == {"pool", "residual", "dwpw", "siblings", "chain", "first", "se"}
    assert [sorted(v.qset) for v in QF.REFUSALS["dwpw"]] == [["dw"], ["pw"], ["dw", "pw"]]
    assert len(QF.REFUSALS["se"]) == 6 and len(QF.REFUSALS["siblings"]) == 3 and len(QF.REFUSALS["first"]) == 2


def test_twin_shapes_are_the_smallest_the_host_predicates_accept():
    from feathercnn_amd import _lib
    lib = _lib.load_library()
    ref = ctypes.byref

    def conv(c, k, h, w, kk=3, p=1, group=1):
        q = _lib.fhip_conv_param(output_channels=k, input_channels=c, input_h=h, input_w=w, kernel_h=kk, kernel_w=kk, stride_h=1, stride_w=1,
                                 pad_left=p, pad_right=p, pad_top=p, pad_bottom=p, group=group, bias_term=1, activation=0)
        lib.fhip_conv_assign_output_dim(ref(q))
        return q

    def algo(q, tuned):
        a = ctypes.c_int()
        assert (lib.fhip_conv_select_algo_tuned if tuned else lib.fhip_conv_select_algo)(ref(q), ref(a)) == 0
        return a.value

    def chains(h, w):
        a = conv(16, 16, h, w)
        return lib.fhip_conv_can_chain_winograd(ref(a), algo(a, True), ref(a), algo(a, True), 0)

    def first(h, w, n):
        f, b = conv(3, 16, h, w), conv(16, 16, h, w)
        return lib.fhip_conv_can_fuse_first_winograd(ref(f), ref(b), algo(b, True), n)

    def siblings(h, w, n, ka=128, kb=72):
        a, b = conv(16, ka, h, w, 1, 0), conv(16, kb, h, w, 1, 0)
        return lib.fhip_conv_can_fuse_siblings(ref(a), algo(a, False), ref(b), algo(b, False), n)

    def dwpw(h, w, n):
        d, p = conv(16, 1, h, w, group=16), conv(16, 72, h, w, 1, 0)
        return lib.fhip_conv_can_fuse_dw_pw(ref(d), ref(p), n)

    assert QF.REFUSALS["chain"][0].shape == (16, 4, 4) and chains(4, 4) and not chains(3, 3)
    assert QF.REFUSALS["first"][0].shape == (3, 4, 4) and first(4, 4, 3) and first(4, 4, 1) and not first(3, 3, 3) and not first(2, 2, 3)
    assert QF.REFUSALS["siblings"][0].shape == (16, 3, 4) and siblings(3, 4, 3) and not siblings(3, 3, 3) and not siblings(3, 4, 1)
    assert not siblings(3, 4, 3, 72, 72) and not siblings(3, 4, 3, 64, 128)  # the first layer's outputs: a multiple of 128
    assert QF.REFUSALS["dwpw"][0].shape == (16, 4, 4) and dwpw(4, 4, 3) and not dwpw(4, 4, 1) and not dwpw(3, 3, 3)
