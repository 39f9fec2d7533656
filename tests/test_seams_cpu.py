"""The seam table and its float64 evaluator without a GPU.

* tests/seam_ref.py agrees with every family's own restatement on that family's models (the tiny nets, and ResNeXt-50, the style-transfer
  and U-Net generators and the ShuffleNets at their smallest input), blob for blob, to 1e-12 relative in float64: it composes their
  functions, so anything above rounding noise is a composition mistake;
* with oracle.netcheck.PortNet (float32 accumulation) on tiny_allsorts and on every case of the table whose layer types PortNet runs, to
  the float32 rounding of PortNet's sums: n * 2^-24 with n = 300 + 300, the terms of the two largest layers a case can chain (5x5 on 12
  channels), on the normalised scale -- 3.6e-5;
* every case of the table builds, parses and evaluates, reads its whole .bin, and every output plane of the float64 result reaches 1e-3 of
  the tensor's maximum, so that the per-plane metric of tests/test_seams_gpu.py is defined everywhere;
* every type string create_layer accepts is on both sides of the table (Input, which has no bottom, on the producers' side only)."""
import os
import re

import numpy as np
import pytest

import atrous_ref
import deconv_ref
import gate_ref
import gconv_ref
import helpers
import inorm_ref
import seam_cases as SC
import seam_ref as R
import shuffle_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PORT_TYPES = {"Input", "Convolution", "ConvolutionDepthWise", "ReLU", "Pooling", "InnerProduct", "BatchNorm", "Scale", "Eltwise", "Concat", "Split",
              "Dropout", "Softmax"}
PORT_TOL = 600 * 2.0 ** -24
ALIVE = 1e-3

FAMILIES = [("tiny_grouped", gconv_ref), ("resnext50_32x4d", gconv_ref), ("tiny_deconv", deconv_ref), ("style_transfer", deconv_ref),
            ("unet_k4", deconv_ref), ("tiny_generative", inorm_ref), ("style_transfer_in", inorm_ref), ("pix2pix_unet", inorm_ref),
            ("tiny_shuffle", shuffle_ref), ("shufflenet_v2_x1_0", shuffle_ref), ("shufflenet_v1_g3", shuffle_ref), ("tiny_dilated", atrous_ref),
            ("tiny_se", gate_ref)]
# the full-size nets at the smallest input their strides allow: five stride-2 levels down to one pixel, or a quarter-resolution trunk
SIZES = {"shufflenet_v2_x1_0": 32, "shufflenet_v1_g3": 32, "resnext50_32x4d": 32, "unet_k4": 32, "pix2pix_unet": 32, "style_transfer": 16,
         "style_transfer_in": 16}


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    m = float(np.abs(b).max())
    return float(np.abs(a - b).max()) / (m if m > 0 else 1.0)


@pytest.mark.parametrize("name,family", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_agrees_with_the_family_restatement(name, family):
    from feathercnn_amd import model_zoo
    size = SIZES.get(name)
    param, weights, inp, out = model_zoo.MODELS[name](**({"size": size} if size else {}))
    c, h = [(pd[2], pd[1]) for t, _, _, _, pd in R.Net(param, weights).layers if t == "Input"][0]
    x = np.random.default_rng(5).normal(0, 1, (2, c, h, h)).astype(np.float32)
    want = family.Net(param, weights).run(inp, x, out, keep=True)
    mine = R.Net(param, weights)
    got = mine.run(inp, x, out, keep=True)
    assert mine.read == len(weights)
    assert set(want) <= set(got)
    worst = max(_rel(got[k], want[k]) for k in want)
    print(f"{name}: {len(want)} blobs, worst relative difference {worst:.1e}")
    for k in want:
        assert got[k].shape == want[k].shape and _rel(got[k], want[k]) <= 1e-12, (name, k)


def test_agrees_with_portnet_on_tiny_allsorts():
    from feathercnn_amd import model_zoo
    from oracle.netcheck import PortNet
    param, weights, inp, out = model_zoo.tiny_allsorts()
    x = np.random.default_rng(6).normal(0, 1, (2, 3, 20, 20)).astype(np.float32)
    want = PortNet(param, weights).run(inp, x, out, keep=True)
    got = R.Net(param, weights).run(inp, x, out, keep=True)
    for k in want:
        assert _rel(got[k], want[k]) <= PORT_TOL, k


_RESULTS = {}


def _beyond_portnet(layer):
    """A layer of a type PortNet has in a form it does not run: a leaky ReLU, a partial group, a two-bottom Scale."""
    type_, _, bottoms, _, pd = layer
    if type_ == "ReLU":
        return pd.get(0, 0.0) != 0.0
    if type_ in ("Convolution", "ConvolutionDepthWise"):
        group = pd.get(7, 1)
        cin = pd.get(6, 0) // pd.get(0, 1) // pd.get(1, 1) ** 2 * group
        return 1 < group < cin
    return R._gated(type_, bottoms, pd)


def _evaluate(pname):
    if pname not in _RESULTS:
        rows = []
        for case in SC.cases_of(pname):
            net = R.Net(case.param, case.weights)
            rows.append((case, net, net.run("data", case.input(), keep=True)))
        _RESULTS[pname] = rows
    return _RESULTS[pname]


@pytest.mark.parametrize("pname", list(SC.PRODUCERS))
def test_every_case_evaluates_and_every_output_plane_is_alive(pname):
    rows = _evaluate(pname)
    assert len(rows) >= len(SC.PLANES) * 20, (pname, len(rows))  # no row may lose most of its consumers to Incompatible
    for case, net, blobs in rows:
        assert net.read == len(case.weights), case.id
        assert case.c_first in [l[1] for l in net.layers] and case.p_top in blobs, case.id
        for o in case.outputs:
            y = blobs[o].astype(np.float64)
            assert y.ndim == 4 and y.shape[0] == SC.BATCH and np.isfinite(y).all(), (case.id, o)
            peak = np.abs(y).max(axis=(2, 3))
            assert peak.min() >= ALIVE * peak.max(), (case.id, o, float(peak.min() / peak.max()))
        # one image alone gives that image's planes: what the batch-1 pass of the GPU test relies on
        alone = net.run("data", case.input()[:1], keep=True)
        assert np.array_equal(alone[case.c_top], blobs[case.c_top][:1]), case.id


@pytest.mark.parametrize("pname", list(SC.PRODUCERS))
def test_agrees_with_portnet_where_portnet_knows_the_layers(pname):
    from oracle.netcheck import PortNet
    ran, worst = 0, 0.0
    for case, net, blobs in _evaluate(pname):
        types = {l[0] for l in net.layers}
        if not types <= PORT_TYPES or case.dilated or any(_beyond_portnet(l) for l in net.layers):
            continue
        want = PortNet(case.param, case.weights).run("data", case.input(), case.c_top, keep=True)
        for o in case.outputs:
            e = _rel(blobs[o], want[o])
            worst = max(worst, e)
            assert e <= PORT_TOL, (case.id, o, e)
        ran += 1
    print(f"{pname}: {ran} cases against PortNet, worst {worst:.1e}")
    assert ran or pname in ("leaky", "gconv3", "dil3x3", "split_gconv3", "split_dil3x3") or not SC.build_case(pname, "tanh", SC.PLANES[0]).p_types <= PORT_TYPES


def test_the_table_is_complete():
    text = helpers.net_runtime_source()
    body = text[text.index("static Layer* create_layer("):]
    body = body[:body.index("\n}\n")]
    accepted = set(re.findall(r'type == "(\w+)"', body))
    assert len(accepted) >= 25 and {"Convolution", "BinaryOp", "ShuffleChannel", "InstanceNorm"} <= accepted, accepted
    produced, consumed = set(), set()
    for pname in SC.PRODUCERS:
        produced |= SC.build_case(pname, "tanh", SC.PLANES[0]).p_types
    for cname in SC.CONSUMERS:
        consumed |= SC.build_case("conv3x3", cname, SC.PLANES[0]).c_types
    assert SC.build_case("input", "tanh", SC.PLANES[0]).p_top in ("data", "tap_0")
    produced.add("Input")  # P = the input blob itself: the layer writes no line of its own in the P phase
    assert accepted - produced == set(), accepted - produced
    assert accepted - consumed == {"Input"}, accepted - consumed  # a layer without a bottom cannot consume


def test_the_claim_column_fires_and_refuses_every_rule():
    fired, refused = set(), set()
    for pname in SC.PRODUCERS:
        for cname in SC.CONSUMERS:
            try:
                SC.build_case(pname, cname, SC.PLANES[0])
            except SC.Incompatible:
                continue
            for level, _ in SC.LEVELS:
                verdict, rule = SC.expect(pname, cname, level)
                assert verdict in ("absorbed", "kept", "collapsed", None) and (rule is None or rule in SC.RULES)
                if rule and level >= 2:
                    (refused if verdict == "kept" else fired).add(rule)
    assert fired == set(SC.RULES) and refused == set(SC.RULES), (fired, refused)
