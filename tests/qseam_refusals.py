"""Refusals with a positive control: for each planner rule one small net in which an int8 layer sits where the rule would fire, and its
fp32 TWIN -- the same builder calls and seed with quantisation off (tests/test_qseams_cpu.py asserts that nothing else differs).  The twin
must fire the rule at that shape and setting, which is what makes the int8 net's refusal mean something; the int8 net must not, must
equal the restatement layer by layer and meet the float64 evaluation behind it (tests/test_qseams_gpu.py).

Shapes: the smallest at which the twin fires, from the rule's own condition (the C-ABI predicates are host code; test_qseams_cpu.py asks
them again, and the GPU test asserts the firing on the planner's answers):
  pool       16 -> 16 3x3 + 2x2 max pooling, 4 x 4, level 2          ConvLayer::Fuse takes the pooling whatever the shape (an even plane)
  residual   16 -> 16 3x3 + Eltwise with an earlier 1x1 branch, 4 x 4, level 2      fuse_layers' residual rule: structural
  dwpw       depthwise 3x3 on 16 channels -> 1x1 to 72 (inside 65 .. 159), 4 x 4, batch 3, level 2
             fhip_conv_can_fuse_dw_pw: W % 4 == 0, and not at batch 1 on this plane; mixes int8 / fp32, fp32 / int8, int8 / int8
  siblings   two 1x1 layers 16 -> 128 and 16 -> 72 on one blob, 3 x 4, batch 3, level 2
             fhip_conv_can_fuse_siblings: the first layer's outputs a multiple of 128, both above 64, more than 32 columns (3 * 12 = 36)
  chain      fp32 3x3 -> int8 3x3 -> fp32 3x3 on 16 channels, 4 x 4, level 3 + tuned
             tuned selection takes Winograd from 4 pixels up and fhip_conv_can_chain_winograd chains a plane of one F(6,3) tile (4 .. 6)
  first      3 -> 16 3x3 pad 1 -> 16 -> 16 3x3, 4 x 4, level 3 + tuned      fhip_conv_can_fuse_first_winograd: an even width, from 4 up
             (a) the first layer int8, (b) the Winograd layer int8
  se         both spellings of se_block on 16 channels (reduction to 4), 4 x 4, level 2, the first / second / both dense layers int8
             collapse_gate_blocks: structural
  concurrency (concurrency_net, no twin: the property is concurrency=True == concurrency=False bit for bit)

FOLD_EDGES: level 2, exact -- an int8 convolution without a bias + a Scale without one, the same + BatchNorm, an int8 depthwise layer +
BatchNorm + Scale + ReLU, and a layer one of whose filters is all zero (s_w = 0, d = 0) + a Scale with a bias, + BatchNorm + ReLU.
"""
from __future__ import annotations

import zlib

import numpy as np

from feathercnn_amd import model_zoo

BATCH = 3
# variant tag -> salt of the seed: the first whose float64 result keeps every compared plane at 2e-2 of its tensor's maximum (6e-3 from 72
# channels); tests/test_qseams_cpu.py asserts the floor, and no variant has needed one
SALT = {}


def setting(level, kw):
    return f"{level}" + "".join(f"+{k}" for k in ("tuned", "concurrency", "graph") if kw.get(k))


class Variant:
    def __init__(self, tag, level, kw, shape, build, qset, fired, refused, batches=(BATCH, 1)):
        self.tag, self.level, self.kw, self.shape, self.qset, self.batches = tag, level, kw, shape, qset, batches
        self.fired, self.refused, self._build = fired, refused, build
        self._nets = None

    def seed(self):
        return zlib.crc32(f"refusal/{self.tag}/{SALT.get(self.tag, 0)}".encode()) % (1 << 31)

    def _make(self, on):
        g = model_zoo.GraphBuilder(self.seed())
        outputs = self._build(g, self.shape, lambda name: bool(on and name in self.qset))
        return g.finish(), list(outputs)

    def _both(self):
        if self._nets is None:
            (q, outputs), (t, _) = self._make(True), self._make(False)
            self._nets = (q, t, outputs)
        return self._nets

    quant = property(lambda self: self._both()[0])
    twin = property(lambda self: self._both()[1])
    outputs = property(lambda self: self._both()[2])

    def input(self):
        return np.random.default_rng(self.seed() + 1).normal(0, 1, (BATCH,) + self.shape).astype(np.float32)


def _names(net):
    return [n for _, n, _ in net.layers()]


def _index(net, name):
    return _names(net).index(name)


def _int8_alone(net, qset):
    """Every int8 layer is a layer of its own on its route, with no mark of a plan on it."""
    info = net.layers()
    for n in qset:
        assert (n, "QCONV") in [(nm, a) for _, nm, a in info], (n, info)
    idx = {_index(net, n) for n in qset}
    for answer in (net.residuals(), net.siblings(), net.chains(raw=True), net.fused_pointwise()):
        assert not idx & set(answer), (qset, answer)


# ---- the nets: build(g, shape, q) -> outputs; q(name) is the layer's `quant=` ------------------------------------------------------------
def _b_pool(g, shape, q):
    c, h, w = shape
    x = g.input("data", c, h, w)
    x = g.conv("conv", x, c, c, 3, 1, 1, quant=q("conv"))
    return [g.pool("pool", x, 2, 2)]


def _b_residual(g, shape, q):
    c, h, w = shape
    a, b = g.split("tap", g.input("data", c, h, w))
    br = g.conv("br", a, c, c, 1)
    x = g.conv("conv", b, c, c, 3, 1, 1, quant=q("conv"))
    return [g.eltwise("sum", x, br)]


def _b_dwpw(g, shape, q):
    c, h, w = shape
    x = g.input("data", c, h, w)
    x = g.conv("dw", x, c, c, 3, 1, 1, group=c, quant=q("dw"))
    return [g.conv("pw", x, c, 72, 1, quant=q("pw"))]


def _b_siblings(g, shape, q):
    c, h, w = shape
    a, b = g.split("tap", g.input("data", c, h, w))
    return [g.conv("sib_a", a, c, 128, 1, quant=q("sib_a")), g.conv("sib_b", b, c, 72, 1, quant=q("sib_b"))]


def _b_chain(g, shape, q):
    c, h, w = shape
    x = g.input("data", c, h, w)
    for name in ("c1", "c2", "c3"):
        x = g.conv(name, x, c, c, 3, 1, 1, quant=q(name))
    return [x]


def _b_first(g, shape, q):
    c, h, w = shape
    x = g.input("data", c, h, w)
    x = g.conv("first", x, c, 16, 3, 1, 1, quant=q("first"))
    return [g.conv("wino", x, 16, 16, 3, 1, 1, quant=q("wino"))]


def _b_se(spelling):
    d1, d2 = ("se_fc1", "se_fc2") if spelling == "caffe" else ("se_conv1", "se_conv2")

    def build(g, shape, q):
        c, h, w = shape
        x = g.input("data", c, h, w)
        return [g.se_block("se", x, c, 4, spelling, mact="relu" if spelling == "caffe" else "swish", quant=(q(d1), q(d2)))]
    return build, d1, d2


# ---- what "fired" and "refused" mean, on the planner's answers ---------------------------------------------------------------------------
def _gone(name):
    def fired(net):
        assert name not in _names(net), (name, net.layers())
    return fired


def _kept(names, qset):
    def refused(net):
        assert all(n in _names(net) for n in names), (names, net.layers())
        _int8_alone(net, qset)
    return refused


def _fired_residual(net):
    assert net.residuals() and "sum" not in _names(net), (net.residuals(), net.layers())


def _refused_residual(net):
    assert not net.residuals() and "sum" in _names(net), (net.residuals(), net.layers())
    _int8_alone(net, {"conv"})


def _fired_dwpw(net):
    fp = net.fused_pointwise()
    assert list(fp) == [_index(net, "dw")] and fp[_index(net, "dw")][1] and "pw" not in _names(net), (fp, net.layers())  # one kernel


def _refused_dwpw(qset):
    def refused(net):
        assert not net.fused_pointwise() and {"dw", "pw"} <= set(_names(net)), (net.fused_pointwise(), net.layers())
        _int8_alone(net, qset)
    return refused


def _fired_siblings(net):
    assert net.siblings() == {_index(net, "sib_a"): 1, _index(net, "sib_b"): 2}, net.siblings()


def _refused_siblings(qset):
    def refused(net):
        assert not net.siblings(), net.siblings()
        _int8_alone(net, qset)
    return refused


def _fired_chain(net):
    ch = net.chains()
    assert ch == {_index(net, "c1"): (False, True), _index(net, "c2"): (True, True), _index(net, "c3"): (True, False)}, ch


def _refused_chain(net):
    assert _index(net, "c2") not in net.chains(raw=True) and not net.chains(), net.chains(raw=True)
    _int8_alone(net, {"c2"})


def _fired_first(net):
    ch = net.chains(raw=True)
    assert ch.get(_index(net, "first")) == (0, 2) and ch.get(_index(net, "wino"), (0, 0))[0] == 2, ch


def _refused_first(qset):
    def refused(net):
        ch = net.chains(raw=True)
        assert not any(2 in v for v in ch.values()) and _index(net, "first") not in ch, ch
        _int8_alone(net, qset)
    return refused


def _fired_se(net):
    assert ("Pooling", "se_gap", "GATE") in net.layers(), net.layers()


def _refused_se(d1, d2, qset):
    def refused(net):
        info = net.layers()
        assert ("Pooling", "se_gap", "GATE") not in info and {"se_gap", d1, d2} <= {n for _, n, _ in info}, info
        _int8_alone(net, qset)
    return refused


def _refusals():
    L2, L3 = (2, {}), (3, {"tuned": True})
    out = {
        "pool": [Variant("pool", *L2, (16, 4, 4), _b_pool, {"conv"}, _gone("pool"), _kept(["conv", "pool"], {"conv"}))],
        "residual": [Variant("residual", *L2, (16, 4, 4), _b_residual, {"conv"}, _fired_residual, _refused_residual)],
        "dwpw": [Variant(f"dwpw/{'+'.join(sorted(qs))}", *L2, (16, 4, 4), _b_dwpw, qs, _fired_dwpw, _refused_dwpw(qs)) for qs in ({"dw"}, {"pw"}, {"dw", "pw"})],
        "siblings": [Variant(f"siblings/{'+'.join(sorted(qs))}", *L2, (16, 3, 4), _b_siblings, qs, _fired_siblings, _refused_siblings(qs))
                     for qs in ({"sib_a", "sib_b"}, {"sib_a"}, {"sib_b"})],
        "chain": [Variant("chain", *L3, (16, 4, 4), _b_chain, {"c2"}, _fired_chain, _refused_chain)],
        "first": [Variant(f"first/{n}", *L3, (3, 4, 4), _b_first, {n}, _fired_first, _refused_first({n})) for n in ("first", "wino")],
        "se": [],
    }
    for spelling in ("caffe", "converter"):
        build, d1, d2 = _b_se(spelling)
        for qs in ({d1}, {d2}, {d1, d2}):
            out["se"].append(Variant(f"se/{spelling}/{'+'.join(sorted(qs))}", *L2, (16, 4, 4), build, qs, _fired_se, _refused_se(d1, d2, qs)))
    return out


REFUSALS = _refusals()


# ---- concurrency ----------------------------------------------------------------------------------------------------------------------
def concurrency_net():
    """-> (param, weights, outputs, x): two branches off a Split -- an int8 3x3 convolution whose only consumer, the Eltwise, stands three
    layers further down, with a fp32 convolution and its TanH in between (a TanH, so that the convolution cannot take the add into its
    epilogue and become the int8 layer's next reader) -- then an int8 1x1 layer and a second output off the joined blob."""
    g = model_zoo.GraphBuilder(zlib.crc32(b"refusal/concurrency") % (1 << 31))
    a, b = g.split("tap", g.input("data", 16, 11, 9))
    qa = g.relu("qa_relu", g.conv("qa", a, 16, 16, 3, 1, 1, quant=True))
    cb = g.tanh("cb_tanh", g.conv("cb", b, 16, 16, 3, 1, 1))
    s1, s2 = g.split("joined", g.eltwise("sum", cb, qa))
    outs = [g.conv("q_tail", s1, 16, 72, 1, quant=True), g.relu("f_tail_relu", g.conv("f_tail", s2, 16, 16, 3, 1, 1))]
    x = np.random.default_rng(77).normal(0, 1, (BATCH, 16, 11, 9)).astype(np.float32)
    return g.finish() + (outs, x)


# ---- fold edges -----------------------------------------------------------------------------------------------------------------------
def _fold_net(tag, build):
    def make():
        g = model_zoo.GraphBuilder(zlib.crc32(f"fold/{tag}".encode()) % (1 << 31))
        x = g.input("data", 16, 11, 9)
        top, zero = build(g, x)
        param, weights = g.finish()
        return param, weights, [top], np.random.default_rng(5).normal(0, 1, (BATCH, 16, 11, 9)).astype(np.float32), zero
    return make


def _zero_filter(g, start, k, per, cout, bias):
    """Filter k of the int8 layer written at offset `start` of the .bin becomes all zero, with the weight scale quantize_weights gives it."""
    w0 = start + 4 + k * per
    g.bin[w0:w0 + per] = bytes(per)
    s0 = start + 4 + (cout * per + 3) // 4 * 4 + (4 * cout if bias else 0) + 4 * k
    g.bin[s0:s0 + 4] = np.float32(0).tobytes()


def _f_zero(relu):
    def build(g, x):
        start = len(g.bin)
        y = g.conv("conv", x, 16, 16, 3, 1, 1, bias=False, quant=True)
        _zero_filter(g, start, 5, 16 * 9, 16, False)
        at = len(g.bin)
        if relu:  # BatchNorm: slope, mean, var, bias -> add = bias - slope * mean / sqrt(var + eps); made negative on channel 5: its ReLU is 0
            y = g.bn("aff1", y, 16)
            g.bin[at + 4 * (48 + 5):at + 4 * (48 + 6)] = np.float32(-0.25).tobytes()
            return g.relu("relu", y), (5, 0.0)
        y = g.scale("aff1", y, 16, bias=True)
        add = np.frombuffer(bytes(g.bin[at + 4 * (16 + 5):at + 4 * (16 + 6)]), "<f4")[0]
        return y, (5, float(add))
    return build


FOLD_EDGES = {
    "nobias+scale_nobias": _fold_net("a", lambda g, x: (g.scale("aff1", g.conv("conv", x, 16, 16, 3, 1, 1, bias=False, quant=True), 16, bias=False), None)),
    "nobias+bn": _fold_net("b", lambda g, x: (g.bn("aff1", g.conv("conv", x, 16, 16, 3, 1, 1, bias=False, quant=True), 16), None)),
    "dw+bn+scale+relu": _fold_net("c", lambda g, x: (g.relu("relu", g.scale("aff2", g.bn("aff1", g.conv("dw", x, 16, 16, 3, 1, 1, group=16, quant=True), 16), 16)), None)),
    "zero_filter+scale": _fold_net("d", _f_zero(False)),
    "zero_filter+bn+relu": _fold_net("e", _f_zero(True)),
}
