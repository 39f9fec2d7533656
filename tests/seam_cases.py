"""The table of two-layer seams: every net `Input -> P -> C` with P from PRODUCERS and C from CONSUMERS, and what feather::Net's planner
must do at that seam (tests/test_seams_cpu.py, tests/test_seams_gpu.py).

Shapes: 12 channels (divisible by 2, 3 and 4; slices as 5 + 7; `Build(c0=...)` builds the same nets on another count for
tests/qseam_cases.py), the planes 11 x 9 (odd, W % 4 != 0) and 12 x 8 (W % 4 == 0), batch 3, then
batch 1 through the same handle.  Inputs are normal(0, 1); weights are GraphBuilder's (He-uniform times `gain`), biases non-zero.

A layer with two bottoms takes its other operand from the input through a 1x1 convolution (`branch`), written BEFORE P in the layer list
so that the residual rule (an add with an EARLIER blob) can fire; the branch reaches the input's plane or, with stride 2, the halved one.
A pair is no case (`Incompatible`) where no such net exists:
  * the other operand of an Eltwise / Concat would need a plane the branch cannot reach (behind a Deconvolution, a 3x3 / stride-2 pooling,
    a global pooling or an InnerProduct);
  * the channel count does not divide (group 3 or a shuffle on Slice's 7 channels) or a plane would be empty.
Behind a global average pooling or an InnerProduct a plane is ONE value of either sign, and a plain ReLU would leave half of them exact
zeros, where the per-plane metric has nothing to normalise by: gap->relu draws its input as normal(0.5, 1) (the plane means, of standard
deviation 0.1, are then positive) and ip->relu gives its InnerProduct biases in (0.05, 0.15) (POSITIVE).
`Input` cannot be a consumer (it has no bottom); every other type create_layer accepts is on both sides.

`expect(case, level)` is the claim column, filled from the conditions of the Net runtime (net_layers.h, net_plan.h: ConvLayer::Fuse, DeconvLayer::Fuse, AffineLayer::Fuse,
InstanceNormLayer::Fuse, InnerProductLayer::Fuse, EltwiseLayer::Fuse, fuse_layers' residual rule, collapse_channel_maps,
collapse_gate_blocks): (verdict, rule) with verdict "absorbed" (C's first layer is gone from the layer list), "kept" (it is there),
"collapsed" (C is a squeeze-and-excitation block that became one layer) or None (no claim).
"""
from __future__ import annotations

import math
import zlib

import numpy as np

from feathercnn_amd import model_zoo

C0 = 12
PLANES = ((11, 9), (12, 8))
BATCH = 3
SE_R = 4
LEVELS = ((0, {}), (1, {}), (2, {}), (3, {"tuned": True}), (3, {"tuned": True, "graph": True}))
RULES = ("affine_main", "affine_side", "relu", "pool", "dwpw", "residual", "maps", "se")


class Incompatible(Exception):
    pass


def conv_out(size, k, s, p, d=1):
    return (size + 2 * p - (d * (k - 1) + 1)) // s + 1


def pool_out(size, k, s, p):  # oracle.netcheck._pool / pooling_layer.h: ceil
    return int(math.ceil(np.float32(size + 2 * p - k) / np.float32(s))) + 1


def _need(ok):
    if not ok:
        raise Incompatible


class Build:
    """One pass over a case.  The first pass is dry: it counts the taps of the input and notes the branches C asks for, whose shapes follow
    from P's top; the second writes Input, the Split of the input, the branches, P and C in that order."""

    def __init__(self, plane, seed, plan=None, c0=C0):
        self.h0, self.w0 = plane
        self.c0 = c0  # the channel count of the input and of every full-width layer (tests/qseam_cases.py builds the same nets on 16)
        self.plan = plan
        self.g = model_zoo.GraphBuilder(seed, dry=plan is None)
        self.taps, self.requests, self.made = 0, [], {}
        self.phase = "b"
        self.types = {"p": set(), "c": set(), "b": set()}
        self.names = {"p": [], "c": [], "b": []}
        inner = self.g.layer

        def layer(type_, name, bottoms, tops, params=None):
            self.types[self.phase].add(type_)
            self.names[self.phase].append(name)
            return inner(type_, name, bottoms, tops, params)

        self.g.layer = layer
        self.tap_tops = []
        self.positive_bias = False  # ip->relu: see POSITIVE
        self.p_scale = 1.0  # the magnitude of P's top where it is far from one (Softmax): a Concat's other operand is scaled to match

    def start(self):
        data = self.g.input("data", self.c0, self.h0, self.w0)
        if self.plan is None:
            return
        self.tap_tops = [data] if self.plan.taps <= 1 else list(self.g.split("tap", data, self.plan.taps))
        for spec in self.plan.requests:
            self.made[spec] = self._branch(spec, len(self.made))

    def tap(self):
        self.taps += 1
        return "data" if self.plan is None else self.tap_tops[self.taps - 1]

    def _branch(self, spec, i):
        kind, c, h, w, gain = spec
        x = self.tap()
        if kind == "gate":  # [n][c][1][1] in (0, 1)
            y = self.g.conv(f"br{i}", x, self.c0, c, 1)
            return self.g.sigmoid(f"br{i}_sig", self.g.pool(f"br{i}_gap", y, 1, 1, avg=True, global_=True))
        s = 1 if (h, w) == (self.h0, self.w0) else 2
        return self.g.conv(f"br{i}", x, self.c0, c, 1, s, gain=gain)

    def branch(self, kind, c, h=1, w=1, gain=1.0):
        """The other operand of a two-bottom consumer: a blob of shape (c, h, w) ("conv") or a gate (c, 1, 1) ("gate") from the input."""
        if kind == "conv":
            _need((h, w) in ((self.h0, self.w0), (conv_out(self.h0, 1, 2, 0), conv_out(self.w0, 1, 2, 0))))
        spec = (kind, c, h, w, gain)
        if self.plan is None:
            self.requests.append(spec)
            self.taps += 1
            return f"br{len(self.requests) - 1}"
        return self.made[spec]


# ---- layers with one bottom, usable on both sides: fn(b, name, x, (c, h, w)) -> (top, (c, h, w)) ----------------------------------------
def _conv(k, s, p, group=None, dilation=1, cout=None):
    def fn(b, n, x, shp, cout=cout):
        c, h, w = shp
        cout = cout or b.c0
        grp = {None: 1, "dw": c}.get(group, group)
        _need(group == "dw" or (c % grp == 0 and cout % grp == 0))
        ko = c if group == "dw" else cout
        _need(grp != c or ko == c)  # group == channels is a depthwise layer, which has one filter per channel: the runtime refuses a multiplier
        ho, wo = conv_out(h, k, s, p, dilation), conv_out(w, k, s, p, dilation)
        _need(ho >= 1 and wo >= 1)
        return b.g.conv(n, x, c, ko, k, s, p, group=grp, dilation=dilation), (ko, ho, wo)
    return fn


def _deconv(dw):
    def fn(b, n, x, shp):
        c, h, w = shp
        return b.g.deconv(n, x, c, c if dw else b.c0, 4, 2, 1, group=c if dw else 1), (c if dw else b.c0, 2 * h, 2 * w)
    return fn


def _pool(k, s, p, avg=False, global_=False):
    def fn(b, n, x, shp):
        c, h, w = shp
        if global_:
            return b.g.pool(n, x, 1, 1, avg=avg, global_=True), (c, 1, 1)
        ho, wo = pool_out(h, k, s, p), pool_out(w, k, s, p)
        _need(ho >= 1 and wo >= 1 and (ho - 1) * s - 2 * p < h and (wo - 1) * s - 2 * p < w)  # no empty window
        return b.g.pool(n, x, k, s, p, avg=avg), (c, ho, wo)
    return fn


def _same(make):
    return lambda b, n, x, shp: (make(b.g, n, x, shp[0]), shp)


def _slice2(b, n, x, shp):
    c, h, w = shp
    _need(c >= 2)
    first = 5 if c == b.c0 else c // 2
    return b.g.slice(n, x, [first, c - first])[1], (c - first, h, w)  # the second piece: a non-zero channel offset


def _shuffle(b, n, x, shp):
    group = 3 if shp[0] % 3 == 0 else 2
    _need(shp[0] % group == 0)
    return b.g.shuffle(n, x, group), shp


def _se(spelling):
    def fn(b, n, x, shp):
        return b.g.se_block(n, x, shp[0], SE_R, spelling, mact="relu" if spelling == "caffe" else "swish"), shp
    return fn


def _ip(b, n, x, shp):
    c, h, w = shp
    # gain 0.01: the value of a plane is bias + sum with |bias| <= 0.1 and a sum of order 0.01, so that no plane is the small difference
    # of large float32 partial sums.  A plane here is ONE value and plane_nerr its relative error: at gain 1 a value at the floor of
    # 1e-3 of the maximum carries the rounding of a 1188-term float32 sum a thousand times enlarged, beyond 1e-4 whatever the kernel.
    # A wrong weight still moves the value by several per cent.  It also keeps |y| below 2.5, where a HardSigmoid behind it clamps.
    top = b.g.fc(n, x, c * h * w, b.c0, gain=0.01)
    if b.positive_bias and n == "p" and not b.g.dry:  # the biases are the last c0 floats written: U(-0.1, 0.1) -> 0.05 + |U|
        bias = np.frombuffer(bytes(b.g.bin[-4 * b.c0:]), "<f4")
        b.g.bin[-4 * b.c0:] = (np.abs(bias) + np.float32(0.05)).astype("<f4").tobytes()
    return top, (b.c0, 1, 1)


def _softmax(b, n, x, shp):
    b.p_scale = 0.005  # one of c * h * w shares of 1
    return b.g.softmax(n, x), shp


UNARY = {
    "conv3x3": _conv(3, 1, 1), "conv1x1": _conv(1, 1, 0), "conv3x3s2": _conv(3, 2, 1), "conv5x5": _conv(5, 1, 2), "dw3x3": _conv(3, 1, 1, "dw"),
    "gconv3": _conv(3, 1, 1, 3), "dil3x3": _conv(3, 1, 2, dilation=2),
    "deconv4": _deconv(False), "deconvdw": _deconv(True),
    "maxpool2": _pool(2, 2, 0), "maxpool3s2": _pool(3, 2, 0), "avgpool3s2p1": _pool(3, 2, 1, avg=True),
    "gap": _pool(0, 0, 0, avg=True, global_=True), "gmp": _pool(0, 0, 0, global_=True),
    "slice2": _slice2, "shuffle": _shuffle,
    "inorm": _same(lambda g, n, x, c: g.instance_norm(n, x, c)), "bn": _same(lambda g, n, x, c: g.bn(n, x, c)),
    "scale_bias": _same(lambda g, n, x, c: g.scale(n, x, c, bias=True)), "scale_nobias": _same(lambda g, n, x, c: g.scale(n, x, c, bias=False)),
    "relu": _same(lambda g, n, x, c: g.relu(n, x)), "leaky": _same(lambda g, n, x, c: g.relu(n, x, 0.2)),
    "prelu": _same(lambda g, n, x, c: g.prelu(n, x, c)), "sigmoid": _same(lambda g, n, x, c: g.sigmoid(n, x)),
    "tanh": _same(lambda g, n, x, c: g.tanh(n, x)), "clip": _same(lambda g, n, x, c: g.clip(n, x, -1.0, 1.0)),
    "swish": _same(lambda g, n, x, c: g.swish(n, x)), "hsigmoid": _same(lambda g, n, x, c: g.hard_sigmoid(n, x)),
    "dropout": _same(lambda g, n, x, c: g.dropout(n, x, 0.5)),
    "se_caffe": _se("caffe"), "se_conv": _se("converter"),
    "ip": _ip, "softmax": _softmax,
}
CONVS = ("conv3x3", "conv1x1", "conv3x3s2", "conv5x5", "dw3x3", "gconv3", "dil3x3")


# ---- producers: fn(b) -> (top, shape) ------------------------------------------------------------------------------------------------------
def _p_unary(op):
    return lambda b: UNARY[op](b, "p", b.tap(), (b.c0, b.h0, b.w0))


def _p_input(b):
    return b.tap(), (b.c0, b.h0, b.w0)


def _p_eltsum(b):
    # the operand written last is no convolution: one would take the add into its epilogue at level 2 and P would be no Eltwise layer
    a = b.g.conv("p_a", b.tap(), b.c0, b.c0, 1)
    c = b.g.tanh("p_b", b.tap())
    return b.g.eltwise("p", a, c), (b.c0, b.h0, b.w0)


def _p_concat(b):
    a = b.g.conv("p_a", b.tap(), b.c0, 5, 1)
    c = b.g.conv("p_b", b.tap(), b.c0, b.c0 - 5, 1)
    return b.g.concat("p", [a, c]), (b.c0, b.h0, b.w0)


PRODUCERS = {"input": _p_input, "eltsum": _p_eltsum, "concat": _p_concat}
PRODUCERS.update({op: _p_unary(op) for op in UNARY})
PRODUCERS.update({"split_" + op: _p_unary(op) for op in CONVS})  # P's top gets a second consumer (build_case)


# ---- consumers: fn(b, x, shape) -> (top, shape) ----------------------------------------------------------------------------------------
def _c_unary(op):
    return lambda b, x, shp: UNARY[op](b, "c", x, shp)


def _c_elt(first):
    def fn(b, x, shp):
        other = b.branch("conv", *shp)
        return b.g.eltwise("c", *((x, other) if first else (other, x))), shp
    return fn


def _c_concat(b, x, shp):
    c, h, w = shp
    return b.g.concat("c", [x, b.branch("conv", 4, h, w, gain=b.p_scale)]), (c + 4, h, w)


def _c_gated(scale_by):
    def fn(b, x, shp):
        gate = b.branch("gate", shp[0])
        return (b.g.scale_by("c", x, gate) if scale_by else b.g.binary_mul("c", x, gate)), shp
    return fn


def _c_gate_source(scale_by):
    def fn(b, x, shp):
        c = shp[0]
        gate = b.g.sigmoid("c_sig", b.g.pool("c", x, 1, 1, avg=True, global_=True))
        full = b.branch("conv", c, b.h0, b.w0)
        # BinaryOp with the gate FIRST among its bottoms (the order a two-bottom Scale cannot have)
        return (b.g.scale_by("c_mul", full, gate) if scale_by else b.g.binary_mul("c_mul", gate, full)), (c, b.h0, b.w0)
    return fn


CONSUMERS = {op: _c_unary(op) for op in UNARY}
CONSUMERS.update({"pw72": lambda b, x, shp: _conv(1, 1, 0, cout=72)(b, "c", x, shp), "elt_first": _c_elt(True), "elt_second": _c_elt(False),
                  "concat": _c_concat, "binop_gated": _c_gated(False), "scaleby_gated": _c_gated(True),
                  "binop_gate": _c_gate_source(False), "scaleby_gate": _c_gate_source(True)})

# A plain ReLU behind one-value planes of either sign would zero half of them (see the module docstring): the mean of the input that keeps
# a global average positive, and the pair whose InnerProduct gets positive biases.
INPUT_MEAN = {("gap", "relu"): 0.5}
POSITIVE = {("ip", "relu")}
# Cases whose first draw left an output plane below 1e-3 of the tensor's maximum in the float64 result (a plane of ONE value -- behind a
# global pooling or an InnerProduct -- that happened to fall next to zero), or no more than twice that floor, where the plane's relative
# error is the float32 rounding of its sum enlarged five hundred times or more; and the one-value-plane cases that came within a factor of
# two of the limit on the device for the same reason (a plane at 2e-3 .. 3e-3 of the maximum).  Each is drawn again with this salt in the
# seed of weights and input, chosen as the first that lifts its smallest plane to 2e-2 of the maximum (6e-3 for the 216 planes of pw72).
SALT = {"conv3x3->gap@11x9": 1, "conv3x3->ip@12x8": 1, "conv3x3s2->gap@12x8": 2, "conv5x5->ip@12x8": 3, "dw3x3->gap@12x8": 4,
        "eltsum->ip@11x9": 6, "gap->binop_gated@12x8": 1, "gap->conv1x1@12x8": 1, "gap->conv3x3@11x9": 1, "gap->dropout@11x9": 1,
        "gap->dropout@12x8": 1, "gap->dw3x3@12x8": 1, "gap->leaky@12x8": 27, "gap->pw72@11x9": 8, "gap->pw72@12x8": 7,
        "gap->scale_bias@11x9": 3, "gap->scale_nobias@12x8": 1, "gap->scaleby_gated@11x9": 1, "gap->se_caffe@11x9": 2,
        "gap->se_conv@11x9": 1, "gmp->conv1x1@11x9": 1, "gmp->conv3x3@12x8": 1, "gmp->conv3x3s2@12x8": 1, "gmp->pw72@11x9": 1,
        "gmp->se_conv@11x9": 1, "ip->binop_gated@12x8": 1, "ip->leaky@11x9": 1, "ip->pw72@11x9": 2, "ip->se_caffe@12x8": 1,
        "ip->se_conv@12x8": 2, "shuffle->gap@12x8": 1, "sigmoid->ip@12x8": 2, "split_conv3x3->ip@11x9": 1,
        "split_conv5x5->ip@11x9": 1, "split_dil3x3->gap@12x8": 2, "split_gconv3->gap@11x9": 7, "split_gconv3->gap@12x8": 1,
        "tanh->gap@12x8": 3}


class Case:
    def __init__(self, pname, cname, plane, param, weights, b, p_top, c_top, outputs):
        self.pname, self.cname, self.plane = pname, cname, plane
        self.param, self.weights = param, weights
        self.p_top, self.c_top, self.outputs = p_top, c_top, outputs
        self.p_types, self.c_types = b.types["p"], b.types["c"]
        self.p_names, self.c_names = b.names["p"], b.names["c"]
        self.c_first = b.names["c"][0]
        self.dilated = "dil3x3" in (pname.removeprefix("split_"), cname)  # such a net needs Net.SetDilated(True)
        self.id = f"{pname}->{cname}@{plane[0]}x{plane[1]}"

    def input(self, batch=BATCH):
        seed = zlib.crc32(f"{self.id}/{SALT.get(self.id, 0)}".encode())
        return np.random.default_rng(seed).normal(INPUT_MEAN.get((self.pname, self.cname), 0.0), 1, (batch, C0) + self.plane).astype(np.float32)


def _one_pass(pname, cname, plane, seed, plan):
    b = Build(plane, seed, plan)
    b.positive_bias = (pname, cname) in POSITIVE
    b.start()
    b.phase = "p"
    p_top, shp = PRODUCERS[pname](b)
    x, outputs = p_top, []
    if pname.startswith("split_"):
        x, rejoin = b.g.split("p_split", p_top)
    b.phase = "c"
    c_top, cshp = CONSUMERS[cname](b, x, shp)
    outputs.append(c_top)
    if pname.startswith("split_"):
        b.phase = "b"
        # the second consumer rejoins behind C through an Eltwise where the shapes allow it (C's top may then be absorbed into the add: the
        # sum is the output), else it ends in a layer of its own
        outputs = [b.g.eltwise("join", c_top, rejoin)] if cshp == shp else [c_top, b.g.relu("side", rejoin)]
    return b, p_top, c_top, outputs


def build_case(pname, cname, plane):
    """-> Case, or raises Incompatible."""
    salt = SALT.get(f"{pname}->{cname}@{plane[0]}x{plane[1]}", 0)
    seed = zlib.crc32(f"{pname}/{cname}/{plane}/{salt}".encode()) % (1 << 31)
    plan, _, _, _ = _one_pass(pname, cname, plane, seed, None)
    b, p_top, c_top, outputs = _one_pass(pname, cname, plane, seed, plan)
    assert b.taps == plan.taps and all(b.names[k] == plan.names[k] for k in "pc"), (pname, cname)
    param, weights = b.g.finish()
    return Case(pname, cname, plane, param, weights, b, p_top, c_top, outputs)


def cases_of(pname, planes=PLANES):
    for cname in CONSUMERS:
        for plane in planes:
            try:
                yield build_case(pname, cname, plane)
            except Incompatible:
                continue


# ---- the claim column --------------------------------------------------------------------------------------------------------------------
PTAG = {"conv3x3": "conv", "conv1x1": "conv", "conv3x3s2": "conv", "conv5x5": "conv", "dw3x3": "dw", "gconv3": "side", "dil3x3": "side",
        "deconv4": "deconv", "deconvdw": "deconv", "inorm": "inorm", "bn": "bn", "scale_bias": "scale", "scale_nobias": "scale", "ip": "ip",
        "shuffle": "map", "slice2": "map", "concat": "cat", "eltsum": "elt", "se_caffe": "se", "se_conv": "se"}
CTAG = {"relu": "relu", "leaky": "leaky", "bn": "affine", "scale_bias": "affine", "scale_nobias": "affine", "maxpool2": "pool2",
        "maxpool3s2": "poolx", "avgpool3s2p1": "poolx", "gap": "poolx", "gmp": "poolx", "conv1x1": "pw12", "pw72": "pw72",
        "elt_first": "elt", "elt_second": "elt", "shuffle": "map", "slice2": "map", "concat": "cat", "se_caffe": "se", "se_conv": "se",
        "scaleby_gated": "gscale", "binop_gated": "gscale"}
CONVLIKE = ("conv", "dw", "side", "deconv")


def expect(pname, cname, level):
    """(verdict, rule): see the module docstring.  `rule` names the rule of RULES the case fires (verdict absorbed / collapsed) or is a near
    miss of (verdict kept); None where the case is neither."""
    if pname.startswith("split_"):
        verdict, rule = expect(pname.removeprefix("split_"), cname, level)
        # P's only consumer is the Split, which nothing absorbs; C's own collapse does not depend on P
        return ("kept", rule) if verdict == "absorbed" else (verdict, rule)
    pt, ct = PTAG.get(pname, "none"), CTAG.get(cname, "other")
    affine_rule = {"conv": "affine_main", "dw": "affine_main", "side": "affine_side", "deconv": "affine_side"}.get(pt)
    if ct == "se":
        return ("collapsed" if level >= 2 else "kept"), "se"
    if ct == "relu":  # every layer with an epilogue takes the plain ReLU
        takes = level >= 1 and pt in CONVLIKE + ("inorm", "bn", "scale", "elt", "ip")
        return ("absorbed" if takes else "kept"), ("relu" if pt in CONVLIKE else None)
    if ct == "leaky":  # only InstanceNorm has a leaky epilogue
        return ("absorbed" if level >= 1 and pt == "inorm" else "kept"), ("relu" if pt in CONVLIKE else None)
    if ct == "affine":
        if pt == "bn" and cname.startswith("scale") and level >= 1:
            return "absorbed", None  # BatchNorm -> Scale folding
        if affine_rule:
            return ("absorbed" if level >= 2 else "kept"), affine_rule
        return "kept", None
    if ct == "gscale":  # a two-bottom Scale / BinaryOp is no affine map: nothing folds it
        return "kept", (affine_rule if level >= 2 else None)
    if ct == "pool2":
        if pt in ("conv", "dw"):
            return ("absorbed" if level >= 2 else "kept"), "pool"
        return "kept", ("pool" if pt == "side" and level >= 2 else None)  # the grouped and dilated routes have no pooled epilogue
    if ct == "poolx":
        return "kept", ("pool" if pt in ("conv", "dw") and level >= 2 else None)
    if ct == "pw72":
        return ("absorbed" if pt == "dw" and level >= 2 else "kept"), ("dwpw" if pt == "dw" else None)
    if ct == "pw12":  # 12 output channels: outside fhip_conv_can_fuse_dw_pw's range (65 .. 159 at stride 1)
        return "kept", ("dwpw" if pt == "dw" and level >= 2 else None)
    if ct == "elt":
        if pname == "input":
            return None, None  # the BRANCH convolution may take the add with the input
        if pt in ("conv", "dw"):
            return ("absorbed" if level >= 2 else "kept"), "residual"
        if pt == "se":
            return ("absorbed" if level >= 2 else "kept"), None  # into the collapsed block
        return "kept", ("residual" if pt == "side" and level >= 2 else None)
    if ct == "map":
        if pt in ("map", "cat"):
            return ("absorbed" if level >= 2 else "kept"), "maps"
        return "kept", None
    if ct == "cat":
        if pt == "map":
            return ("absorbed" if level >= 2 else "kept"), "maps"
        return "kept", ("maps" if pt == "cat" and level >= 2 else None)  # a run of Concat layers alone is left as it is
    if pname == "gap" and cname == "ip":
        return "kept", ("se" if level >= 2 else None)  # global average Pooling -> InnerProduct that is no squeeze-and-excitation block
    if pt == "map":
        return "kept", ("maps" if level >= 2 else None)  # a consumer that needs a dense blob: the channel map runs as its own layer
    return None, None


def check_claim(case, level, net):
    """Assert the claim on a net that has run Forward; -> (rule, fired) for the summary, or None."""
    verdict, rule = expect(case.pname, case.cname, level)
    if verdict is None:
        return None
    info = net.layers()
    names = [n for _, n, _ in info]
    if verdict == "collapsed":
        dense = "c_fc1" if case.cname == "se_caffe" else "c_conv1"
        assert ("Pooling", "c_gap", "GATE") in info and dense not in names, (case.id, level, info)
    elif verdict == "absorbed":
        assert case.c_first not in names, (case.id, level, info)
        if rule == "residual":
            assert net.residuals(), (case.id, level)
        if rule == "dwpw":
            assert net.fused_pointwise(), (case.id, level)
    else:
        assert case.c_first in names, (case.id, level, info)
        if case.pname.startswith("split_"):
            assert "p" in names and not net.fused_pointwise(), (case.id, level, info)
        if rule == "maps":  # the refusal: P still runs as a layer of its own, a channel map on the SHUFFLE route or a plain Concat
            own = {"shuffle": ("ShuffleChannel", "p", "SHUFFLE"), "slice2": ("Slice", "p", "SHUFFLE"), "concat": ("Concat", "p", None)}
            assert own[case.pname] in info, (case.id, level, info)
    return None if rule is None else (rule, verdict != "kept")
