"""The two-layer seams of the framing layers Padding, Crop and PixelShuffle (Net.SetFrame()): every net `Input -> P -> C` with one of them on
one side and, on the other, a layer of tests/seam_cases.py's table or another framing layer (tests/test_frame_seams_cpu.py,
tests/test_frame_seams_gpu.py).

Built as tests/resample_seam_cases.py builds its pairs: tests/seam_cases.py's Build passes, shapes (12 channels, planes 11 x 9 and 12 x 8,
batch 3 then batch 1 through the same handle), branches for two-bottom consumers, Incompatible rule and SALT rule, with the tables extended
in this module's own dictionaries -- the three types are not in create_layer, so tests/seam_cases.py does not (and must not) hold them.

New layers, usable on both sides (margins as (top, bottom, left, right)):
  pad_same     zero Padding (0, 1, 0, 1): TensorFlow's "SAME" in front of a stride-2 layer
  pad_sym1     zero Padding (1, 1, 1, 1)
  pad_value    constant 0.5, margins (1, 0, 2, 1)
  pad_rep      replicate (1, 2, 0, 3)
  pad_reflect  reflect (2, 1, 3, 0)
  pad_pc       per-channel values in the .bin, (1, 1, 1, 1): a weight reader between its neighbours' weights
  pad_ch       channel margins, front 1 and behind 2 (12 -> 15 channels), value 0.5 (a zero plane would have nothing to normalise by)
  pad_none     all margins 0: a no-op, its top aliases its bottom
  crop_in      woffset 1, hoffset 2, woffset2 1
  crop_c       coffset 2, outc 8
  crop_none    the whole blob: a no-op
  ps2          PixelShuffle r = 2, mode 0 (12 -> 3 channels)
  ps2m1        r = 2, mode 1
  ps1          r = 1: a no-op
and as a consumer only:
  crop_like    the two-bottom Crop; its reference is a stride-2 branch with 4 channels, whose (c, h, w) the top takes

`expect(pname, cname, level)` -> {"p": verdict, "c": verdict}: the claim on the framing layer of either side (None where that side holds
none), filled from fold_zero_paddings, ConvLayer::FoldPadding, PaddingLayer::zero_pad_margins and PixelShuffleLayer::Fuse:
  "folded"    level >= 2, P a plain zero Padding (pad_same, pad_sym1, pad_none: type 0, value +0.0, no per-channel values, no channel margins)
              and C a Convolution / ConvolutionDepthWise on the main or the grouped route: the Padding is gone from net.layers(), its top
              refuses Extract, the convolution reports its own pads plus the margins;
  "absorbed"  level >= 2, P a PixelShuffle and C a ReLU, plain or leaky: C is gone and P's top is the activation of the shuffle;
  "alias"     the layer stays and changes nothing (pad_none, crop_none, ps1): ExtractDevice of its top and of its bottom give one address;
  "kept"      the layer stays and owns its top.
A Padding with a non-zero value, a replicate or reflect border, per-channel values or channel margins is never folded; nor is a zero Padding
in front of dil3x3 (the dilated route), a Deconvolution or anything that is no convolution.  PixelShuffle in front of a PReLU keeps both
layers (a PReLU has per-channel slopes; relu_slope() is a ReLU layer's).  Every framing layer that stays reports the route FRAME, and no
other layer does.
"""
from __future__ import annotations

import zlib

import numpy as np

import resample_seam_cases as RS
import seam_cases as SC

LEVELS = ((0, {}), (2, {}), (3, {"tuned": True}))
FRAME_TYPES = {"Padding", "Crop", "PixelShuffle"}
REF_C = 4  # channels of crop_like's reference


def _pad(margins, **kw):
    def fn(b, n, x, shp):
        c, h, w = shp
        t, bo, l, r = margins
        if kw.get("type_") == 2:
            SC._need(max(t, bo) < h and max(l, r) < w)  # a reflect pad must be smaller than the plane it pads
        extra = dict(kw)
        if extra.pop("pc", False):
            extra["per_channel"] = c
        top = b.g.padding(n, x, t, bo, l, r, **extra)
        return top, (c + kw.get("front", 0) + kw.get("behind", 0), h + t + bo, w + l + r)
    return fn


def _crop(woffset=0, hoffset=0, coffset=0, outc=None, woffset2=0):
    def fn(b, n, x, shp):
        c, h, w = shp
        oc = c - coffset if outc is None else outc
        SC._need(coffset + oc <= c and oc >= 1 and h - hoffset >= 1 and w - woffset - woffset2 >= 1)
        return b.g.crop(n, x, woffset, hoffset, coffset, outc=outc, woffset2=woffset2), (oc, h - hoffset, w - woffset - woffset2)
    return fn


def _ps(r, mode=None):
    def fn(b, n, x, shp):
        c, h, w = shp
        SC._need(c % (r * r) == 0)
        return b.g.pixel_shuffle(n, x, r, mode), (c // (r * r), h * r, w * r)
    return fn


def _crop_like(b, n, x, shp):
    c, h, w = shp
    rh, rw = SC.conv_out(b.h0, 1, 2, 0), SC.conv_out(b.w0, 1, 2, 0)
    SC._need(c >= REF_C and h >= rh and w >= rw)  # the reference must fit into the blob
    ref = b.branch("conv", REF_C, rh, rw)
    return b.g.crop(n, x, like=ref), (REF_C, rh, rw)


NEW_UNARY = {
    "pad_same": _pad((0, 1, 0, 1)), "pad_sym1": _pad((1, 1, 1, 1)), "pad_value": _pad((1, 0, 2, 1), value=0.5),
    "pad_rep": _pad((1, 2, 0, 3), type_=1), "pad_reflect": _pad((2, 1, 3, 0), type_=2), "pad_pc": _pad((1, 1, 1, 1), pc=True),
    "pad_ch": _pad((0, 0, 0, 0), value=0.5, front=1, behind=2), "pad_none": _pad((0, 0, 0, 0)),
    "crop_in": _crop(woffset=1, hoffset=2, woffset2=1), "crop_c": _crop(coffset=2, outc=8), "crop_none": _crop(),
    "ps2": _ps(2, 0), "ps2m1": _ps(2, 1), "ps1": _ps(1),
}
ZERO_PADS = {"pad_same": (0, 1, 0, 1), "pad_sym1": (1, 1, 1, 1), "pad_none": (0, 0, 0, 0)}  # the plain zero Paddings and their margins
NOOPS = ("pad_none", "crop_none", "ps1")
SHUFFLES = ("ps2", "ps2m1", "ps1")
# the consumers a zero Padding folds into, and their own pad: Convolution / ConvolutionDepthWise on the main or the grouped route
FOLD_INTO = {"conv3x3": 1, "conv1x1": 0, "conv3x3s2": 1, "conv5x5": 2, "dw3x3": 1, "gconv3": 1, "pw72": 0}

UNARY = dict(SC.UNARY, **NEW_UNARY)
NEW_PRODUCERS = {op: (lambda op: lambda b: UNARY[op](b, "p", b.tap(), (SC.C0, b.h0, b.w0)))(op) for op in NEW_UNARY}
NEW_CONSUMERS = {op: (lambda op: lambda b, x, shp: UNARY[op](b, "c", x, shp))(op) for op in NEW_UNARY}
NEW_CONSUMERS["crop_like"] = lambda b, x, shp: _crop_like(b, "c", x, shp)
PRODUCERS = dict(SC.PRODUCERS, **NEW_PRODUCERS)
CONSUMERS = dict(SC.CONSUMERS, **NEW_CONSUMERS)

OLD_PRODUCERS = RS.OLD_PRODUCERS + ("conv1x1", "conv3x3s2", "conv5x5", "gconv3", "dil3x3", "relu", "slice2")
OLD_CONSUMERS = RS.OLD_CONSUMERS + ("conv1x1", "conv3x3s2", "conv5x5", "gconv3", "dil3x3", "pw72", "leaky", "prelu", "ip", "softmax", "dropout")

# The pairs no net exists for, each with its reason; none of them exists on one plane only.  tests/test_frame_seams_cpu.py asserts that the
# pairs that raise Incompatible are exactly these, on both planes.
_PS = "PixelShuffle r = 2 needs a multiple of 4 channels"
_BRANCH = "the other operand would need a plane no 1x1 branch of the input reaches (the input's plane, or at stride 2 the halved one)"
INCOMPATIBLE = {
    ("gap", "pad_reflect"): "a 1 x 1 plane: a reflect pad must be smaller than the plane it pads",
    ("gap", "crop_in"): "a 1 x 1 plane: the offsets leave no pixel",
    ("gap", "crop_like"): "a 1 x 1 plane: the reference, a stride-2 branch, does not fit into the blob",
    ("slice2", "crop_c"): "7 channels: coffset 2 + outc 8 leave the blob",
    ("slice2", "ps2"): "7 channels: " + _PS, ("slice2", "ps2m1"): "7 channels: " + _PS,
    ("pad_ch", "ps2"): "15 channels: " + _PS, ("pad_ch", "ps2m1"): "15 channels: " + _PS,
    ("crop_c", "gconv3"): "8 channels: group 3 does not divide them",
    ("crop_c", "crop_c"): "8 channels behind the first: coffset 2 + outc 8 leave the blob",
}
for _q in ("ps2", "ps2m1"):  # 3 channels behind a shuffle of 12
    INCOMPATIBLE[(_q, "crop_c")] = "3 channels: coffset 2 + outc 8 leave the blob"
    INCOMPATIBLE[(_q, "crop_like")] = "3 channels: the reference has 4"
    for _c in ("ps2", "ps2m1"):
        INCOMPATIBLE[(_q, _c)] = "3 channels: " + _PS
    # this pair showed that such a layer loaded and ran as a plain depthwise layer with 3 output channels; ConvLayer::LoadParam now refuses it
    INCOMPATIBLE[(_q, "gconv3")] = "3 channels in 3 groups with 12 filters: a depthwise layer with a channel multiplier, which the runtime refuses"
# a two-bottom consumer behind a layer that changes the plane to one that is neither the input's nor its half
for _p in ("pad_same", "pad_sym1", "pad_value", "pad_rep", "pad_reflect", "pad_pc", "crop_in", "ps2", "ps2m1"):
    for _c in ("elt_first", "elt_second", "concat"):
        INCOMPATIBLE[(_p, _c)] = _BRANCH


class Case(SC.Case):
    def __init__(self, *a):
        super().__init__(*a)
        self.p_bottom = self.c_bottom = None

    def input(self, batch=SC.BATCH):
        seed = zlib.crc32(f"{self.id}/{SALT.get(self.id, 0)}".encode())
        return np.random.default_rng(seed).normal(INPUT_MEAN.get((self.pname, self.cname), 0.0), 1, (batch, SC.C0) + self.plane).astype(np.float32)


# pad_ch -> gap: 15 one-value planes per image of which three are the constant 0.5 and twelve the means of 99 or 96 normal(0, 1) values, of
# standard deviation 0.1 -- among 36 of them one next to zero is the rule, and no redraw helps.  As tests/seam_cases.py does for gap -> relu,
# the input is drawn as normal(0.5, 1): the plane means are then 0.5 +- 0.1.
INPUT_MEAN = {("pad_ch", "gap"): 0.5}
# Cases whose first draw left a plane of an output or of P's top (the GPU test compares both) below 1e-3 of the tensor's maximum in the float64
# result, or no more than twice that floor (a plane of ONE value behind a global pooling or an InnerProduct that fell next to zero): each is drawn again with this salt in the seed of
# weights and input, the first that lifts its smallest plane to 2e-2 of the maximum (the rule of tests/seam_cases.py's SALT).
SALT = {"gap->pad_value@11x9": 2, "gap->pad_rep@12x8": 2, "gap->pad_ch@12x8": 23, "gap->pad_none@12x8": 3, "ps2->ip@12x8": 1, "ps2m1->ip@12x8": 1, "ps1->gap@11x9": 1}


def _one_pass(pname, cname, plane, seed, plan):
    """tests/seam_cases.py's _one_pass over this module's tables."""
    b = SC.Build(plane, seed, plan)
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
        outputs = [b.g.eltwise("join", c_top, rejoin)] if cshp == shp else [c_top, b.g.relu("side", rejoin)]
    return b, p_top, c_top, outputs


def build_case(pname, cname, plane):
    """-> Case, or raises SC.Incompatible."""
    salt = SALT.get(f"{pname}->{cname}@{plane[0]}x{plane[1]}", 0)
    seed = zlib.crc32(f"{pname}/{cname}/{plane}/{salt}".encode()) % (1 << 31)
    plan, _, _, _ = _one_pass(pname, cname, plane, seed, None)
    b, p_top, c_top, outputs = _one_pass(pname, cname, plane, seed, plan)
    assert b.taps == plan.taps and all(b.names[k] == plan.names[k] for k in "pc"), (pname, cname)
    param, weights = b.g.finish()
    return Case(pname, cname, plane, param, weights, b, p_top, c_top, outputs)


def pairs():
    """(pname, cname): a framing layer on at least one side."""
    out = [(p, c) for p in OLD_PRODUCERS for c in NEW_CONSUMERS]
    out += [(p, c) for p in NEW_PRODUCERS for c in OLD_CONSUMERS + tuple(NEW_CONSUMERS)]
    return out


def cases_of(pname, planes=SC.PLANES):
    for p, cname in pairs():
        if p != pname:
            continue
        for plane in planes:
            try:
                yield build_case(pname, cname, plane)
            except SC.Incompatible:
                continue


def row_names():
    return list(dict.fromkeys(p for p, _ in pairs()))


def expect(pname, cname, level):
    """-> {"p": verdict | None, "c": verdict | None}: see the module docstring."""
    out = {"p": None, "c": None}
    if pname in NEW_UNARY:
        if pname in ZERO_PADS and cname in FOLD_INTO and level >= 2:
            out["p"] = "folded"
        elif pname in SHUFFLES and cname in ("relu", "leaky") and level >= 2:
            out["p"] = "absorbed"
        else:
            out["p"] = "alias" if pname in NOOPS else "kept"
    if cname in NEW_CONSUMERS:
        # nothing in front of a framing layer absorbs it (no epilogue computes a window or a shuffle), and C is the net's last layer
        out["c"] = "alias" if cname in NOOPS else "kept"
    return out


def folded_pads(pname, cname):
    """(top, bottom, left, right) the convolution `cname` must report behind the folded zero Padding `pname`."""
    own = FOLD_INTO[cname]
    return tuple(own + m for m in ZERO_PADS[pname])


def _layer(case, name):
    import frame_ref
    return [l for l in frame_ref.parse_param(case.param) if l[1] == name][0]


def check_claim(case, level, net, same_address=None):
    """Assert the claim on a net that has run its fusion pass; with `same_address(top, bottom) -> bool | None` (None: the bottom is not
    extractable) also the aliasing state.  -> the verdicts."""
    verdict = expect(case.pname, case.cname, level)
    info = net.layers()
    names = [n for _, n, _ in info]
    for t, n, a in info:
        assert (a == "FRAME") == (t in FRAME_TYPES), (case.id, level, info)
    for side, name in (("p", "p"), ("c", case.c_first)):
        v = verdict[side]
        if v is None:
            continue
        if v == "folded":
            assert "p" not in names and "c" in names, (case.id, level, info)
            cp = net.conv_params()
            if cp:  # filled at Reshape: present once the net has run
                q = cp[names.index("c")][0]
                assert (q.pad_top, q.pad_bottom, q.pad_left, q.pad_right) == folded_pads(case.pname, case.cname), (case.id, level)
        elif v == "absorbed":
            assert "p" in names and "c" not in names, (case.id, level, info)
        else:
            assert name in names, (case.id, level, side, info)
            if same_address is not None:
                layer = _layer(case, name)
                same = same_address(layer[3][0], layer[2][0])
                assert same is None or same == (v == "alias"), (case.id, level, side, v, same)
    if verdict["p"] in ("kept", "alias") and case.cname in ("relu", "leaky", "prelu") + tuple(FOLD_INTO):
        assert case.c_first in names, (case.id, level, info)  # the near misses: the consumer stays a layer of its own
    return verdict
