"""The two-layer seams of the Interp and HardSwish layers: every net `Input -> P -> C` with one of the two types on one side and, on the
other, each of Convolution 3x3, depthwise, Pooling, Eltwise, Concat, BatchNorm, Scale, a gate BinaryOp, InstanceNorm, Deconvolution and
the two types themselves (tests/test_resample_seams_cpu.py, tests/test_resample_seams_gpu.py).

The nets are built as tests/seam_cases.py builds its pairs -- its Build passes, shapes (12 channels, planes 11 x 9 and 12 x 8, batch 3),
branches for two-bottom consumers and Incompatible rule -- with the tables extended here, in this module's own dictionaries: the two
types are not in create_layer, so tests/seam_cases.py does not (and must not) hold them.

New layers, usable on both sides:
  hswish          HardSwish(1/6, 0.5)
  hswish_default  HardSwish with ncnn's defaults
  up2             Interp nearest, scale 2 (the 16-byte x2 kernel on the 12 x 8 plane, the general one on 11 x 9)
  bil_up          Interp bilinear, scales 1.5 x 1.25, align_corner
  half            Interp bilinear, scale 0.5: the plane a stride-2 branch reaches on 12 x 8, so that an Eltwise or a Concat can follow it
and as consumers only:
  like            Interp bilinear to the size of a second bottom, a branch on the input's plane

`expect(pname, cname, level)`: "collapsed" where fusion level 2 must make P (an Interp) and C (a two-bottom Eltwise) one layer, "kept"
where C must stay a layer of its own, None where this table makes no claim.
"""
from __future__ import annotations

import zlib

import numpy as np

import seam_cases as SC

LEVELS = ((0, {}), (2, {}))


def _interp(mode, scale, align=False):
    def fn(b, n, x, shp):
        c, h, w = shp
        hs, ws = scale if isinstance(scale, tuple) else (scale, scale)
        ho, wo = int(np.float32(h) * np.float32(hs)), int(np.float32(w) * np.float32(ws))
        SC._need(ho >= 1 and wo >= 1)
        return b.g.interp(n, x, mode, scale=scale, align_corner=align), (c, ho, wo)
    return fn


def _like(b, n, x, shp):
    ref = b.branch("conv", 4, b.h0, b.w0)
    return b.g.interp(n, x, "bilinear", like=ref), (shp[0], b.h0, b.w0)


NEW_UNARY = {
    "hswish": SC._same(lambda g, n, x, c: g.hard_swish(n, x, 1.0 / 6, 0.5)), "hswish_default": SC._same(lambda g, n, x, c: g.hard_swish(n, x)),
    "up2": _interp("nearest", 2.0), "bil_up": _interp("bilinear", (1.5, 1.25), True), "half": _interp("bilinear", 0.5),
}
NEW_TYPES = {"Interp", "HardSwish"}

UNARY = dict(SC.UNARY, **NEW_UNARY)
NEW_PRODUCERS = {op: (lambda op: lambda b: UNARY[op](b, "p", b.tap(), (SC.C0, b.h0, b.w0)))(op) for op in NEW_UNARY}
NEW_CONSUMERS = {op: (lambda op: lambda b, x, shp: UNARY[op](b, "c", x, shp))(op) for op in NEW_UNARY}
NEW_CONSUMERS["like"] = lambda b, x, shp: _like(b, "c", x, shp)
PRODUCERS = dict(SC.PRODUCERS, **NEW_PRODUCERS)
CONSUMERS = dict(SC.CONSUMERS, **NEW_CONSUMERS)

# the neighbours the two types must meet: Convolution 3x3, depthwise, Pooling, Eltwise, Concat, BatchNorm, Scale, a gate BinaryOp (as a
# producer: the last layer of a squeeze-and-excitation block), InstanceNorm, Deconvolution
OLD_PRODUCERS = ("conv3x3", "dw3x3", "split_conv3x3", "maxpool2", "gap", "eltsum", "concat", "bn", "scale_bias", "se_conv", "inorm", "deconv4")
OLD_CONSUMERS = ("conv3x3", "dw3x3", "maxpool2", "gap", "elt_first", "elt_second", "concat", "bn", "scale_bias", "binop_gated", "binop_gate", "inorm", "deconv4",
                 "relu")
NEIGHBOURS = {"Convolution", "ConvolutionDepthWise", "Pooling", "Eltwise", "Concat", "BatchNorm", "Scale", "BinaryOp", "InstanceNorm", "Deconvolution"}

# Cases whose first draw left a one-value plane (behind a global pooling) below 4e-3 of the tensor's maximum in the float64 result, where the
# plane's relative error is the float32 rounding of its sum enlarged hundreds of times: each is drawn again with this salt in the seed of
# weights and input, the first that lifts its smallest plane to 2e-2 of the maximum (the rule of tests/seam_cases.py's SALT).
SALT = {"gap->hswish@11x9": 2, "gap->up2@11x9": 4, "up2->gap@11x9": 1, "half->gap@11x9": 5, "half->gap@12x8": 3}


class Case(SC.Case):
    def input(self, batch=SC.BATCH):
        seed = zlib.crc32(f"{self.id}/{SALT.get(self.id, 0)}".encode())
        return np.random.default_rng(seed).normal(SC.INPUT_MEAN.get((self.pname, self.cname), 0.0), 1, (batch, SC.C0) + self.plane).astype(np.float32)


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
    """(pname, cname): a new type on at least one side."""
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
    """The claim on the one fusion that takes these layers (collapse_upsample_adds): an Interp whose top is read by a two-bottom Eltwise
    alone becomes one layer with it from level 2 on; behind any other producer, and in front of any other consumer, the new layers stay."""
    interp_p = pname in ("up2", "bil_up", "half")
    if interp_p and cname in ("elt_first", "elt_second"):
        return "collapsed" if level >= 2 else "kept"
    if pname in NEW_UNARY or cname in NEW_CONSUMERS:
        # a convolution in front of a HardSwish or an Interp keeps it as a layer (no epilogue computes them); a ReLU, a BatchNorm or a
        # pooling behind them is not absorbed (they have no epilogue of their own)
        return "kept"
    return None


def check_claim(case, level, net):
    verdict = expect(case.pname, case.cname, level)
    info = net.layers()
    names = [n for _, n, _ in info]
    if verdict == "collapsed":
        assert "c" not in names and ("Interp", "p", "RESAMPLE") in info and not net.residuals(), (case.id, level, info)
    elif verdict == "kept":
        assert case.c_first in names, (case.id, level, info)
        if case.pname in NEW_UNARY:
            assert "p" in names, (case.id, level, info)
    for t, n, a in info:
        assert (a == "RESAMPLE") == (t in NEW_TYPES), (case.id, level, info)
    return verdict
