"""The table of seams between an int8 layer and every other layer type of feather::Net (tests/test_qseams_cpu.py, tests/test_qseams_gpu.py):
the nets `Input -> P -> C` of tests/seam_cases.py -- its Build, producers, consumers, planes (11 x 9 and 12 x 8), batch 3 then batch 1 and
the five settings of LEVELS -- with an int8 layer (8=1, input scale QUANT_DEFAULT_SCALE, Net.SetQuantized) as P, as C or as both.

The channel count is 16, not 12: with C % 16 != 0 every int8 layer would fall to the generic kernels and the MFMA routes would never meet
a neighbour.  Channel counts that are no multiple of 16 arrive through the producers that make them (slice2 leaves 11).

Int8 ops (QOPS), each usable as P and as C; the kernel fhip_qconv_route names on the 16-channel input / on slice2's 11 channels:
  q3x3 q1x1 q3x3s2 q5x5   16 outputs                          qconv_mfma_kernel<2, 2> / qconv_generic_kernel<16>
  qpw72                   1x1, 72 outputs (> 64)              qconv_mfma_kernel<4, 1> / qconv_generic_kernel<16>
  q1x1k8                  1x1, 8 outputs (< 16)               qconv_mfma_kernel<2, 2> / qconv_generic_kernel<4>
  qdw3x3 qdw3x3s2         depthwise                           qconv_dw3x3_kernel<1> / <2>
  qdw5x5                  depthwise, no kernel of its own     qconv_generic_kernel<4>
  qip                     InnerProduct over the whole C x H x W plane (the flattening order)

Rows (one GPU test id each):
  "P->q"   every producer of seam_cases.PRODUCERS -> each int8 op         (id: the producer)
  "q->C"   each int8 op and its split_ form -> every consumer of seam_cases.CONSUMERS, and -> each int8 op   (id: the int8 producer)
seam_cases' gconv3 (group 3) does not divide 16 channels and would drop out of every row; gconv4 (group 4) takes its place on both sides.
`Incompatible` pairs drop out as in seam_cases.  Thinning: none was needed -- every row runs every consumer on both planes (the slowest
row takes about a second on the MI355X); a row that grows past twice the slowest row of test_seams_gpu.py is to be split by plane into
two ids (PLANES_OF gives the planes of a row), never thinned by consumer.

What is compared, and why not end to end, is in tests/qseam_ref.py.  Every compared fp32 plane keeps seam_cases' floor (2e-2 of its
tensor's maximum in the float64 result, 6e-3 where a tensor has 72 channels or more); a case whose first draw misses it is drawn again with
the salt recorded in SALT (the first that passes), which tests/test_qseams_cpu.py asserts.

`expect(pname, cname, level)` is the claim for C's first layer, from ConvLayer::Fuse / InnerProductLayer::Fuse / ConvLayer::FuseResidual /
plan_chains / plan_siblings / collapse_gate_blocks for a layer off the main route:
  * the int8 layer is a layer of its own on route QCONV at every level and setting, whatever stands in front of or behind it;
  * behind an int8 P: a plain ReLU is absorbed at level >= 1; a leaky one is kept; BatchNorm / Scale is absorbed at level 2 by a
    convolution (kept below, and kept by an InnerProduct, which folds nothing); every pooling (2x2 max included), Eltwise in either
    order, a two-bottom Scale / BinaryOp, a 1x1 convolution of either kind and everything else is kept; a squeeze-and-excitation block
    behind it collapses on its own; behind split_ nothing is absorbed;
  * no layer pair is one kernel (fused_pointwise() is empty), no int8 layer holds a residual, a sibling mark or a chain mark.
"""
from __future__ import annotations

import zlib

import numpy as np

import seam_cases as SC
from seam_cases import Incompatible, LEVELS, PLANES, BATCH  # noqa: F401

C0 = 16
FLOOR, FLOOR_WIDE = 2e-2, 6e-3


def _qconv(k, s, p, dw=False, cout=None):
    def fn(b, n, x, shp):
        c, h, w = shp
        ko = c if dw else (cout or b.c0)
        ho, wo = SC.conv_out(h, k, s, p), SC.conv_out(w, k, s, p)
        SC._need(ho >= 1 and wo >= 1)
        return b.g.conv(n, x, c, ko, k, s, p, group=c if dw else 1, quant=True), (ko, ho, wo)
    return fn


def _qip(b, n, x, shp):
    c, h, w = shp
    top = b.g.fc(n, x, c * h * w, b.c0, gain=0.01, quant=True)  # gain and biases: seam_cases._ip
    if b.positive_bias and n == "p" and not b.g.dry:  # the biases stand in front of the c0 weight scales and the input scale
        lo, hi = -4 * (2 * b.c0 + 1), -4 * (b.c0 + 1)
        bias = np.frombuffer(bytes(b.g.bin[lo:hi]), "<f4")
        b.g.bin[lo:hi] = (np.abs(bias) + np.float32(0.05)).astype("<f4").tobytes()
    return top, (b.c0, 1, 1)


QOPS = {"q3x3": _qconv(3, 1, 1), "q1x1": _qconv(1, 1, 0), "q3x3s2": _qconv(3, 2, 1), "q5x5": _qconv(5, 1, 2), "qpw72": _qconv(1, 1, 0, cout=72),
        "q1x1k8": _qconv(1, 1, 0, cout=8), "qdw3x3": _qconv(3, 1, 1, dw=True), "qdw3x3s2": _qconv(3, 2, 1, dw=True), "qdw5x5": _qconv(5, 1, 2, dw=True),
        "qip": _qip}

QPRODUCERS = {op: (lambda op: lambda b: QOPS[op](b, "p", b.tap(), (b.c0, b.h0, b.w0)))(op) for op in QOPS}
QPRODUCERS.update({"split_" + op: QPRODUCERS[op] for op in QOPS})
QCONSUMERS = {op: (lambda op: lambda b, x, shp: QOPS[op](b, "c", x, shp))(op) for op in QOPS}
# group 3 does not divide 16 channels: gconv3 is Incompatible with everything here, and gconv4 stands in for it on both sides
_GCONV4 = SC._conv(3, 1, 1, 4)
FP_PRODUCERS = {("gconv4" if p == "gconv3" else "split_gconv4" if p == "split_gconv3" else p): fn for p, fn in SC.PRODUCERS.items()}
FP_PRODUCERS["gconv4"] = FP_PRODUCERS["split_gconv4"] = lambda b: _GCONV4(b, "p", b.tap(), (b.c0, b.h0, b.w0))
FP_CONSUMERS = {("gconv4" if c == "gconv3" else c): fn for c, fn in SC.CONSUMERS.items()}
FP_CONSUMERS["gconv4"] = lambda b, x, shp: _GCONV4(b, "c", x, shp)
PRODUCERS = dict(FP_PRODUCERS, **QPRODUCERS)
CONSUMERS = dict(FP_CONSUMERS, **QCONSUMERS)

INPUT_MEAN = dict(SC.INPUT_MEAN)
POSITIVE = set(SC.POSITIVE) | {("qip", "relu")}
SALT = {}  # filled below: SALT.update(...)


def PLANES_OF(pname):
    return PLANES


class Case(SC.Case):
    def __init__(self, *a):
        super().__init__(*a)
        self.id = "q:" + self.id
        self.quantized = True

    def input(self, batch=BATCH):
        seed = zlib.crc32(f"{self.id}/{SALT.get(self.id, 0)}".encode())
        return np.random.default_rng(seed).normal(INPUT_MEAN.get((self.pname, self.cname), 0.0), 1, (batch, C0) + self.plane).astype(np.float32)


def _one_pass(pname, cname, plane, seed, plan):
    b = SC.Build(plane, seed, plan, c0=C0)
    # split_qip: the second consumer of the one-value planes is a plain ReLU (`side`), as in POSITIVE
    b.positive_bias = (pname, cname) in POSITIVE or pname == "split_qip"
    b.start()
    b.phase = "p"
    p_top, shp = PRODUCERS[pname](b)
    x, outputs = p_top, []
    if pname.startswith("split_"):
        x, rejoin = b.g.split("p_split", p_top)
    b.phase = "c"
    c_top, cshp = CONSUMERS[cname](b, x, shp)
    outputs.append(c_top)
    if pname.startswith("split_"):  # as seam_cases._one_pass
        b.phase = "b"
        outputs = [b.g.eltwise("join", c_top, rejoin)] if cshp == shp else [c_top, b.g.relu("side", rejoin)]
    return b, p_top, c_top, outputs


def build_case(pname, cname, plane, salt=None):
    """-> Case, or raises Incompatible.  At least one of P and C is an int8 op."""
    assert pname.removeprefix("split_") in QOPS or cname in QOPS, (pname, cname)
    cid = f"q:{pname}->{cname}@{plane[0]}x{plane[1]}"
    salt = SALT.get(cid, 0) if salt is None else salt
    seed = zlib.crc32(f"q/{pname}/{cname}/{plane}/{salt}".encode()) % (1 << 31)
    plan, _, _, _ = _one_pass(pname, cname, plane, seed, None)
    b, p_top, c_top, outputs = _one_pass(pname, cname, plane, seed, plan)
    assert b.taps == plan.taps and all(b.names[k] == plan.names[k] for k in "pc"), (pname, cname)
    param, weights = b.g.finish()
    return Case(pname, cname, plane, param, weights, b, p_top, c_top, outputs)


def rows():
    """{row id: (pname, [consumer names])}: see the module docstring."""
    out = {f"{p}->q": (p, list(QOPS)) for p in FP_PRODUCERS}
    out.update({f"{p}->C": (p, list(CONSUMERS)) for p in QPRODUCERS})
    return out


def cases_of(row):
    pname, cnames = rows()[row]
    for cname in cnames:
        for plane in PLANES_OF(pname):
            try:
                yield build_case(pname, cname, plane)
            except Incompatible:
                continue


# ---- the claim column --------------------------------------------------------------------------------------------------------------------
def expect(pname, cname, level):
    """(verdict, rule) for C's first layer: "absorbed", "kept", "collapsed" (a squeeze-and-excitation block, on its own) or None (P is no
    int8 op: seam_cases.expect's business, but for C being an int8 layer, which is always kept)."""
    if cname in QOPS:
        return "kept", None
    if pname.removeprefix("split_") not in QOPS:
        return None, None
    ct = SC.CTAG.get(cname, "other")
    if ct == "se":
        return ("collapsed" if level >= 2 else "kept"), "se"
    if pname.startswith("split_"):
        return "kept", None
    if ct == "relu":
        return ("absorbed" if level >= 1 else "kept"), "relu"
    if ct == "affine":
        return ("absorbed" if level >= 2 and pname != "qip" else "kept"), "affine_side"
    return "kept", {"pool2": "pool", "poolx": "pool", "pw12": "dwpw", "pw72": "dwpw", "elt": "residual", "gscale": "affine_side"}.get(ct)


def check_claim(case, level, net):
    """Assert the claim on a net that has run Forward (the planner's answers only: this runs before any blob is looked at)."""
    info = net.layers()
    names = [n for _, n, _ in info]
    routes = {n: a for _, n, a in info}
    qnames = [n for n, q in (("p", case.pname.removeprefix("split_") in QOPS), ("c", case.cname in QOPS)) if q]
    for n in qnames:
        assert routes.get(n) == "QCONV", (case.id, level, n, info)
    qidx = {names.index(n) for n in qnames}
    assert not net.fused_pointwise() and not net.siblings(), (case.id, level, net.fused_pointwise(), net.siblings())
    assert not qidx & set(net.residuals()) and not qidx & set(net.chains(raw=True)), (case.id, level, net.residuals(), net.chains(raw=True))
    verdict, _ = expect(case.pname, case.cname, level)
    if verdict == "collapsed":
        dense = "c_fc1" if case.cname == "se_caffe" else "c_conv1"
        assert ("Pooling", "c_gap", "GATE") in info and dense not in names, (case.id, level, info)
    elif verdict == "absorbed":
        assert case.c_first not in names, (case.id, level, info)
    elif verdict == "kept":
        assert case.c_first in names, (case.id, level, info)


# {case id without its "q:"}: salt -- see the module docstring (304 of the table's cases)
SALT.update({"q:" + k: v for k, v in {
    "gconv4->qip@12x8": 1, "split_gconv4->qip@12x8": 2, "qip->gconv4@11x9": 3, "qip->gconv4@12x8": 6, "split_qip->gconv4@11x9": 1, "split_qip->gconv4@12x8": 6,
    "avgpool3s2p1->qip@11x9": 3, "avgpool3s2p1->qip@12x8": 1, "clip->qip@11x9": 1, "concat->qip@11x9": 4, "concat->qip@12x8": 1, "conv1x1->qip@12x8":
    2, "conv3x3->qip@11x9": 1, "conv3x3->qip@12x8": 3, "conv3x3s2->qip@11x9": 8, "conv3x3s2->qip@12x8": 1, "conv5x5->qip@11x9": 1,
    "conv5x5->qip@12x8": 6, "deconvdw->qip@11x9": 1, "dil3x3->qip@11x9": 3, "dil3x3->qip@12x8": 2, "dropout->qip@11x9": 3, "dropout->qip@12x8": 2,
    "dw3x3->qip@12x8": 1, "eltsum->qip@12x8": 4, "gap->q1x1@11x9": 1, "gap->q1x1@12x8": 60, "gap->q1x1k8@11x9": 3, "gap->q1x1k8@12x8": 8,
    "gap->q3x3@11x9": 22, "gap->q3x3@12x8": 54, "gap->q3x3s2@12x8": 16, "gap->q5x5@11x9": 19, "gap->q5x5@12x8": 7, "gap->qdw3x3@11x9": 5,
    "gap->qdw3x3@12x8": 25, "gap->qdw3x3s2@11x9": 11, "gap->qdw3x3s2@12x8": 53, "gap->qdw5x5@11x9": 6, "gap->qdw5x5@12x8": 109, "gap->qip@11x9": 6,
    "gap->qip@12x8": 4, "gap->qpw72@11x9": 99, "gap->qpw72@12x8": 360, "gmp->q1x1@11x9": 2, "gmp->q3x3@12x8": 7, "gmp->q3x3s2@12x8": 1,
    "gmp->q5x5@11x9": 8, "gmp->qdw3x3@11x9": 1, "gmp->qip@11x9": 1, "gmp->qip@12x8": 6, "gmp->qpw72@11x9": 2, "hsigmoid->qip@11x9": 1,
    "hsigmoid->qip@12x8": 1, "inorm->qip@11x9": 1, "inorm->qip@12x8": 1, "input->qip@12x8": 1, "ip->q1x1@11x9": 2, "ip->q1x1@12x8": 7,
    "ip->q1x1k8@11x9": 9, "ip->q3x3@12x8": 2, "ip->q3x3s2@11x9": 26, "ip->q3x3s2@12x8": 2, "ip->q5x5@11x9": 16, "ip->q5x5@12x8": 1, "ip->qdw3x3@11x9":
    4, "ip->qdw3x3@12x8": 3, "ip->qdw3x3s2@11x9": 3, "ip->qdw3x3s2@12x8": 7, "ip->qdw5x5@11x9": 1, "ip->qdw5x5@12x8": 3, "ip->qip@11x9": 3,
    "ip->qip@12x8": 3, "ip->qpw72@11x9": 21, "ip->qpw72@12x8": 9, "leaky->qip@12x8": 1, "maxpool3s2->qip@11x9": 2, "maxpool3s2->qip@12x8": 2,
    "prelu->qip@11x9": 1, "prelu->qip@12x8": 3, "q1x1->gap@11x9": 10, "q1x1->gap@12x8": 4, "q1x1->ip@11x9": 2, "q1x1->ip@12x8": 7, "q1x1->qip@11x9":
    3, "q1x1k8->gap@11x9": 7, "q1x1k8->ip@11x9": 4, "q1x1k8->ip@12x8": 6, "q1x1k8->qip@11x9": 2, "q1x1k8->qip@12x8": 2, "q3x3->gap@11x9": 2,
    "q3x3->gap@12x8": 2, "q3x3->ip@11x9": 3, "q3x3->ip@12x8": 2, "q3x3->qip@11x9": 8, "q3x3s2->gap@11x9": 5, "q3x3s2->gap@12x8": 1, "q3x3s2->ip@11x9":
    1, "q3x3s2->ip@12x8": 1, "q3x3s2->qip@11x9": 2, "q3x3s2->qip@12x8": 1, "q5x5->gap@11x9": 9, "q5x5->gap@12x8": 6, "q5x5->ip@11x9": 1,
    "q5x5->ip@12x8": 2, "q5x5->qip@11x9": 1, "q5x5->qip@12x8": 4, "qdw3x3->gap@11x9": 2, "qdw3x3->gap@12x8": 23, "qdw3x3->ip@11x9": 1,
    "qdw3x3->ip@12x8": 3, "qdw3x3->qip@11x9": 4, "qdw3x3->qip@12x8": 2, "qdw3x3s2->gap@11x9": 3, "qdw3x3s2->gap@12x8": 16, "qdw3x3s2->ip@12x8": 1,
    "qdw3x3s2->qip@12x8": 5, "qdw3x3s2->softmax@12x8": 1, "qdw5x5->gap@11x9": 15, "qdw5x5->gap@12x8": 3, "qdw5x5->ip@11x9": 1, "qdw5x5->ip@12x8": 7,
    "qdw5x5->qip@12x8": 1, "qip->avgpool3s2p1@11x9": 2, "qip->avgpool3s2p1@12x8": 2, "qip->binop_gate@12x8": 1, "qip->binop_gated@11x9": 2,
    "qip->bn@12x8": 5, "qip->clip@11x9": 1, "qip->clip@12x8": 5, "qip->conv1x1@11x9": 4, "qip->conv1x1@12x8": 6, "qip->conv3x3@11x9": 7,
    "qip->conv3x3@12x8": 7, "qip->conv3x3s2@11x9": 5, "qip->conv3x3s2@12x8": 10, "qip->conv5x5@11x9": 6, "qip->conv5x5@12x8": 2, "qip->deconv4@12x8":
    2, "qip->deconvdw@11x9": 2, "qip->deconvdw@12x8": 1, "qip->dil3x3@12x8": 19, "qip->dropout@11x9": 1, "qip->dropout@12x8": 3, "qip->dw3x3@11x9": 2,
    "qip->dw3x3@12x8": 28, "qip->gmp@11x9": 1, "qip->gmp@12x8": 2, "qip->hsigmoid@11x9": 3, "qip->hsigmoid@12x8": 7, "qip->ip@11x9": 1,
    "qip->ip@12x8": 1, "qip->leaky@11x9": 9, "qip->leaky@12x8": 23, "qip->maxpool2@11x9": 1, "qip->prelu@11x9": 25, "qip->prelu@12x8": 2,
    "qip->pw72@11x9": 29, "qip->pw72@12x8": 50, "qip->q1x1@12x8": 24, "qip->q1x1k8@12x8": 14, "qip->q3x3@11x9": 1, "qip->q3x3@12x8": 5,
    "qip->q3x3s2@11x9": 5, "qip->q3x3s2@12x8": 6, "qip->q5x5@11x9": 4, "qip->q5x5@12x8": 15, "qip->qdw3x3@12x8": 2, "qip->qdw3x3s2@11x9": 4,
    "qip->qdw3x3s2@12x8": 5, "qip->qdw5x5@12x8": 4, "qip->qip@12x8": 5, "qip->qpw72@11x9": 25, "qip->qpw72@12x8": 58, "qip->scale_bias@11x9": 19,
    "qip->scale_bias@12x8": 3, "qip->scale_nobias@12x8": 8, "qip->scaleby_gate@11x9": 1, "qip->scaleby_gate@12x8": 2, "qip->scaleby_gated@11x9": 1,
    "qip->se_caffe@11x9": 2, "qip->se_caffe@12x8": 1, "qip->se_conv@12x8": 6, "qip->shuffle@11x9": 7, "qip->shuffle@12x8": 2, "qip->sigmoid@11x9": 3,
    "qip->sigmoid@12x8": 2, "qip->slice2@11x9": 9, "qip->softmax@11x9": 6, "qip->swish@11x9": 1, "qip->swish@12x8": 2, "qip->tanh@11x9": 1,
    "qip->tanh@12x8": 2, "qpw72->gap@11x9": 72, "qpw72->gap@12x8": 10, "qpw72->ip@11x9": 1, "qpw72->ip@12x8": 1, "qpw72->qip@12x8": 1,
    "relu->qip@12x8": 3, "scale_bias->qip@12x8": 1, "scale_nobias->qip@11x9": 1, "scale_nobias->qip@12x8": 1, "se_caffe->qip@12x8": 4,
    "se_conv->qip@11x9": 2, "se_conv->qip@12x8": 1, "shuffle->qip@11x9": 2, "shuffle->qip@12x8": 5, "sigmoid->qip@11x9": 1, "sigmoid->qip@12x8": 5,
    "softmax->q1x1@12x8": 1, "softmax->q1x1k8@11x9": 2, "softmax->q1x1k8@12x8": 1, "softmax->q3x3@12x8": 2, "softmax->q3x3s2@11x9": 3,
    "softmax->q5x5@11x9": 2, "softmax->qdw3x3@11x9": 2, "softmax->qdw3x3s2@12x8": 3, "split_conv1x1->qip@11x9": 6, "split_conv1x1->qip@12x8": 1,
    "split_conv3x3->qip@11x9": 2, "split_conv3x3->qip@12x8": 1, "split_conv3x3s2->qip@11x9": 5, "split_conv5x5->qip@11x9": 2,
    "split_conv5x5->qip@12x8": 3, "split_dil3x3->qip@12x8": 9, "split_dw3x3->qip@12x8": 1, "split_q1x1->gap@11x9": 13, "split_q1x1->gap@12x8": 1,
    "split_q1x1->ip@11x9": 4, "split_q1x1->qip@11x9": 2, "split_q1x1->qip@12x8": 3, "split_q1x1k8->gap@11x9": 6, "split_q1x1k8->ip@12x8": 2,
    "split_q1x1k8->qip@11x9": 5, "split_q3x3->gap@11x9": 11, "split_q3x3->gap@12x8": 3, "split_q3x3->ip@12x8": 2, "split_q3x3->qip@11x9": 4,
    "split_q3x3->qip@12x8": 2, "split_q3x3s2->gap@11x9": 11, "split_q3x3s2->ip@11x9": 3, "split_q3x3s2->ip@12x8": 1, "split_q3x3s2->qip@12x8": 4,
    "split_q5x5->gap@11x9": 1, "split_q5x5->ip@11x9": 3, "split_q5x5->ip@12x8": 4, "split_q5x5->qip@11x9": 1, "split_qdw3x3->gap@11x9": 3,
    "split_qdw3x3->gap@12x8": 29, "split_qdw3x3->ip@11x9": 1, "split_qdw3x3->qip@11x9": 1, "split_qdw3x3s2->gap@11x9": 58, "split_qdw3x3s2->gap@12x8":
    6, "split_qdw3x3s2->ip@11x9": 3, "split_qdw3x3s2->qip@12x8": 2, "split_qdw5x5->gap@11x9": 28, "split_qdw5x5->gap@12x8": 38,
    "split_qdw5x5->ip@12x8": 3, "split_qdw5x5->qip@11x9": 1, "split_qdw5x5->qip@12x8": 4, "split_qip->bn@11x9": 1, "split_qip->bn@12x8": 1,
    "split_qip->conv1x1@11x9": 4, "split_qip->conv3x3@11x9": 1, "split_qip->conv3x3s2@11x9": 1, "split_qip->conv5x5@11x9": 1,
    "split_qip->conv5x5@12x8": 1, "split_qip->dil3x3@11x9": 2, "split_qip->dil3x3@12x8": 2, "split_qip->dw3x3@11x9": 1, "split_qip->inorm@11x9": 2,
    "split_qip->inorm@12x8": 1, "split_qip->ip@12x8": 3, "split_qip->pw72@11x9": 13, "split_qip->pw72@12x8": 5, "split_qip->q1x1@11x9": 1,
    "split_qip->q1x1@12x8": 5, "split_qip->q1x1k8@11x9": 1, "split_qip->q1x1k8@12x8": 1, "split_qip->q3x3@11x9": 1, "split_qip->q3x3@12x8": 1,
    "split_qip->q3x3s2@11x9": 1, "split_qip->q3x3s2@12x8": 2, "split_qip->q5x5@11x9": 3, "split_qip->q5x5@12x8": 1, "split_qip->qdw3x3@11x9": 2,
    "split_qip->qdw3x3@12x8": 2, "split_qip->qdw3x3s2@11x9": 1, "split_qip->qdw3x3s2@12x8": 7, "split_qip->qdw5x5@12x8": 3, "split_qip->qip@11x9": 1,
    "split_qip->qip@12x8": 2, "split_qip->qpw72@11x9": 16, "split_qip->qpw72@12x8": 4, "split_qpw72->gap@11x9": 25, "split_qpw72->gap@12x8": 68,
    "split_qpw72->ip@11x9": 2, "split_qpw72->ip@12x8": 7, "split_qpw72->qip@11x9": 5, "split_qpw72->qip@12x8": 7, "swish->qip@11x9": 5,
    "swish->qip@12x8": 1, "tanh->qip@11x9": 1, "tanh->qip@12x8": 1
}.items()})
