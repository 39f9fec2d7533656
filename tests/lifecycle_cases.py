"""The life-cycle table of feather::Net: ONE handle walked through shapes and settings (tests/test_lifecycle_cpu.py,
tests/test_lifecycle_gpu.py).  The invariant the walks test: a Net after any legal history equals a fresh Net in its final state, bit for bit.

The model (`model()`, 3 input channels, at most 128 anywhere, seeded, built in memory) holds every plan kind of the Net runtime's re-plan path (feathercnn_amd/csrc/net_plan.h) at once:

  data -> conv0 (3 -> 16, 3x3 p1) + ReLU               the RGB first layer, computed inside conv1's input transform (plan_chains: head / head_of)
       -> conv1 (16 -> 32) + ReLU -> conv2 (32 -> 32) + ReLU + 2x2 max pool -> conv3 (32 -> 32) + ReLU -> conv4 (32 -> 64) + ReLU
                                                        3x3 s1 p1 each: one Winograd chain with a fused pool inside; behind the pool a 14-pixel
                                                        plane at a batch that is a multiple of 4 runs on 2x2 image canvases (ENTRY conv2 -> conv3,
                                                        INSIDE conv3 -> conv4, the canvas output transform of conv4)
       -> Split -> sib_a, sib_b (64 -> 128, 1x1)        two 1x1 layers with more than 64 output channels on one bottom: siblings
       -> res (128 -> 128, 3x3 p1, on sib_a) + Eltwise with sib_b + ReLU   the residual add: in the GEMM epilogue where res is an IM2COL
                                                        layer (residuals() 1), a launch of its own behind a Winograd res (2)
       -> dw (3x3 depthwise, 128) + ReLU -> pw (128 -> 96, 1x1) + ReLU  the depthwise + pointwise pair (`mid` where it runs as two kernels)
       -> SE block (GAP, 96 -> 16 -> 96 InnerProduct, Sigmoid, Scale -233), hidden width 16: stepwise where 32 > H * W
       -> InstanceNorm + ReLU
       -> Split -> Dropout(scale 1) -> GAP -> InnerProduct (96 -> 10) -> Softmax = "prob"      (Split and Dropout tops are aliases)
                -> tail3 (96 -> 32, 3x3 p1) + ReLU = "tail3_relu"                               a 3x3 layer at the deep end

Where this departs from the wording of the plan it was written to: a convolution that took an Eltwise into its epilogue is no sibling
candidate (plan_siblings' `plain` refuses a layer with a residual), so the residual add sits on a THIRD layer that reads sibling a and
adds sibling b -- the pair and the residual both exist, on neighbouring layers; that layer is 3x3, because a 1x1 layer is IM2COL on every
plane and residuals() would never change.  The 14-pixel canvas stretch leaves through the canvas
output transform and not through a pooled EXIT boundary: a second pool would land on a 7-pixel plane, which is F(4,3) and refuses chains; the
EXIT form needs the 56 -> 28 boundary, whose 112-pixel input costs the float64 reference a second per image.

Every plane is kept well-conditioned for plane_nerr, which divides a plane's error by that plane's own maximum while the float32 error of a
layer scales with the magnitude of the whole tensor.  With GraphBuilder's weights as drawn, a channel's mean is a random multiple of the
(positive) mean of the ReLU output it reads, and among some 300 000 planes hundreds are nearly dead: a few values just above zero behind the
ReLU, whose error relative to themselves is a hundred times the tensor's (1e-3 .. 0.18 measured on the device for planes at 1e-3 .. 1e-5
of the maximum, on a net that equalled a fresh one bit for bit).  So the convolutions are calibrated against the float64 evaluator, layer
by layer in the order of the net, on CALIB's inputs (the data-dependent initialisation of LSUV, Mishkin & Matas 2016): the filters of a
layer are scaled by one factor to unit mean variance of its output (the depthwise layer per channel), and each bias is set so that the
channel's mean is SHIFT standard deviations above zero (for `res`: of the sum it feeds).  About 2 % of the values are still clipped by a
ReLU.  tests/test_lifecycle_cpu.py asserts what this is for: on every fed input no plane of any blob is below PLANE_FLOOR of its tensor's
maximum.  The one-value planes behind the InnerProduct layers are bias + a small sum, as in tests/seam_cases.py: gain 0.01 and biases in
(0.05, 0.15), so that a wrong weight still moves a value by per cents.

Sizes (H x W of the input; `plane` = what conv3 .. tail3 see behind the pool), each the smallest of its class by the rules of the code:
  28 x 28 -> 14   fhip_winograd_f63_canvas_param: canvases at batch % 4 == 0; the dw + pw pair is two kernels (14 % 4 != 0)
  16 x 16 -> 8    wino_f43: F(4,3) under tuned selection (IM2COL without: select_algo wants more than 8 pixels); no chain behind the pool;
  14 x 14 -> 7      at 16 the pair runs as one kernel (8 % 4 == 0)
  12 x 12 -> 6    one F(6,3) tile under tuned selection: the chain is whole again, no canvas
  13 x 21 -> 7x11 odd and not square: conv2's pool falls back to pre_pool (odd output), the first layer is not fused (odd width), 77 pixels
                  per plane are ragged 1x1 columns
   6 x  6 -> 3    below 4 pixels tuned selection keeps IM2COL; 9 pixels: the SE block runs stepwise (32 > 9) and at batch 1 .. 3 the
                  siblings are un-planned (fhip_conv_can_fuse_siblings wants more than 32 columns: 4 x 9 = 36 has them)

A second, two-layer model (`deep_model()`) is the one place that needs more than 128 channels: a 1x1 convolution 1024 -> 256, whose packed
weights hold a second image for the streamed 1x1 kernel on planes of at least 4 pixels and a third one for the InnerProduct stream on a 1x1
plane -- the two have the same size, so the byte count of the packed buffer does not tell them apart.

A walk is a list of steps:
  ("feed", key[, variant])   FeedInput of input(key, variant), key into SHAPES
  ("forward", k)             k Forwards; the test compares after each
  ("set_tuned", flip) / ("set_concurrency", flip) / ("set_graph", flip)   flip=True: the opposite of the setting the walk started with, False: back to it
  ("stream",)                use_current_stream() under a torch side stream
  ("extract", blob, at3)     Extract of one blob; at fusion level 3 it must be refused as chained iff at3 == "chained" (else, and below level
                             3, it must succeed and match float64)
"""
from __future__ import annotations

import zlib

import numpy as np

from feathercnn_amd import model_zoo
from seam_cases import LEVELS

SEED = 20
SHAPES = {
    "p14b4": (4, 3, 28, 28), "p14b5": (5, 3, 28, 28), "p14b8": (8, 3, 28, 28),
    "p8b4": (4, 3, 16, 16), "p7b1": (1, 3, 14, 14),
    "p6b4": (4, 3, 12, 12),
    "odd5": (5, 3, 13, 21),
    "p3b1": (1, 3, 6, 6), "p3b4": (4, 3, 6, 6),
    # the replica walk: 3 replicas take 3 + 2 + 2, 1 + 1 + 0 and 1 + 0 + 0 images
    "p8b7": (7, 3, 16, 16), "p8b2": (2, 3, 16, 16), "p8b1": (1, 3, 16, 16), "p6b1": (1, 3, 12, 12), "p6b7": (7, 3, 12, 12),
}
CLASS = {"p14b4": "canvas14", "p14b5": "canvas14", "p14b8": "canvas14", "p8b4": "f43", "p7b1": "f43", "p6b4": "one_tile", "odd5": "odd",
         "p3b1": "below4", "p3b4": "below4", "p8b7": "f43", "p8b2": "f43", "p8b1": "f43", "p6b1": "one_tile", "p6b7": "one_tile"}
CLASSES = ("canvas14", "f43", "one_tile", "odd", "below4")
DEEP_SHAPES = {"d2x2": (2, 1024, 2, 2), "d1x1": (2, 1024, 1, 1), "d3x1": (3, 1024, 3, 1)}
OUTPUTS = ("prob", "tail3_relu")
CONV3X3 = ("conv1", "conv2", "conv3", "conv4", "res", "tail3")
STEP_KINDS = ("feed", "forward", "set_tuned", "set_concurrency", "set_graph", "stream", "extract")


def _positive_bias(g, n):
    """The biases are the last n floats written, U(-0.1, 0.1) -> 0.05 + |U| (seam_cases._ip)."""
    bias = np.frombuffer(bytes(g.bin[-4 * n:]), "<f4")
    g.bin[-4 * n:] = (np.abs(bias) + np.float32(0.05)).astype("<f4").tobytes()


def _fc(g, name, x, cin, cout):
    top = g.fc(name, x, cin, cout, gain=0.01)
    _positive_bias(g, cout)
    return top


_MODEL = {}
SHIFT = 2.0                             # a channel's mean above zero, in standard deviations of the channel
CALIB = (("p8b4", 0), ("p3b4", 0))      # the inputs the calibration evaluates
PLANE_FLOOR = 0.05                      # min over planes of max|plane| / max|tensor| that test_lifecycle_cpu.py asserts
# (layer, the blob whose channels are measured, scale the filters): in the order of the net
CALIBRATED = (("conv0", "conv0", True), ("conv1", "conv1", True), ("conv2", "conv2", True), ("conv3", "conv3", True), ("conv4", "conv4", True),
              ("sib_a", "sib_a", True), ("sib_b", "sib_b", True), ("res", "sum", False), ("dw", "dw", True), ("pw", "pw", True), ("tail3", "tail3", True))


def _calibrate(param, image, at):
    """Scale the filters and set the biases of CALIBRATED in the .bin `image` (a bytearray); at[layer] = (offset of the filters, their
    count, output channels).  See the module docstring."""
    import seam_ref
    xs = [input(k, v) for k, v in CALIB]
    for name, blob, rescale in CALIBRATED:
        net = seam_ref.Net(param, bytes(image))
        net.layers = net.layers[:1 + [i for i, layer in enumerate(net.layers) if blob in layer[3]][0]]
        wo, wn, cout = at[name]
        vals = np.concatenate([np.moveaxis(net.run("data", x, keep=True)[blob].astype(np.float64), 1, 0).reshape(cout, -1) for x in xs], axis=1)
        mu, sd = vals.mean(axis=1), vals.std(axis=1)
        w = np.frombuffer(bytes(image[wo:wo + 4 * wn]), "<f4").astype(np.float64).reshape(cout, -1)
        bias = np.frombuffer(bytes(image[wo + 4 * wn:wo + 4 * (wn + cout)]), "<f4").astype(np.float64)
        scale = np.ones(cout)
        if rescale:
            scale = 1.0 / sd if name == "dw" else np.full(cout, 1.0 / np.sqrt((sd ** 2).mean()))
        image[wo:wo + 4 * wn] = (w * scale[:, None]).astype("<f4").tobytes()
        image[wo + 4 * wn:wo + 4 * (wn + cout)] = (SHIFT * sd * scale - (mu - bias) * scale).astype("<f4").tobytes()


def model():
    """-> (param, weights, input name, outputs)."""
    if "m" not in _MODEL:
        g = model_zoo.GraphBuilder(SEED)
        at = {}

        def conv(name, x, cin, cout, k, s=1, p=0, group=1):
            start = len(g.bin)  # a tag of 4 bytes, the filters, the biases
            top = g.conv(name, x, cin, cout, k, s, p, group=group)
            at[name] = (start + 4, cout * (cin // group) * k * k, cout)
            return top

        x = g.input("data", 3, 28, 28)
        x = g.relu("relu0", conv("conv0", x, 3, 16, 3, 1, 1))
        x = g.relu("relu1", conv("conv1", x, 16, 32, 3, 1, 1))
        x = g.relu("relu2", conv("conv2", x, 32, 32, 3, 1, 1))
        x = g.pool("pool2", x, 2, 2)
        x = g.relu("relu3", conv("conv3", x, 32, 32, 3, 1, 1))
        x = g.relu("relu4", conv("conv4", x, 32, 64, 3, 1, 1))
        ta, tb = g.split("trunk", x)
        a = conv("sib_a", ta, 64, 128, 1)
        b = conv("sib_b", tb, 64, 128, 1)
        x = g.relu("sum_relu", g.eltwise("sum", conv("res", a, 128, 128, 3, 1, 1), b))
        x = g.relu("dw_relu", conv("dw", x, 128, 128, 3, 1, 1, group=128))
        x = g.relu("pw_relu", conv("pw", x, 128, 96, 1))
        keep, sq = g.split("se_split", x)
        s = g.pool("se_gap", sq, 1, 1, avg=True, global_=True)
        s = g.relu("se_relu", _fc(g, "se_fc1", s, 96, 16))
        s = g.sigmoid("se_sigmoid", _fc(g, "se_fc2", s, 16, 96))
        x = g.scale_by("se_scale", keep, s)
        x = g.relu("in_relu", g.instance_norm("in", x, 96))
        h, t = g.split("heads", x)
        h = g.dropout("drop", h, 1.0)
        h = g.pool("gap", h, 1, 1, avg=True, global_=True)
        g.softmax("prob", _fc(g, "fc", h, 96, 10))
        g.relu("tail3_relu", conv("tail3", t, 96, 32, 3, 1, 1))
        param, _ = g.finish()
        _calibrate(param, g.bin, at)
        _MODEL["m"] = (param, bytes(g.bin), "data", OUTPUTS)
    return _MODEL["m"]


def deep_model():
    """-> (param, weights, input name, outputs): a 1x1 convolution 1024 -> 256 and its ReLU."""
    if "d" not in _MODEL:
        g = model_zoo.GraphBuilder(SEED + 1)
        x = g.input("data", 1024, 2, 2)
        x = g.conv("deep", x, 1024, 256, 1, gain=0.01)  # one-value planes: bias + a small sum, as the InnerProduct layers above
        _positive_bias(g, 256)
        g.relu("deep_relu", x)
        _MODEL["d"] = g.finish() + ("data", ("deep_relu",))
    return _MODEL["d"]


def shape_of(key):
    return SHAPES[key] if key in SHAPES else DEEP_SHAPES[key] if key in DEEP_SHAPES else MIXED_SHAPES[key]


def input(key, variant=0):
    """The input of a feed step: normal(0, 1), seeded by the step's key and variant."""
    return np.random.default_rng(zlib.crc32(f"lifecycle/{key}/{variant}".encode())).normal(0, 1, shape_of(key)).astype(np.float32)


_REF = {}


def reference(key, variant=0):
    """{blob: float32 array} of the float64 evaluator for one fed input; computed once, shared by every test, never written to."""
    if (key, variant) not in _REF:
        import seam_ref
        param, weights, name, _ = deep_model() if key in DEEP_SHAPES else model()
        blobs = seam_ref.Net(param, weights).run(name, input(key, variant), keep=True)
        for v in blobs.values():
            v.setflags(write=False)
        _REF[(key, variant)] = blobs
    return _REF[(key, variant)]


def _cycle():
    # A, B < A, C > A, A again
    return [("feed", "p14b4"), ("forward", 1), ("feed", "p7b1"), ("forward", 1), ("feed", "p14b8"), ("forward", 1), ("feed", "p14b4", 1), ("forward", 1)]


WALK_CYCLE = _cycle() * 3  # the second and third pass: net.memory() as after the first (PASS_ENDS)
PASS_ENDS = (len(_cycle()), 2 * len(_cycle()), 3 * len(_cycle()))

WALK_ROUTES = [
    ("feed", "p14b4"), ("forward", 1), ("extract", "relu1", "chained"), ("extract", "relu3", "chained"), ("extract", "relu4", "ok"),
    ("feed", "p8b4"), ("forward", 1), ("extract", "relu1", "chained"), ("extract", "pool2", "ok"), ("extract", "relu3", "ok"),
    ("feed", "p6b4"), ("forward", 1), ("extract", "pool2", "chained"), ("extract", "relu3", "chained"),
    ("feed", "odd5"), ("forward", 1), ("extract", "relu0", "ok"), ("extract", "relu1", "chained"), ("extract", "pool2", "ok"), ("extract", "relu3", "chained"),
    ("feed", "p3b1"), ("forward", 1), ("extract", "relu3", "ok"), ("extract", "sib_b", "ok"),
    ("feed", "p3b4"), ("forward", 1),
    ("feed", "p3b1", 1), ("forward", 1),
    ("feed", "odd5", 1), ("forward", 1), ("extract", "relu0", "ok"),
    ("feed", "p6b4", 1), ("forward", 1), ("extract", "relu0", "chained"),
    ("feed", "p7b1"), ("forward", 1), ("extract", "relu3", "ok"),
    ("feed", "p14b5"), ("forward", 1), ("extract", "relu3", "chained"),
    ("feed", "p14b4", 1), ("forward", 1), ("extract", "relu3", "chained"), ("extract", "relu4", "ok"),
    # the largest jumps: from the canvas plane to the smallest one and back up
    ("feed", "p3b4"), ("forward", 1), ("extract", "pool2", "ok"),
    ("feed", "p8b4", 1), ("forward", 1), ("extract", "relu3", "ok"),
    ("feed", "p14b4"), ("forward", 1), ("extract", "pool2", "chained"),
]

WALK_SETTERS = [
    ("feed", "p14b4"), ("forward", 1),
    ("set_tuned", True), ("forward", 1), ("set_tuned", False), ("forward", 1),
    ("set_concurrency", True), ("forward", 1), ("set_concurrency", False), ("forward", 1),
    ("set_graph", True), ("forward", 2), ("set_graph", False), ("forward", 2),
    ("stream",), ("forward", 2),
    # each setter once more, with a shape change in the same gap
    ("set_tuned", True), ("feed", "p8b4"), ("forward", 1),
    ("set_concurrency", True), ("feed", "p3b1"), ("forward", 1),
    ("set_graph", True), ("feed", "p14b4", 1), ("forward", 2),
    ("stream",), ("feed", "p6b4"), ("forward", 2),
    ("set_tuned", False), ("set_concurrency", False), ("set_graph", False), ("feed", "p14b4"), ("forward", 2),
]

# starts with the graph on: capture, replay twice, new VALUES at the same shape (the replay must see them), a new shape, replay, off, on
WALK_GRAPH = [
    ("feed", "p14b4"), ("forward", 1), ("forward", 2),
    ("feed", "p14b4", 1), ("forward", 1),
    ("feed", "p8b4"), ("forward", 1), ("forward", 1),
    ("feed", "p14b4"), ("forward", 2),
    ("set_graph", True), ("forward", 1), ("feed", "p6b4"), ("forward", 1),
    ("set_graph", False), ("forward", 1), ("forward", 1), ("feed", "p14b4", 1), ("forward", 2),
]

# sub_batches = 3: 7 -> 2 -> 1 images (replicas sit out), a size change while two of them sit out, and all of them back at the new size
WALK_REPLICAS = [
    ("feed", "p8b7"), ("forward", 1), ("feed", "p8b2"), ("forward", 1), ("feed", "p8b1"), ("forward", 1),
    ("feed", "p6b1"), ("forward", 1), ("feed", "p6b7"), ("forward", 1), ("feed", "p8b7", 1), ("forward", 2),
    ("feed", "p8b2", 1), ("forward", 1), ("feed", "p8b7"), ("forward", 1),
]

# the 1024 -> 256 1x1 layer between planes that pack a different second weight image behind the same byte count, in both directions
WALK_DEEP = [
    ("feed", "d2x2"), ("forward", 1), ("feed", "d1x1"), ("forward", 1), ("feed", "d2x2", 1), ("forward", 1),
    ("feed", "d3x1"), ("forward", 1), ("feed", "d1x1", 1), ("forward", 1),
]

WALKS = {"cycle": WALK_CYCLE, "routes": WALK_ROUTES, "setters": WALK_SETTERS, "graph": WALK_GRAPH, "replicas": WALK_REPLICAS, "deep": WALK_DEEP}


# ---- a third model: int8 layers among fp32 ones ---------------------------------------------------------------------------------------
# (3 input channels, at most 128 anywhere; Net.SetQuantized)  What is checked after every Forward is the fresh-net invariant above, bit for bit,
# and every int8 layer against its restatement from the device's own bottom blob (tests/qseam_ref.py); the fp32 layers against float64
# from there.
#
#   data -> conv0 (3 -> 16, 3x3 p1, fp32) + ReLU                            a fp32 first layer in front of an int8 layer: never absorbed
#        -> q1 (16 -> 32) + ReLU -> q2 (32 -> 32) + ReLU + 2x2 max pool     an int8 3x3 run; the pooling stays a layer
#        -> qdw (depthwise 3x3, 32) + ReLU -> qpw (32 -> 72, 1x1) + ReLU    an int8 depthwise + 1x1 pair (72: inside the fp32 pair's range)
#        -> qbn (72 -> 64, 3x3 p1) + BatchNorm + Scale + ReLU                the level-2 fold into d[] and the bias
#        -> Split -> qa (64 -> 64, 1x1, int8)
#                 -> fb (64 -> 64, 3x3 p1, fp32) + Eltwise with qa + ReLU    the fp32 branch takes the add with the int8 branch's top
#        -> global average pooling -> out (InnerProduct 64 -> 10, int8)
MIXED_SHAPES = {
    "m16b4": (4, 3, 16, 16), "m16b5": (5, 3, 16, 16), "m16b1": (1, 3, 16, 16), "m12b4": (4, 3, 12, 12), "modd4": (4, 3, 13, 21),
    "m16b7": (7, 3, 16, 16), "m16b2": (2, 3, 16, 16), "m12b1": (1, 3, 12, 12), "m12b7": (7, 3, 12, 12),
}
MIXED_INT8 = ("q1", "q2", "qdw", "qpw", "qbn", "qa", "out")
MIXED_OUTPUTS = ("out", "sum_relu")
MIXED_SHIFT = 3.0
MIXED_FP32 = ("conv0", "relu0", "fb", "sum", "sum_relu")  # the convolution planes float64 is the yardstick of: they keep PLANE_FLOOR


def mixed_model():
    """-> (param, weights, input name, outputs)."""
    if "x" not in _MODEL:
        g = model_zoo.GraphBuilder(SEED + 2)
        x = g.input("data", 3, 16, 16)
        x = g.relu("relu0", g.conv("conv0", x, 3, 16, 3, 1, 1))
        x = g.relu("relu1", g.conv("q1", x, 16, 32, 3, 1, 1, quant=True))
        x = g.relu("relu2", g.conv("q2", x, 32, 32, 3, 1, 1, quant=True))
        x = g.pool("pool2", x, 2, 2)
        x = g.relu("qdw_relu", g.conv("qdw", x, 32, 32, 3, 1, 1, group=32, quant=True))
        x = g.relu("qpw_relu", g.conv("qpw", x, 32, 72, 1, quant=True))
        x = g.conv("qbn", x, 72, 64, 3, 1, 1, quant=True)
        x = g.relu("qbn_relu", g.scale("qbn_scale", g.bn("qbn_bn", x, 64), 64))
        ta, tb = g.split("trunk", x)
        a = g.conv("qa", ta, 64, 64, 1, quant=True)
        fb = g.conv("fb", tb, 64, 64, 3, 1, 1)
        # no plane behind the sum's ReLU may die (see the module docstring): the fp32 branch's biases, the last 64 floats written, lift every
        # channel of the sum by MIXED_SHIFT, one and a half of its standard deviations (the global average behind it sums values >= 0)
        g.bin[-4 * 64:] = (np.frombuffer(bytes(g.bin[-4 * 64:]), "<f4") + np.float32(MIXED_SHIFT)).astype("<f4").tobytes()
        x = g.relu("sum_relu", g.eltwise("sum", fb, a))
        x = g.pool("gap", x, 1, 1, avg=True, global_=True)
        g.fc("out", x, 64, 10, quant=True)
        _MODEL["x"] = g.finish() + ("data", MIXED_OUTPUTS)
    return _MODEL["x"]


# batches 4 -> 5 -> 1 -> 4; planes 16 -> 12 -> 13 x 21 and back; the three setters flipped between Forwards; graph on with a feed of a new
# shape; use_current_stream
WALK_MIXED = [
    ("feed", "m16b4"), ("forward", 1), ("feed", "m16b5"), ("forward", 1), ("feed", "m16b1"), ("forward", 1), ("feed", "m16b4", 1), ("forward", 1),
    ("feed", "m12b4"), ("forward", 1), ("feed", "modd4"), ("forward", 1), ("feed", "m16b4"), ("forward", 1),
    ("set_tuned", True), ("forward", 1), ("set_concurrency", True), ("forward", 1), ("set_graph", True), ("forward", 2),
    ("feed", "m12b4", 1), ("forward", 2), ("feed", "modd4", 1), ("forward", 1),
    ("set_graph", False), ("set_tuned", False), ("set_concurrency", False), ("forward", 1),
    ("stream",), ("forward", 2), ("feed", "m16b5", 1), ("forward", 1),
]
# sub_batches = 3 at batches 7, 2 and 1 (one replica, then two, get no image), a new size while they sit out, and all back
WALK_MIXED_REPLICAS = [
    ("feed", "m16b7"), ("forward", 1), ("feed", "m16b2"), ("forward", 1), ("feed", "m16b1"), ("forward", 1),
    ("feed", "m12b1"), ("forward", 1), ("feed", "m12b7"), ("forward", 1), ("feed", "m16b7", 1), ("forward", 2),
]
MIXED_WALKS = {"mixed": WALK_MIXED, "mixed_replicas": WALK_MIXED_REPLICAS}


def mixed_table():
    """[(walk name, fusion level, Net keywords)]: the mixed walk at the five settings of LEVELS; the replica walk at levels 2 and 3 + tuned,
    with and without graph."""
    rows = [("mixed", lv, dict(kw)) for lv, kw in LEVELS]
    rows += [("mixed_replicas", lv, dict(kw, sub_batches=3, **g)) for lv, kw in ((2, {}), (3, {"tuned": True})) for g in ({}, {"graph": True})]
    return rows


def setting_id(level, kw):
    return f"{level}" + "".join(f"+{k}" for k in ("tuned", "concurrency", "graph") if kw.get(k)) + (f"+r{kw['sub_batches']}" if kw.get("sub_batches") else "")


def table():
    """[(walk name, fusion level, Net keywords)]: cycle, routes and setters at the five settings of seam_cases.LEVELS; graph at levels 1 and
    3 + tuned, graph on from the start; replicas (sub_batches = 3) at levels 2 and 3 + tuned, with and without graph; deep at 1 and 3 + tuned + graph."""
    rows = [(w, lv, dict(kw)) for w in ("cycle", "routes", "setters") for lv, kw in LEVELS]
    rows += [("graph", 1, {"graph": True}), ("graph", 3, {"tuned": True, "graph": True})]
    rows += [("replicas", lv, dict(kw, sub_batches=3, **g)) for lv, kw in ((2, {}), (3, {"tuned": True})) for g in ({}, {"graph": True})]
    rows += [("deep", 1, {}), ("deep", 3, {"tuned": True, "graph": True})]
    return rows


def row_id(row):
    return f"{row[0]}@{setting_id(row[1], row[2])}"
