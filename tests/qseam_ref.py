"""The re-based comparison of a net that holds int8 layers next to fp32 ones (tests/test_qseams_cpu.py, tests/test_qseams_gpu.py).

An int8 layer rounds x * s_in to an integer, so a last-bit difference in its producer can move a value across a half and an output by
|w_q| * d: an end-to-end float64 comparison would fail at random.  The net is compared in three stages, each from what the device produced:

  1. the fp32 layers in front of the first int8 layer against seam_ref (float64) by plane_nerr;
  2. every int8 layer restated with qconv_ref from the DEVICE's own bottom blob (the fed input where the layer reads it), with what the
     fusion level absorbed applied -- a plain ReLU, and at level 2 the BatchNorm / Scale / BatchNorm + Scale composition through
     qconv_ref.fold -- and compared with the first blob behind it that has storage by np.array_equal;
  3. the fp32 layers behind it in float64 from the device's int8 output (seam_ref.Net.run's `given`), by plane_nerr.

`plan(R, i, level)` is the claim: which layers the int8 layer i absorbs, from the conditions of ConvLayer::Fuse / InnerProductLayer::Fuse
(net_layers.h) for a side route -- `side_epilogues_only()`: a plain ReLU at level >= 1 and, for a convolution that has no activation yet,
an affine layer over its channels at level 2; nothing else, whatever follows.  `int8_layers(R, x, dev, level)` runs stage 2 on a device
(anything with Extract() and layers()) and asserts the claim on its layer list first; `own(R, x, level)` is the same evaluation fed its own
blobs, which needs no device.
"""
from __future__ import annotations

import zlib

import numpy as np

import qconv_ref as Q
import seam_ref as R_

F = np.float32


def _readers(layers, blob):
    return [j for j, l in enumerate(layers) if blob in l[2]]


def _plain_relu(layer):
    return layer[0] == "ReLU" and float(layer[4].get(0, 0.0)) == 0.0


def _affine(layer, k):
    return layer[0] in ("BatchNorm", "Scale") and len(layer[2]) == 1 and layer[4].get(0, 0) == k


def _next(layers, i, top):
    """The layer fuse_layers would offer layer i behind `top`: its sole reader, further down the list, with one bottom and one top."""
    rd = _readers(layers, top)
    if len(rd) != 1 or rd[0] <= i or len(layers[rd[0]][2]) != 1 or len(layers[rd[0]][3]) != 1:
        return None
    return rd[0]


def plan(net, i, level):
    """[indices of the layers that int8 layer i absorbs at fusion `level`], in order."""
    layers = net.layers
    type_, _, _, tops, pd = layers[i]
    k, out, relu, top = pd.get(0, 0), [], False, tops[0]
    while level >= 1:
        j = _next(layers, i, top)
        if j is None:
            break
        if _plain_relu(layers[j]):
            relu = True
        elif not (level >= 2 and type_ != "InnerProduct" and not relu and _affine(layers[j], k)):
            break
        out.append(j)
        top = layers[j][3][0]
    return out


def restate(net, i, bottom, absorbed):
    """Layer i of `net` (a seam_ref.Net) on the fp32 array `bottom`, with the layers `absorbed` (indices, in order) taken into it."""
    type_, name, _, _, pd = net.layers[i]
    q = net.q[name]
    v = np.asarray(bottom, F)
    if type_ == "InnerProduct":
        v, s, p = v.reshape(v.shape[0], -1, 1, 1), 1, 0
    else:
        s, p = pd.get(3, 1), pd.get(4, 0)
        assert pd.get(13, s) == s and pd.get(14, p) == p and pd.get(2, 1) == 1
    # the integer sums depend on the bottom alone, and the settings of one case mostly hand over the same bits: kept per layer and bottom
    memo = net.__dict__.setdefault("_acc", {})
    key = (i, v.shape, zlib.crc32(v.tobytes()))
    if key not in memo or not np.array_equal(memo[key][0].view(np.int32), v.view(np.int32)):
        memo[key] = (v.copy(), Q.accumulate(Q.quantise(v, q["s_in"]), q["wq"], q["group"], (s, s), (p, p, p, p)))
    acc = memo[key][1]
    d, b, relu, affine = Q.dequant_scales(q["s_w"], q["s_in"]), q["b"], False, None
    for j in absorbed:
        layer = net.layers[j]
        if _plain_relu(layer):
            relu = True
            continue
        assert layer[0] in ("BatchNorm", "Scale") and not relu and type_ != "InnerProduct", (name, layer[:2], "cannot be absorbed by an int8 layer")
        m, a = net.w[layer[1]]
        m = np.asarray(m, F)
        a = np.zeros_like(m) if a is None else np.asarray(a, F)
        affine = (m, a) if affine is None else ((affine[0] * m).astype(F), ((affine[1] * m).astype(F) + a).astype(F))
    if affine is not None:
        d, b = Q.fold(d, b, *affine)
    return Q.dequantise(acc, d, b, relu)


def int8_indices(net):
    return [i for i, l in enumerate(net.layers) if R_.is_int8(l)]


def int8_layers(net, x, dev, level, route="QCONV"):
    """Stage 2 on a device that has run Forward on `x`: -> `given` for seam_ref.Net.run (the device's int8 outputs; None for the blobs
    inside an int8 layer's fusion).  Asserts, in this order, that the device's layer list shows each int8 layer on `route` with exactly the
    layers of plan() gone behind it, that its bottom blob can be extracted, and that its output equals the restatement bit for bit."""
    info = dev.layers()
    names = {n: a for _, n, a in info}
    given = {}
    for i in int8_indices(net):
        type_, name, bottoms, tops, _ = net.layers[i]
        assert name in names, f"int8 layer {name} is not a layer of its own at level {level}: {info}"
        if route is not None:
            assert names[name] == route, (name, names[name])
        want = plan(net, i, level)
        gone, top = [], tops[0]
        while True:  # what the device absorbed: the run of missing layers behind it
            j = _next(net.layers, i, top)
            if j is None or net.layers[j][1] in names:
                break
            gone.append(j)
            top = net.layers[j][3][0]
        assert gone == want, f"int8 layer {name} at level {level} absorbed {[net.layers[j][1] for j in gone]}, the claim is {[net.layers[j][1] for j in want]}"
        fed = any(l[0] == "Input" and bottoms[0] in l[3] for l in net.layers)
        bottom = np.asarray(x, F) if fed else dev.Extract(bottoms[0])  # an Extract that is refused (a chained blob) fails the test
        y = restate(net, i, bottom, gone)
        got = dev.Extract(top)
        assert got.shape == y.shape, (name, got.shape, y.shape)
        bad = int((got != y).sum()) if not np.array_equal(got, y) else 0
        assert bad == 0 and np.array_equal(got, y), f"int8 layer {name} (level {level}, batch {len(x)}): {bad} of {y.size} values differ from the restatement, max |diff| {np.abs(got.astype(np.float64) - y).max():.3e}"
        for j in [i] + gone:
            given[net.layers[j][3][0]] = None
        given[top] = got
    return given


def own(net, x, level):
    """Every blob of `net` on `x` with no device: float64 (seam_ref) for the fp32 layers, the restatement at `level` for the int8 ones, each
    fed the blob this evaluation itself computed.  Blobs inside an int8 layer's fusion are absent."""
    all_layers, given = net.layers, {}
    name = all_layers[0][3][0]
    try:
        for i in int8_indices(net):
            if all_layers[i][3][0] in given:
                continue
            net.layers = all_layers[:i]
            given.update(net.run(name, x, keep=True, given=given))
            gone = plan(_View(all_layers), i, level)
            net.layers = all_layers
            y = restate(net, i, given[all_layers[i][2][0]], gone)
            for j in [i] + gone:
                given[all_layers[j][3][0]] = None
            given[all_layers[([i] + gone)[-1]][3][0]] = y
        net.layers = all_layers
        blobs = net.run(name, x, keep=True, given=given)
    finally:
        net.layers = all_layers
    return {k: v for k, v in blobs.items() if v is not None}


class _View:
    """Another layer list for plan() (own() shortens the net's own while it runs)."""

    def __init__(self, layers):
        self.layers = layers
