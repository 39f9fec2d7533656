"""The plan snapshot of feather::Net (tests/test_net_plan_snapshot_gpu.py, tests/golden/make_net_plan_snapshot.py): a table of nets, fusion
levels and fed shapes, and `run(row)`, which walks one Net handle through a row's shapes and records after each Forward everything the
introspection API reports -- the planned layer list with route names, every convolution's geometry as it runs, the absorbed pointwise
layers, sibling pairs, residual adds, chained runs, canvases and the memory sums.  Structure only, no tensor data: the record depends on
the host-side planning code (feathercnn_amd/csrc/net_conv.h, net_layers.h, net_plan.h) and on what the library's can_* / select_algo
entry points answer, not on what a kernel computes.  The committed record (tests/golden/net_plan_snapshot.json) was generated from the
commit before the convolution layer's state was regrouped; a change of what is fused or planned has to regenerate it and say so.

Rows:
  * the life-cycle model of lifecycle_cases.py (a first layer, 3x3 runs, a sibling pair, a dw + pw pair, residuals, pooling) at one shape of
    each of its classes, and one three-step row that un-plans and re-plans the canvases, the chain and the siblings (28 px batch 4 -> 6 px
    batch 1 -> 28 px batch 8);
  * tiny_allsorts, tiny_plain, tiny_grouped, tiny_dilated, tiny_deconv, tiny_se, tiny_quant at batch 4, and tiny_allsorts through batch 4 -> 3;
  all of these at fusion levels 0 .. 3 (level 3 with tuned selection, as seam_cases.LEVELS);
  * VGG-16, ResNet-50 and MobileNet-V1 (10 classes: small fc weights) at 224 px, fusion level 3 with tuned selection, batch 4 then batch 8 on
    one handle: the 14- and 56-px canvas stretches, the head fusion, the sibling pairs and the one-kernel dw + pw pairs, and a re-plan each.
"""
from __future__ import annotations

import zlib

import numpy as np

LEVELS = ((0, {}), (1, {}), (2, {}), (3, {"tuned": True}))
LIFE = (("canvas14", "p14b4"), ("f43", "p8b4"), ("one_tile", "p6b4"), ("odd", "odd5"), ("below4", "p3b4"))
LIFE_WALK = ("p14b4", "p3b1", "p14b8")
# net -> (input size, the Net switches it needs)
TINY = {"tiny_allsorts": (20, ()), "tiny_plain": (8, ()), "tiny_grouped": (21, ()), "tiny_dilated": (16, ("SetDilated",)),
        "tiny_deconv": (16, ()), "tiny_se": (24, ()), "tiny_quant": (16, ("SetQuantized",))}
BIG = ("vgg16", "resnet50", "mobilenet_v1")


def table():
    """[(id, net, fusion level, Net keywords, (fed shape, ...))]"""
    import lifecycle_cases as lc
    rows = []
    for lv, kw in LEVELS:
        rows += [(f"life/{cls}@{lv}", "life", lv, kw, (lc.SHAPES[key],)) for cls, key in LIFE]
        rows.append((f"life/walk@{lv}", "life", lv, kw, tuple(lc.SHAPES[k] for k in LIFE_WALK)))
        rows += [(f"{name}@{lv}", name, lv, kw, ((4, 3, size, size),)) for name, (size, _) in TINY.items()]
        rows.append((f"tiny_allsorts/walk@{lv}", "tiny_allsorts", lv, kw, ((4, 3, 20, 20), (3, 3, 20, 20))))
    rows += [(f"{name}/walk@3", name, 3, {"tuned": True}, ((4, 3, 224, 224), (8, 3, 224, 224))) for name in BIG]
    return rows


_MODELS = {}


def model(name):
    """-> (param, weights, input name, Net switches); built once per process."""
    if name not in _MODELS:
        from feathercnn_amd import model_zoo
        if name == "life":
            import lifecycle_cases as lc
            _MODELS[name] = lc.model()[:3] + ((),)
        elif name in TINY:
            _MODELS[name] = getattr(model_zoo, name)()[:3] + (TINY[name][1],)
        else:
            _MODELS[name] = getattr(model_zoo, name)(classes=10)[:3] + ((),)
    return _MODELS[name]


def _fields(p):
    return [int(getattr(p, f)) for f, _ in p._fields_]


def snapshot(net):
    """Everything the introspection API reports, as JSON types (integer keys as strings, tuples as lists)."""
    return {
        "layers": [list(t) for t in net.layers()],
        "conv_params": {str(i): _fields(p) + [b] for i, (p, b) in net.conv_params().items()},
        "fused_pointwise": {str(i): _fields(p) + [int(one)] for i, (p, one) in net.fused_pointwise().items()},
        "siblings": {str(i): v for i, v in net.siblings().items()},
        "residuals": {str(i): v for i, v in net.residuals().items()},
        "chains": {str(i): list(v) for i, v in net.chains(raw=True).items()},
        "canvases": list(net.canvases()),
        "memory": net.memory(),
    }


def conv_param_fields():
    """The order of a conv_params / fused_pointwise row (the batch, or the one-kernel flag, follows)."""
    from feathercnn_amd import _lib
    return [f for f, _ in _lib.fhip_conv_param._fields_]


def run(row):
    """One Net handle through the row's shapes: [snapshot after the Forward of each]."""
    from feathercnn_amd.net import Net
    rid, name, level, kw, shapes = row
    param, weights, inp, switches = model(name)
    net = Net(fusion=level, **kw)
    for sw in switches:
        getattr(net, sw)(True)
    net.LoadParam(param)
    net.LoadWeights(weights)
    out = []
    for k, shape in enumerate(shapes):
        net.FeedInput(inp, np.random.default_rng(zlib.crc32(f"plan/{rid}/{k}".encode())).uniform(-1, 1, shape).astype(np.float32))
        net.Forward()
        net.synchronize()
        out.append(snapshot(net))
    net.close()
    return out
