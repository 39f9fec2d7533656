"""Child process of tests/test_side_contract_gpu.py: `side_missing_child.py <library>` runs, on an 8-channel 8x8 input at batch 1, first a net
that does not need the side library and then each of the smallest nets that route a layer to it, and prints one line per net: `<tag> ran`
or `<tag> refused: <message>`, followed by whether /proc/self/maps holds the library.  NETS is the table of those nets."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# library -> (the Net switch its layers need, the fusion level or None for the default, {tag: the layers behind the input `x` of builder `g`})
NETS = {
    "gconv": (None, None, {"grouped": lambda g, x: g.conv("l", x, 8, 8, 3, 1, 1, group=2)}),
    "deconv": (None, None, {"deconv": lambda g, x: g.deconv("l", x, 8, 8, 4, 2, 1)}),
    "inorm": (None, None, {"inorm": lambda g, x: g.instance_norm("l", x, 8, affine=False), "leaky": lambda g, x: g.relu("l", x, slope=0.2),
                           "tanh": lambda g, x: g.tanh("l", x)}),
    "shuffle": (None, None, {"shuffle": lambda g, x: g.shuffle("l", x, 2)}),
    "atrous": ("SetDilated", None, {"dilated": lambda g, x: g.conv("l", x, 8, 8, 3, 1, 2, dilation=2)}),
    "gate": (None, None, {"swish": lambda g, x: g.swish("l", x)}),
    "resample": ("SetExtendedLayers", None, {"hardswish": lambda g, x: g.hard_swish("l", x)}),
    "lrn": ("SetExtendedLayers", 2, {"lrn": lambda g, x: g.lrn("l", x, 5, 1.0, 0.75), "lrnpool": lambda g, x: g.pool("l", g.lrn("n", x, 3, 1.0, 0.75), 3, 2)}),
    "qconv": ("SetQuantized", 1, {"quant": lambda g, x: g.conv("l", x, 8, 8, 3, 1, 1, quant=True)}),
}


def main(name):
    from feathercnn_amd import FeatherHipError, model_zoo
    from feathercnn_amd.net import Net
    switch, fusion, needing = NETS[name]
    mapped = lambda: "mapped" if f"libfeather_{name}." in open("/proc/self/maps").read() else "unmapped"
    for tag, layers in [("plain", lambda g, x: g.relu("l", x))] + list(needing.items()):
        g = model_zoo.GraphBuilder(7)
        layers(g, g.input("data", 8, 8, 8))
        param, weights = g.finish()
        net = Net() if fusion is None else Net(fusion=fusion)
        if switch:
            getattr(net, switch)(True)  # the switch alone opens nothing
        net.LoadParam(param)
        net.LoadWeights(weights)
        try:
            net.FeedInput("data", np.ones((1, 8, 8, 8), np.float32))
            net.Forward()
            net.Extract("l")
            print(tag, "ran", mapped())
        except FeatherHipError as e:
            print(tag, "refused:", str(e).replace("\n", " "), mapped())


if __name__ == "__main__":
    main(sys.argv[1])
