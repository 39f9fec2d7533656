"""Child process of tests/test_detect_gpu.py, the way tests/side_missing_child.py serves the routed libraries: on an 8-channel 8x8 input at
batch 1 it runs a net that does not need libfeather_detect.so -- with the detection switch on, Concat and Softmax included -- and then the
smallest nets that route a layer to it, and prints one line per net: `<tag> ran` or `<tag> refused: <message>`, followed by whether
/proc/self/maps holds the library."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NETS = {
    "plain": lambda g, x: g.flatten("l", g.concat("c", g.split("s", g.relu("r", x)), 2)),  # views and copies: no kernel of the library
    "permute": lambda g, x: g.permute("l", x, 3),
    "normalize": lambda g, x: g.normalize("l", x, 8),
    "priorbox": lambda g, x: g.priorbox("l", x, x, [2.0]),
}


def main():
    from feathercnn_amd import FeatherHipError, model_zoo
    from feathercnn_amd.net import Net
    mapped = lambda: "mapped" if "libfeather_detect." in open("/proc/self/maps").read() else "unmapped"
    for tag, layers in NETS.items():
        g = model_zoo.GraphBuilder(7)
        layers(g, g.input("data", 8, 8, 8))
        param, weights = g.finish()
        net = Net()
        net.SetDetection(True)  # the switch alone opens nothing
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
    main()
