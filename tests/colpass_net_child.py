"""Child of tests/test_colpass_net_gpu.py: `colpass_net_child.py <mode>` runs the four-convolution net 3 -> 64 -> 64 (pool) -> 128 -> 128 at
224 pixels and batch 1, fusion level 3, at fhip_net_set_colpass `mode`, two eager forwards, and prints the layers on the column-passed
route; a refused Reshape prints `refused: <message>`.  net() builds the net for the tests as well."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def net(mode, batch=1, graph=False, seed=3):
    """-> (Net at `mode` with its input fed, the input)"""
    from feathercnn_amd import model_zoo
    from feathercnn_amd.net import Net
    g = model_zoo.GraphBuilder(21)
    x = g.input("data", 3, 224, 224)
    x = g.relu("r1", g.conv("c1", x, 3, 64, 3, 1, 1))
    x = g.pool("p2", g.relu("r2", g.conv("c2", x, 64, 64, 3, 1, 1)), 2, 2)
    x = g.relu("r3", g.conv("c3", x, 64, 128, 3, 1, 1))
    x = g.relu("r4", g.conv("c4", x, 128, 128, 3, 1, 1))
    param, weights = g.finish()
    n = Net(fusion=3, graph=graph, tuned=True)
    if mode is not None:
        n.SetColpass(mode)
    n.LoadParam(param)
    n.LoadWeights(weights)
    img = np.random.default_rng(seed).uniform(-1, 1, (batch, 3, 224, 224)).astype(np.float32)
    n.FeedInput("data", img)
    return n, img


def main(mode):
    from feathercnn_amd import FeatherHipError
    mapped = "mapped" if "libfeather_colpass." in open("/proc/self/maps").read() else "unmapped"
    try:
        n, _ = net(mode)
        for _ in range(2):
            n.Forward()
        assert np.isfinite(n.Extract("r4")).all()
        names = [n.layers()[k][1] for k in n.colpasses()]
        mapped = "mapped" if "libfeather_colpass." in open("/proc/self/maps").read() else "unmapped"
        print("colpass layers:", ",".join(names) or "none", mapped)
        print("child ok")
    except FeatherHipError as e:
        print("refused:", str(e).replace("\n", " "), mapped)


if __name__ == "__main__":
    main(int(sys.argv[1]))
