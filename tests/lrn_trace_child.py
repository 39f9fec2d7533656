"""Child process of tests/test_lrn_gpu.py's kernel-trace test: one Forward of each of two nets at fusion level 2 -- `fused`, an LRN (across
96 channels of 27 x 27, local_size 5) with a 3 x 3 / stride-2 max pooling behind it, which level 2 makes one layer, and `plain`, the same
LRN alone -- separated by three fhip_relu launches so that the trace can be cut at them.  Prints the kernel names fhip_lrn_pool_route and
fhip_lrn_route report for the shapes ("route <name>", in that order) and checks both results against the library called directly."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

SHAPE = (4, 96, 27, 27)
LRN = dict(local_size=5, alpha=5.0, beta=0.75)


def models():
    from feathercnn_amd import model_zoo
    g = model_zoo.GraphBuilder(3)
    g.pool("pool", g.lrn("norm", g.input("x", *SHAPE[1:]), LRN["local_size"], LRN["alpha"], LRN["beta"]), 3, 2)
    h = model_zoo.GraphBuilder(3)
    h.lrn("norm", h.input("x", *SHAPE[1:]), LRN["local_size"], LRN["alpha"], LRN["beta"])
    return g.finish(), h.finish()


def main():
    import ktrace
    import torch
    from feathercnn_amd import lrn, lrn_pool, lrn_pool_route, lrn_route
    from feathercnn_amd.net import Net
    x = np.random.default_rng(1).normal(0, 1, SHAPE).astype(np.float32)
    nets = []
    for (p, w), want in zip(models(), ([("Input", "x", None), ("LRN", "norm", "LRN")],) * 2):
        net = Net(fusion=2)
        net.SetExtendedLayers(True)
        net.LoadParam(p)
        net.LoadWeights(w)
        net.FeedInput("x", x)
        net.Forward()  # the first Forward reshapes; the traced one only launches
        assert net.layers() == want, net.layers()
        nets.append(net)
    ktrace.marker()
    nets[0].Forward()
    ktrace.marker()
    nets[1].Forward()
    ktrace.marker()
    fused, plain = nets[0].Extract("pool"), nets[1].Extract("norm")
    for net in nets:
        net.close()
    xd = torch.from_numpy(x).cuda()
    pool = {"kernel": 3, "stride": 2}
    print("route", lrn_pool_route(xd, pool, LRN["local_size"]))
    print("route", lrn_route(xd, LRN["local_size"]))
    assert np.array_equal(fused.view(np.int32), lrn_pool(xd, pool, **LRN).cpu().numpy().view(np.int32)) and fused.shape == (4, 96, 13, 13)
    assert np.array_equal(plain.view(np.int32), lrn(xd, **LRN).cpu().numpy().view(np.int32))
    print("child ok")


if __name__ == "__main__":
    main()
