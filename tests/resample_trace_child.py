"""Child process of tests/test_resample_gpu.py's kernel-trace test: one Forward of an upsample-add-ReLU (a nearest x2 Interp of `x`, an
Eltwise SUM with `lat`, a ReLU; 32 channels, 14 x 14 -> 28 x 28) between two Input blobs at fusion level 2, bracketed by two fhip_relu
launches so that the trace can be cut at them.  Prints the kernel name fhip_interp_route reports for the shapes ("route <name>") and
checks the result against the float32 restatement, bit for bit."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def model():
    from feathercnn_amd import model_zoo
    g = model_zoo.GraphBuilder(3)
    x = g.input("x", 32, 14, 14)
    lat = g.input("lat", 32, 28, 28)
    g.relu("out", g.eltwise("sum", lat, g.interp("up", x, "nearest", scale=2.0)))
    return g.finish()


def main():
    import ktrace
    import resample_ref as R
    import torch
    from feathercnn_amd.net import Net
    from feathercnn_amd.resample import interp_route
    rng = np.random.default_rng(1)
    x = rng.normal(0, 1, (4, 32, 14, 14)).astype(np.float32)
    lat = rng.normal(0, 1, (4, 32, 28, 28)).astype(np.float32)
    p, w = model()
    net = Net(fusion=2)
    net.SetExtendedLayers(True)
    net.LoadParam(p)
    net.LoadWeights(w)
    net.FeedInput("x", x)
    net.FeedInput("lat", lat)
    net.Forward()  # the first Forward reshapes; the traced one only launches
    assert [(t, nm, a) for t, nm, a in net.layers()][-1] == ("Interp", "up", "RESAMPLE") and len(net.layers()) == 3, net.layers()
    ktrace.marker()
    net.Forward()
    ktrace.marker()
    got = net.Extract("out")
    net.close()
    print("route", interp_route(torch.from_numpy(x).cuda(), "nearest", scale=2.0))
    want = R.interp(x, R.NEAREST, 28, 28, height_scale=2.0, width_scale=2.0, residual=lat, relu=True)
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    print("child ok")


if __name__ == "__main__":
    main()
