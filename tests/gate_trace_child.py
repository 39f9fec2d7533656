"""Child process of tests/test_gate_gpu.py's kernel-trace test: one Forward of a residual squeeze-and-excitation block (Caffe spelling, 64
channels on 14 x 14, Eltwise + ReLU) between two Input blobs at fusion level 2, bracketed by two fhip_relu launches so that the trace can be
cut at them.  Prints the three kernel names fhip_gate_route reports for the block's shapes ("route <name>") and checks the result."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def model():
    from feathercnn_amd import model_zoo
    g = model_zoo.GraphBuilder(3)
    x = g.input("x", 64, 14, 14)
    short = g.input("short", 64, 14, 14)
    y = g.se_block("se", x, 64, 4, "caffe")
    g.relu("out", g.eltwise("sum", short, y))
    return g.finish()


def main():
    import gate_ref as R
    import ktrace
    import torch
    from feathercnn_amd.gate import gate_route
    from feathercnn_amd.net import Net
    rng = np.random.default_rng(1)
    x, short = (rng.normal(0, 1, (4, 64, 14, 14)).astype(np.float32) for _ in range(2))
    p, w = model()
    net = Net(fusion=2)
    net.LoadParam(p)
    net.LoadWeights(w)
    net.FeedInput("x", x)
    net.FeedInput("short", short)
    net.Forward()  # the first Forward reshapes and uploads the weights; the traced one only launches
    assert [(t, nm, a) for t, nm, a in net.layers()][-1] == ("Pooling", "se_gap", "GATE"), net.layers()
    ktrace.marker()
    net.Forward()
    ktrace.marker()
    got = net.Extract("out")
    net.close()
    xt = torch.from_numpy(x).cuda()
    for op in ("squeeze", "excite", "apply"):
        print("route", gate_route(op, xt))
    assert R.nerr(got, _want(R, p, w, x, short)) <= 1e-4
    print("child ok")


def _want(R, p, w, x, short):
    net = R.Net(p, w)
    blobs = {"x": x, "short": short}
    # two inputs: run the layers on both (R.Net.run feeds one)
    layers = net.layers
    net.layers = [l for l in layers if l[0] != "Input"]
    try:
        out = None
        for layer in net.layers:
            type_, name, bottoms, tops, pd = layer
            if type_ == "Split":
                for t in tops:
                    blobs[t] = blobs[bottoms[0]]
                continue
            if len(bottoms) == 2:
                a, b = blobs[bottoms[0]], blobs[bottoms[1]]
                y = R.channel_gate(a, b) if type_ == "ScaleBy" else a + b
            else:
                net.layers = [layer]
                y = R.Net.run(net, bottoms[0], blobs[bottoms[0]], tops[0], keep=True)[tops[0]]
            blobs[tops[0]] = out = np.ascontiguousarray(y, np.float32)
        return out
    finally:
        net.layers = layers


if __name__ == "__main__":
    main()
