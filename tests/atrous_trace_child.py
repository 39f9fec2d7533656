"""Child of tests/test_atrous_gpu.py's kernel-trace test, run under rocprofv3 in a process of its own: one forward of tiny_dilated, and on
stdout one `ROUTE <instantiation>` line per dilated layer -- what fhip_atrous_route reports for the layer as it runs."""
import numpy as np

from feathercnn_amd import AtrousConv, AtrousParam, model_zoo
from feathercnn_amd.net import Net

import atrous_ref as R


def main():
    p, b, i, o = model_zoo.tiny_dilated()
    x = np.random.default_rng(1).uniform(-1, 1, (2, 3, 16, 16)).astype(np.float32)
    net = Net(fusion=2)
    net.SetDilated(True)
    net.LoadParam(p)
    net.LoadWeights(b)
    net.FeedInput(i, x)
    net.Forward()
    y = net.Extract(o)
    blobs = R.Net(p, b).run(i, x, o, keep=True)
    assert R.nerr(y, blobs[o]) <= 1e-4
    for type_, name, bottoms, tops, pd in R.Net(p, b).layers:
        if name not in model_zoo.DILATED_LAYERS["tiny_dilated"]:
            continue
        cin, (dh, dw) = blobs[bottoms[0]].shape[1], R.dilation_of(pd)
        q = AtrousParam(output_channels=pd.get(0, 0), input_channels=cin, input_h=blobs[bottoms[0]].shape[2], input_w=blobs[bottoms[0]].shape[3],
                        kernel_h=pd.get(1, 0), kernel_w=pd.get(1, 0), stride_h=pd.get(3, 1), stride_w=pd.get(3, 1), pad_left=pd.get(4, 0),
                        pad_right=pd.get(4, 0), pad_top=pd.get(4, 0), pad_bottom=pd.get(4, 0), group=pd.get(7, 1), bias_term=bool(pd.get(5, 0)),
                        dilation_h=dh, dilation_w=dw, batch=2)
        q.AssignOutputDim()
        print("ROUTE", AtrousConv().Route(q))
    print("child ok")


if __name__ == "__main__":
    main()
