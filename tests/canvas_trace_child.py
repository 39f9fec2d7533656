"""Child of tests/test_canvas_gpu.py::test_kernel_trace_shows_the_canvas_gemm_grids: VGG-16 at batch 32, fusion level 3, a few eager forwards."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from feathercnn_amd import model_zoo  # noqa: E402
from feathercnn_amd.net import Net  # noqa: E402

p, b, i, o = model_zoo.vgg16()
net = Net(fusion=3, graph=False, tuned=True)
net.LoadParam(p)
net.LoadWeights(b)
net.FeedInput(i, np.random.default_rng(1).uniform(-1, 1, (32, 3, 224, 224)).astype(np.float32))
for _ in range(2):
    net.Forward()
assert len(net.canvases()) == 6, net.canvases()
assert np.isfinite(net.Extract(o)).all()
print("child ok")
