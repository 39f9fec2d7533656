"""Writes tests/golden/se_golden.npz: a squeeze-and-excitation block, Swish and HardSigmoid computed by torch on the CPU in float64
(adaptive_avg_pool2d, linear, relu / silu, sigmoid / hardsigmoid, the multiply, the residual add and its ReLU).  tests/test_gate_cpu.py
compares tests/gate_ref.py with it.  torch's hardsigmoid is relu6(x + 3) / 6: alpha = 1 / 6, beta = 0.5.

    python tests/golden/make_se_golden.py
"""
import os

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    g = torch.Generator().manual_seed(41)
    out = {}
    for tag, (n, c, r, h, w, mact, gact) in {"relu_sigmoid": (2, 6, 2, 5, 7, "relu", "sigmoid"), "swish_hsig": (3, 5, 3, 4, 4, "swish", "hard_sigmoid"),
                                             "none_sigmoid": (1, 4, 1, 3, 3, "none", "sigmoid")}.items():
        x = torch.rand((n, c, h, w), generator=g, dtype=torch.float64) * 2 - 1
        res = torch.rand((n, c, h, w), generator=g, dtype=torch.float64) * 2 - 1
        w1 = torch.rand((r, c), generator=g, dtype=torch.float64) * 2 - 1
        b1 = torch.rand((r,), generator=g, dtype=torch.float64) - 0.5
        w2 = (torch.rand((c, r), generator=g, dtype=torch.float64) * 2 - 1) * 40  # wide enough to reach both clamps of hardsigmoid
        b2 = torch.rand((c,), generator=g, dtype=torch.float64) - 0.5
        mean = F.adaptive_avg_pool2d(x, 1)
        hid = F.linear(mean.flatten(1), w1, b1)
        hid = F.relu(hid) if mact == "relu" else F.silu(hid) if mact == "swish" else hid
        pre = F.linear(hid, w2, b2)
        gate = torch.sigmoid(pre) if gact == "sigmoid" else F.hardsigmoid(pre)
        y = x * gate.reshape(n, c, 1, 1)
        for k, v in (("x", x), ("res", res), ("w1", w1), ("b1", b1), ("w2", w2), ("b2", b2), ("mean", mean), ("gate", gate.reshape(n, c, 1, 1)), ("y", y),
                     ("y_res", y + res), ("y_res_relu", F.relu(y + res))):
            out[f"{tag}.{k}"] = v.numpy()
    a = torch.linspace(-9, 9, 181, dtype=torch.float64).reshape(1, 1, 181)
    out["act.x"], out["act.swish"], out["act.hardsigmoid"] = a.numpy(), F.silu(a).numpy(), F.hardsigmoid(a).numpy()
    np.savez_compressed(os.path.join(HERE, "se_golden.npz"), **out)


if __name__ == "__main__":
    main()
