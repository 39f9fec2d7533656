"""fp64 restatement of the squeeze-and-excitation definitions of include/feather_hip/feather_gate.h (channel gate, squeeze, excite, Swish,
HardSigmoid) and of whole nets that hold such layers: the yardstick of tests/test_gate_cpu.py and tests/test_gate_gpu.py.  The reference
project has none of these layers; tests/golden/se_golden.npz (torch on the CPU) keeps this file from resting on itself.

`Net` runs every other layer as tests/inorm_ref.py's Net does; a two-bottom `Scale 0=-233` and a `BinaryOp 0=2` are the channel gate.
"""
from __future__ import annotations

import numpy as np

import inorm_ref
from gconv_ref import nerr  # noqa: F401  (the project's parity metric, re-exported)
from inorm_ref import plane_nerr  # noqa: F401

GATE_TYPES = ("BinaryOp", "ScaleBy", "Swish", "HardSigmoid")  # ScaleBy: a two-bottom Scale, as Net names it


def channel_gate(x, gate, residual=None, relu=False, dtype=np.float64) -> np.ndarray:
    """x [N][C][H][W], gate N * C values: x * gate [+ residual], then ReLU.  With dtype float32 this is the library's arithmetic bit for
    bit (numpy rounds the product and the sum separately)."""
    x = np.asarray(x, dtype)
    y = x * np.asarray(gate, dtype).reshape(x.shape[0], x.shape[1], 1, 1)
    if residual is not None:
        y = y + np.asarray(residual, dtype)
    return np.maximum(y, 0) if relu else y


def squeeze(x, dtype=np.float64) -> np.ndarray:
    """mean over every (n, c) plane -> [N][C][1][1]."""
    x = np.asarray(x, dtype)
    return x.sum(axis=(2, 3), keepdims=True, dtype=dtype) / dtype(x.shape[2] * x.shape[3])


def swish(x, dtype=np.float64):
    x = np.asarray(x, dtype)
    with np.errstate(over="ignore"):
        return x / (1.0 + np.exp(-x))


def hard_sigmoid(x, alpha=0.2, beta=0.5, dtype=np.float64):
    """min(max(alpha * x + beta, 0), 1); with dtype float32 the library's arithmetic bit for bit."""
    x = np.asarray(x, dtype)
    return np.minimum(np.maximum(dtype(alpha) * x + dtype(beta), dtype(0)), dtype(1))


def sigmoid(x, dtype=np.float64):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-np.asarray(x, dtype)))


def gate_activation(x, kind, alpha=0.2, beta=0.5, dtype=np.float64):
    return swish(x, dtype) if kind == "swish" else hard_sigmoid(x, alpha, beta, dtype)


def excite(mean, w1, b1, w2, b2, mact="relu", gact="sigmoid", alpha=0.2, beta=0.5) -> np.ndarray:
    """mean N * C values, w1 [R][C], w2 [C][R] -> gate [N][C][1][1] in float64.  alpha / beta are taken as the float32 values the library
    is handed."""
    w1, w2 = np.asarray(w1, np.float64), np.asarray(w2, np.float64)
    r, c = w1.shape
    m = np.asarray(mean, np.float64).reshape(-1, c)
    h = m @ w1.T
    if b1 is not None:
        h = h + np.asarray(b1, np.float64)
    h = np.maximum(h, 0) if mact == "relu" else swish(h) if mact == "swish" else h
    g = h @ w2.reshape(c, r).T
    if b2 is not None:
        g = g + np.asarray(b2, np.float64)
    g = sigmoid(g) if gact == "sigmoid" else hard_sigmoid(g, np.float64(np.float32(alpha)), np.float64(np.float32(beta)))
    return g.reshape(-1, c, 1, 1)


def _rename_gated_scale(param: bytes) -> bytes:
    out = []
    for line in param.decode().split("\n"):
        tok = line.split()
        if len(tok) > 3 and tok[0] == "Scale" and tok[2] == "2":
            line = "ScaleBy" + line[len("Scale"):]
        out.append(line)
    return "\n".join(out).encode()


class Net(inorm_ref.Net):
    """inorm_ref.Net plus the channel gate (BinaryOp mul, two-bottom Scale), Swish and HardSigmoid (float64, rounded to float32 per blob)."""

    def __init__(self, param: bytes, weights: bytes):
        super().__init__(_rename_gated_scale(param), weights)

    def run(self, input_name: str, x: np.ndarray, output_name: str, keep: bool = False):
        blobs = {input_name: np.ascontiguousarray(x, np.float32)}
        all_layers = self.layers
        try:
            for layer in all_layers:
                type_, name, bottoms, tops, pd = layer
                if type_ == "Input":
                    continue
                a = blobs[bottoms[0]]
                if type_ == "Split":
                    for t in tops:
                        blobs[t] = a
                    continue
                if type_ == "ScaleBy":
                    assert pd.get(0, 0) == -233 and not pd.get(1, 0)
                    y = channel_gate(a, blobs[bottoms[1]])
                elif type_ == "BinaryOp":
                    assert pd.get(0, 0) == 2 and len(bottoms) == 2
                    b = blobs[bottoms[1]]
                    gate_first = a.shape[2:] == (1, 1) and b.shape[2:] != (1, 1)
                    y = channel_gate(b, a) if gate_first else channel_gate(a, b)
                elif type_ == "Swish":
                    y = swish(a)
                elif type_ == "HardSigmoid":
                    y = hard_sigmoid(a, np.float64(np.float32(pd.get(0, 0.2))), np.float64(np.float32(pd.get(1, 0.5))))
                elif type_ == "Eltwise":
                    y = a + blobs[bottoms[1]]
                elif type_ == "Concat":
                    y = np.concatenate([blobs[b] for b in bottoms], axis=1)
                else:
                    self.layers = [layer]
                    y = inorm_ref.Net.run(self, bottoms[0], a, tops[0], keep=True)[tops[0]]
                blobs[tops[0]] = np.ascontiguousarray(y, np.float32)
        finally:
            self.layers = all_layers
        return blobs if keep else blobs[output_name]
