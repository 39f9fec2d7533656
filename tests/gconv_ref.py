"""fp64 restatement of grouped convolution (1 < group < C) and of whole nets that hold such layers: the yardstick of
tests/test_gconv_cpu.py and tests/test_gconv_gpu.py.

`conv(x, w, b, group, stride, pads, relu)` is the definition of include/feather_hip/feather_gconv.h (Caffe's / ncnn's), written with numpy
and accumulated in float64: output channel k belongs to group k // (K // group) and reads input channels [g * C/group, (g + 1) * C/group).
It is NOT restricted to partial groups -- group 1 and group == C follow from the same formula -- so `Net` below can run every convolution
of a model with it.  `Net` restates the other layers the way oracle/netcheck.py's PortNet does (whose readers and pooling it imports);
PortNet itself sizes a partial group's bias and output wrongly, as the reference's Net does, and cannot run one.
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle.netcheck import _Bin, _pool, parse_param  # noqa: E402


def out_dim(size: int, k: int, s: int, p0: int, p1: int) -> int:
    return (size + p0 + p1 - k) // s + 1


def conv(x, w, b=None, group=1, stride=(1, 1), pads=(0, 0, 0, 0), relu=False, dtype=np.float64) -> np.ndarray:
    """x [N][C][H][W], w [K][C/group][kh][kw], b [K] or None; stride (sh, sw); pads (left, right, top, bottom).  -> float64 [N][K][Ho][Wo]."""
    x = np.asarray(x, dtype)
    w = np.asarray(w, dtype)
    n, c, h, wd = x.shape
    k, cg, kh, kw = w.shape
    assert c % group == 0 and k % group == 0 and cg == c // group, (x.shape, w.shape, group)
    sh, sw = stride
    pl, pr, pt, pb = pads
    ho, wo = out_dim(h, kh, sh, pt, pb), out_dim(wd, kw, sw, pl, pr)
    xp = np.zeros((n, c, h + pt + pb, wd + pl + pr), dtype)
    xp[:, :, pt:pt + h, pl:pl + wd] = x
    kg = k // group
    y = np.zeros((n, k, ho, wo), dtype)
    for g in range(group):
        xs = xp[:, g * cg:(g + 1) * cg]
        ws = w[g * kg:(g + 1) * kg]
        acc = np.zeros((n, kg, ho, wo), dtype)
        for i in range(kh):
            for j in range(kw):
                win = xs[:, :, i:i + (ho - 1) * sh + 1:sh, j:j + (wo - 1) * sw + 1:sw]  # [N][cg][Ho][Wo]
                acc += np.einsum("kc,nchw->nkhw", ws[:, :, i, j], win, optimize=True)
        y[:, g * kg:(g + 1) * kg] = acc
    if b is not None:
        y += np.asarray(b, dtype).reshape(1, k, 1, 1)
    if relu:
        y = np.maximum(y, 0)
    return y


def nerr(a, ref) -> float:
    """max|a - ref| / max|ref|: the project's parity metric."""
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    m = float(np.abs(ref).max())
    d = float(np.abs(a - ref).max())
    return d / m if m > 0 else d


def synth(c, k, h, w, kh, kw, group, batch, seed):
    """Seeded tensors as oracle.synth draws them: input U(-1, 1), weights U(-1, 1) / sqrt(C/group * kh * kw), bias U(-.1, .1)."""
    rng = np.random.default_rng(seed)
    cg = c // group
    x = rng.uniform(-1, 1, (batch, c, h, w)).astype(np.float32)
    wt = (rng.uniform(-1, 1, (k, cg, kh, kw)) / np.sqrt(cg * kh * kw)).astype(np.float32)
    b = rng.uniform(-0.1, 0.1, (k,)).astype(np.float32)
    return x, wt, b


class Net:
    """A .param / .bin pair evaluated layer by layer: convolutions by `conv` in float64 (rounded to float32 per blob, as every blob of
    the device net is float32), the rest as oracle/netcheck.py's PortNet."""

    def __init__(self, param: bytes, weights: bytes):
        self.layers = parse_param(param)
        mb = _Bin(weights)
        self.w = {}
        for type_, name, _, _, pd in self.layers:
            if type_ in ("Convolution", "ConvolutionDepthWise"):
                group, kw = pd.get(7, 1), pd.get(1, 0)
                kh, k = pd.get(11, kw), pd.get(0, 0)
                cg = pd.get(6, 0) // k // kh // kw  # weight_data_size = K * C/group * kh * kw
                wgt = mb.load(k * cg * kh * kw, True).reshape(k, cg, kh, kw)
                self.w[name] = (wgt, mb.load(k, False) if pd.get(5, 0) else None, group)
            elif type_ == "InnerProduct":
                out = pd.get(0, 0)
                wgt = mb.load(pd.get(2, 0), True).reshape(out, -1)
                self.w[name] = (wgt, mb.load(out, False) if pd.get(1, 0) else None)
            elif type_ == "BatchNorm":
                c = pd.get(0, 0)
                slope, mean, var, bias = (mb.load(c, False) for _ in range(4))
                sq = np.sqrt(var + np.float32(pd.get(1, 0.0)), dtype=np.float32)
                self.w[name] = (slope / sq, bias - slope * mean / sq)
            elif type_ == "Scale":
                c = pd.get(0, 0)
                s = mb.load(c, False)
                self.w[name] = (s, mb.load(c, False) if pd.get(1, 0) else None)
        self.read = mb.o  # bytes of the .bin consumed

    def run(self, input_name: str, x: np.ndarray, output_name: str, keep: bool = False):
        blobs = {input_name: np.ascontiguousarray(x, np.float32)}
        for type_, name, bottoms, tops, pd in self.layers:
            if type_ == "Input":
                continue
            a = blobs[bottoms[0]]
            if type_ in ("Convolution", "ConvolutionDepthWise"):
                wgt, b, group = self.w[name]
                sw, pw = pd.get(3, 1), pd.get(4, 0)
                sh, ph = pd.get(13, sw), pd.get(14, pw)
                y = conv(a, wgt, b, group, (sh, sw), (pw, pw, ph, ph))
            elif type_ == "ReLU":
                y = np.where(a > 0, a, np.float32(0))
            elif type_ == "Pooling":
                y = _pool(a, pd)
            elif type_ == "InnerProduct":
                wgt, b = self.w[name]
                y = a.reshape(a.shape[0], -1).astype(np.float64) @ wgt.T.astype(np.float64)
                if b is not None:
                    y = y + b
                y = y.astype(np.float32).reshape(a.shape[0], -1, 1, 1)
            elif type_ == "BatchNorm":
                beta, alpha = self.w[name]
                y = a * beta[None, :, None, None] + alpha[None, :, None, None]
            elif type_ == "Scale":
                s, b = self.w[name]
                y = a * s[None, :, None, None]
                if b is not None:
                    y = y + b[None, :, None, None]
            elif type_ == "Eltwise":
                y = a + blobs[bottoms[1]]
            elif type_ == "Split":
                for t in tops:
                    blobs[t] = a
                continue
            elif type_ == "Softmax":
                f = a.reshape(a.shape[0], -1)
                e = np.exp(f - f.max(axis=1, keepdims=True), dtype=np.float32)
                y = (e / e.sum(axis=1, keepdims=True, dtype=np.float32)).reshape(a.shape)
            else:
                raise RuntimeError(f"layer {type_} is not restated here")
            blobs[tops[0]] = np.ascontiguousarray(y, np.float32)
        return blobs if keep else blobs[output_name]
