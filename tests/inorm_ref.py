"""fp64 restatement of ncnn's InstanceNorm and of the element-wise activations of generative nets (leaky ReLU, PReLU, Sigmoid, TanH, Clip),
and of whole nets that hold such layers: the yardstick of tests/test_inorm_cpu.py and tests/test_inorm_gpu.py.

`instance_norm(x, gamma, beta, eps, act, slope)` is the definition of include/feather_hip/feather_inorm.h written with numpy in float64: per
(n, c) plane mean = sum(x) / HW, var = sum((x - mean)^2) / HW (biased, two-pass), y = (x - mean) * gamma / sqrt(var + eps) + beta.
`Net` runs every other layer as tests/deconv_ref.py's Net does; a `ReLU` with param 0 is the leaky one.
"""
from __future__ import annotations

import numpy as np

import deconv_ref
import gconv_ref
from gconv_ref import nerr  # noqa: F401  (the project's parity metric, re-exported)

ACTIVATION_TYPES = ("PReLU", "Sigmoid", "TanH", "Clip")
FLT_MAX = float(np.finfo(np.float32).max)


def leaky(y, slope):
    return np.where(y > 0, y, y * slope)


def instance_norm(x, gamma=None, beta=None, eps=1e-3, act=None, slope=0.0, dtype=np.float64) -> np.ndarray:
    """x [N][C][H][W]; gamma / beta [C] or None (1 / 0); act None / "relu" / "leaky_relu"."""
    x = np.asarray(x, dtype)
    mean = x.mean(axis=(2, 3), keepdims=True, dtype=dtype)
    d = x - mean
    var = (d * d).mean(axis=(2, 3), keepdims=True, dtype=dtype)
    a = 1.0 / np.sqrt(var + dtype(eps))
    if gamma is not None:
        a = a * np.asarray(gamma, dtype).reshape(1, -1, 1, 1)
    y = d * a
    if beta is not None:
        y = y + np.asarray(beta, dtype).reshape(1, -1, 1, 1)
    if act == "relu":
        y = np.maximum(y, 0)
    elif act == "leaky_relu":
        y = leaky(y, dtype(slope))
    else:
        assert act is None, act
    return y


def instance_norm_one_pass(x, gamma=None, beta=None, eps=1e-3, dtype=np.float32) -> np.ndarray:
    """The form the library must NOT use, var = E[x^2] - E[x]^2, here only so that a test can show the offset-plane bound tells them apart."""
    x = np.asarray(x, dtype)
    mean = x.mean(axis=(2, 3), keepdims=True, dtype=dtype)
    var = np.maximum((x * x).mean(axis=(2, 3), keepdims=True, dtype=dtype) - mean * mean, 0)
    y = (x - mean) / np.sqrt(var + dtype(eps))
    if gamma is not None:
        y = y * np.asarray(gamma, dtype).reshape(1, -1, 1, 1)
    if beta is not None:
        y = y + np.asarray(beta, dtype).reshape(1, -1, 1, 1)
    return y


def activation(x, kind, slope=0.0, lo=-FLT_MAX, hi=FLT_MAX, slopes=None, dtype=np.float64) -> np.ndarray:
    """kind "leaky_relu" / "prelu" / "sigmoid" / "tanh" / "clip" on x [N][C][...]; slopes [C] for a per-channel PReLU."""
    x = np.asarray(x, dtype)
    if kind in ("leaky_relu", "prelu"):
        s = dtype(slope) if slopes is None else np.asarray(slopes, dtype).reshape((1, -1) + (1,) * (x.ndim - 2))
        return leaky(x, s)
    if kind == "sigmoid":
        with np.errstate(over="ignore"):
            return 1.0 / (1.0 + np.exp(-x))
    if kind == "tanh":
        return np.tanh(x)
    if kind == "clip":
        return np.minimum(np.maximum(x, dtype(lo)), dtype(hi))
    raise ValueError(kind)


def plane_nerr(y, ref) -> float:
    """The worst per-plane normalised error max|y - ref| / max|ref| over the (n, c) planes of [N][C][H][W] tensors."""
    y, ref = np.asarray(y, np.float64), np.asarray(ref, np.float64)
    d = np.abs(y - ref).max(axis=(2, 3))
    m = np.abs(ref).max(axis=(2, 3))
    return float(np.where(m > 0, d / np.where(m > 0, m, 1), d).max())


class Net(deconv_ref.Net):
    """deconv_ref.Net plus InstanceNorm, ReLU with a slope, PReLU, Sigmoid, TanH and Clip (float64, rounded to float32 per blob)."""

    def __init__(self, param: bytes, weights: bytes):
        from oracle.netcheck import _Bin, parse_param
        self.layers = parse_param(param)
        mb = _Bin(weights)
        self.w = {}
        for type_, name, _, _, pd in self.layers:
            if type_ in deconv_ref.DECONV_TYPES:
                k, kh, kw, _, _, _, bias, wsize, group = deconv_ref.deconv_geometry(pd)
                cg = wsize // k // kh // kw
                wgt = mb.load(k * cg * kh * kw, True).reshape(k, cg, kh, kw)
                self.w[name] = (wgt, mb.load(k, False) if bias else None, group)
            elif type_ in ("Convolution", "ConvolutionDepthWise"):
                group, kw = pd.get(7, 1), pd.get(1, 0)
                kh, k = pd.get(11, kw), pd.get(0, 0)
                cg = pd.get(6, 0) // k // kh // kw
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
            elif type_ == "InstanceNorm":
                c = pd.get(0, 0)
                self.w[name] = (mb.load(c, False), mb.load(c, False)) if pd.get(2, 1) else (None, None)
            elif type_ == "PReLU":
                self.w[name] = mb.load(pd.get(0, 0), False)
        self.read = mb.o

    def run(self, input_name: str, x: np.ndarray, output_name: str, keep: bool = False):
        blobs = {input_name: np.ascontiguousarray(x, np.float32)}
        all_layers = self.layers
        try:
            for layer in all_layers:
                type_, name, bottoms, tops, pd = layer
                if type_ == "Input":
                    continue
                a = blobs[bottoms[0]]
                if type_ == "InstanceNorm":
                    gamma, beta = self.w[name]
                    assert pd.get(0, 0) == a.shape[1]
                    y = instance_norm(a, gamma, beta, np.float32(pd.get(1, 0.001)))
                elif type_ == "ReLU":
                    y = leaky(a.astype(np.float64), np.float64(np.float32(pd.get(0, 0.0))))
                elif type_ == "PReLU":
                    s = self.w[name]
                    assert s.size in (1, a.shape[1])
                    y = activation(a, "prelu", slope=s[0], slopes=None if s.size == 1 else s)
                elif type_ == "Sigmoid":
                    y = activation(a, "sigmoid")
                elif type_ == "TanH":
                    y = activation(a, "tanh")
                elif type_ == "Clip":
                    y = activation(a, "clip", lo=np.float32(pd.get(0, -FLT_MAX)), hi=np.float32(pd.get(1, FLT_MAX)))
                elif type_ in deconv_ref.DECONV_TYPES:
                    wgt, b, group = self.w[name]
                    _, _, _, stride, pads, out_pads, _, _, _ = deconv_ref.deconv_geometry(pd)
                    y = deconv_ref.deconv(a, wgt, b, group, stride, pads, out_pads)
                elif type_ == "Concat":
                    y = np.concatenate([blobs[b] for b in bottoms], axis=1)
                elif type_ == "Eltwise":
                    y = a + blobs[bottoms[1]]
                elif type_ == "Dropout":
                    y = a
                elif type_ == "Split":
                    for t in tops:
                        blobs[t] = a
                    continue
                else:
                    self.layers = [layer]
                    y = gconv_ref.Net.run(self, bottoms[0], a, tops[0], keep=True)[tops[0]]
                blobs[tops[0]] = np.ascontiguousarray(y, np.float32)
        finally:
            self.layers = all_layers
        return blobs if keep else blobs[output_name]


# ---- the pixel round trip of tests/test_inorm_gpu.py (FeedPixels -> style_transfer_in -> ExtractPixels), host side --------------------
PIXEL_SIZE = 64
PIXEL_MEAN_IN, PIXEL_NORM_IN = [104.0, 117.0, 123.0], [0.017, 0.017, 0.017]
PIXEL_MEAN_OUT, PIXEL_NORM_OUT = [-1.0, -1.0, -1.0], [127.5, 127.5, 127.5]  # TanH's [-1, 1] -> [0, 255]
PIXEL_CAP = 0.005  # at most this share of the bytes may differ from the restatement's, and none by more than 1


def pixel_input():
    """The seeded uint8 images [2][70][90][3] and the float input the net sees (ncnn from_pixels_resize to 64 x 64, mean / norm)."""
    import pixels_ref as P
    px = np.random.default_rng(19).integers(0, 256, (2, 70, 90, 3), dtype=np.uint8)
    return px, P.from_pixels_resize(px, P.PIXEL_RGB, PIXEL_SIZE, PIXEL_SIZE, PIXEL_MEAN_IN, PIXEL_NORM_IN)


def pixel_output(y) -> np.ndarray:
    """The net's output blob [N][3][64][64] as uint8 images, by the repo's restatements of mean / norm and ncnn's to_pixels."""
    import pixels_ref as P
    import yuv_ref as Y
    m = P.mean_norm(np.asarray(y, np.float32), np.float32(PIXEL_MEAN_OUT), np.float32(PIXEL_NORM_OUT))
    return np.stack([Y.to_pixels_resize(v, P.PIXEL_RGB, PIXEL_SIZE, PIXEL_SIZE) for v in m])
