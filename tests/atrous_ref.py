"""The dilated convolution of include/feather_hip/feather_atrous.h restated on the host in float64, and a layer-by-layer evaluation of a
.param / .bin pair that holds such layers: what the GPU tests of libfeather_atrous.so compare against.  `atrous` is written from the
definition (a gather per tap at offset (i * dh, j * dw)); tests/test_atrous_cpu.py checks it against torch's conv2d(dilation=) in float64
and against the plain convolution with the zero-stuffed kernel.
"""
from __future__ import annotations

import numpy as np

import gconv_ref
import shuffle_ref
from gconv_ref import nerr  # noqa: F401  (the project's parity metric, re-exported)


def out_dim(size: int, k: int, s: int, d: int, p0: int, p1: int) -> int:
    return (size + p0 + p1 - (d * (k - 1) + 1)) // s + 1


def atrous(x, w, b=None, group=1, stride=(1, 1), pads=(0, 0, 0, 0), dilation=(1, 1), relu=False, dtype=np.float64) -> np.ndarray:
    """x [N][C][H][W], w [K][C/group][kh][kw], b [K] or None; stride (sh, sw); pads (left, right, top, bottom); dilation (dh, dw)."""
    x = np.asarray(x, dtype)
    w = np.asarray(w, dtype)
    n, c, h, wd = x.shape
    k, cg, kh, kw = w.shape
    assert c % group == 0 and k % group == 0 and cg == c // group, (x.shape, w.shape, group)
    (sh, sw), (pl, pr, pt, pb), (dh, dw) = stride, pads, dilation
    ho, wo = out_dim(h, kh, sh, dh, pt, pb), out_dim(wd, kw, sw, dw, pl, pr)
    assert ho >= 1 and wo >= 1
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
                win = xs[:, :, i * dh:i * dh + (ho - 1) * sh + 1:sh, j * dw:j * dw + (wo - 1) * sw + 1:sw]
                acc += np.einsum("kc,nchw->nkhw", ws[:, :, i, j], win, optimize=True)
        y[:, g * kg:(g + 1) * kg] = acc
    if b is not None:
        y += np.asarray(b, dtype).reshape(1, k, 1, 1)
    if relu:
        y = np.maximum(y, 0)
    return y


def stuffed_kernel(w, dilation):
    """[K][Cg][kh][kw] -> [K][Cg][dh * (kh - 1) + 1][dw * (kw - 1) + 1] with zeros between the taps: the plain convolution with it IS the
    dilated convolution."""
    dh, dw = dilation
    k, cg, kh, kw = w.shape
    z = np.zeros((k, cg, dh * (kh - 1) + 1, dw * (kw - 1) + 1), w.dtype)
    z[:, :, ::dh, ::dw] = w
    return z


synth = gconv_ref.synth


def dilation_of(pd):
    dw = pd.get(2, 1)
    return pd.get(12, dw), dw


class Net(shuffle_ref.Net):
    """shuffle_ref.Net plus ncnn's dilation params 2 / 12 on Convolution / ConvolutionDepthWise (by `atrous`, rounded to float32 per blob)."""

    def run(self, input_name: str, x: np.ndarray, output_name: str, keep: bool = False):
        blobs = {input_name: np.ascontiguousarray(x, np.float32)}
        all_layers = self.layers
        try:
            for layer in all_layers:
                type_, name, bottoms, tops, pd = layer
                if type_ == "Input":
                    continue
                if type_ in ("Convolution", "ConvolutionDepthWise") and dilation_of(pd) != (1, 1):
                    wgt, b, group = self.w[name]
                    sw, pw = pd.get(3, 1), pd.get(4, 0)
                    sh, ph = pd.get(13, sw), pd.get(14, pw)
                    blobs[tops[0]] = np.ascontiguousarray(atrous(blobs[bottoms[0]], wgt, b, group, (sh, sw), (pw, pw, ph, ph), dilation_of(pd)), np.float32)
                    continue
                self.layers = [layer]
                sub = {b: blobs[b] for b in bottoms}
                if len(bottoms) == 1 and type_ != "Split":
                    out = shuffle_ref.Net.run(self, bottoms[0], blobs[bottoms[0]], tops[0], keep=True)
                else:
                    out = self._many(layer, sub)
                for t in tops:
                    blobs[t] = out[t]
        finally:
            self.layers = all_layers
        return blobs if keep else blobs[output_name]
