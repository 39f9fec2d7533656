"""fp64 restatement of transposed convolution (ncnn's Deconvolution / DeconvolutionDepthWise) and of whole nets that hold such layers: the
yardstick of tests/test_deconv_cpu.py and tests/test_deconv_gpu.py.

`deconv(x, w, b, group, stride, pads, out_pads, relu)` is the definition of include/feather_hip/feather_deconv.h in its scatter form,
written with numpy and accumulated in float64: input pixel (iy, ix) adds w[k][c][i][j] * x to output (iy * sh + i - pad_top,
ix * sw + j - pad_left); the kernel is not flipped; weights are [K][C/group][kh][kw].  The full scatter range is computed first and then
cropped by the pads (output pads extend the bottom / right: they are refused beyond the pad of that side, so the crop never leaves the
scatter range).  `Net` runs every other layer as tests/gconv_ref.py's Net does and adds Concat and Dropout.
"""
from __future__ import annotations

import numpy as np

import gconv_ref
from gconv_ref import nerr  # noqa: F401  (the project's parity metric, re-exported)


def out_dim(size: int, k: int, s: int, p0: int, p1: int, op: int) -> int:
    return (size - 1) * s + k - p0 - p1 + op


def deconv(x, w, b=None, group=1, stride=(1, 1), pads=(0, 0, 0, 0), out_pads=(0, 0), relu=False, dtype=np.float64) -> np.ndarray:
    """x [N][C][H][W], w [K][C/group][kh][kw], b [K] or None; stride (sh, sw); pads (left, right, top, bottom); out_pads (right, bottom)."""
    x = np.asarray(x, dtype)
    w = np.asarray(w, dtype)
    n, c, h, wd = x.shape
    k, cg, kh, kw = w.shape
    assert c % group == 0 and k % group == 0 and cg == c // group, (x.shape, w.shape, group)
    sh, sw = stride
    pl, pr, pt, pb = pads
    opr, opb = out_pads
    assert opb <= pb and opr <= pr and opb < sh and opr < sw
    ho, wo = out_dim(h, kh, sh, pt, pb, opb), out_dim(wd, kw, sw, pl, pr, opr)
    fh, fw = (h - 1) * sh + kh, (wd - 1) * sw + kw
    full = np.zeros((n, k, fh, fw), dtype)
    kg = k // group
    for g in range(group):
        xs = x[:, g * cg:(g + 1) * cg]
        ws = w[g * kg:(g + 1) * kg]
        for i in range(kh):
            for j in range(kw):
                full[:, g * kg:(g + 1) * kg, i:i + (h - 1) * sh + 1:sh, j:j + (wd - 1) * sw + 1:sw] += np.einsum("kc,nchw->nkhw", ws[:, :, i, j], xs, optimize=True)
    y = full[:, :, pt:pt + ho, pl:pl + wo].copy()
    assert y.shape == (n, k, ho, wo), (y.shape, ho, wo)
    if b is not None:
        y += np.asarray(b, dtype).reshape(1, k, 1, 1)
    if relu:
        y = np.maximum(y, 0)
    return y


def synth(c, k, h, w, kh, kw, group, batch, seed, sh=1, sw=1):
    """Seeded tensors as oracle.synth draws them: input U(-1, 1), weights U(-1, 1) / sqrt(terms per output), bias U(-.1, .1)."""
    rng = np.random.default_rng(seed)
    cg = c // group
    terms = max(cg * -(-kh // sh) * -(-kw // sw), 1)
    x = rng.uniform(-1, 1, (batch, c, h, w)).astype(np.float32)
    wt = (rng.uniform(-1, 1, (k, cg, kh, kw)) / np.sqrt(terms)).astype(np.float32)
    b = rng.uniform(-0.1, 0.1, (k,)).astype(np.float32)
    return x, wt, b


DECONV_TYPES = ("Deconvolution", "DeconvolutionDepthWise")


def deconv_geometry(pd):
    """(K, kh, kw, (sh, sw), pads (l, r, t, b), out_pads (right, bottom), bias_term, weight_data_size, group) from a layer's ParamDict."""
    kw = pd.get(1, 0)
    sw = pd.get(3, 1)
    pl = pd.get(4, 0)
    pt = pd.get(14, pl)
    return (pd.get(0, 0), pd.get(11, kw), kw, (pd.get(13, sw), sw), (pl, pd.get(15, pl), pt, pd.get(16, pt)), (pd.get(18, 0), pd.get(19, 0)),
            pd.get(5, 0), pd.get(6, 0), pd.get(7, 1))


class Net(gconv_ref.Net):
    """gconv_ref.Net plus Deconvolution / DeconvolutionDepthWise (by `deconv`, rounded to float32 per blob), Concat and Dropout."""

    def __init__(self, param: bytes, weights: bytes):
        from oracle.netcheck import _Bin, parse_param
        self.layers = parse_param(param)
        # gconv_ref.Net reads the .bin in layer order; the deconvolution layers are read here in the same pass
        mb = _Bin(weights)
        self.w = {}
        for type_, name, _, _, pd in self.layers:
            if type_ in DECONV_TYPES:
                k, kh, kw, _, _, _, bias, wsize, group = deconv_geometry(pd)
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
        self.read = mb.o

    def run(self, input_name: str, x: np.ndarray, output_name: str, keep: bool = False):
        # layers gconv_ref.Net does not restate are evaluated here; the rest by a one-layer gconv_ref.Net.run over the same blob table
        blobs = {input_name: np.ascontiguousarray(x, np.float32)}
        all_layers = self.layers
        try:
            for layer in all_layers:
                type_, name, bottoms, tops, pd = layer
                if type_ == "Input":
                    continue
                if type_ in DECONV_TYPES:
                    wgt, b, group = self.w[name]
                    _, _, _, stride, pads, out_pads, _, _, _ = deconv_geometry(pd)
                    blobs[tops[0]] = np.ascontiguousarray(deconv(blobs[bottoms[0]], wgt, b, group, stride, pads, out_pads), np.float32)
                elif type_ == "Concat":
                    blobs[tops[0]] = np.ascontiguousarray(np.concatenate([blobs[b] for b in bottoms], axis=1), np.float32)
                elif type_ == "Dropout":
                    blobs[tops[0]] = blobs[bottoms[0]]
                else:
                    self.layers = [layer]
                    got = gconv_ref.Net.run(self, bottoms[0], blobs[bottoms[0]], tops[0], keep=True) if type_ != "Eltwise" else None
                    if type_ == "Eltwise":
                        got = {tops[0]: np.ascontiguousarray(blobs[bottoms[0]] + blobs[bottoms[1]], np.float32)}
                    for t in tops:
                        blobs[t] = got[t]
        finally:
            self.layers = all_layers
        return blobs if keep else blobs[output_name]
