"""The numpy restatement of include/feather_hip/feather_q8.h on top of tests/qconv_ref.py (the rules it inherits from feather_qconv.h): the
q8 tensor, the requantised output, the int8-input convolution, ReLU and max pooling on a q8 tensor.  Everything is exact, so every
comparison against it is np.array_equal.

Integers travel as int32 NCHW arrays ("q"); pack() / unpack() move them into and out of the q8 layout signed char [n][CB][h][w][16]."""
from __future__ import annotations

import numpy as np

import qconv_ref as R

F = np.float32


def blocks(c: int) -> int:
    return (c + 15) // 16


def pack(q, pad=0) -> np.ndarray:
    """int NCHW -> q8 tensor int8 [n][CB][h][w][16]; the bytes of channels >= C are `pad` (0 by the definition; a test may put garbage)."""
    q = np.asarray(q)
    n, c, h, w = q.shape
    cb = blocks(c)
    full = np.full((n, cb * 16, h, w), pad, np.int8)
    full[:, :c] = q.astype(np.int8)
    return np.ascontiguousarray(full.reshape(n, cb, 16, h, w).transpose(0, 1, 3, 4, 2))


def unpack(t, c: int) -> np.ndarray:
    """q8 tensor -> int32 NCHW of its first c channels."""
    t = np.asarray(t, np.int8)
    n, cb, h, w, _ = t.shape
    return t.transpose(0, 1, 4, 2, 3).reshape(n, cb * 16, h, w)[:, :c].astype(np.int32)


def pad_bytes(t, c: int) -> np.ndarray:
    """The bytes of a q8 tensor that belong to no channel."""
    t = np.asarray(t, np.int8)
    n, cb, h, w, _ = t.shape
    return t.transpose(0, 1, 4, 2, 3).reshape(n, cb * 16, h, w)[:, c:]


def quantize(x, s) -> np.ndarray:
    """fhip_q8_quantize_forward: the q8 tensor of quantise(x; s)."""
    return pack(R.quantise(x, s))


def dequantize(t, c, s) -> np.ndarray:
    """fhip_q8_dequantize_forward: float(q) / s, one fp32 division."""
    return (unpack(t, c).astype(F) / F(s)).astype(F)


def conv(x, wq, d, b=None, group=1, strides=(1, 1), pads=(0, 0, 0, 0), relu=False, s_in=None, s_out=None):
    """The layer of feather_q8.h.  x: fp32 NCHW with s_in, or int NCHW (the content of a q8 input) with s_in None.  -> fp32 NCHW with
    s_out None, else the int32 NCHW content of the q8 output: quantise(y; s_out)."""
    q = R.quantise(x, s_in) if s_in is not None else np.asarray(x, np.int64)
    y = R.dequantise(R.accumulate(q, wq, group, strides, pads), d, b, relu)
    return y if s_out is None else R.quantise(y, s_out)


def relu(q) -> np.ndarray:
    return np.maximum(np.asarray(q), 0)


def pool_dims(h, w, kernel, stride, pad, global_pooling=False):
    """fhip_pooling_output_dim: ceil."""
    if global_pooling:
        return 1, 1
    oh = int(np.ceil(F(h + 2 * pad - kernel) / F(stride))) + 1
    ow = int(np.ceil(F(w + 2 * pad - kernel) / F(stride))) + 1
    return oh, ow


def max_pool(q, kernel=2, stride=2, pad=0, global_pooling=False) -> np.ndarray:
    """fhip_q8_max_pool_forward on int NCHW: the max over the taps inside the plane, the window origin o * stride - 2 * pad (both pads),
    an empty window gives -127."""
    q = np.asarray(q, np.int32)
    n, c, h, w = q.shape
    oh, ow = pool_dims(h, w, kernel, stride, pad, global_pooling)
    kh, kw, s = (h, w, 1) if global_pooling else (kernel, kernel, stride)
    out = np.full((n, c, oh, ow), -127, np.int32)
    for oy in range(oh):
        for ox in range(ow):
            y0, x0 = oy * s - 2 * pad, ox * s - 2 * pad
            ya, yb, xa, xb = max(y0, 0), min(y0 + kh, h), max(x0, 0), min(x0 + kw, w)
            if ya < yb and xa < xb:
                out[:, :, oy, ox] = np.maximum(q[:, :, ya:yb, xa:xb].max(axis=(2, 3)), -127)
    return out


# ---- a net with q8 blobs: tiny_requant and anything built from the same layer types --------------------------------------------------
class Q8Blob:
    """The content of a q8 blob: int32 NCHW."""
    def __init__(self, q):
        self.q = np.asarray(q, np.int32)


class Refused(Exception):
    """A layer that cannot read a q8 blob met one: feather::Net refuses the net with NET_E_TOPOLOGY."""


def net_forward(model, x, level=0):
    """Every blob of a net of int8 Convolution / ConvolutionDepthWise / InnerProduct layers (int8_scale_term 1, or 101 with one more scale
    in the .bin: a q8 top), plain ReLU, BatchNorm, Scale, max Pooling, Split and Eltwise SUM, as feather::Net computes it at fusion
    `level` (tests/qconv_ref.net_forward has the levels; on a net without q8 blobs, Split or Eltwise this function is that one).  fp32
    blobs are arrays, q8 blobs Q8Blob.  The ReLU behind a requantised layer is applied to the integers: quantise commutes with it, so
    whether the Net fuses it into the producer or not does not change a bit."""
    param, weights = model[0], model[1]
    rd = R._Bin(weights)
    blobs = {}
    rows = list(R._layers(param))
    pending = None  # level 2: (acc, d, b, s_out) of a convolution whose dequantisation waits for the layers folded into it
    affine = None   # level >= 1: (mul, add) composed so far
    for idx, (type_, name, bottoms, tops, pd) in enumerate(rows):
        top = tops[0]
        if type_ == "Input":
            blobs[top] = np.asarray(x, F)
            continue
        v = blobs.get(bottoms[0])
        nxt = rows[idx + 1][0] if idx + 1 < len(rows) else ""
        q8_in = isinstance(v, Q8Blob)
        if q8_in and type_ not in ("Convolution", "ConvolutionDepthWise", "ReLU", "Pooling", "Split"):
            raise Refused(f"{type_} {name} reads the q8 blob {bottoms[0]}")
        if type_ in ("Convolution", "ConvolutionDepthWise", "InnerProduct"):
            term = int(pd[8])
            assert term in (1, 101) and not (term == 101 and type_ == "InnerProduct")
            if type_ == "InnerProduct":
                k, bias_term = int(pd[0]), int(pd[1])
                c, kh, s, p, group = int(pd[2]) // k, 1, 1, 0, 1
                v = v.reshape(v.shape[0], c, 1, 1)
            else:
                k, kh, s, p, bias_term, group = int(pd[0]), int(pd[1]), int(pd[3]), int(pd[4]), int(pd[5]), int(pd[7])
                c = int(pd[6]) * group // (k * kh * kh)
            wq = rd.int8(k * (c // group) * kh * kh).reshape(k, c // group, kh, kh)
            b = rd.raw(k) if bias_term else None
            s_w, s_in = rd.raw(k), rd.raw(1)[0]
            s_out = rd.raw(1)[0] if term == 101 else None
            d = R.dequant_scales(s_w, s_in)
            acc = R.accumulate(v.q if q8_in else R.quantise(v, s_in), wq, group, (s, s), (p, p, p, p))
            if level >= 2 and nxt in ("BatchNorm", "Scale"):
                pending = (acc, d, b, s_out)
            else:
                y = R.dequantise(acc, d, b)
                blobs[top] = y if s_out is None else Q8Blob(R.quantise(y, s_out))
        elif type_ in ("BatchNorm", "Scale"):
            c = int(pd[0])
            if type_ == "BatchNorm":
                slope, mean, var, bias = rd.raw(c), rd.raw(c), rd.raw(c), rd.raw(c)
                root = np.sqrt((var + F(float(pd[1]))).astype(F))
                m, a = (slope / root).astype(F), (bias - ((slope * mean).astype(F) / root).astype(F)).astype(F)
            else:
                m = rd.raw(c)
                a = rd.raw(c) if int(pd[1]) else np.zeros(c, F)
            if level == 0:
                blobs[top] = R.fma32(v, m.reshape(1, -1, 1, 1), a.reshape(1, -1, 1, 1))
                continue
            affine = (m, a) if affine is None else ((affine[0] * m).astype(F), ((affine[1] * m).astype(F) + a).astype(F))
            if level == 1 and not (type_ == "BatchNorm" and nxt == "Scale"):
                src = bottoms[0] if bottoms[0] in blobs else rows[idx - 1][2][0]
                if isinstance(blobs[src], Q8Blob):
                    raise Refused(f"{type_} {name} reads the q8 blob {src}")
                blobs[top] = R.fma32(blobs[src], affine[0].reshape(1, -1, 1, 1), affine[1].reshape(1, -1, 1, 1))
                affine = None
            elif level >= 2 and nxt not in ("BatchNorm", "Scale"):
                acc, d, b, s_out = pending
                d2, b2 = R.fold(d, b, *affine)
                y = R.dequantise(acc, d2, b2)
                blobs[top] = y if s_out is None else Q8Blob(R.quantise(y, s_out))
                pending = affine = None
        elif type_ == "ReLU":
            blobs[top] = Q8Blob(relu(v.q)) if q8_in else np.maximum(v, F(0))
        elif type_ == "Pooling":
            assert (int(pd[0]), int(pd[1]), int(pd[2]), int(pd.get(3, 0)), int(pd.get(4, 0))) == (0, 2, 2, 0, 0)
            if q8_in:
                blobs[top] = Q8Blob(max_pool(v.q, 2, 2))
            else:
                n, c, h, w = v.shape
                blobs[top] = v.reshape(n, c, h // 2, 2, w // 2, 2).max(axis=(3, 5))
        elif type_ == "Split":
            for t in tops:
                blobs[t] = v
        elif type_ == "Eltwise":
            o = blobs[bottoms[1]]
            if isinstance(o, Q8Blob):
                raise Refused(f"Eltwise {name} reads the q8 blob {bottoms[1]}")
            blobs[top] = (v + o).astype(F)
        else:
            raise ValueError(type_)
    assert rd.at == len(weights)
    return blobs
