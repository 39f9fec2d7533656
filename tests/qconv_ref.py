"""The numpy restatement of include/feather_hip/feather_qconv.h: what libfeather_qconv.so and the quantised layers of feather::Net must
equal BIT FOR BIT.  Quantisation and dequantisation are written step by step in float32 (every operation one rounding, no fused
multiply-add), the convolution is an integer sum in int64 (exact, order-free), so the comparison needs no tolerance.
"""
from __future__ import annotations

import numpy as np

F = np.float32
MAX_R = 133144


def quantise(x, s_in) -> np.ndarray:
    """q = clamp(roundf(x * s_in), -127, 127) as int32: halves away from zero, NaN -> 0, +-inf -> +-127."""
    with np.errstate(invalid="ignore", over="ignore"):
        t = (np.asarray(x, F) * F(s_in)).astype(F)  # one fp32 rounding
        nan = np.isnan(t)
        t = np.where(nan, F(0), t)
        a = np.minimum(np.abs(t), F(1000))  # everything past 127 clamps anyway; keeps floor() of inf out of the arithmetic
        f = np.floor(a)
        r = np.where(a - f >= F(0.5), f + F(1), f)  # a - f is exact in fp32
        r = np.where(np.signbit(t), -r, r)
        return np.clip(r, -127, 127).astype(np.int32)


def dequant_scales(s_w, s_in) -> np.ndarray:
    """d[k] = 1 / (s_in * s_w[k]): the product rounded to fp32, then the reciprocal rounded; 0 where s_w[k] == 0."""
    s_w = np.asarray(s_w, F)
    with np.errstate(divide="ignore", over="ignore", under="ignore"):
        prod = (F(s_in) * s_w).astype(F)
        return np.where(s_w == 0, F(0), (F(1) / prod).astype(F)).astype(F)


def fold(d, b, mul, add):
    """A BatchNorm / Scale y * mul + add folded into the dequantisation: d' = d * mul, b' = b * mul + add (b = 0 without a bias)."""
    d, mul, add = np.asarray(d, F), np.asarray(mul, F), np.asarray(add, F)
    b = np.zeros_like(d) if b is None else np.asarray(b, F)
    return (d * mul).astype(F), ((b * mul).astype(F) + add).astype(F)


def out_dims(h, w, kh, kw, strides, pads):
    pl, pr, pt, pb = pads
    return (h + pt + pb - kh) // strides[0] + 1, (w + pl + pr - kw) // strides[1] + 1


def accumulate(q, wq, group=1, strides=(1, 1), pads=(0, 0, 0, 0)) -> np.ndarray:
    """acc[n][k][oy][ox] as int64; q [N][C][H][W] integers, wq [K][C/group][kh][kw] int8, pads = (left, right, top, bottom).  A tap
    outside the plane is q = 0."""
    q = np.asarray(q, np.int64)
    wq = np.asarray(wq, np.int64)
    n, c, h, w = q.shape
    k, cg, kh, kw = wq.shape
    assert c == cg * group and k % group == 0
    pl, pr, pt, pb = pads
    sh, sw = strides
    ho, wo = out_dims(h, w, kh, kw, strides, pads)
    qp = np.zeros((n, c, h + pt + pb, w + pl + pr), np.int64)
    qp[:, :, pt:pt + h, pl:pl + w] = q
    acc = np.zeros((n, k, ho, wo), np.int64)
    kg = k // group
    for g in range(group):
        xs = qp[:, g * cg:(g + 1) * cg]
        ws = wq[g * kg:(g + 1) * kg]
        for i in range(kh):
            for j in range(kw):
                win = xs[:, :, i:i + (ho - 1) * sh + 1:sh, j:j + (wo - 1) * sw + 1:sw]
                acc[:, g * kg:(g + 1) * kg] += np.einsum("nchw,kc->nkhw", win, ws[:, :, i, j])
    assert np.abs(acc).max(initial=0) < 2 ** 31
    return acc


def dequantise(acc, d, b=None, relu=False) -> np.ndarray:
    """y = act(float(acc) * d[k] + b[k]): the conversion rounds to nearest even, the product and the sum each round on their own."""
    with np.errstate(invalid="ignore", over="ignore"):
        y = (acc.astype(F) * np.asarray(d, F).reshape(1, -1, 1, 1)).astype(F)
        if b is not None:
            y = (y + np.asarray(b, F).reshape(1, -1, 1, 1)).astype(F)
        return np.maximum(y, F(0)) if relu else y


def qconv(x, wq, d, s_in, b=None, group=1, strides=(1, 1), pads=(0, 0, 0, 0), relu=False) -> np.ndarray:
    """The whole layer of the header on fp32 `x`; `d` from dequant_scales (or fold)."""
    return dequantise(accumulate(quantise(x, s_in), wq, group, strides, pads), d, b, relu)


def quantise_weights(w):
    """fp32 [K][...] -> (int8 weights, s_w[K]) with s_w = 127 / absmax(w[k]) (0 for an all-zero filter), ncnn's per-channel rule."""
    w = np.asarray(w, F)
    k = w.shape[0]
    amax = np.abs(w.reshape(k, -1)).max(axis=1).astype(F)
    with np.errstate(divide="ignore"):
        s_w = np.where(amax == 0, F(0), (F(127) / amax).astype(F)).astype(F)
    wq = quantise(w * s_w.reshape((k,) + (1,) * (w.ndim - 1)), 1.0).astype(np.int8)
    return wq, s_w


def synth(c, k, h, w, kh, kw, group, batch, seed, q_range=True):
    """(x, wq, s_w, s_in, bias): random int8 weights over the whole range, inputs that quantise over the whole q range (and past it)."""
    rng = np.random.default_rng(seed)
    wq = rng.integers(-127, 128, (k, c // group, kh, kw)).astype(np.int8)
    s_in = F(rng.uniform(0.7, 9.0))
    x = (rng.uniform(-140, 140, (batch, c, h, w)) / s_in).astype(F) if q_range else rng.standard_normal((batch, c, h, w)).astype(F)
    s_w = rng.uniform(0.5, 200.0, k).astype(F)
    bias = rng.standard_normal(k).astype(F)
    return x, wq, s_w, s_in, bias


# ---- a quantised net: tiny_quant and anything built from the same layer types ----------------------------------------------------------
def fma32(v, m, a) -> np.ndarray:
    """fl32(v * m + a) with ONE rounding, as the device's fused multiply-add gives it (the BatchNorm / Scale kernel), from float64
    arithmetic: the product of two fp32 values is exact in float64; the sum is rounded to odd (TwoSum tells whether it was inexact and in
    which direction), after which the rounding to fp32 is the rounding of the exact value."""
    p = np.asarray(v, np.float64) * np.asarray(m, np.float64)
    a = np.broadcast_to(np.asarray(a, np.float64), p.shape)
    s = p + a
    bb = s - p
    err = (p - (s - bb)) + (a - bb)
    even = (s.view(np.int64) & 1) == 0
    s = np.where((err != 0) & even, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(F)


def _layers(param: bytes):
    rows = param.decode().splitlines()[2:]
    for row in rows:
        t = row.split()
        nb, nt = int(t[2]), int(t[3])
        pd = {int(k): v for k, v in (x.split("=") for x in t[4 + nb + nt:])}
        yield t[0], t[1], t[4:4 + nb], t[4 + nb:4 + nb + nt], pd


class _Bin:
    def __init__(self, data: bytes):
        self.d, self.at = data, 0

    def raw(self, n):
        a = np.frombuffer(self.d, "<f4", n, self.at).copy()
        self.at += 4 * n
        return a

    def int8(self, n):
        assert int.from_bytes(self.d[self.at:self.at + 4], "little") == 0x000D4B38
        a = np.frombuffer(self.d, np.int8, n, self.at + 4).copy()
        self.at += 4 + (n + 3) // 4 * 4
        return a


def net_forward(model, x, level=0):
    """Every blob of a net of int8 Convolution / ConvolutionDepthWise / InnerProduct layers, plain ReLU, BatchNorm, Scale and 2x2 max
    Pooling, as feather::Net computes it at fusion `level`:
      0: layer by layer; BatchNorm and Scale are one fused multiply-add per element each;
      1: BatchNorm + Scale are one layer -- mul = mul_bn * mul_s, add = add_bn * mul_s + add_s on the host, each operation rounded -- of one
         fused multiply-add per element (the ReLU fusions do not change a bit);
      2: the composed map is folded into the convolution before it as feather_qconv.h defines (fold()).
    Blobs a fusion removes are absent (level 1: the BatchNorm top; level 2: also the convolution's own top)."""
    param, weights = model[0], model[1]
    rd = _Bin(weights)
    blobs = {}
    rows = list(_layers(param))
    pending = None  # level 2: (acc, d, b) of a convolution whose dequantisation waits for the layers folded into it
    affine = None   # level >= 1: (mul, add) composed so far, applied at the next layer that is not an affine one

    def flush_affine(src, top_name):
        nonlocal affine
        m, a = affine
        blobs[top_name] = fma32(blobs[src], m.reshape(1, -1, 1, 1), a.reshape(1, -1, 1, 1))
        affine = None

    for idx, (type_, name, bottoms, tops, pd) in enumerate(rows):
        top = tops[0]
        if type_ == "Input":
            blobs[top] = np.asarray(x, F)
            continue
        v = blobs.get(bottoms[0])
        if type_ in ("Convolution", "ConvolutionDepthWise", "InnerProduct"):
            assert int(pd[8]) == 1
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
            d = dequant_scales(s_w, s_in)
            acc = accumulate(quantise(v, s_in), wq, group, (s, s), (p, p, p, p))
            nxt = rows[idx + 1][0] if idx + 1 < len(rows) else ""
            if level >= 2 and nxt in ("BatchNorm", "Scale"):
                pending = (acc, d, b)
            else:
                blobs[top] = dequantise(acc, d, b)
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
                blobs[top] = fma32(v, m.reshape(1, -1, 1, 1), a.reshape(1, -1, 1, 1))
                continue
            affine = (m, a) if affine is None else ((affine[0] * m).astype(F), ((affine[1] * m).astype(F) + a).astype(F))
            nxt = rows[idx + 1][0] if idx + 1 < len(rows) else ""
            if level == 1 and not (type_ == "BatchNorm" and nxt == "Scale"):
                src = bottoms[0] if bottoms[0] in blobs else rows[idx - 1][2][0]
                flush_affine(src, top)
            elif level >= 2 and nxt not in ("BatchNorm", "Scale"):
                acc, d, b = pending
                d2, b2 = fold(d, b, *affine)
                blobs[top] = dequantise(acc, d2, b2)
                pending = affine = None
        elif type_ == "ReLU":
            blobs[top] = np.maximum(v, F(0))
        elif type_ == "Pooling":
            assert (int(pd[0]), int(pd[1]), int(pd[2]), int(pd.get(3, 0)), int(pd.get(4, 0))) == (0, 2, 2, 0, 0)
            n, c, h, w = v.shape
            blobs[top] = v.reshape(n, c, h // 2, 2, w // 2, 2).max(axis=(3, 5))
        else:
            raise ValueError(type_)
    assert rd.at == len(weights)
    return blobs
