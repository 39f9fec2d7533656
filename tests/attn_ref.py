"""The numpy restatement of include/feather_hip/feather_attn.h, line by line: the attention core, LayerNorm, GELU and the element-wise binary
operations.  Sums run in float64 (`dtype=np.float64` arguments stay float64 throughout), results are returned in float64: the tests compare
the device's float32 with them by the project's normalised error.  model_zoo.numpy_forward's transformer layers are this text, not a second
one."""
import math

import numpy as np

ADD, SUB, MUL, DIV, MAX, MIN = range(6)
MFMA_MAX_D, DIRECT_MAX_D, LN_WAVE_MAX = 128, 4096, 256  # FHIP_ATTN_MFMA_MAX_D, FHIP_ATTN_DIRECT_MAX_D, FHIP_ATTN_LN_WAVE_MAX


def attention(q, k, v, heads):
    """q [n][Tq][E], k and v [n][Tk][E] -> [n][Tq][E]: per image and head, softmax over the keys of q k^T (the row maximum subtracted), times v.
    The caller has scaled q."""
    q, k, v = (np.asarray(t, np.float64) for t in (q, k, v))
    n, tq, e = q.shape
    tk = k.shape[1]
    if e % heads or tk < 1:
        raise ValueError("E % heads != 0, or no key")
    d = e // heads
    out = np.empty((n, tq, e))
    for i in range(n):
        for h in range(heads):
            c = slice(h * d, (h + 1) * d)
            s = q[i, :, c] @ k[i, :, c].T
            p = np.exp(s - s.max(axis=1, keepdims=True))
            out[i, :, c] = (p / p.sum(axis=1, keepdims=True)) @ v[i, :, c]
    return out


def attention_route(e, heads):
    d = e // heads
    return "fhip::attention_mfma_kernel<%d>" % ((d + 31) // 32) if d % 4 == 0 and d <= MFMA_MAX_D else "fhip::attention_direct_kernel"


def layer_norm(x, gamma=None, beta=None, eps=1e-3):
    """Over the last dimension: mean, then the biased variance of the centred row."""
    x = np.asarray(x, np.float64)
    mean = x.mean(axis=-1, keepdims=True)
    c = x - mean
    var = (c * c).mean(axis=-1, keepdims=True)
    y = c / np.sqrt(var + np.float64(np.float32(eps)))
    if gamma is not None:
        y = y * np.asarray(gamma, np.float64)
    if beta is not None:
        y = y + np.asarray(beta, np.float64)
    return y


_erf = np.vectorize(math.erf, otypes=[np.float64])


def gelu(x, fast=False):
    x = np.asarray(x, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        if fast:
            return 0.5 * x * (1 + np.tanh(np.float64(np.float32(0.79788452)) * (x + np.float64(np.float32(0.044715)) * x * x * x)))
        return 0.5 * x * (1 + _erf(np.float64(np.float32(0.70710678)) * x))


def binary(op, a, b, swap=False):
    """a op b (b op a with swap) in the dtype of the operands: float32 inputs give the float32 result the device must equal bit for bit (div
    aside).  b: a scalar, an array of a's shape, or one image's worth of it (broadcast over the leading dimension)."""
    a = np.asarray(a)
    b = np.asarray(b, a.dtype)
    if b.ndim and b.size != a.size:
        b = np.broadcast_to(b.reshape((1,) + a.shape[1:]), a.shape)
    x, y = (b, a) if swap else (a, b)
    with np.errstate(all="ignore"):
        return [np.add, np.subtract, np.multiply, np.divide, np.fmax, np.fmin][op](x, y)


def multi_head_attention(q, k, v, heads, weights, scale=None):
    """ncnn's MultiHeadAttention on tokens q [n][Tq][E], k, v [n][Tk][E]: weights = (wq, bq, wk, bk, wv, bv, wo, bo), rows [out][in]; q is scaled
    after its bias."""
    wq, bq, wk, bk, wv, bv, wo, bo = (np.asarray(t, np.float64) for t in weights)
    e = wq.shape[0]
    scale = 1.0 / np.sqrt(np.float32(e // heads)) if scale is None else scale
    f = np.float64(np.float32(scale))
    qp = (np.asarray(q, np.float64) @ wq.T + bq) * f
    kp = np.asarray(k, np.float64) @ wk.T + bk
    vp = np.asarray(v, np.float64) @ wv.T + bv
    return attention(qp, kp, vp, heads) @ wo.T + bo


def normalised_error(got, want):
    """The project's error measure (tests/test_net_gpu.py): the largest difference over the largest magnitude of the reference."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-30))
