"""include/feather_hip/feather_decoder.h restated in float64 numpy, line by line: what tests/test_decoder_gpu.py holds libfeather_decoder.so to."""
import numpy as np


def normalised_error(got, want):
    """The project's error: max|got - want| / max(|want|, 1e-30), NaN anywhere counts as infinite."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if got.shape != want.shape or not np.isfinite(got).all():
        return float("inf")
    return float(np.abs(got - want).max() / max(float(np.abs(want).max()), 1e-30))


def sdpa(q, k, v, mask=None, causal=False, scale=None):
    """q [n][heads][tq][d], k and v [n][kv_heads][tk][d], mask broadcastable to [n][heads][tq][tk] -> [n][heads][tq][d].  A row that sees no
    key is zeros."""
    q, k, v = (np.asarray(a, np.float64) for a in (q, k, v))
    n, heads, tq, d = q.shape
    tk, group = k.shape[2], heads // k.shape[1]
    k, v = np.repeat(k, group, axis=1), np.repeat(v, group, axis=1)  # query head h reads key/value head h / group
    s = np.einsum("nhtc,nhuc->nhtu", q, k) * (1 / np.sqrt(d) if scale is None else float(np.float32(scale)))
    if mask is not None:
        s = s + np.broadcast_to(np.asarray(mask, np.float64).reshape((1,) * (4 - np.ndim(mask)) + np.shape(mask)), s.shape)
    if causal:
        s = np.where(np.arange(tk)[None, :] <= np.arange(tq)[:, None] + (tk - tq), s, -np.inf)
    top = s.max(axis=3, keepdims=True)
    p = np.exp(s - np.where(np.isfinite(top), top, 0.0))  # a row of -inf: every weight 0
    total = p.sum(axis=3, keepdims=True)
    return np.einsum("nhtu,nhuc->nhtc", p / np.where(total > 0, total, 1.0), v)


def kv_concat(past, fresh):
    return fresh.copy() if past is None else np.concatenate([past, fresh], axis=2)


def rms_norm(x, gamma=None, eps=1e-6):
    x = np.asarray(x, np.float64)
    y = x / np.sqrt((x * x).mean(axis=-1, keepdims=True) + float(np.float32(eps)))
    return y if gamma is None else y * np.asarray(gamma, np.float64)


def rotary(x, cos, sin, interleaved=False):
    """x [n][heads][T][d]; cos, sin [T][d / 2] or [n][T][d / 2]."""
    x, cos, sin = (np.asarray(a, np.float64) for a in (x, cos, sin))
    cos, sin = (a[:, None] if a.ndim == 3 else a for a in (cos, sin))
    half = x.shape[3] // 2
    a, b = (x[..., 0::2], x[..., 1::2]) if interleaved else (x[..., :half], x[..., half:])
    ya, yb = a * cos - b * sin, a * sin + b * cos
    y = np.empty_like(x)
    if interleaved:
        y[..., 0::2], y[..., 1::2] = ya, yb
    else:
        y[..., :half], y[..., half:] = ya, yb
    return y


def embed(ids, weight, bias=None):
    out = weight[np.clip(ids, 0, weight.shape[0] - 1)]
    return out if bias is None else out + bias
