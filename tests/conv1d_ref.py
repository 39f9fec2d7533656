"""include/feather_hip/feather_conv1d.h restated in numpy: ncnn's Convolution1D / ConvolutionDepthWise1D (sums in `dtype`, float64 unless a
test asks what float32 gives) and Pooling1D (in the input's own type and order, so that a float32 input gives the kernel's very bits)."""
import numpy as np

SAME_UPPER, SAME_LOWER = -233, -234
FLT_MAX = np.float32(np.finfo(np.float32).max)


def conv_dims(l, kw, d=1, s=1, pl=0, pr=None):
    """-> (pad_left, pad_right, Lo)."""
    ke = d * (kw - 1) + 1
    if pl in (SAME_UPPER, SAME_LOWER):
        total = max(0, (-(-l // s) - 1) * s + ke - l)
        left = total // 2 if pl == SAME_UPPER else total - total // 2
        pl, pr = left, total - left
    elif pr is None:
        pr = pl
    return pl, pr, (l + pl + pr - ke) // s + 1


def activate(v, act, a0=0.0, a1=0.0):
    if act == 1:
        return np.maximum(v, 0)
    if act == 2:
        return np.where(v > 0, v, v * a0)
    if act == 3:
        return np.minimum(np.maximum(v, a0), a1)
    if act == 4:
        return 1 / (1 + np.exp(-v))
    if act == 5:
        return v * np.tanh(np.log(1 + np.exp(v)))
    if act == 6:
        return v * np.minimum(np.maximum(v * a0 + a1, 0), 1)
    return v


def conv1d(x, w, bias=None, s=1, d=1, pl=0, pr=None, pad_value=0.0, group=1, act=0, a0=0.0, a1=0.0, dtype=np.float64):
    """x [n][C][L], w [K][C / group][kw] -> [n][K][Lo]."""
    n, c, l = x.shape
    k, cg, kw = w.shape
    pl, pr, lo = conv_dims(l, kw, d, s, pl, pr)
    xp = np.full((n, c, l + pl + pr), pad_value, dtype)
    xp[:, :, pl:pl + l] = x
    y = np.zeros((n, k, lo), dtype)
    kg = k // group
    for g in range(group):
        for t in range(kw):
            win = xp[:, g * cg:(g + 1) * cg, t * d:t * d + (lo - 1) * s + 1:s]
            y[:, g * kg:(g + 1) * kg] += np.einsum("ncl,kc->nkl", win, w[g * kg:(g + 1) * kg, :, t].astype(dtype))
    if bias is not None:
        y += bias.astype(dtype)[None, :, None]
    return activate(y, act, dtype(a0), dtype(a1))


def pool_dims(l, kw, s=1, pl=0, pr=None, pad_mode=0):
    """-> (pad_left, pad_right, Lo) by ncnn's pad_mode."""
    pr = pl if pr is None else pr
    if pad_mode >= 2:
        total = max(0, kw + (l - 1) // s * s - l)
        pl = total // 2 if pad_mode == 2 else total - total // 2
        pr = total - pl
    room = l + pl + pr - kw
    return pl, pr, (-(-room // s) if pad_mode == 0 else room // s) + 1


def pool1d(x, kw=0, s=1, pl=0, pr=None, pad_mode=0, avg=False, include_pad=False, global_=False, out_w=None):
    """x [n][C][L] -> [n][C][Lo] in x's type."""
    l = x.shape[2]
    if global_ or out_w is not None:
        lo = 1 if global_ else out_w
        windows = [(o * l // lo, -(-(o + 1) * l // lo), -(-(o + 1) * l // lo) - o * l // lo) for o in range(lo)]
    else:
        pl, pr, lo = pool_dims(l, kw, s, pl, pr, pad_mode)
        windows = [(max(o * s - pl, 0), min(o * s - pl + kw, l), min(o * s - pl + kw, l + pr) - (o * s - pl)) for o in range(lo)]
    y = np.zeros(x.shape[:2] + (lo,), x.dtype)
    for o, (a, b, padded) in enumerate(windows):
        if not avg:
            y[:, :, o] = x[:, :, a:b].max(axis=2) if b > a else -FLT_MAX
        elif b > a:
            total = x[:, :, a].copy()
            for p in range(a + 1, b):
                total += x[:, :, p]
            y[:, :, o] = total / x.dtype.type(padded if include_pad else b - a)
    return y
