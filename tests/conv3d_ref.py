"""include/feather_hip/feather_conv3d.h restated in numpy: Convolution3D / ConvolutionDepthWise3D in float64 (or the dtype asked for) and
Pooling3D -- the maximum in the input's own float32 (the kernel's very bits), the average in float64."""
import numpy as np

SAME_UPPER, SAME_LOWER = -233, -234


def three(v):
    return (int(v),) * 3 if isinstance(v, (int, np.integer)) else tuple(int(e) for e in v)


def six(p):
    """an int, (d, h, w) or (front, behind, top, bottom, left, right) -> (lo per axis, hi per axis); -233 / -234 first: SAME on every axis"""
    p = (p,) * 6 if isinstance(p, (int, np.integer)) else (tuple(q for q in p for _ in (0, 1)) if len(p) == 3 else tuple(p))
    return ((p[0],) * 3, (0,) * 3) if p[0] in (SAME_UPPER, SAME_LOWER) else (p[0::2], p[1::2])


def conv_axis(extent, k, d, s, lo, hi):
    """-> (lo, hi, out) of one axis"""
    ke = d * (k - 1) + 1
    if lo in (SAME_UPPER, SAME_LOWER):
        total = max(0, (-(-extent // s) - 1) * s + ke - extent)
        lo = total // 2 if lo == SAME_UPPER else total - total // 2
        hi = total - lo
    return lo, hi, (extent + lo + hi - ke) // s + 1


def pool_axis(extent, k, s, lo, hi, mode):
    if mode >= 2:
        total = max(0, k + (extent - 1) // s * s - extent)
        lo = total // 2 if mode == 2 else total - total // 2
        hi = total - lo
    room = extent + lo + hi - k
    return lo, hi, (-(-room // s) if mode == 0 else room // s) + 1


def activate(v, act, a0, a1):
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


def conv3d(x, w, bias=None, stride=1, dilation=1, pads=0, pad_value=0.0, group=1, act=0, a0=0.0, a1=0.0, dtype=np.float64):
    """x [n][C][D][H][W], w [K][C / group][kd][kh][kw] -> [n][K][Do][Ho][Wo]: a sum over the taps of matrix products over the channels."""
    x, w = np.asarray(x, dtype), np.asarray(w, dtype)
    n, c = x.shape[:2]
    k, cg, *kern = w.shape
    lo, hi = six(pads)
    axes = [conv_axis(e, kk, d, s, l, h) for e, kk, d, s, l, h in zip(x.shape[2:], kern, three(dilation), three(stride), lo, hi)]
    (sd, sh, sw), (dd, dh, dw), (od, oh, ow) = three(stride), three(dilation), [a[2] for a in axes]
    xp = np.pad(x, [(0, 0), (0, 0)] + [(a[0], a[1]) for a in axes], constant_values=dtype(pad_value))
    y = np.zeros((n, k, od, oh, ow), dtype)
    kg = k // group
    for g in range(group):
        for z in range(kern[0]):
            for i in range(kern[1]):
                for j in range(kern[2]):
                    win = xp[:, g * cg:(g + 1) * cg, z * dd:z * dd + (od - 1) * sd + 1:sd, i * dh:i * dh + (oh - 1) * sh + 1:sh, j * dw:j * dw + (ow - 1) * sw + 1:sw]
                    y[:, g * kg:(g + 1) * kg] += np.moveaxis(np.tensordot(w[g * kg:(g + 1) * kg, :, z, i, j], win, axes=([1], [1])), 0, 1)
    if bias is not None:
        y += np.asarray(bias, dtype).reshape(1, -1, 1, 1, 1)
    return activate(y, act, dtype(a0), dtype(a1))


def _window(extent, out, o, k, s, lo, hi, include):
    """-> (from, to, the divisor's factor) of output o of one axis; k == 0: adaptive"""
    if k == 0:
        a, b = o * extent // out, -(-(o + 1) * extent // out)
        return a, b, b - a
    start = o * s - lo
    a, b = max(start, 0), min(start + k, extent)
    return a, b, (min(start + k, extent + hi) - start) if include else b - a


def pool3d(x, kernel=0, stride=1, pads=0, pad_mode=0, avg=False, include_pad=False, global_=False, out_dhw=None):
    """x [n][C][D][H][W] -> [n][C][Do][Ho][Wo]: float32 for the maximum, float64 for the average."""
    x = np.asarray(x)
    ext, kern, st = x.shape[2:], three(kernel), three(stride)
    lo, hi = six(pads)
    if global_ or out_dhw is not None:
        kern, outs, lo, hi = (0, 0, 0), (1, 1, 1) if global_ else tuple(out_dhw), (0,) * 3, (0,) * 3
    else:
        axes = [pool_axis(e, k, s, l, h, pad_mode) for e, k, s, l, h in zip(ext, kern, st, lo, hi)]
        lo, hi, outs = [a[0] for a in axes], [a[1] for a in axes], [a[2] for a in axes]
    y = np.zeros(x.shape[:2] + tuple(outs), np.float64 if avg else np.float32)
    for o in np.ndindex(*outs):
        (z0, z1, cz), (y0, y1, cy), (x0, x1, cx) = [_window(ext[i], outs[i], o[i], kern[i], st[i], lo[i], hi[i], include_pad) for i in range(3)]
        cells = x[:, :, z0:z1, y0:y1, x0:x1]
        at = (slice(None), slice(None)) + o
        if not avg:
            y[at] = cells.max(axis=(2, 3, 4)) if cells.size else -np.finfo(np.float32).max
        elif cells.size and cz * cy * cx > 0:
            y[at] = cells.astype(np.float64).sum(axis=(2, 3, 4)) / (cz * cy * cx)
    return y
