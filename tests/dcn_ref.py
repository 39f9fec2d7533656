"""include/feather_hip/feather_dcn.h restated in numpy: deformable convolution (DCN v1 / v2, ncnn's DeformableConv2D), with loops over the
taps only.  Sums and coordinates in `dtype`: float64 unless a test asks what float32 gives."""
import numpy as np

from conv1d_ref import activate


def output_dim(h, w, kernel, dilation=(1, 1), stride=(1, 1), pads=(0, 0, 0, 0)):
    """-> (Ho, Wo); kernel, dilation, stride (vertical, horizontal), pads (top, bottom, left, right)."""
    (kh, kw), (dh, dw), (sh, sw), (pt, pb, pl, pr) = kernel, dilation, stride, pads
    return (h + pt + pb - (dh * (kh - 1) + 1)) // sh + 1, (w + pl + pr - (dw * (kw - 1) + 1)) // sw + 1


def sample(x, py, px, dtype=np.float64):
    """x [n][C][H][W] at py, px [n][C][Ho][Wo] -> [n][C][Ho][Wo]: 0 outside the open range (-1, H) x (-1, W), else bilinear over the four
    neighbours, a corner outside the plane contributing 0."""
    n, c, h, w = x.shape
    inside = (py > -1) & (px > -1) & (py < h) & (px < w)
    y0, x0 = np.floor(py), np.floor(px)
    ly, lx = py - y0, px - x0
    ni, ci = np.arange(n)[:, None, None, None], np.arange(c)[None, :, None, None]
    out = np.zeros(py.shape, dtype)
    for cy, cx, wt in ((0, 0, (1 - ly) * (1 - lx)), (0, 1, (1 - ly) * lx), (1, 0, ly * (1 - lx)), (1, 1, ly * lx)):
        yy, xx = (y0 + cy).astype(np.int64), (x0 + cx).astype(np.int64)
        ok = inside & (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
        out += np.where(ok, wt * x[ni, ci, np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)], 0)
    return out


def deform_conv2d(x, offset, mask, w, bias=None, stride=(1, 1), dilation=(1, 1), pads=(0, 0, 0, 0), offset_groups=1, act=0, a0=0.0, a1=0.0, dtype=np.float64):
    """x [n][C][H][W], offset [n][G * 2 * kh * kw][Ho][Wo], mask [n][G * kh * kw][Ho][Wo] or None, w [K][C][kh][kw] -> [n][K][Ho][Wo]."""
    n, c, h, wd = x.shape
    k, _, kh, kw = w.shape
    g, (sh, sw), (dh, dw), (pt, _, pl, _) = offset_groups, stride, dilation, pads
    ho, wo = output_dim(h, wd, (kh, kw), dilation, stride, pads)
    x, offset = x.astype(dtype), offset.astype(dtype).reshape(n, g, kh * kw, 2, ho, wo)
    m = None if mask is None else mask.astype(dtype).reshape(n, g, kh * kw, ho, wo)
    rows, cols = np.arange(ho, dtype=dtype)[:, None] * sh - pt, np.arange(wo, dtype=dtype)[None, :] * sw - pl
    per = c // g  # channel c reads the offsets of group c // per
    y = np.zeros((n, k, ho, wo), dtype)
    for i in range(kh):
        for j in range(kw):
            t = i * kw + j
            py = np.repeat((rows + dtype(i * dh))[None, None] + offset[:, :, t, 0], per, axis=1)
            px = np.repeat((cols + dtype(j * dw))[None, None] + offset[:, :, t, 1], per, axis=1)
            v = sample(x, py, px, dtype)
            if m is not None:
                v = v * np.repeat(m[:, :, t], per, axis=1)
            y += np.einsum("nchw,kc->nkhw", v, w[:, :, i, j].astype(dtype))
    if bias is not None:
        y += bias.astype(dtype)[None, :, None, None]
    return activate(y, act, dtype(a0), dtype(a1))


def conv2d(x, w, bias=None, stride=(1, 1), dilation=(1, 1), pads=(0, 0, 0, 0), dtype=np.float64):
    """The plain convolution of the same geometry: what zero offsets and no mask must give."""
    n, c, h, wd = x.shape
    k, _, kh, kw = w.shape
    (sh, sw), (dh, dw), (pt, pb, pl, pr) = stride, dilation, pads
    ho, wo = output_dim(h, wd, (kh, kw), dilation, stride, pads)
    xp = np.zeros((n, c, h + pt + pb, wd + pl + pr), dtype)
    xp[:, :, pt:pt + h, pl:pl + wd] = x
    y = np.zeros((n, k, ho, wo), dtype)
    for i in range(kh):
        for j in range(kw):
            win = xp[:, :, i * dh:i * dh + (ho - 1) * sh + 1:sh, j * dw:j * dw + (wo - 1) * sw + 1:sw]
            y += np.einsum("nchw,kc->nkhw", win, w[:, :, i, j].astype(dtype))
    if bias is not None:
        y += bias.astype(dtype)[None, :, None, None]
    return y
