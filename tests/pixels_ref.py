"""ncnn's pixel input path restated in numpy (the project's own code): Mat::from_pixels_resize (reference src/ncnn/mat_pixel.cpp:1369-1410)
with the fixed-point bilinear resize of mat_pixel_resize.cpp, the channel conversions of mat_pixel.cpp, and upstream ncnn's
substract_mean_normalize (mean only: x - mean; norm only: x * norm; both: x * norm + (-(mean * norm)), two roundings).

Every step is written with the same integer / float32 / float64 operations as the reference, so the result is bit-exact, not close.
tests/golden/pixel_golden.npz (recorded from the reference's own functions) checks this module; the GPU tests check the kernel against it.
"""
from __future__ import annotations

import numpy as np

PIXEL_CONVERT_SHIFT = 16
PIXEL_RGB, PIXEL_BGR, PIXEL_GRAY, PIXEL_RGBA = 1, 2, 4, 8
PIXEL_RGB2BGR = PIXEL_RGB | (PIXEL_BGR << 16)
PIXEL_RGB2GRAY = PIXEL_RGB | (PIXEL_GRAY << 16)
PIXEL_BGR2RGB = PIXEL_BGR | (PIXEL_RGB << 16)
PIXEL_BGR2GRAY = PIXEL_BGR | (PIXEL_GRAY << 16)
PIXEL_GRAY2RGB = PIXEL_GRAY | (PIXEL_RGB << 16)
PIXEL_GRAY2BGR = PIXEL_GRAY | (PIXEL_BGR << 16)
PIXEL_RGBA2RGB = PIXEL_RGBA | (PIXEL_RGB << 16)
PIXEL_RGBA2BGR = PIXEL_RGBA | (PIXEL_BGR << 16)
PIXEL_RGBA2GRAY = PIXEL_RGBA | (PIXEL_GRAY << 16)

TYPES = {"RGB": PIXEL_RGB, "BGR": PIXEL_BGR, "GRAY": PIXEL_GRAY, "RGBA": PIXEL_RGBA, "RGB2BGR": PIXEL_RGB2BGR,
         "RGB2GRAY": PIXEL_RGB2GRAY, "BGR2RGB": PIXEL_BGR2RGB, "BGR2GRAY": PIXEL_BGR2GRAY, "GRAY2RGB": PIXEL_GRAY2RGB,
         "GRAY2BGR": PIXEL_GRAY2BGR, "RGBA2RGB": PIXEL_RGBA2RGB, "RGBA2BGR": PIXEL_RGBA2BGR, "RGBA2GRAY": PIXEL_RGBA2GRAY}
_CH = {PIXEL_RGB: 3, PIXEL_BGR: 3, PIXEL_GRAY: 1, PIXEL_RGBA: 4}


def channels(ptype: int):
    """(source channels, output channels) of a pixel type; ValueError for a type ncnn's from_pixels does not know."""
    if ptype not in TYPES.values():
        raise ValueError(f"unknown pixel type {ptype:#x}")
    src, dst = ptype & 0xFFFF, ptype >> 16
    return _CH[src], _CH[dst or src]


def _coef(src: int, dst: int):
    """(offsets, k0, k1) along one axis, resize_bilinear_c1's coefficient loop (mat_pixel_resize.cpp:46-71)."""
    scale = np.float64(src) / np.float64(dst)
    d = np.arange(dst, dtype=np.float64)
    f = ((d + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = (f - s.astype(np.float32)).astype(np.float32)
    lo = s < 0
    s[lo], f[lo] = 0, np.float32(0)
    hi = s >= src - 1
    s[hi], f[hi] = src - 2, np.float32(1)

    def sat(x):  # SATURATE_CAST_SHORT: (int)(x + (x >= 0 ? 0.5f : -0.5f)), clamped to short
        r = (x + np.where(x >= 0, np.float32(0.5), np.float32(-0.5)).astype(np.float32)).astype(np.float32)
        return np.clip(np.trunc(r).astype(np.int64), -32768, 32767)

    k0 = sat((np.float32(1) - f).astype(np.float32) * np.float32(2048))
    k1 = sat((f * np.float32(2048)).astype(np.float32))
    return s, k0, k1


def resize_bilinear(src: np.ndarray, tw: int, th: int) -> np.ndarray:
    """resize_bilinear_c1 / c3 / c4 on [N][h][w][c] uint8 -> [N][th][tw][c] uint8 (each channel the same way)."""
    n, h, w, c = src.shape
    if w < 2 or h < 2:
        raise ValueError("a source 1 pixel wide or high cannot be resized (the reference reads index -1)")
    sx, a0, a1 = _coef(w, tw)
    sy, b0, b1 = _coef(h, th)
    S = src.astype(np.int64)

    def hrow(rows):  # (S[sx]*a0 + S[sx+1]*a1) >> 4, stored as short
        r = S[:, rows]  # [N][th][w][c]
        v = (r[:, :, sx] * a0[None, None, :, None] + r[:, :, sx + 1] * a1[None, None, :, None]) >> 4
        return v.astype(np.int16).astype(np.int64)

    row0, row1 = hrow(sy), hrow(sy + 1)
    B0, B1 = b0[None, :, None, None], b1[None, :, None, None]
    t0 = ((B0 * row0) >> 16).astype(np.int16).astype(np.int64)
    t1 = ((B1 * row1) >> 16).astype(np.int16).astype(np.int64)
    return (((t0 + t1 + 2) >> 2) & 0xFF).astype(np.uint8)


def convert(px: np.ndarray, ptype: int) -> np.ndarray:
    """Mat::from_pixels on [N][h][w][cin] uint8 -> [N][cout][h][w] float32 (mat_pixel.cpp:1329-1367)."""
    cin, cout = channels(ptype)
    src, dst = ptype & 0xFFFF, (ptype >> 16) or (ptype & 0xFFFF)
    p = px.astype(np.int64)
    if cout == 1 and cin > 1:
        r, g, b = (p[..., 2], p[..., 1], p[..., 0]) if src == PIXEL_BGR else (p[..., 0], p[..., 1], p[..., 2])
        return ((r * 77 + g * 150 + b * 29) >> 8).astype(np.float32)[:, None]
    if cin == 1:
        return np.repeat(p[..., 0:1], cout, axis=-1).transpose(0, 3, 1, 2).astype(np.float32)
    swap = (dst == PIXEL_BGR) != (src == PIXEL_BGR)  # RGB <-> BGR, RGBA -> BGR
    order = [2, 1, 0] if swap else list(range(cout))
    return p[..., order].transpose(0, 3, 1, 2).astype(np.float32)


def mean_norm(x: np.ndarray, mean=None, norm=None) -> np.ndarray:
    """substract_mean_normalize over [N][C][H][W] float32, float32 arithmetic rounded after every operation."""
    x = np.asarray(x, np.float32)
    c = x.shape[1]
    m = None if mean is None else np.asarray(mean, np.float32).reshape(1, c, 1, 1)
    s = None if norm is None else np.asarray(norm, np.float32).reshape(1, c, 1, 1)
    if m is not None and s is not None:
        mb = -(m * s)
        return ((x * s).astype(np.float32) + mb).astype(np.float32)
    if m is not None:
        return (x - m).astype(np.float32)
    if s is not None:
        return (x * s).astype(np.float32)
    return x.copy()


def from_pixels_resize(pixels: np.ndarray, ptype: int, tw: int, th: int, mean=None, norm=None) -> np.ndarray:
    """[N][h][w][cin] (or [h][w][cin]) uint8 -> [N][cout][th][tw] float32: resize in the source format when the size changes, then
    the conversion, then mean / norm."""
    px = np.asarray(pixels, np.uint8)
    if px.ndim == 3:
        px = px[None]
    cin, _ = channels(ptype)
    if px.shape[3] != cin:
        raise ValueError(f"pixel type {ptype:#x} has {cin} source channels, the array {px.shape[3]}")
    _, h, w, _ = px.shape
    if (w, h) != (tw, th):
        px = resize_bilinear(px, tw, th)
    return mean_norm(convert(px, ptype), mean, norm)
