"""NV21 (yuv420sp) camera frames to the fp32 input tensor, restated in numpy (the project's own code): the reference's two chains

    resize_first = 1: resize_bilinear_yuv420sp (mat_pixel_resize.cpp:1174-1189) -> yuv420sp2rgb -> Mat::from_pixels(rgb, type)
    resize_first = 0: yuv420sp2rgb -> Mat::from_pixels_resize(rgb, type, w, h, tw, th)

with yuv420sp2rgb's C path (mat_pixel.cpp:1266-1320), then substract_mean_normalize.  The resize, the conversions and mean / norm are
tests/pixels_ref.py's; tests/golden/yuv_golden.npz (recorded from the reference's own functions) checks this module, and the GPU tests
check the kernel against it.  A frame is [h*3/2][w] uint8: h rows of Y, then h/2 rows of w/2 interleaved V,U pairs.
"""
from __future__ import annotations

import numpy as np

import pixels_ref as R

TYPES = {"RGB": R.PIXEL_RGB, "RGB2BGR": R.PIXEL_RGB2BGR, "RGB2GRAY": R.PIXEL_RGB2GRAY}


def frames(yuv: np.ndarray, w: int = None, h: int = None) -> np.ndarray:
    """[N][h*3/2][w] uint8 (or one [h*3/2][w] frame, or flat bytes with w / h given) -> [N][h*3/2][w]."""
    f = np.asarray(yuv, np.uint8)
    if w is not None:
        f = f.reshape(-1, h * 3 // 2, w)
    if f.ndim == 2:
        f = f[None]
    n, rows, fw = f.shape
    if fw % 2 or rows % 3 or (rows * 2 // 3) % 2:
        raise ValueError(f"not an NV21 frame: {f.shape}")
    return f


def planes(f: np.ndarray):
    """(Y [N][h][w][1], VU [N][h/2][w/2][2]) of [N][h*3/2][w] frames."""
    n, rows, w = f.shape
    h = rows * 2 // 3
    return f[:, :h, :, None], f[:, h:, :].reshape(n, h // 2, w // 2, 2)


def join(Y: np.ndarray, VU: np.ndarray) -> np.ndarray:
    """The inverse of planes()."""
    n, h, w, _ = Y.shape
    return np.concatenate([Y.reshape(n, h, w), VU.reshape(n, h // 2, w)], axis=1)


def yuv420sp2rgb(f: np.ndarray) -> np.ndarray:
    """[N][h*3/2][w] NV21 -> [N][h][w][3] RGB bytes: v = V - 128, u = U - 128 per 2x2 block; (Y<<6) + 90v, (Y<<6) - 46v - 22u,
    (Y<<6) + 113u; arithmetic >> 6, clamped to 0..255."""
    Y, VU = planes(f)
    y = Y[..., 0].astype(np.int64) << 6
    vu = np.repeat(np.repeat(VU.astype(np.int64) - 128, 2, axis=1), 2, axis=2)
    v, u = vu[..., 0], vu[..., 1]
    rgb = np.stack([y + 90 * v, y - 46 * v - 22 * u, y + 113 * u], axis=-1) >> 6
    return np.clip(rgb, 0, 255).astype(np.uint8)


def resize_bilinear_yuv420sp(f: np.ndarray, tw: int, th: int) -> np.ndarray:
    """[N][h*3/2][w] -> [N][th*3/2][tw]: Y as resize_bilinear_c1, VU as resize_bilinear_c2 at (w/2, h/2) -> (tw/2, th/2)."""
    Y, VU = planes(f)
    if (tw | th) & 1:
        raise ValueError("resize_bilinear_yuv420sp needs an even target size")
    return join(R.resize_bilinear(Y, tw, th), R.resize_bilinear(VU, tw // 2, th // 2))


def check(ptype: int, w: int, h: int, tw: int, th: int, resize_first: bool):
    """The refusals of fhip_yuv420sp_to_float, as ValueError."""
    if ptype not in TYPES.values():
        raise ValueError(f"pixel type {ptype:#x}: an NV21 frame converts as PIXEL_RGB, PIXEL_RGB2BGR or PIXEL_RGB2GRAY")
    if min(w, h, tw, th) < 1 or (w | h) & 1:
        raise ValueError("an NV21 frame has a positive, even width and height")
    if resize_first and ((tw | th) & 1 or w < 4 or h < 4):
        raise ValueError("resize_first needs an even target size and a frame of at least 4x4 pixels")


def yuv420sp_to_float(yuv: np.ndarray, ptype: int, tw: int, th: int, resize_first: bool = True, mean=None, norm=None) -> np.ndarray:
    """[N][h*3/2][w] (or [h*3/2][w]) NV21 uint8 -> [N][cout][th][tw] float32, the chain resize_first picks, then mean / norm."""
    f = frames(yuv)
    _, rows, w = f.shape
    h = rows * 2 // 3
    check(ptype, w, h, tw, th, resize_first)
    if resize_first:
        return R.mean_norm(R.convert(yuv420sp2rgb(resize_bilinear_yuv420sp(f, tw, th)), ptype), mean, norm)
    return R.from_pixels_resize(yuv420sp2rgb(f), ptype, tw, th, mean, norm)


def to_pixels(m: np.ndarray, ptype: int) -> np.ndarray:
    """Mat::to_pixels of a [C][h][w] float32 Mat -> [h][w][cn] bytes (mat_pixel.cpp:1412-1430): (int) truncation, clamp 0..255;
    RGB2BGR / BGR2RGB reverse the channel order.  None for a type the reference writes nothing for."""
    m = np.asarray(m, np.float32)
    if ptype in (R.PIXEL_RGB2BGR, R.PIXEL_BGR2RGB):
        order = [2, 1, 0]
    elif ptype in (R.PIXEL_RGB, R.PIXEL_BGR):
        order = [0, 1, 2]
    elif ptype == R.PIXEL_GRAY:
        order = [0]
    elif ptype == R.PIXEL_RGBA:
        order = [0, 1, 2, 3]
    else:
        return None
    return np.clip(np.trunc(m[order]).astype(np.int64), 0, 255).astype(np.uint8).transpose(1, 2, 0)


def to_pixels_resize(m: np.ndarray, ptype: int, tw: int, th: int) -> np.ndarray:
    """Mat::to_pixels_resize (mat_pixel.cpp:1432-1468): to_pixels, then the bilinear resize in the output format."""
    px = to_pixels(m, ptype)
    if px is None or px.shape[:2] == (th, tw):
        return px
    return R.resize_bilinear(px[None], tw, th)[0]
