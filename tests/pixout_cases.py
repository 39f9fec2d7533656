"""The case table of the image output path (libfeather_pixout.so, fhip_float_to_pixels), shared by tests/test_pixout_cpu.py (coverage of
the library's instantiations) and tests/test_pixout_gpu.py (the sweep that runs every case).

A case is (pixel type, geometry, mean / norm form, batch, dense or pitched).  `instance()` restates the library's dispatch
(feathercnn_amd/csrc_pixout/pixout.hip, launch()): the vector kernel when the first row and the pitch are aligned for its stores (4 bytes,
16 for 4 channels), the one-pixel-per-lane kernel otherwise.
"""
from __future__ import annotations

import itertools
import os

import numpy as np

import pixels_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "feathercnn_amd", "libfeather_pixout.so")

# the six types Mat::to_pixels writes anything for (mat_pixel.cpp:1412-1430) and their channels
TYPES = {"RGB": R.PIXEL_RGB, "BGR": R.PIXEL_BGR, "GRAY": R.PIXEL_GRAY, "RGBA": R.PIXEL_RGBA, "RGB2BGR": R.PIXEL_RGB2BGR,
         "BGR2RGB": R.PIXEL_BGR2RGB}
CHANNELS = {R.PIXEL_RGB: 3, R.PIXEL_BGR: 3, R.PIXEL_GRAY: 1, R.PIXEL_RGBA: 4, R.PIXEL_RGB2BGR: 3, R.PIXEL_BGR2RGB: 3}
REFUSED = sorted(set(R.TYPES.values()) - set(TYPES.values()))  # the converting-to-gray and from-gray / from-RGBA types

# name -> (w, h, target_w, target_h)
GEOMETRIES = {
    "equal_w4": (36, 20, 36, 20),          # equal size, rows a multiple of 4: the float4 loads
    "equal_odd": (37, 29, 37, 29),         # equal size, w odd: scalar loads, a byte tail
    "equal_224": (224, 224, 224, 224),
    "down_vga": (640, 480, 224, 224),
    "up_vga": (224, 224, 640, 480),
    "aspect": (200, 3, 7, 150),            # extreme aspect both ways, target width odd
    "up_tw_not4": (17, 13, 42, 31),        # target width not a multiple of 4
    "down_w_odd_tw4": (45, 33, 24, 18),    # w odd, target width a multiple of 4
}
BATCHES = (1, 3, 32)
POOL = 32  # images drawn per (type, geometry, mean / norm): batch 1 and 3 take windows of it, batch 32 all

_MEAN = np.array([-1.5, 2.25, 0.5, -3.0], np.float32)
_NORM = np.array([0.5, 2.0, 1.25, 0.75], np.float32)
MEAN_NORM = ("none", "mean", "norm", "both")


def mean_norm(form: str, cn: int):
    """(mean, norm) of a form: float32 arrays of cn values or None."""
    return (_MEAN[:cn] if form in ("mean", "both") else None, _NORM[:cn] if form in ("norm", "both") else None)


def pitch_of(tw: int, cn: int, pitched: bool) -> int:
    """Row pitch in bytes: dense, or the row rounded up to 16 bytes plus 16 (so a pitched case keeps the rows aligned and the dense cases
    with rows that are not a multiple of the alignment are the misaligned ones)."""
    row = tw * cn
    return (row + 15) // 16 * 16 + 16 if pitched else row


def instance(cn: int, pitch: int, address: int = 0) -> str:
    """The instantiation fhip_float_to_pixels launches for an output at `address` with rows `pitch` bytes apart."""
    align = 16 if cn == 4 else 4
    vec = address % align == 0 and pitch % align == 0
    return f"fhip::float_to_pixels_kernel<{cn}, {'true' if vec else 'false'}>"


def window(batch: int) -> slice:
    """Which images of the pool a batch takes."""
    return {1: slice(5, 6), 3: slice(7, 10), 32: slice(0, 32)}[batch]


def make_input(seed: int, n: int, cn: int, h: int, w: int, mean, norm) -> np.ndarray:
    """x[n][cn][h][w] float32 whose mean / norm image is about uniform(-60, 320) with fractions: both clamps and the truncation are hit."""
    rng = np.random.default_rng(seed)
    u = rng.uniform(-60.0, 320.0, (n, cn, h, w))
    if norm is not None:
        u = u / norm.astype(np.float64).reshape(1, cn, 1, 1)
    if mean is not None:
        u = u + mean.astype(np.float64).reshape(1, cn, 1, 1)
    return u.astype(np.float32)


def combos():
    """(type name, type, geometry name, (w, h, tw, th), mean / norm form): one pool of inputs and one restated result each."""
    return [(tn, t, gn, g, f) for (tn, t), (gn, g), f in itertools.product(TYPES.items(), GEOMETRIES.items(), MEAN_NORM)]


def cases():
    """Every case of the sweep: (type name, type, geometry name, (w, h, tw, th), form, batch, pitched)."""
    return [c + (b, p) for c in combos() for b in BATCHES for p in (False, True)]


def targets() -> set:
    """The instantiations the sweep's cases launch (outputs come from the allocator, 256-byte aligned)."""
    return {instance(CHANNELS[t], pitch_of(g[2], CHANNELS[t], p)) for _, t, _, g, _, _, p in cases()}
