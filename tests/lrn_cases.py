"""The shape table of libfeather_lrn.so's tests (tests/test_lrn_cpu.py, tests/test_lrn_gpu.py): the smallest shapes at which each path of
csrc_lrn/lrn.hip can go wrong, and the tolerance they are held to.

Tolerance, element-wise against the float64 restatement:  |y - y64| <= T * |y64|,  T = E_REF + 16 * 2^-24.
  E_REF  the float32 restatement's own worst element-wise relative error against float64 over every row of this table (LRN_ROWS and the
         inputs of POOL_ROWS): the roundings of the squares, the sum, the product, the bias and the last product, and numpy's float32 power
  16 ulp the accuracy bound the OpenCL specification sets for pow, which the device math library is built to meet
Measured on the CPU with
    python tests/lrn_cases.py
which prints:  E_ref = 2.2925e-07 (row 'across c=17 4x12 ls=9 n=1 beta=1.25')   T = 1.1829e-06
E_REF below is that figure rounded up in its last digit; tests/test_lrn_cpu.py asserts that the restatements still agree within E_REF.

Inputs: every row but PUBLISHED uses alpha = local_size (across) or local_size^2 (within), so that a = 1, bias = 1 and x ~ N(0, 1): a tap
that is missing or read from the wrong place then moves y by several percent (tests/test_lrn_cpu.py proves it for every across-channel row).
With AlexNet's alpha = 1e-4 it would move y by 1e-5 and hide under any sensible tolerance.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

CHUNK = 16               # FHIP_LRN_CHUNK
CHUNKS = (4, 8, 16)      # the channels of a block: 16, halved to 8 and to 4 while the grid stays below 2048 blocks (every row here gets 4)
POOL_LDS_FLOATS = 8192   # FHIP_LRN_POOL_LDS_FLOATS
KERNELS = {"lrn_across_kernel", "lrn_within_kernel", "lrn_pool_lds_kernel", "lrn_pool_direct_kernel"}


def targets():
    """Every instantiation the library holds, as rocprofv3, fhip_lrn_route and fhip_lrn_pool_route name it."""
    return ({f"fhip::lrn_across_kernel<{v}, {l}>" for v in (1, 4) for l in (0, 3, 5)} | {"fhip::lrn_within_kernel", "fhip::lrn_pool_direct_kernel"} |
            {f"fhip::lrn_pool_lds_kernel<{l}>" for l in (0, 3, 5)})


E_REF = 2.2926e-07
T = E_REF + 16 * 2.0 ** -24


class Row(NamedTuple):
    id: str
    region: int
    n: int
    c: int
    h: int
    w: int
    local_size: int
    alpha: float
    beta: float = 0.75
    bias: float = 1.0


class PoolRow(NamedTuple):
    id: str
    lrn: Row
    kernel: int
    stride: int
    pad: int
    avg: bool
    route: str


PLANES = [(1, 1), (3, 5), (7, 7), (8, 8), (13, 13), (4, 12)]
SIZES = [1, 3, 5, 9]


def _channels(ls):
    return sorted({max(ls - 1, 1), 1, 2, ls} | {c for k in CHUNKS for c in (k - 1, k, k + 1, 2 * k + 3)})


def _across(c, hw, ls, n, beta=0.75):
    return Row(f"across c={c} {hw[0]}x{hw[1]} ls={ls} n={n}" + ("" if beta == 0.75 else f" beta={beta}"), 0, n, c, hw[0], hw[1], ls, float(ls), beta)


def _rows():
    rows, k = [], 0
    for ls in SIZES:  # every channel count with every local_size, the planes and batches taking turns
        for c in _channels(ls):
            rows.append(_across(c, PLANES[k % len(PLANES)], ls, 1 + 2 * (k % 2)))
            k += 5
    for ls in SIZES:  # every plane with every local_size, on more than one chunk
        for j, hw in enumerate(PLANES):
            rows.append(_across(CHUNK + 1 if j % 2 else 2 * CHUNK + 3, hw, ls, 3 - 2 * (j % 2)))
    rows.append(_across(2 * CHUNK + 3, (8, 8), 5, 2, beta=0.5))    # the second short form of the power
    rows.append(_across(2 * CHUNK + 3, (7, 7), 3, 2, beta=0.6))    # the device powf
    rows.append(_across(CHUNK + 1, (4, 12), 9, 1, beta=1.25))
    # a block of lrn_across_kernel owns 1024 pixels, a lane four of them (adjacent, or 256 apart): planes of more than one block, whose last
    # block is partly empty (1155 = 1024 + 131, 1156 = 1024 + 132), and a plane whose lanes own two or three pixels (600 = 2 * 256 + 88)
    rows.append(_across(CHUNK + 1, (33, 35), 5, 1))
    rows.append(_across(CHUNK + 1, (34, 34), 3, 2))
    rows.append(_across(5, (24, 25), 9, 1))
    seen, out = set(), []
    for r in rows:
        if r.id not in seen:
            seen.add(r.id)
            out.append(r)
    return out


ACROSS_ROWS = _rows()
# AlexNet's norm layers as published: the one row whose a is not 1
PUBLISHED = Row("across published 5 / 1e-4 / 0.75, c=35 13x13", 0, 2, 35, 13, 13, 5, 1e-4)
WITHIN_ROWS = [
    Row("within 2x2 ls=5 (plane smaller than the window)", 1, 2, 3, 2, 2, 5, 25.0),
    Row("within 5x5 ls=5 (plane = window)", 1, 1, 2, 5, 5, 5, 25.0),
    Row("within 3x3 ls=3 (plane = window)", 1, 3, 2, 3, 3, 3, 9.0),
    Row("within 9x7 ls=3", 1, 2, 3, 9, 7, 3, 9.0),
    Row("within 9x7 ls=5 beta=0.5", 1, 1, 5, 9, 7, 5, 25.0, 0.5),
    Row("within 9x7 ls=1 beta=0.6", 1, 1, 2, 9, 7, 1, 1.0, 0.6),
]
LRN_ROWS = ACROSS_ROWS + [PUBLISHED] + WITHIN_ROWS


def _pool(tag, c, h, w, ls, kernel, stride, pad, avg, route, n=2, region=0, beta=0.75):
    row = Row(f"{tag}: {'within' if region else 'across'} c={c} {h}x{w} ls={ls}", region, n, c, h, w, ls, float(ls * ls if region else ls), beta)
    return PoolRow(row.id, row, kernel, stride, pad, avg, route)


LDS, DIRECT = "fhip::lrn_pool_lds_kernel<%d>", "fhip::lrn_pool_direct_kernel"
# a band of lrn_pool_lds_kernel holds 8192 / 16 / w input rows: 5 rows of a 100-pixel-wide plane = two pooled rows of a 3 x 3 / stride-2
# pooling, so 7 input rows (three pooled rows) are the smallest height that spans two bands; 170 pixels a row leave 3 input rows, one
# pooled row a band, and are the widest plane of the LDS kernel (16 * 3 * 170 = 8160); 171 the narrowest of the direct one
POOL_ROWS = [
    _pool("max 3x3/2 on 7x7", 19, 7, 7, 5, 3, 2, 0, False, LDS % 5),
    _pool("max 3x3/2 on 8x8 (last window hangs over)", 35, 8, 8, 5, 3, 2, 0, False, LDS % 5),
    _pool("max 3x3/2 on 13x13 -> 6x6", 17, 13, 13, 3, 3, 2, 0, False, LDS % 3),
    _pool("max 2x2/2 on 8x8", 16, 8, 8, 9, 2, 2, 0, False, LDS % 0),
    _pool("avg 3x3/2 pad 1 on 7x7", 19, 7, 7, 5, 3, 2, 1, True, LDS % 5),
    _pool("avg 3x3/1 pad 1 on 5x6, 3 channels", 3, 5, 6, 5, 3, 1, 1, True, LDS % 5),
    _pool("two bands: max 3x3/2 on 7x100", 17, 7, 100, 5, 3, 2, 0, False, LDS % 5, n=1),
    _pool("one pooled row a band, the widest plane: avg 3x3/2 on 6x170", 3, 6, 170, 3, 3, 2, 0, True, LDS % 3, n=1),
    _pool("a band whose lanes own up to two pixels: max 3x3/2 on 9x50", 17, 9, 50, 5, 3, 2, 0, False, LDS % 5, n=1),
    # the channels of a block are 16 only on a grid of 2048 blocks, 8 from 2048 blocks of 8 on: the smallest tensors that get there are thin
    # planes of many channels (every other row of this table runs 4 channels a block)
    _pool("16 channels a block: max 2x2/1 on 3x3", 16 * 2048 - 3, 3, 3, 5, 2, 1, 0, False, LDS % 5, n=1),
    _pool("8 channels a block: avg 2x2/1 on 3x3", 8 * 2048 - 3, 3, 3, 3, 2, 1, 0, True, LDS % 3, n=1),
    _pool("too wide for a band: max 3x3/2 on 5x171", 6, 5, 171, 5, 3, 2, 0, False, DIRECT, n=1),
    _pool("within: max 3x3/2 on 8x8", 3, 8, 8, 3, 3, 2, 0, False, DIRECT, region=1),
    _pool("within: avg 2x2/2 on 9x7 beta 0.5", 2, 9, 7, 5, 2, 2, 0, True, DIRECT, region=1, beta=0.5),
]


def make_input(row: Row) -> np.ndarray:
    """x ~ N(0, 1), the same for a row wherever it is asked for."""
    seed = sum(ord(ch) * (i + 1) for i, ch in enumerate(row.id)) % (2 ** 31)
    return np.random.default_rng(seed).standard_normal((row.n, row.c, row.h, row.w)).astype(np.float32)


def rel_err(y, y64):
    """max |y - y64| / |y64| over the elements (y64 is never zero: x is not)."""
    return float(np.max(np.abs(y.astype(np.float64) - y64) / np.abs(y64)))


def measure_e_ref():
    """(E_ref, the row that gives it): the float32 restatement against the float64 one over the whole table."""
    import lrn_ref
    worst, at = 0.0, None
    for r in LRN_ROWS + [p.lrn for p in POOL_ROWS]:
        x = make_input(r)
        e = rel_err(lrn_ref.lrn(x, r.local_size, r.alpha, r.beta, r.bias, r.region), lrn_ref.lrn(x, r.local_size, r.alpha, r.beta, r.bias, r.region, np.float64))
        if e > worst:
            worst, at = e, r.id
    return worst, at


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    e, at = measure_e_ref()
    print(f"E_ref = {e:.4e} (row {at!r})   T = {e + 16 * 2.0 ** -24:.4e}")
