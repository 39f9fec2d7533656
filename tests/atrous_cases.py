"""The case table of the dilated-convolution route (libfeather_atrous.so), shared by tests/test_atrous_cpu.py (the definition against
torch, coverage of the library's instantiations) and tests/test_atrous_gpu.py (the sweep that runs every case).

A case is (name, C, K, group, H, W, kh, kw, stride, pads (left, right, top, bottom), dilation (dh, dw), offset): `offset` floats past a
16-byte boundary for the input and output tensors (0: allocator-aligned, 1: the 4-byte-aligned forms).  `instance()` restates the library's
dispatch (feathercnn_amd/csrc_atrous/atrous.hip, select()):
  * group == C == K > 1, 3x3, stride 1 or 2 in both directions: the depthwise kernel; its 16-byte form when Wo % 4 == 0 (stride 1: and W >= 4);
  * group 1, C % 16 == 0, K >= 48: the fp32-MFMA implicit GEMM, the 128-row tile from 96 output channels on, else the 64-row tile; always the
    scalar B-operand form (ROW4 -- stride_w == 1, Wo % 4 == 0, W >= 4 -- is never selected: it measured slower at batch 1; it runs by name
    through fhip_atrous_forward_route, which the sweep does for every case it accepts); tap skipping when the kernel has at most 16 taps
    and (pad_top // stride_h) * Wo >= the tile's columns (64 for the 128-row tile, 128 for the 64-row tile);
  * the generic kernel for everything else -- other groups, K < 48, and group 1 with C % 16 != 0 (a k-tile of 16 would straddle two taps).
Every case also launches one of the three weight packers.
"""
from __future__ import annotations

import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "feathercnn_amd", "libfeather_atrous.so")
GENERIC = "fhip::atrous_generic_kernel<4>"
PACK_GENERIC, PACK_COPY, PACK_MFMA = "fhip::atrous_pack_generic_kernel", "fhip::atrous_pack_copy_kernel", "fhip::atrous_pack_mfma_kernel"
BIG, SMALLM = "fhip::GemmShape<128, 64, 16, 2, 2, 4>", "fhip::GemmShape<64, 128, 16, 1, 4, 4>"


def _b(v):
    return "true" if v else "false"


def mfma(shape, row4, skip):
    return f"fhip::gemm_mfma_kernel<{shape}, fhip::AtrousGemmPolicy<{_b(row4)}, {_b(skip)}> >"


def dw(stride, vec):
    return f"fhip::atrous_dw3x3_kernel<{stride}, {_b(vec)}>"


def P(v):
    return (v, v, v, v)


# name, C, K, group, H, W, kh, kw, stride, pads (l, r, t, b), dilation (dh, dw), offset
CASES = [
    # MFMA, ROW4 (stride_w 1, Wo % 4 == 0)
    ("row4_c16_k64_9x8_d2", 16, 64, 1, 9, 8, 3, 3, 1, P(2), (2, 2), 0),          # the stride-1 "same" layer of every segmentation net
    ("row4_k72", 16, 72, 1, 6, 8, 3, 3, 1, P(2), (2, 2), 0),                    # a partial second row tile (64-row tile)
    ("row4_k50", 16, 50, 1, 5, 4, 3, 3, 1, P(2), (2, 2), 0),                    # a partial row tile; the narrowest ROW4 plane
    ("row4_big_k100", 16, 100, 1, 7, 8, 3, 3, 1, P(2), (2, 2), 0),              # the 128-row tile, partial
    ("row4_c32", 32, 64, 1, 6, 8, 3, 3, 1, P(3), (3, 3), 0),                    # two k-tiles per tap
    ("row4_d2x3_asym", 16, 64, 1, 7, 8, 3, 3, 1, (2, 4, 1, 3), (2, 3), 0),      # dilation (2, 3), asymmetric pads
    ("row4_centre_only_d12", 16, 96, 1, 8, 8, 3, 3, 1, P(12), (12, 12), 0),     # only the centre tap is ever inside: a 1x1 convolution; skipping
    ("row4_5x8_d6", 16, 64, 1, 5, 8, 3, 3, 1, P(6), (6, 6), 0),
    ("row4_small_skip_d16", 16, 64, 1, 8, 8, 3, 3, 1, P(16), (16, 16), 1),      # the 64-row tile with tap skipping
    ("row4_offset1", 16, 64, 1, 6, 12, 3, 3, 1, P(2), (2, 2), 1),               # tensors 4 bytes past a 16-byte boundary
    ("row4_valid_p0", 16, 64, 1, 10, 12, 3, 3, 1, P(0), (2, 2), 0),             # no padding: the output shrinks
    ("row4_k5_d2", 16, 64, 1, 9, 8, 5, 5, 1, P(4), (2, 2), 0),                  # 25 taps: never skipping
    ("row4_s2x1", 16, 64, 1, 9, 8, 3, 3, (2, 1), P(2), (2, 2), 0),              # stride_h 2 keeps ROW4
    ("row4_big_skip_d9_b3", 32, 128, 1, 6, 8, 3, 3, 1, P(9), (9, 9), 1),
    # MFMA, scalar
    ("scalar_w7", 16, 64, 1, 8, 7, 3, 3, 1, P(2), (2, 2), 0),                   # Wo % 4 != 0
    ("scalar_s2_d2", 16, 96, 1, 9, 9, 3, 3, 2, P(2), (2, 2), 0),                # stride 2
    ("scalar_s2x1", 16, 64, 1, 9, 7, 3, 3, (2, 1), P(2), (2, 2), 1),
    ("scalar_k1x3_d1x2", 16, 64, 1, 6, 9, 1, 3, 1, (2, 2, 0, 0), (1, 2), 0),    # one axis only
    ("scalar_k3x1_d3x1", 16, 64, 1, 8, 7, 3, 1, 1, (0, 0, 3, 3), (3, 1), 0),
    ("scalar_big_skip_d12", 16, 96, 1, 8, 7, 3, 3, 1, P(12), (12, 12), 0),
    ("scalar_small_skip_d20", 32, 50, 1, 7, 7, 3, 3, 1, P(20), (20, 20), 1),
    ("scalar_s3_skip", 16, 100, 1, 10, 10, 3, 3, 3, P(12), (6, 6), 0),          # skipping with a stride: (12 // 3) * 9 rows of padding
    # depthwise 3x3
    ("dw_c21_8x8_d2", 21, 21, 21, 8, 8, 3, 3, 1, P(2), (2, 2), 0),
    ("dw_c8_7x9_d4", 8, 8, 8, 7, 9, 3, 3, 1, P(4), (4, 4), 0),
    ("dw_c8_7x9_d2", 8, 8, 8, 7, 9, 3, 3, 1, P(2), (2, 2), 1),
    ("dw_s2_d2", 8, 8, 8, 9, 9, 3, 3, 2, P(2), (2, 2), 0),
    ("dw_s2_vec", 21, 21, 21, 7, 15, 3, 3, 2, P(2), (2, 2), 1),
    ("dw_plane_smaller_than_d", 8, 8, 8, 4, 4, 3, 3, 1, P(6), (6, 6), 0),
    ("dw_offset1", 8, 8, 8, 6, 8, 3, 3, 1, P(2), (2, 2), 1),
    ("dw_w3", 5, 5, 5, 5, 3, 3, 3, 1, P(2), (2, 2), 0),
    ("dw_d2x1_asym", 8, 8, 8, 6, 9, 3, 3, 1, (1, 2, 2, 1), (2, 1), 0),
    # generic
    ("gen_group2", 16, 16, 2, 7, 8, 3, 3, 1, P(2), (2, 2), 0),
    ("gen_group3", 6, 9, 3, 5, 5, 3, 3, 1, P(2), (2, 2), 1),
    ("gen_c3", 3, 8, 1, 7, 9, 3, 3, 1, P(2), (2, 2), 0),
    ("gen_k3", 16, 3, 1, 8, 8, 3, 3, 1, P(3), (3, 3), 0),                       # few output channels: a class head
    ("gen_k7x3_mixed", 6, 4, 2, 10, 9, 7, 3, (2, 1), (1, 1, 3, 2), (2, 3), 1),
    ("gen_c24_not_16", 24, 64, 1, 6, 8, 3, 3, 1, P(2), (2, 2), 0),              # group 1, C % 16 != 0: not the MFMA route
    ("gen_k32_few_rows", 16, 32, 1, 6, 8, 3, 3, 1, P(2), (2, 2), 0),            # fewer than 48 output channels
    ("gen_dw_k5", 8, 8, 8, 7, 7, 5, 5, 1, P(4), (2, 2), 0),                     # depthwise, but not 3x3
    ("gen_dw_multiplier", 8, 16, 8, 6, 6, 3, 3, 1, P(2), (2, 2), 0),            # group == C, K == 2 C
    ("gen_dw_s2x1", 8, 8, 8, 7, 7, 3, 3, (2, 1), P(2), (2, 2), 0),              # depthwise with unequal strides
]
EPILOGUES = [(0, 0), (1, 0), (0, 1), (1, 1)]  # (bias_term, activation)
BATCHES = (1, 3)


def strides(s):
    return s if isinstance(s, tuple) else (s, s)


def out_dims(case):
    _, c, k, group, h, w, kh, kw, stride, (pl, pr, pt, pb), (dh, dw_), _ = case
    sh, sw = strides(stride)
    return (h + pt + pb - (dh * (kh - 1) + 1)) // sh + 1, (w + pl + pr - (dw_ * (kw - 1) + 1)) // sw + 1


def instance(case) -> str:
    """The forward instantiation fhip_atrous_forward launches for a case."""
    _, c, k, group, h, w, kh, kw, stride, (pl, pr, pt, pb), _, _ = case
    sh, sw = strides(stride)
    ho, wo = out_dims(case)
    row4 = sw == 1 and wo % 4 == 0 and w >= 4
    if group == c and c > 1 and k == c and (kh, kw) == (3, 3) and sh == sw and sh in (1, 2):
        return dw(sh, row4 if sh == 1 else wo % 4 == 0)
    if group != 1 or c % 16 or k < 48:
        return GENERIC
    shape, bn = (BIG, 64) if k >= 96 else (SMALLM, 128)
    skip = kh * kw <= 16 and (pt // sh) * wo >= bn
    return mfma(shape, False, skip)


def packer(case) -> str:
    inst = instance(case)
    return PACK_GENERIC if inst == GENERIC else PACK_COPY if "dw3x3" in inst else PACK_MFMA


def sweep_routes(case) -> list:
    """The routes the sweep runs a case on: the selected one, and the ROW4 and tap-skipping variants of it on the same tile that accept the
    case (they are launched by name only)."""
    inst = instance(case)
    if "AtrousGemmPolicy" not in inst:
        return [inst]
    shape = BIG if BIG in inst else SMALLM
    return [inst] + [r for r in accepted_routes(case) if shape in r and r != inst]


def targets() -> set:
    return {r for c in CASES for r in sweep_routes(c)} | {packer(c) for c in CASES}


def accepted_routes(case) -> list:
    """Every route name fhip_atrous_forward_route accepts for a case (restating accepts() of atrous.hip)."""
    _, c, k, group, h, w, kh, kw, stride, _, _, _ = case
    sh, sw = strides(stride)
    ho, wo = out_dims(case)
    row4 = sw == 1 and wo % 4 == 0 and w >= 4
    routes = [GENERIC]
    if group == c and k == c and (kh, kw) == (3, 3) and sh == sw and sh in (1, 2):
        routes.append(dw(sh, False))
        if (row4 if sh == 1 else wo % 4 == 0):
            routes.append(dw(sh, True))
    if group == 1 and c % 16 == 0:
        for shape in (BIG, SMALLM):
            for r4 in ((False, True) if row4 else (False,)):
                for skip in ((False, True) if kh * kw <= 16 else (False,)):
                    routes.append(mfma(shape, r4, skip))
    return routes
