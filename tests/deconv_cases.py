"""The case table of the transposed-convolution route (libfeather_deconv.so), shared by tests/test_deconv_cpu.py (the definition against
torch, coverage of the library's instantiations) and tests/test_deconv_gpu.py (the sweep that runs every case).

A case is (name, C, K, group, H, W, kh, kw, stride, pads (left, right, top, bottom), out_pads (right, bottom), offset): `offset` floats past
a 16-byte boundary for the input and output tensors (0: allocator-aligned, 1: the 4-byte-aligned forms).  `instance()` restates the
library's dispatch (feathercnn_amd/csrc_deconv/deconv.hip, select()): the fp32-MFMA phase GEMM for group 1 with C a multiple of 16 and at
most 16 phases, where the GEMM has at least 48 rows -- rows = K, or 2 * round_up(K, 8) when stride_w == 2 stacks the two x-phases (PAIR);
the 128-row tile from 96 rows on, else the 64-row tile -- and the generic kernel for everything else.  Every case also launches one of
the weight packers.
"""
from __future__ import annotations

import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "feathercnn_amd", "libfeather_deconv.so")
GENERIC = "fhip::deconv_generic_kernel<4>"
PACK_GENERIC = "fhip::deconv_pack_generic_kernel"
BIG, SMALLM = "fhip::GemmShape<128, 64, 16, 2, 2, 4>", "fhip::GemmShape<64, 128, 16, 1, 4, 4>"


def mfma(shape, pair):
    return f"fhip::gemm_mfma_kernel<{shape}, fhip::DeconvGemmPolicy<{'true' if pair else 'false'}> >"


P0, P1, P2 = (0, 0, 0, 0), (1, 1, 1, 1), (2, 2, 2, 2)
N0 = (0, 0)

# name, C, K, group, H, W, kh, kw, stride, pads, out_pads, offset
CASES = [
    # MFMA, x-phases paired (stride_w == 2), 128-row tile
    ("pair_big_k4s2p1", 32, 64, 1, 8, 8, 4, 4, 2, P1, N0, 0),          # the pix2pix / U-Net up-sampling layer
    ("pair_big_k4s2p1_odd", 16, 72, 1, 5, 7, 4, 4, 2, P1, N0, 1),      # K not a multiple of the tile, odd plane, misaligned tensors
    ("pair_big_k2s2", 32, 48, 1, 6, 9, 2, 2, 2, P0, N0, 0),            # one tap per phase: a pure 1x1 GEMM per phase
    ("pair_big_k3s2p1_op1", 16, 64, 1, 7, 6, 3, 3, 2, P1, (1, 1), 0),  # phases of 4 and 2 taps; style transfer's up-sampling layer
    ("pair_big_k3s2_asym", 16, 50, 1, 6, 5, 3, 3, 2, (0, 1, 1, 0), N0, 1),
    ("pair_big_k5x3_s3x2", 16, 48, 1, 5, 6, 5, 3, (3, 2), (2, 1, 1, 2), (0, 1), 0),  # stride_h 3: three y-phases of different depth
    ("pair_big_k1s2", 16, 48, 1, 4, 5, 1, 1, 2, P0, N0, 0),            # a kernel smaller than the stride: phases without a tap give act(bias)
    ("pair_big_pad3", 16, 48, 1, 6, 6, 4, 4, 2, (3, 3, 3, 3), N0, 0),   # pad >= stride: the first phase rows / columns are cropped away
    # MFMA, paired, 64-row tile
    ("pair_small_k4s2p1", 16, 32, 1, 9, 10, 4, 4, 2, P1, N0, 0),
    ("pair_small_k3s2_op", 32, 24, 1, 5, 8, 3, 3, 2, P1, (1, 0), 1),
    ("pair_small_k2s2", 16, 40, 1, 7, 7, 2, 2, 2, P0, N0, 0),
    # MFMA, one phase per block (stride_w != 2), 128-row and 64-row tiles
    ("phase_big_k3s1p1", 16, 96, 1, 7, 9, 3, 3, 1, P1, N0, 0),         # stride 1: a convolution with the kernel read backwards
    ("phase_big_k5s3", 16, 100, 1, 4, 5, 5, 5, 3, P2, (1, 1), 1),
    ("phase_big_k8s4p2", 16, 128, 1, 3, 4, 8, 8, 4, P2, N0, 0),        # 16 phases
    ("phase_small_k3s1", 32, 64, 1, 6, 6, 3, 3, 1, P0, N0, 0),
    ("phase_small_k4x3_s2x3", 16, 50, 1, 5, 4, 4, 3, (2, 3), (1, 1, 1, 1), N0, 1),
    # generic: everything else
    ("gen_rgb_head_k4s2p1", 16, 3, 1, 8, 8, 4, 4, 2, P1, N0, 0),       # few output channels
    ("gen_c3_k4s2p1", 3, 8, 1, 7, 9, 4, 4, 2, P1, N0, 1),              # C not a multiple of 16
    ("gen_group2_k4s2p1", 8, 12, 2, 6, 7, 4, 4, 2, P1, N0, 0),
    ("gen_group3_k3s2_op", 6, 9, 3, 5, 5, 3, 3, 2, P1, (1, 1), 1),
    ("gen_depthwise_bilinear", 21, 21, 21, 8, 9, 4, 4, 2, P1, N0, 0),  # FCN's bilinear up-sampling
    ("gen_depthwise_k16s8", 5, 5, 5, 3, 3, 16, 16, 8, (4, 4, 4, 4), N0, 0),
    ("gen_k2s2", 12, 20, 1, 9, 6, 2, 2, 2, P0, N0, 0),
    ("gen_k3s1p1", 10, 7, 1, 6, 7, 3, 3, 1, P1, N0, 1),
    ("gen_k5s5_32phases", 16, 64, 1, 3, 3, 5, 5, 5, P0, N0, 0),        # 25 phases: more than the MFMA route takes
    ("gen_k7x3_s3x1_asym", 6, 4, 2, 5, 9, 7, 3, (3, 1), (1, 1, 3, 2), (0, 2), 0),
]
EPILOGUES = [(0, 0), (1, 0), (0, 1), (1, 1)]  # (bias_term, activation)
BATCHES = (1, 3)


def strides(s):
    return s if isinstance(s, tuple) else (s, s)


def instance(case) -> str:
    """The forward instantiation fhip_deconv_forward launches for a case."""
    _, c, k, group, h, w, kh, kw, stride, pads, out_pads, offset = case
    sh, sw = strides(stride)
    if group != 1 or c % 16 or sh * sw > 16:
        return GENERIC
    pair = sw == 2
    rows = 2 * ((k + 7) // 8 * 8) if pair else k
    if rows < 48:
        return GENERIC
    return mfma(BIG if rows >= 96 else SMALLM, pair)


def packer(case) -> str:
    inst = instance(case)
    if inst == GENERIC:
        return PACK_GENERIC
    return "fhip::deconv_pack_mfma_kernel<%s>" % ("true" if "<true>" in inst else "false")


def targets() -> set:
    return {instance(c) for c in CASES} | {packer(c) for c in CASES}


def out_dims(case):
    _, c, k, group, h, w, kh, kw, stride, (pl, pr, pt, pb), (opr, opb), _ = case
    sh, sw = strides(stride)
    return (h - 1) * sh + kh - pt - pb + opb, (w - 1) * sw + kw - pl - pr + opr
