"""The case table of the grouped-convolution route (libfeather_gconv.so), shared by tests/test_gconv_cpu.py (coverage of the library's
instantiations) and tests/test_gconv_gpu.py (the sweep that runs every case).

A case is (name, C, K, group, H, W, kh, kw, stride, pads (left, right, top, bottom), offset): `offset` floats past a 16-byte boundary for
the input and output tensors (0: allocator-aligned, 1: the 4-byte-aligned forms).  `instance()` restates the library's dispatch
(feathercnn_amd/csrc_gconv/gconv.hip, plan_of() and select()): the register-tiled 3x3 kernel for stride 1 / 2, pad 1 and 4 / 8 / 16 / 32
channels per group on both sides, KT = min(K/group, 16) output channels per lane, float4 rows when the input width is a multiple of
4 * stride and both tensors are 16-byte aligned; the generic kernel for everything else.  Every case also launches the weight packer.
"""
from __future__ import annotations

import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "feathercnn_amd", "libfeather_gconv.so")
PACK = "fhip::gconv_pack_kernel"
GENERIC = "fhip::gconv_generic_kernel<4>"

P1 = (1, 1, 1, 1)
P0 = (0, 0, 0, 0)

# name, C, K, group, H, W, kh, kw, stride, pads, offset
CASES = [
    # tuned 3x3, every (KT, stride, VEC) instantiation; VEC needs W % (4 * stride) == 0 and offset 0
    ("k4_s1_vec", 16, 16, 4, 12, 16, 3, 3, 1, P1, 0),
    ("k4_s1_ragged", 16, 16, 4, 9, 13, 3, 3, 1, P1, 0),
    ("k4_s2_vec", 8, 8, 2, 10, 16, 3, 3, 2, P1, 0),
    ("k4_s2_ragged", 32, 8, 2, 11, 14, 3, 3, 2, P1, 0),        # C/g 16 into K/g 4
    ("k8_s1_vec", 16, 16, 2, 7, 8, 3, 3, 1, P1, 0),
    ("k8_s1_misaligned", 16, 16, 2, 7, 8, 3, 3, 1, P1, 1),      # a width that allows float4 at an address that does not
    ("k8_s2_vec", 12, 24, 3, 9, 24, 3, 3, 2, P1, 0),            # C/g 4 into K/g 8, three groups
    ("k8_s2_ragged", 16, 16, 2, 13, 7, 3, 3, 2, P1, 0),
    ("k16_s1_vec", 32, 32, 2, 6, 20, 3, 3, 1, P1, 0),
    ("k16_s1_ragged", 32, 32, 2, 5, 7, 3, 3, 1, P1, 0),
    ("k16_s2_vec", 32, 32, 2, 14, 8, 3, 3, 2, P1, 0),
    ("k16_s2_ragged", 64, 64, 2, 7, 7, 3, 3, 2, P1, 1),         # K/g 32: two chunks of 16 per group
    ("k32_s1_vec_two_chunks", 64, 64, 2, 8, 12, 3, 3, 1, P1, 0),
    ("resnext_128_g32", 128, 128, 32, 14, 28, 3, 3, 1, P1, 0),  # ResNeXt-50's first grouped shape on a small plane
    # generic: everything the tuned kernel does not take
    ("gen_1x1", 32, 24, 4, 9, 10, 1, 1, 1, P0, 0),              # ShuffleNet's grouped 1x1, K/g = 6
    ("gen_1x1_s2", 12, 18, 3, 9, 9, 1, 1, 2, P0, 1),
    ("gen_5x5", 10, 15, 5, 11, 12, 5, 5, 1, (2, 2, 2, 2), 0),   # C/g 2, K/g 3
    ("gen_3x3_odd_cg", 9, 6, 3, 10, 11, 3, 3, 1, P1, 0),        # 3x3 / pad 1 but C/g = 3
    ("gen_3x3_asym_pad", 16, 16, 4, 9, 12, 3, 3, 1, (0, 1, 1, 0), 0),
    ("gen_3x3_s2_asym_pad", 8, 8, 2, 10, 11, 3, 3, 2, (0, 1, 0, 1), 0),
    ("gen_3x3_nopad", 16, 16, 4, 8, 8, 3, 3, 1, P0, 0),
    ("gen_7x3_s3x1", 6, 4, 2, 15, 9, 7, 3, (3, 1), (1, 1, 3, 3), 0),  # rectangular kernel, different strides
    ("gen_alexnet_g2", 6, 10, 2, 13, 13, 5, 5, 1, (2, 2, 2, 2), 1),   # AlexNet's group 2
]
EPILOGUES = [(0, 0), (1, 0), (0, 1), (1, 1)]  # (bias_term, activation)
BATCHES = (1, 3)


def strides(s):
    return s if isinstance(s, tuple) else (s, s)


def plan(c, k, group, kh, kw, stride, pads):
    """(tuned, KT) as gconv.hip's plan_of()."""
    sh, sw = strides(stride)
    cg, kg = c // group, k // group
    tuned = (kh, kw) == (3, 3) and sh == sw and sh in (1, 2) and tuple(pads) == P1 and cg in (4, 8, 16, 32) and kg in (4, 8, 16, 32)
    return tuned, (min(kg, 16) if tuned else 4)


def packed_floats(c, k, group, kh, kw, stride, pads) -> int:
    tuned, kt = plan(c, k, group, kh, kw, stride, pads)
    cg, kg = c // group, k // group
    return group * ((kg + kt - 1) // kt) * cg * kh * kw * kt


def instance(case, in_address: int = None, out_address: int = None) -> str:
    """The forward instantiation fhip_gconv_forward launches for a case (tensor addresses default to 16-byte aligned + 4 * offset)."""
    _, c, k, group, h, w, kh, kw, stride, pads, offset = case
    tuned, kt = plan(c, k, group, kh, kw, stride, pads)
    if not tuned:
        return GENERIC
    ia = 4 * offset if in_address is None else in_address
    oa = 4 * offset if out_address is None else out_address
    s = strides(stride)[0]
    vec = w % (4 * s) == 0 and ia % 16 == 0 and oa % 16 == 0
    return f"fhip::gconv3x3_kernel<{kt}, {s}, {'true' if vec else 'false'}>"


def targets() -> set:
    return {instance(c) for c in CASES} | {PACK}


def out_dims(case):
    _, c, k, group, h, w, kh, kw, stride, (pl, pr, pt, pb), _ = case
    sh, sw = strides(stride)
    return (h + pt + pb - kh) // sh + 1, (w + pl + pr - kw) // sw + 1
