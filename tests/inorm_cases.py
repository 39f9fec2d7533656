"""The case table of libfeather_inorm.so, shared by tests/test_inorm_cpu.py (coverage of the library's instantiations, the route report)
and tests/test_inorm_gpu.py (the sweep that runs every case).

An InstanceNorm case is (name, N, C, H, W, offset): `offset` floats past a 16-byte boundary for the input and output tensors (0:
allocator-aligned, 1: the 4-byte-aligned forms).  `instance()` restates the library's dispatch (feathercnn_amd/csrc_inorm/inorm.hip,
select_route()): a thread holds 16 floats, so a wave holds a plane of up to 1024, a 256-thread block up to 4096 and a 1024-thread block up
to 16384; the last only with at least 256 planes, everything else is split into chunks of 4096 floats (two kernels).  16-byte accesses
need H * W a multiple of 4 and aligned tensors.  An activation case is (name, N, C, HW, offset).
"""
from __future__ import annotations

import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "feathercnn_amd", "libfeather_inorm.so")
CHUNK = 4096
SPLIT_MIN_PLANES = 256

# name, N, C, H, W, offset
CASES = [
    # one wave per plane
    ("wave_vec_8x8", 3, 7, 8, 8, 0),
    ("wave_vec_32x32", 3, 5, 32, 32, 0),          # a full wave: 1024 floats
    ("wave_vec_2x2_tail_block", 1, 5, 2, 2, 0),   # five planes: the second block has one live wave
    ("wave_scalar_7x7", 3, 6, 7, 7, 0),
    ("wave_scalar_13x13", 5, 3, 13, 13, 1),
    ("wave_scalar_1x1", 3, 9, 1, 1, 0),           # a plane of one pixel: y = act(beta)
    ("wave_scalar_32x32_odd_offset", 3, 4, 32, 32, 1),
    # one 256-thread block per plane
    ("block256_vec_64x64", 3, 5, 64, 64, 0),      # the full 4096
    ("block256_vec_36x30", 5, 3, 36, 30, 0),
    ("block256_scalar_33x33", 3, 4, 33, 33, 0),
    ("block256_scalar_64x64_odd_offset", 3, 3, 64, 64, 1),
    # one 1024-thread block per plane: at least 256 planes
    ("block1024_vec_128x128", 3, 86, 128, 128, 0),  # the full 16384
    ("block1024_vec_68x68", 3, 86, 68, 68, 0),
    ("block1024_scalar_65x65", 3, 87, 65, 65, 0),
    ("block1024_scalar_68x68_odd_offset", 5, 52, 68, 68, 1),
    # split planes: two launches
    ("split_vec_128x128_few_planes", 3, 5, 128, 128, 0),   # would fit a 1024-thread block, too few planes to fill the chip
    ("split_vec_256x256", 3, 2, 256, 256, 0),              # 16 chunks
    ("split_vec_100x130_short_last_chunk", 3, 3, 100, 130, 0),
    ("split_scalar_129x127", 3, 2, 129, 127, 0),
    ("split_scalar_256x256_odd_offset", 3, 2, 256, 256, 1),
    ("split_scalar_65x65_few_planes", 5, 7, 65, 65, 1),
]
EPILOGUES = [(None, 0.0), ("relu", 0.0), ("leaky_relu", 0.2)]

# name, N, C, HW, offset
ACT_CASES = [
    ("act_vec_64", 3, 5, 64, 0),
    ("act_vec_large", 3, 6, 48 * 1024, 0),   # more float4s than 2048 blocks of 256 threads: the grid-stride loop
    ("act_scalar_49", 3, 5, 49, 0),
    ("act_scalar_odd_offset", 5, 3, 64, 1),
    ("act_scalar_large", 3, 2, 300 * 1000 + 1, 1),
]
KINDS = ("leaky_relu", "prelu_shared", "prelu", "sigmoid", "tanh", "clip")


def vec(hw, offset) -> bool:
    return hw % 4 == 0 and offset == 0


def route(case) -> str:
    _, n, c, h, w, _ = case
    hw, planes = h * w, n * c
    if hw <= 1024:
        return "wave"
    if hw <= 4096:
        return "block256"
    if hw <= 16384 and planes >= SPLIT_MIN_PLANES:
        return "block1024"
    return "split"


def instances(case) -> list:
    """The kernel instantiations fhip_instance_norm_forward launches for a case, in order."""
    _, n, c, h, w, offset = case
    v = "true" if vec(h * w, offset) else "false"
    r = route(case)
    if r == "split":
        return [f"fhip::inorm_partial_kernel<{v}>", f"fhip::inorm_apply_kernel<{v}>"]
    return ["fhip::inorm_plane_kernel<%s, %s>" % ({"wave": "256, 64", "block256": "256, 256", "block1024": "1024, 1024"}[r], v)]


def instance(case) -> str:
    """What fhip_instance_norm_route reports: the first launch."""
    return instances(case)[0]


def scratch_bytes(case) -> int:
    _, n, c, h, w, _ = case
    return n * c * (-(-h * w // CHUNK)) * 8 if route(case) == "split" else 0


def act_instance(case) -> str:
    _, n, c, hw, offset = case
    return "fhip::activation_kernel<%s>" % ("true" if vec(hw, offset) else "false")


def targets() -> set:
    return {i for c in CASES for i in instances(c)} | {act_instance(c) for c in ACT_CASES}
