"""The case table of tests/test_shuffle_cpu.py and tests/test_shuffle_gpu.py: shapes, groups, slices and tables that together reach every
kernel instantiation of libfeather_shuffle.so -- channel_map_kernel<KIND, VEC>, KIND 0 table / 1 shuffle / 2 slice, VEC 16-byte / 4-byte."""
from __future__ import annotations

import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "feathercnn_amd", "libfeather_shuffle.so")

PLANES = [(1, 1), (7, 7), (13, 9), (14, 14), (28, 28), (56, 56)]
BATCHES = [1, 3, 32]
OFFSETS = [0, 1, 2, 3]  # floats past a 16-byte boundary: 0, 4, 8 and 12 bytes

# (channels, group): multiples and non-multiples of 4, groups 2, 3, 4, 8
SHUFFLES = [(116, 2), (232, 2), (30, 3), (60, 3), (15, 3), (24, 4), (20, 4), (64, 8), (40, 8), (6, 2), (9, 3)]

# (channels, sizes): equal, unequal, shares, a remainder that is dropped
SLICES = [(116, [58, 58]), (32, [-233, -233]), (32, [5, -233, 14]), (30, [7, 3, 11, 9]), (21, [4, -233, -233]), (10, [3, 4]), (9, [-233, -233])]

# a table reading from three sources: (source channels, steps, outputs) for shuffle_ref.compose
THREE_SOURCES = ([5, 13, 14], [("concat", ["s0", "s1", "s2"], "cat"), ("shuffle", "cat", "sh", 4, True), ("slice", "sh", ["a", "b", "c"], [9, -233, 12])],
                 ["a", "b", "c"])
# ShuffleNet v2's unit boundary: Concat(a, b) -> ShuffleChannel(2) -> Slice(2)
V2_BOUNDARY = lambda half: ([half, half], [("concat", ["s0", "s1"], "cat"), ("shuffle", "cat", "sh", 2, False),  # noqa: E731
                                           ("slice", "sh", ["keep", "work"], [-233, -233])], ["keep", "work"])


def vec(h, w, offsets) -> bool:
    return (h * w) % 4 == 0 and not any(offsets)


def instance(kind: int, h: int, w: int, offsets) -> str:
    return f"fhip::channel_map_kernel<{kind}, {'true' if vec(h, w, offsets) else 'false'}>"


def targets() -> set:
    return {f"fhip::channel_map_kernel<{k}, {v}>" for k in (0, 1, 2) for v in ("true", "false")}
