"""The shape table of libfeather_gate.so (squeeze-and-excitation channel gating), shared by tests/test_gate_cpu.py and
tests/test_gate_gpu.py."""
from __future__ import annotations

import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "feathercnn_amd", "libfeather_gate.so")

# apply: every plane with every channel count at every batch
APPLY_PLANES = [(1, 1), (3, 3), (7, 7), (14, 14), (5, 12), (56, 56)]
APPLY_CHANNELS = [1, 3, 24, 72]
APPLY_BATCHES = [1, 3, 32]
OFFSETS = [0, 1, 2, 3]  # floats past a 16-byte boundary

# squeeze: (h, w); the planes above 16384 floats take the split route (132 x 132 = 17424 floats, a multiple of 4; 129 x 129 = 16641, not one);
# 72 x 72 = 5184 floats is the one-block-per-plane route
SQUEEZE_PLANES = [(1, 1), (7, 7), (14, 14), (56, 56), (72, 72), (132, 132), (129, 129)]
SPLIT_CHUNK = 16384
GROUP_MAX_HW = 4096

# excite: (C, R); R = 1030 takes the kernel's second tile of hidden values (1024 a tile), with a short last tile
EXCITE = [(16, 4), (24, 6), (72, 18), (960, 240), (2048, 128), (3, 1), (8, 1030)]
EXCITE_BATCHES = [1, 3, 32]

KERNELS = {"gate_apply_kernel", "squeeze_group_kernel", "squeeze_block_kernel", "squeeze_merge_kernel", "excite_kernel", "gate_activation_kernel"}


def targets():
    """Every kernel instantiation the library holds, as tests/kernel_instances.py names them."""
    t = {f"fhip::{k}<{v}>" for k in ("gate_apply_kernel", "squeeze_group_kernel", "squeeze_block_kernel", "gate_activation_kernel") for v in ("true", "false")}
    return t | {"fhip::squeeze_merge_kernel", "fhip::excite_kernel"}


def squeeze_route(h, w, aligned=True):
    hw = h * w
    v = "true" if hw % 4 == 0 and aligned else "false"
    return f"fhip::squeeze_{'group' if hw <= GROUP_MAX_HW else 'block'}_kernel<{v}>"
