"""The tables of the 3-D layer tests (tests/test_conv3d_cpu.py, tests/test_conv3d_gpu.py, tests/test_later_contract_cpu.py): the kernel
instantiations of libfeather_conv3d.so, the cases of its entry points and the inputs of the net-level tests.

Shapes are the smallest at which the kernels can go wrong, against the tiles of feather_conv3d.h.  The matrix kernel owns 8 x 8 pixels of one
output depth and 64 or 128 output channels and walks chunks of 8 input channels per depth tap: C of 1, 3, 8, 9 and 17 (the chunk tail), K of
1, 31, 33, 64, 65 and 130 (a wave's tiles, the TILE_K switch, the last K tile), planes of 1 x 1, 7 x 9 and 9 x 17 (partial tiles, tiles across
the edge), D of 1, 2 and 5 with kd of 1 and 3, depth planes wholly in the padding with pad_value 0 and 0.5, strides 1 and 2 mixed per axis,
dilation 2 on one axis, asymmetric pads on every axis, SAME pads, batch 1 and 3, pointers 1 to 3 floats off a 16-byte boundary.  The direct
kernel takes the 3 x 7 x 7 stem, groups, depthwise, and one shape of the matrix kernel's forced onto it.  Weights are U(-1, 1) * sqrt(3 /
(Cg taps)), inputs U(-1, 1)."""
import functools
import os

import numpy as np

import conv3d_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "feathercnn_amd", "libfeather_conv3d.so")
F = np.float32
TOL = 1e-4  # max|y - ref| / max|ref|, the TOL of tests/test_net_gpu.py
U, LW = R.SAME_UPPER, R.SAME_LOWER

KERNELS = {"conv3d_mfma_kernel", "conv3d_direct_kernel", "conv3d_pack_kernel", "pool3d_kernel"}
M64, M128, DIRECT, PACK, POOL = ("fhip::conv3d_mfma_kernel<64>", "fhip::conv3d_mfma_kernel<128>", "fhip::conv3d_direct_kernel", "fhip::conv3d_pack_kernel",
                                 "fhip::pool3d_kernel")


def targets():
    """Every instantiation of the library, by the names fhip_conv3d_route reports (the pack kernel runs before every matrix-kernel case)."""
    return {M64, M128, DIRECT, PACK, POOL}


# (n, C, (D, H, W), K, kernel, stride, dilation, pads, pad_value, group, act, (a0, a1), bias, floats off a 16-byte boundary, forced direct, kernel)
CONV_CASES = [
    (1, 8, (2, 7, 9), 64, 3, 1, 1, 1, 0.0, 1, 1, (0, 0), 1, 0, 0, M64), (1, 8, (2, 7, 9), 64, 3, 1, 1, 1, 0.0, 1, 1, (0, 0), 1, 0, 1, DIRECT),
    (3, 17, (5, 9, 17), 65, 3, (1, 2, 1), 1, (1, 1, 0, 1, 1, 2), 0.5, 1, 0, (0, 0), 1, 1, 0, M128), (1, 9, (1, 1, 1), 1, 1, 1, 1, 0, 0.0, 1, 0, (0, 0), 0, 0, 0, M64),
    (1, 3, (5, 9, 9), 31, (3, 1, 1), (2, 1, 1), 1, (1, 0, 0, 0, 0, 0), 0.0, 1, 2, (0.1, 0), 1, 2, 0, M64),
    (1, 1, (2, 7, 9), 33, (1, 3, 3), (1, 1, 2), 1, (0, 0, 1, 2, 2, 0), 0.0, 1, 0, (0, 0), 1, 3, 0, M64),
    (1, 8, (5, 9, 17), 130, 3, 2, 1, 1, 0.0, 1, 1, (0, 0), 1, 0, 0, M128), (1, 9, (5, 9, 9), 64, 3, 1, (1, 2, 1), (2, 1, 2, 2, 0, 1), 0.5, 1, 0, (0, 0), 1, 0, 0, M64),
    (1, 8, (2, 9, 9), 8, 3, 2, 1, U, 0.0, 1, 0, (0, 0), 1, 0, 0, M64), (3, 3, (1, 7, 9), 70, (1, 3, 3), 1, (1, 1, 2), LW, 0.0, 1, 0, (0, 0), 0, 1, 0, M128),
    (1, 3, (2, 9, 17), 8, (3, 7, 7), (1, 2, 2), 1, (1, 1, 3, 3, 3, 3), 0.0, 1, 1, (0, 0), 1, 0, 0, DIRECT),
    (3, 8, (2, 7, 9), 6, 3, 1, 1, 1, 0.0, 2, 0, (0, 0), 1, 2, 0, DIRECT), (1, 5, (5, 7, 9), 5, 3, (1, 2, 2), 1, U, 0.25, 5, 0, (0, 0), 1, 0, 0, DIRECT),
    (1, 4, (2, 9, 9), 4, 3, 2, 2, 2, 0.0, 1, 0, (0, 0), 1, 0, 0, DIRECT),  # a patch plane of 19 x 19 cells
] + [(1, 3, (2, 7, 9), 8, (1, 3, 3), 1, 1, (0, 0, 1, 1, 1, 1), 0.0, 1, act, p, 1, 0, 0, M64) for act, p in ((3, (-0.5, 0.75)), (4, (0, 0)), (5, (0, 0)), (6, (1 / 6, 0.5)))]

# (n, C, (D, H, W), kernel, stride, pads, pad_mode, avg, count_include_pad, global, out_dhw, floats off a 16-byte boundary)
POOL_CASES = [
    (1, 3, (4, 9, 9), 2, 2, 0, 0, 0, 0, 0, None, 0), (1, 2, (5, 10, 7), 3, 2, 1, 0, 1, 0, 0, None, 1), (1, 2, (5, 10, 7), 3, 2, (1, 2, 1, 1, 0, 2), 0, 1, 1, 0, None, 2),
    (1, 2, (4, 10, 10), (1, 2, 2), (1, 2, 2), 0, 1, 0, 0, 0, None, 0), (1, 2, (5, 11, 6), (2, 4, 3), (1, 3, 2), 0, 2, 1, 1, 0, None, 3),
    (1, 2, (5, 11, 6), (2, 4, 3), (1, 3, 2), 0, 3, 0, 0, 0, None, 0), (2, 3, (3, 10, 30), 0, 1, 0, 0, 0, 0, 1, None, 0), (2, 3, (3, 10, 30), 0, 1, 0, 0, 1, 0, 1, None, 1),
    (1, 2, (5, 9, 20), 0, 1, 0, 0, 1, 0, 0, (2, 4, 7), 0), (3, 40, (2, 5, 5), 2, 1, 0, 1, 1, 0, 0, None, 0), (1, 1, (3, 7, 7), 3, 3, (2, 0, 2, 0, 2, 0), 0, 1, 0, 0, None, 0),
]


def case_id(c):
    return "-".join(str(v).replace(" ", "").replace("fhip::", "") for v in c)


@functools.lru_cache(maxsize=None)
def conv_case(case):
    """-> dict(x, w, bias, y): the inputs and the float64 result of a case, shared among the tests, which leave them unchanged.  A case and
    its twin on the other kernel draw the same inputs."""
    n, c, dhw, k, kernel, _, _, _, _, group = case[:10]
    rng = np.random.default_rng(16000 + CONV_CASES.index(case[:14] + (0, M64) if case[14] else case))  # a forced case: the matrix kernel's twin
    x = rng.uniform(-1, 1, (n, c) + dhw).astype(F)
    kern = R.three(kernel)
    w = (rng.uniform(-1, 1, (k, c // group) + kern) * np.sqrt(3.0 / (c // group * np.prod(kern)))).astype(F)
    b = rng.uniform(-0.5, 0.5, k).astype(F) if case[12] else None
    out = dict(x=x, w=w, bias=b, y=conv_float(case, x, w, b, np.float64))
    for a in out.values():
        if a is not None:
            a.setflags(write=False)
    return out


def conv_float(case, x, w, b, dtype):
    _, _, _, _, _, stride, dilation, pads, pad_value, group, act, (a0, a1) = case[:12]
    return R.conv3d(x, w, b, stride, dilation, pads, pad_value, group, act, F(a0), F(a1), dtype)


@functools.lru_cache(maxsize=None)
def pool_case(case):
    """-> (x, the result: float32 bits for the maximum, float64 for the average)."""
    n, c, dhw, kernel, stride, pads, mode, avg, include, global_, out_dhw, _ = case
    x = np.random.default_rng(16500 + POOL_CASES.index(case)).uniform(-1, 1, (n, c) + dhw).astype(F)
    y = R.pool3d(x, kernel, stride, pads, mode, bool(avg), bool(include), bool(global_), out_dhw)
    x.setflags(write=False), y.setflags(write=False)
    return x, y


# ---- net level -------------------------------------------------------------------------------------------------------------------------
# the input volume (C, D, H, W) each zoo net is tested at, and its other arguments: C3D with a narrower classifier
NETS = {"tiny_c3d": ((3, 5, 12, 14), {}), "r3d_18": ((3, 4, 32, 32), dict(classes=10)), "c3d": ((3, 16, 32, 32), dict(classes=10, fc=256))}


@functools.lru_cache(maxsize=None)
def net_model(name="tiny_c3d"):
    """-> ((param, bin, input, output), the trace for model_zoo.numpy_forward) of a zoo net at its test size."""
    from feathercnn_amd import model_zoo
    trace = []
    return getattr(model_zoo, name)(size=NETS[name][0][1:], trace=trace, **NETS[name][1]), trace


@functools.lru_cache(maxsize=None)
def net_input(name="tiny_c3d", batch=2):
    """-> (x, every blob of the numpy forward)."""
    from feathercnn_amd import model_zoo
    (p, b, i, o), trace = net_model(name)
    x = np.random.default_rng(17000 + batch).uniform(-1, 1, (batch,) + NETS[name][0]).astype(F)
    return x, model_zoo.numpy_forward(trace, i, x)
