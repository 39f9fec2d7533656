"""The tables of the 1-D layer tests (tests/test_conv1d_cpu.py, tests/test_conv1d_gpu.py, tests/test_later_contract_cpu.py): the kernel
instantiations of libfeather_conv1d.so, the cases of its entry points and the inputs of the net-level test.

Shapes are the smallest at which the kernels can go wrong, against the tiles of feather_conv1d.h.  The matrix kernel owns 64 output channels
x 64 positions and walks chunks of 16 (kw 1, 2), 8 (kw 3) or 4 (kw 31, the 96 KiB instantiation) input channels: K and Lo of 63, 64, 65, 70
and 128, C one past a chunk (17, 9, 5), strides 1, 2, 3 (the phase-split slab, with dilations that are and are not multiples of the stride),
dilations 1, 2, 5.  The direct kernel takes one or two channels a group, a filter whose slab passes the budget (kw 200) and a depthwise
stride whose segment passes its LDS (9); more than one block of 256 positions.  The depthwise kernel owns 1024 outputs: Lo 1024 and 1030,
taps 1, 2, 4, 5, 31 on the 16-byte path and strided / dilated ones off it.  Weights are U(-1, 1) * sqrt(3 / (Cg kw)), inputs U(-1, 1)."""
import functools
import os

import numpy as np

import conv1d_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "feathercnn_amd", "libfeather_conv1d.so")
F = np.float32
TOL = 1e-4  # max|y - ref| / max|ref|, the bound of tests/test_atrous_gpu.py
U, LW = R.SAME_UPPER, R.SAME_LOWER

KERNELS = {"conv1d_mfma_kernel", "conv1d_direct_kernel", "conv1d_depthwise_kernel", "pool1d_kernel"}
SMALL, LARGE, DIRECT, DW, POOL = ("fhip::conv1d_mfma_kernel<8192>", "fhip::conv1d_mfma_kernel<24576>", "fhip::conv1d_direct_kernel", "fhip::conv1d_depthwise_kernel",
                                  "fhip::pool1d_kernel")


def targets():
    """Every instantiation of the library, by the names fhip_conv1d_route reports."""
    return {SMALL, LARGE, DIRECT, DW, POOL}


# (n, C, L, K, kw, s, d, pl, pr, pad_value, group, act, (a0, a1), bias, row slack of x and y, floats off a 16-byte boundary, kernel)
CONV_CASES = [
    (1, 16, 70, 64, 3, 1, 1, 1, 1, 0.0, 1, 1, (0, 0), 1, 0, 0, SMALL), (3, 17, 63, 63, 1, 1, 1, 0, 0, 0.0, 1, 0, (0, 0), 1, 3, 1, SMALL),
    (1, 9, 66, 65, 3, 1, 2, 2, 1, 0.5, 1, 2, (0.1, 0), 1, 1, 2, SMALL), (1, 8, 131, 32, 2, 2, 1, 0, 0, 0.0, 1, 3, (-0.5, 0.75), 0, 0, 3, SMALL),
    (1, 6, 200, 8, 3, 3, 5, U, 0, 0.0, 1, 4, (0, 0), 1, 5, 0, SMALL), (1, 4, 50, 10, 3, 2, 2, LW, 0, 0.0, 1, 5, (0, 0), 1, 0, 1, SMALL),
    (1, 5, 40, 7, 31, 1, 1, 15, 15, 0.0, 1, 6, (1 / 6, 0.5), 1, 2, 0, LARGE), (3, 8, 30, 12, 3, 1, 1, 1, 1, 0.0, 2, 0, (0, 0), 1, 0, 0, SMALL),
    (1, 3, 100, 5, 3, 3, 2, 0, 2, -1.0, 1, 0, (0, 0), 1, 0, 0, SMALL), (1, 4, 64, 128, 1, 1, 1, 0, 0, 0.0, 1, 1, (0, 0), 0, 0, 0, SMALL),
    (1, 1, 300, 5, 3, 1, 1, 1, 1, 0.0, 1, 1, (0, 0), 1, 0, 1, DIRECT), (1, 2, 50, 4, 2, 2, 1, 1, 0, -1.0, 1, 0, (0, 0), 1, 3, 0, DIRECT),
    (3, 4, 33, 6, 3, 1, 2, U, 0, 0.0, 2, 2, (0.2, 0), 1, 0, 2, DIRECT), (1, 4, 260, 3, 200, 1, 1, 100, 99, 0.0, 1, 0, (0, 0), 0, 0, 0, DIRECT),
    (1, 3, 40, 3, 3, 9, 1, 1, 1, 0.0, 3, 0, (0, 0), 1, 0, 0, DIRECT),
    (1, 8, 1030, 8, 31, 1, 1, U, 0, 0.0, 8, 1, (0, 0), 1, 0, 1, DW), (3, 3, 37, 3, 1, 1, 1, 0, 0, 0.0, 3, 0, (0, 0), 0, 2, 0, DW),
    (1, 4, 50, 4, 2, 2, 1, 1, 0, 0.25, 4, 0, (0, 0), 1, 0, 3, DW), (1, 5, 80, 5, 3, 3, 5, LW, 0, 0.0, 5, 2, (0.1, 0), 1, 1, 0, DW),
    (1, 2, 1027, 2, 4, 1, 1, 0, 0, 0.0, 2, 0, (0, 0), 1, 0, 0, DW), (1, 2, 40, 2, 5, 1, 1, 3, 1, 2.0, 2, 6, (0.2, 0.5), 1, 0, 2, DW),
]

# (n, C, L, kw, s, pl, pr, pad_mode, avg, count_include_pad, global, out_w, row slack, floats off a 16-byte boundary)
POOL_CASES = [
    (1, 3, 9, 2, 2, 0, 0, 0, 0, 0, 0, None, 0, 0), (1, 2, 10, 3, 2, 1, 1, 0, 1, 0, 0, None, 1, 1), (1, 2, 10, 3, 2, 1, 2, 0, 1, 1, 0, None, 0, 2),
    (1, 2, 10, 3, 2, 0, 0, 1, 0, 0, 0, None, 0, 0), (1, 2, 11, 4, 3, 0, 0, 2, 1, 1, 0, None, 0, 3), (1, 2, 11, 4, 3, 0, 0, 3, 0, 0, 0, None, 2, 0),
    (2, 3, 300, 0, 1, 0, 0, 0, 0, 0, 1, None, 0, 0), (2, 3, 300, 0, 1, 0, 0, 0, 1, 0, 1, None, 0, 1), (1, 2, 20, 0, 1, 0, 0, 0, 1, 0, 0, 7, 0, 0),
    (1, 2, 10, 0, 1, 0, 0, 0, 0, 0, 0, 3, 1, 0), (3, 40, 50, 2, 1, 0, 0, 1, 1, 0, 0, None, 0, 0), (1, 1, 7, 3, 3, 2, 0, 0, 1, 0, 0, None, 0, 0),
]


def case_id(c):
    return "-".join(str(v).replace(" ", "").replace("fhip::", "") for v in c)


@functools.lru_cache(maxsize=None)
def conv_case(case):
    """-> dict(x, w, bias, y): the inputs and the float64 result of a case, shared among the tests, which leave them unchanged."""
    n, c, l, k, kw, s, d, pl, pr, pad_value, group, act, (a0, a1), bias, _, _, _ = case
    rng = np.random.default_rng(13000 + CONV_CASES.index(case))
    x = rng.uniform(-1, 1, (n, c, l)).astype(F)
    w = (rng.uniform(-1, 1, (k, c // group, kw)) * np.sqrt(3.0 / (c // group * kw))).astype(F)
    b = rng.uniform(-0.5, 0.5, k).astype(F) if bias else None
    out = dict(x=x, w=w, bias=b, y=conv_float(case, x, w, b, np.float64))
    for a in out.values():
        if a is not None:
            a.setflags(write=False)
    return out


def conv_float(case, x, w, b, dtype):
    _, _, _, _, _, s, d, pl, pr, pad_value, group, act, (a0, a1), _, _, _, _ = case
    return R.conv1d(x.astype(dtype), w, b, s, d, pl, pr, pad_value, group, act, F(a0), F(a1), dtype)


@functools.lru_cache(maxsize=None)
def pool_case(case):
    """-> (x, the result in float32: the kernel's very bits)."""
    n, c, l, kw, s, pl, pr, mode, avg, include, global_, out_w, _, _ = case
    x = np.random.default_rng(13500 + POOL_CASES.index(case)).uniform(-1, 1, (n, c, l)).astype(F)
    y = R.pool1d(x, kw, s, pl, pr, mode, bool(avg), bool(include), bool(global_), out_w)
    x.setflags(write=False), y.setflags(write=False)
    return x, y


# ---- net level -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def net_model(length=40):
    """-> ((param, bin, input, output), the trace for model_zoo.numpy_forward) of tiny_tcn at a length: the same weights at every length."""
    from feathercnn_amd import model_zoo
    trace = []
    return model_zoo.tiny_tcn(size=(5, length), trace=trace), trace


@functools.lru_cache(maxsize=None)
def net_input(batch=3, length=40):
    """-> (x, every blob of the numpy forward)."""
    from feathercnn_amd import model_zoo
    (p, b, i, o), trace = net_model(length)
    x = np.random.default_rng(14000 + batch + 3 * length).uniform(-1, 1, (batch, 1, 5, length)).astype(F)
    return x, model_zoo.numpy_forward(trace, i, x)


def net_shapes(length=40, classes=7):
    """Every blob of tiny_tcn: name -> (c, h, w); all but the Input are of rank 2 (c == 1)."""
    t = length // 2
    return {"data": (1, 5, length), "c1": (1, 8, t), "c2": (1, 8, t), "dw": (1, 8, t), "pw": (1, 12, t), "pool": (1, 12, t // 2), "to_tokens": (1, t // 2, 12),
            "gru": (1, t // 2, 6), "classes": (1, t // 2, classes)}
