"""The tables of the deformable-convolution tests (tests/test_dcn_cpu.py, tests/test_dcn_gpu.py, tests/test_later_contract_cpu.py): the
kernel instantiations of libfeather_dcn.so, the cases of its forward call and the inputs of the net-level test.

Shapes are the smallest at which the kernel can go wrong, against the tile of feather_dcn.h: a block owns 64 flattened output pixels and 64
or 128 output channels and walks chunks of 16 input channels.  Ho * Wo of 63, 64, 65 and 130 (9x7 and 7x9, 8x8, 5x13, 10x13: tiles that
span rows, a pixel tail, two pixel tiles), K of 63, 64, 65, 128 and 130 (both instantiations, a K tail, two K tiles), C of 1, 3, 16, 17 and
33 (a chunk, its tail, three chunks), taps 1x1, 3x3, 1x3 and 3x1, unequal strides, dilation, seven sets of pads, 1, 2 and 4 offset groups.
Weights are U(-1, 1) * sqrt(3 / (C kh kw)), inputs U(-1, 1), masks U(0, 1); offsets are U(-3, 3) on planes of 5 to 13 pixels, so a good share
of the samples crosses the border or falls wholly outside."""
import functools
import os

import numpy as np

import dcn_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "feathercnn_amd", "libfeather_dcn.so")
F = np.float32
TOL = 1e-4  # max|y - ref| / max|ref|, the project's bound for convolutions

KERNELS = {"dcn_mfma_kernel", "dcn_pack_kernel"}
SMALL, LARGE, PACK = "fhip::dcn_mfma_kernel<64>", "fhip::dcn_mfma_kernel<128>", "fhip::dcn_pack_kernel"


def targets():
    """Every instantiation of the library: the two fhip_dcn_route reports, and the packer."""
    return {SMALL, LARGE, PACK}


# (n, C, H, W, K, (kh, kw), stride, dilation, (top, bottom, left, right), G, mask, act, (a0, a1), bias, floats off a 16-byte boundary, (Ho, Wo), kernel)
CASES = [
    (1, 16, 8, 8, 64, (3, 3), (1, 1), (1, 1), (1, 1, 1, 1), 1, 1, 1, (0, 0), 1, 1, (8, 8), SMALL),
    (3, 17, 7, 9, 63, (1, 1), (1, 1), (1, 1), (0, 0, 0, 0), 1, 0, 0, (0, 0), 1, 2, (7, 9), SMALL),
    (1, 33, 5, 13, 65, (3, 3), (1, 1), (2, 2), (2, 2, 2, 2), 1, 1, 2, (0.1, 0), 1, 3, (5, 13), LARGE),
    (1, 3, 10, 13, 128, (1, 3), (1, 1), (1, 1), (0, 0, 1, 1), 1, 0, 3, (-0.5, 0.75), 0, 1, (10, 13), LARGE),
    (1, 1, 10, 13, 130, (3, 1), (2, 1), (1, 1), (1, 0, 0, 0), 1, 1, 4, (0, 0), 1, 2, (5, 13), LARGE),
    (3, 16, 9, 13, 64, (3, 3), (1, 2), (1, 1), (2, 0, 1, 1), 4, 1, 5, (0, 0), 1, 3, (9, 7), SMALL),
    (1, 16, 8, 8, 64, (3, 3), (1, 1), (1, 2), (1, 1, 2, 2), 2, 0, 6, (1 / 6, 0.5), 1, 1, (8, 8), SMALL),
    (1, 17, 10, 13, 130, (3, 3), (1, 1), (1, 1), (1, 1, 1, 1), 1, 1, 1, (0, 0), 0, 2, (10, 13), LARGE),
]


def case_id(c):
    return "-".join(str(v).replace(" ", "").replace("fhip::", "") for v in c)


@functools.lru_cache(maxsize=None)
def case(c):
    """-> dict(x, offset, mask, w, bias, y): the inputs and the float64 result of a case, shared among the tests, which leave them unchanged."""
    n, ch, h, w, k, (kh, kw), _, _, _, g, mask, _, _, bias, _, (ho, wo), _ = c
    rng = np.random.default_rng(16000 + CASES.index(c))
    out = dict(x=rng.uniform(-1, 1, (n, ch, h, w)).astype(F), offset=rng.uniform(-3, 3, (n, g * 2 * kh * kw, ho, wo)).astype(F),
               mask=rng.uniform(0, 1, (n, g * kh * kw, ho, wo)).astype(F) if mask else None,
               w=(rng.uniform(-1, 1, (k, ch, kh, kw)) * np.sqrt(3.0 / (ch * kh * kw))).astype(F), bias=rng.uniform(-0.5, 0.5, k).astype(F) if bias else None)
    out["y"] = in_float(c, out, np.float64)
    for a in out.values():
        if a is not None:
            a.setflags(write=False)
    return out


def in_float(c, t, dtype):
    _, _, _, _, _, _, stride, dilation, pads, g, _, act, (a0, a1), _, _, _, _ = c
    return R.deform_conv2d(t["x"], t["offset"], t["mask"], t["w"], t["bias"], stride, dilation, pads, g, act, F(a0), F(a1), dtype)


# ---- net level -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def net_model(size=(10, 12)):
    """-> ((param, bin, input, output), the trace for model_zoo.numpy_forward) of tiny_dcn at a size: the same weights at every size."""
    from feathercnn_amd import model_zoo
    trace = []
    return model_zoo.tiny_dcn(size=size, trace=trace), trace


@functools.lru_cache(maxsize=None)
def net_input(batch=3, size=(10, 12)):
    """-> (x, every blob of the numpy forward)."""
    from feathercnn_amd import model_zoo
    (p, b, i, o), trace = net_model(size)
    x = np.random.default_rng(17000 + batch + 3 * size[0]).uniform(-1, 1, (batch, 3) + size).astype(F)
    return x, model_zoo.numpy_forward(trace, i, x)
