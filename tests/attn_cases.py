"""The tables of the transformer-layer tests (tests/test_attn_cpu.py, tests/test_attn_gpu.py, tests/test_later_contract_cpu.py): the kernel
instantiations of libfeather_attn.so, the attention, LayerNorm, GELU and binary cases and the inputs of the net-level tests.

Shapes are the smallest at which the kernels can still go wrong.  The matrix route of the attention core owns 64 queries a block (two waves
of 32) and walks the keys in tiles of 32: lengths of 1, 2, 31, 32, 33, 65 and 197 end inside a tile, on its edge and one past it, and 65 and
197 take more than one block.  A head is 1 .. 4 chunks of 32 columns wide: 4, 8 and 32 are one chunk, 64 two, 96 three, 128 four; 1, 3, 6
and 132 take the direct kernel.  LayerNorm takes a wave per row up to 256 floats and a block per row above."""
import functools
import os

import numpy as np

import attn_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "feathercnn_amd", "libfeather_attn.so")
F = np.float32
ATTENTION, LAYER_NORM, GELU, BINARY = range(4)  # fhip_attn_op
SCALAR, TENSOR, BROADCAST = range(3)

KERNELS = {"attention_mfma_kernel", "attention_direct_kernel", "layer_norm_kernel", "gelu_kernel", "binary_kernel"}


def targets():
    """Every instantiation of the library, by the names fhip_attn_route reports."""
    return ({"fhip::attention_mfma_kernel<%d>" % dc for dc in (1, 2, 3, 4)} | {"fhip::attention_direct_kernel"} |
            {"fhip::layer_norm_kernel<%d, %d>" % (b, a) for b in (0, 1) for a in (0, 1)} | {"fhip::gelu_kernel<%d, %d>" % (f, v) for f in (0, 1) for v in (0, 1)} |
            {"fhip::binary_kernel<%d, %d>" % (f, v) for f in (0, 1, 2) for v in (0, 1)})


# (tq, tk, d, heads, n, layout, offset, kind).  layout: "dense" three tensors; "fused" one [n * T][3E] buffer (tq == tk); "kv" q dense, k and v one
# [n * tk][2E] buffer.  offset: floats past a 16-byte boundary, every buffer.  kind: "plain"; "pm80" the scores scaled to reach +-80;
# "equal" the first query of the first image is zero, so its scores are all equal
ATTENTION_CASES = [
    # the matrix route: every length against every other at d = 32, one chunk
    (1, 1, 32, 1, 1, "dense", 0, "plain"), (2, 197, 32, 1, 1, "dense", 1, "plain"), (31, 2, 32, 3, 1, "kv", 2, "plain"), (32, 32, 32, 1, 3, "fused", 3, "plain"),
    (33, 65, 32, 3, 3, "kv", 0, "plain"), (65, 33, 32, 1, 1, "dense", 0, "plain"), (197, 31, 32, 1, 1, "dense", 0, "plain"), (197, 197, 32, 3, 1, "fused", 0, "plain"),
    (1, 33, 32, 1, 3, "kv", 1, "plain"), (65, 1, 32, 3, 1, "dense", 2, "plain"),
    # every head width of it
    (33, 33, 4, 3, 3, "fused", 0, "plain"), (65, 31, 4, 1, 1, "dense", 1, "plain"), (33, 65, 8, 3, 1, "kv", 3, "plain"), (2, 2, 8, 1, 3, "fused", 0, "plain"),
    (197, 197, 64, 3, 1, "fused", 0, "plain"), (65, 197, 64, 1, 3, "kv", 2, "plain"), (31, 33, 96, 1, 1, "dense", 0, "plain"), (65, 65, 96, 3, 1, "fused", 1, "plain"),
    (197, 197, 128, 1, 1, "fused", 0, "plain"), (33, 32, 128, 3, 3, "dense", 3, "plain"),
    # the direct route
    (1, 1, 1, 1, 1, "dense", 0, "plain"), (33, 65, 1, 3, 3, "kv", 1, "plain"), (65, 33, 3, 3, 1, "dense", 2, "plain"), (197, 197, 3, 1, 1, "fused", 3, "plain"),
    (31, 197, 6, 3, 3, "kv", 0, "plain"), (2, 32, 6, 1, 1, "dense", 0, "plain"), (33, 65, 132, 1, 1, "dense", 1, "plain"), (65, 2, 132, 3, 3, "kv", 0, "plain"),
    # the softmax's corners on both routes
    (65, 197, 64, 3, 1, "dense", 0, "pm80"), (33, 33, 32, 1, 3, "fused", 1, "pm80"), (33, 65, 6, 3, 1, "dense", 0, "pm80"),
    (33, 65, 64, 1, 3, "dense", 0, "equal"), (2, 197, 3, 3, 1, "dense", 0, "equal"),
]


def attention_id(c):
    return "tq%d-tk%d-d%d-h%d-n%d-%s-off%d-%s" % c


@functools.lru_cache(maxsize=None)
def attention_case(case):
    """-> (q, k, v, want in float64) of a case, shared among the tests, which leave them unchanged."""
    tq, tk, d, heads, n, layout, offset, kind = case
    e = d * heads
    rng = np.random.default_rng(7000 + ATTENTION_CASES.index(case))
    q = rng.uniform(-1, 1, (n, tq, e)).astype(F)
    k = rng.uniform(-1, 1, (n, tk, e)).astype(F)
    v = rng.uniform(-1, 1, (n, tk, e)).astype(F)
    if kind == "pm80":
        s = max(float(np.abs(q[i, :, h * d:(h + 1) * d].astype(np.float64) @ k[i, :, h * d:(h + 1) * d].astype(np.float64).T).max()) for i in range(n) for h in range(heads))
        q = (q * F(80.0 / s)).astype(F)
    if kind == "equal":
        q[0, 0] = 0
    want = R.attention(q, k, v, heads)
    for a in (q, k, v, want):
        a.setflags(write=False)
    return q, k, v, want


LN_LENGTHS = (1, 2, 3, 63, 64, 65, 192, 256, 257, 768, 1025)  # 256 / 257: the last row a wave takes and the first a block takes
LN_ROWS = (1, 197)


@functools.lru_cache(maxsize=None)
def layer_norm_case(rows, l, offset_mean=False):
    """-> (x, gamma, beta): U(-1, 1) rows, or rows of mean 10^4 and spread 1."""
    rng = np.random.default_rng(8000 + 7 * l + rows + int(offset_mean))
    x = rng.uniform(-1, 1, (rows, l)).astype(F)
    if offset_mean:
        x = (x + F(1e4)).astype(F)
    gamma, beta = rng.uniform(0.5, 1.5, l).astype(F), rng.uniform(-0.5, 0.5, l).astype(F)
    for a in (x, gamma, beta):
        a.setflags(write=False)
    return x, gamma, beta


BINARY_COUNTS = (1, 3, 4, 5, 1023)
SPECIALS = np.array([0.0, -0.0, np.inf, -np.inf, np.nan], F)


# ---- net level -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def net_model():
    """-> ((param, bin, input, output), the trace for model_zoo.numpy_forward) of tiny_vit."""
    from feathercnn_amd import model_zoo
    trace = []
    return model_zoo.tiny_vit(trace=trace), trace


@functools.lru_cache(maxsize=None)
def net_input(batch=3, size=16):
    """-> (x, every blob of the numpy forward); size: 16, or (height, width) of another input with 16 patches -- the same weights."""
    from feathercnn_amd import model_zoo
    if size == 16:
        (p, b, i, o), trace = net_model()
    else:
        trace = []
        p, b, i, o = model_zoo.tiny_vit(size=size, trace=trace)
    h, w = size if isinstance(size, tuple) else (size, size)
    x = np.random.default_rng(9000 + batch + h + 3 * w).uniform(-1, 1, (batch, 3, h, w)).astype(F)
    return x, model_zoo.numpy_forward(trace, i, x)


# every blob of tiny_vit at 16 px: name -> ((c, h, w), rank)
def net_shapes(tokens=17, patches=16, embed=16, hidden=32):
    t = {"data": ((3, 16, 16), 3), "patch_embed": ((embed, 4, 4), 3), "flat": ((1, embed, patches), 2), "to_tokens": ((1, patches, embed), 2),
         "split_patches_0": ((1, patches, embed), 2), "split_patches_1": ((1, patches, embed), 2), "cls_token": ((1, 1, embed), 2),
         "with_cls": ((1, tokens, embed), 2), "pos_embed": ((1, tokens, embed), 2), "add_pos": ((1, tokens, embed), 2), "norm": ((1, tokens, embed), 2),
         "norm_mem": ((1, patches, embed), 2), "cross": ((1, tokens, embed), 2), "halve": ((1, tokens, embed), 2), "gelu_fast": ((1, tokens, embed), 2),
         "as_rank3": ((1, tokens, embed), 3), "cls": ((1, 1, embed), 3), "head": ((10, 1, 1), 3)}
    for b in ("blk0", "blk1"):
        for name in ("_s1_0", "_s1_1", "_ln1", "_attn", "_add1", "_s2_0", "_s2_1", "_ln2", "_fc2", "_add2"):
            t[b + name] = ((1, tokens, embed), 2)
        t[b + "_fc1"] = t[b + "_gelu"] = ((1, tokens, hidden), 2)
    return t
