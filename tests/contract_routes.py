"""Route table of the C-ABI contract tests (tests/test_contract_gpu.py): one entry per kernel route of include/feather_hip/feather_hip.h and
feather_net.h, with the `__global__` kernels the entry is meant to reach and the host-side predicate that confirms the route.

Geometries come from the route tests that own them (imported where they are lists); batches are small.  `cus256` marks a geometry cut for
the MI355X's 256 CUs (tail split, row split, persistent grids): on another CU count the entry skips loudly, as the owning tests do.
tests/test_guarded_cpu.py checks that every kernel of feathercnn_amd/csrc appears in some entry (or in EXCLUDED, with a reason).
"""
from __future__ import annotations

from dataclasses import dataclass

import test_misaligned_gpu
import test_row_split_gpu
import test_stream_gemm_gpu
import test_tail_split_gpu
import test_wino_chain_gpu
import test_wino_first_gpu

NAIVE, IM2COL, DEPTHWISE, WINO = 0, 1, 3, 4

EXCLUDED = {"mfma_calibration_kernel": "measurement only (fhip_calibrate_mfma_f32): no tensor operands"}

DW_PACK = "depthwise_pack12_kernel"
IG_PACK = "igemm_pack_weights_kernel"
WINO_U = "wino_filter_transform_kernel"
WINO43_U = "wino43_filter_transform_kernel"


@dataclass
class Route:
    name: str
    kind: str     # conv | residual | maxpool2 | dw_pw | siblings | chained | first | out_to_next | wino_stages | relu | add | affine | pooling | softmax
    args: dict
    kernels: tuple
    confirm: str  # the host-side predicate the test evaluates: see test_contract_gpu._confirm
    cus256: bool = False


def conv(name, c, k, h, ks, s, p, group, batch, algo, kernels, confirm, w=None, bias=True, act=1, cus256=False):
    return Route(name, "conv", dict(c=c, k=k, h=h, w=h if w is None else w, ks=ks, s=s, p=p, group=group, batch=batch, algo=algo, bias=bias,
                                    act=act), tuple(kernels), confirm, cus256)


def _mis(name):
    return next(c for c in test_misaligned_gpu.CASES if c[0] == name)


def _from_mis(name, algo, kernels, confirm):
    _, c, k, h, ks, s, p, g, batch = _mis(name)
    return conv("mis: " + name, c, k, h, ks, s, p, g, batch, algo, kernels, confirm)


def _stream(name, kernels):
    _, c, k, h, w, batch, bias, relu = next(r for r in test_stream_gemm_gpu.ON_ROUTE if r[0] == name)
    return conv("stream 1x1 " + name, c, k, h, 1, 1, 0, 1, batch, IM2COL, kernels, "streams_1x1", w=w, bias=bias, act=int(relu))


_T = test_tail_split_gpu.TAIL
_RS = test_row_split_gpu.CASES
_CHAIN = {r[0]: r for r in test_wino_chain_gpu.RUNS}
_FIRST = {r[0]: r for r in test_wino_first_gpu.CASES}
GEMM = "gemm_mfma_kernel"
RED = "igemm_splitk_reduce_kernel"
FLAT, BAND, DIRECT, CHUNK = "depthwise3x3_flat_kernel", "depthwise3x3_band_kernel", "depthwise3x3_direct_kernel", "depthwise3x3_chunk_kernel"
LDS_SCALAR, GENERIC = "depthwise_lds_scalar_kernel", "depthwise_generic_kernel"
W_IN, W_IN_ST, W_OUT, W_OUT_ST, W_OUT_P = ("wino_input_transform_kernel", "wino_input_staged_kernel", "wino_output_transform_kernel",
                                           "wino_output_transform_staged_kernel", "wino_output_transform_persist_kernel")
GLDS, GLDS96 = "wino_gemm_glds_kernel", "wino_gemm_glds96_kernel"

ROUTES = [
    # ---- fhip_conv_forward, depthwise -------------------------------------------------------------------------------------------------------------
    _from_mis("dw flat 14", DEPTHWISE, (FLAT, DW_PACK), "dw_flat"),
    _from_mis("dw flat 20 s2", DEPTHWISE, (FLAT, DW_PACK), "dw_flat"),
    conv("dw flat 10 s2 (straddling dwordx4 stores)", 16, 16, 10, 3, 2, 1, 16, 3, DEPTHWISE, (FLAT, DW_PACK), "dw_flat"),
    conv("dw flat 5 row-per-lane", 44, 44, 5, 3, 1, 1, 44, 2, DEPTHWISE, (FLAT, DW_PACK), "dw_flat"),
    conv("dw flat 9 row-per-lane", 12, 12, 9, 3, 1, 1, 12, 3, DEPTHWISE, (FLAT, DW_PACK), "dw_flat"),
    conv("dw flat 7 ragged chunk", 37, 37, 7, 3, 1, 1, 37, 5, DEPTHWISE, (FLAT, DW_PACK), "dw_flat"),
    _from_mis("dw band 56", DEPTHWISE, (BAND, DW_PACK), "dw_band"),
    _from_mis("dw direct 30", DEPTHWISE, (DIRECT, DW_PACK), "dw_k3"),
    conv("dw direct 40 s2", 8, 8, 40, 3, 2, 1, 8, 2, DEPTHWISE, (DIRECT, DW_PACK), "dw_k3"),
    _from_mis("dw chunk 7 s2", DEPTHWISE, (CHUNK, DW_PACK), "dw_k3"),
    conv("dw 5x5 lds_scalar", 8, 8, 16, 5, 1, 2, 8, 2, DEPTHWISE, (LDS_SCALAR,), "dw_not_k3"),
    conv("dw 7x7 global lds_scalar", 16, 16, 7, 7, 1, 0, 16, 3, DEPTHWISE, (LDS_SCALAR,), "dw_not_k3"),
    conv("dw 3x3 unpadded lds_scalar", 8, 8, 16, 3, 1, 0, 8, 2, DEPTHWISE, (LDS_SCALAR, DW_PACK), "dw_not_k3"),
    conv("dw 5x5 64px generic", 4, 4, 64, 5, 1, 2, 4, 1, DEPTHWISE, (GENERIC,), "dw_generic"),
    # ---- fhip_conv_forward, implicit GEMM -------------------------------------------------------------------------------------------------------
    _from_mis("1x1 aligned planes", IM2COL, (GEMM, IG_PACK), "igemm_no_scratch"),                       # mode 2, Big
    conv("1x1 mode 2 SmallM", 64, 64, 28, 1, 1, 0, 1, 2, IM2COL, (GEMM, IG_PACK), "igemm_no_scratch"),
    conv("1x1 mode 2 Narrow", 128, 128, 4, 1, 1, 0, 1, 1, IM2COL, (GEMM, IG_PACK), "igemm_no_scratch"),
    _from_mis("1x1 stride 2", IM2COL, (GEMM, IG_PACK), "igemm_no_scratch"),                             # mode 1, Big
    conv("1x1 s2 mode 1 SmallM", 32, 48, 20, 1, 2, 0, 1, 2, IM2COL, (GEMM, IG_PACK), "igemm_no_scratch"),
    conv("1x1 s2 mode 1 Narrow", 64, 128, 8, 1, 2, 0, 1, 1, IM2COL, (GEMM, IG_PACK), "igemm_no_scratch"),
    conv("3x3 mode 0 Big", 16, 128, 12, 3, 1, 1, 1, 2, IM2COL, (GEMM, IG_PACK), "igemm_no_scratch"),
    conv("3x3 mode 0 SmallM", 16, 64, 12, 3, 1, 1, 1, 2, IM2COL, (GEMM, IG_PACK), "igemm_no_scratch"),
    conv("5x5 s2 mode 0 Narrow", 5, 7, 9, 5, 2, 2, 1, 2, IM2COL, (GEMM, IG_PACK), "igemm_no_scratch", w=14),
    _from_mis("1x1 ragged planes", IM2COL, (GEMM, IG_PACK), "igemm_no_scratch"),                        # mode 5, Big
    conv("1x1 mode 5 SmallM", 48, 40, 7, 1, 1, 0, 1, 5, IM2COL, (GEMM, IG_PACK), "igemm_no_scratch"),
    conv("split-K mode 0 Big", 32, 128, 12, 3, 1, 1, 1, 2, IM2COL, (GEMM, IG_PACK, RED), "scratch"),
    conv("split-K mode 0 Narrow", 64, 128, 4, 3, 1, 1, 1, 1, IM2COL, (GEMM, IG_PACK, RED), "scratch"),
    conv("split-K mode 2", 1024, 256, 14, 1, 1, 0, 1, 2, IM2COL, (GEMM, IG_PACK, RED), "scratch"),
    conv("split-K mode 5 slots", 2048, 64, 7, 1, 1, 0, 1, 8, IM2COL, (GEMM, IG_PACK, RED), "scratch"),
    conv("tail split mode 2", *_T[0][:3], 1, _T[0][4], 0, 1, _T[0][5], IM2COL, (GEMM, IG_PACK, RED), "scratch", w=_T[0][3], cus256=True),
    conv("tail split mode 1", *_T[1][:3], 1, _T[1][4], 0, 1, _T[1][5], IM2COL, (GEMM, IG_PACK, RED), "scratch", w=_T[1][3], cus256=True),
    conv("tail split mode 5", *_T[2][:3], 1, _T[2][4], 0, 1, _T[2][5], IM2COL, (GEMM, IG_PACK, RED), "scratch", w=_T[2][3], cus256=True),
    _stream("ring_depth_8", ("stream_gemm_kernel", "stream_pack_weights_kernel", IG_PACK)),         # 8-deep ring, ragged last pixel tile
    _stream("no_bias", ("stream_gemm_kernel", "stream_pack_weights_kernel")),                        # 16-deep ring
    _stream("ragged_54", ("stream_gemm_kernel",)),                                                   # planes of 54 pixels
    conv("ip stream padded octet", 1028, 300, 1, 1, 1, 0, 1, 7, IM2COL, ("ip_pack_input_kernel", "ip_stream_kernel", "ip_reduce_kernel",
                                                                          "ip_pack_weights_kernel"), "scratch"),
    conv("ip stream fc6", 25088, 256, 1, 1, 1, 0, 1, 32, IM2COL, ("ip_pack_input_kernel", "ip_stream_kernel", "ip_reduce_kernel"), "scratch"),
    _from_mis("first 7x7 s2", IM2COL, ("conv_smallc_kernel", IG_PACK), "smallc"),
    _from_mis("first 3x3", IM2COL, ("conv_smallc_kernel",), "smallc"),
    conv("NAIVE", 16, 32, 18, 3, 1, 1, 1, 2, NAIVE, (GEMM, IG_PACK), "igemm_no_scratch"),
    # ---- fhip_conv_forward, Winograd --------------------------------------------------------------------------------------------------------------
    conv("wino plain input, SmallM gemm", 8, 8, 31, 3, 1, 1, 1, 3, WINO, (W_IN, GEMM, W_OUT_ST, WINO_U), "f63", w=17),
    conv("wino staged input", 32, 64, 28, 3, 1, 1, 1, 2, WINO, (W_IN_ST, GEMM, W_OUT_ST), "f63"),
    conv("wino unpadded, C % 16 != 0", 24, 36, 12, 3, 1, 0, 1, 2, WINO, (W_IN, GEMM, W_OUT_ST), "f63"),
    conv("wino glds", 128, 128, 14, 3, 1, 1, 1, 2, WINO, (GLDS, W_IN_ST, W_OUT_ST), "f63"),
    conv("wino glds96 P = 90", 128, 128, 14, 3, 1, 1, 1, 10, WINO, (GLDS96,), "f63"),
    conv("wino gemm_mfma Big", 48, 192, 13, 3, 1, 1, 1, 5, WINO, (GEMM,), "f63"),
    conv("wino row split 4", *_RS[3][:3], 3, 1, 1, 1, _RS[3][3], WINO, (GLDS,), "f63", cus256=True),
    conv("wino row split 2", *_RS[4][:3], 3, 1, 1, 1, _RS[4][3], WINO, (GLDS,), "f63", cus256=True),
    conv("wino column blocks n = 90", 12, 20, 17, 3, 1, 1, 1, 90, WINO, (GEMM,), "column_blocks", w=23),
    conv("wino persistent output", 16, 1024, 12, 3, 1, 1, 1, 1, WINO, (W_OUT_P,), "f63", cus256=True),
    conv("wino one-shot output (TX > 256)", 16, 16, 4, 3, 1, 1, 1, 1, WINO, (W_OUT,), "f63", w=1560),
    _from_mis("winograd f43", WINO, ("wino43_input_transform_kernel", "wino43_output_transform_kernel", WINO43_U), "f43"),
    conv("winograd f43 8px", 64, 64, 8, 3, 1, 1, 1, 4, WINO, ("wino43_input_transform_kernel", "wino43_output_transform_kernel"), "f43"),
    # ---- fused entry points -----------------------------------------------------------------------------------------------------------------------
    Route("maxpool2", "maxpool2", dict(c=16, k=32, h=20, w=20, batch=2), (W_OUT_ST,), "can_fuse_maxpool2"),
    Route("residual aligned", "residual", dict(c=64, k=256, h=28, w=28, batch=2), (GEMM,), "can_fuse_residual"),
    Route("residual ragged", "residual", dict(c=64, k=96, h=7, w=7, batch=9), (GEMM,), "can_fuse_residual"),
    Route("residual tail split", "residual", dict(c=_T[0][0], k=_T[0][1], h=_T[0][2], w=_T[0][3], batch=_T[0][5]), (GEMM, RED),
          "can_fuse_residual+scratch", cus256=True),
    Route("dw_pw s1", "dw_pw", dict(c=16, k=72, h=16, w=16, s=1, batch=3), (GEMM,), "can_fuse_dw_pw"),
    Route("dw_pw s2", "dw_pw", dict(c=8, k=200, h=24, w=16, s=2, batch=2), (GEMM,), "can_fuse_dw_pw"),
    Route("dw_pw band", "dw_pw", dict(c=32, k=64, h=37, w=112, s=1, batch=3), ("dwpw_band_kernel",), "can_fuse_dw_pw"),
    Route("siblings s2", "siblings", dict(c=64, ka=128, kb=32, h=28, s=2, batch=12), (GEMM,), "can_fuse_siblings"),
    Route("siblings odd plane", "siblings", dict(c=20, ka=128, kb=40, h=7, s=1, batch=96), (GEMM,), "can_fuse_siblings"),
    Route("chained, no pooling", "chained", dict(run=_CHAIN["no_bias_no_relu"]), ("wino_chain_kernel", W_IN_ST), "can_chain"),
    Route("chained, pooling between", "chained", dict(run=_CHAIN["odd_then_pool"]), ("wino_chain_kernel", W_IN), "can_chain"),
    Route("chained, pooled last", "chained", dict(run=("pooled_last", 2, 8, 28, 28, [(8, False), (16, True)], 1, True, True)),
          ("wino_chain_kernel", W_OUT_ST), "can_chain"),
    Route("first layer staged", "first", dict(case=_FIRST["two_blocks_per_image"]), ("wino_input_from_first_staged_kernel",), "can_fuse_first"),
    Route("first layer plain", "first", dict(case=_FIRST["small_plane_direct_form"]), ("wino_input_from_first_kernel",), "can_fuse_first"),
    Route("output_to_next_input", "out_to_next", dict(batch=2, c=16, k=24, k2=8, h=28, w=28, pool=0), ("wino_chain_kernel",), "can_chain"),
    Route("output_to_next_input pooled", "out_to_next", dict(batch=2, c=8, k=16, k2=8, h=20, w=26, pool=1), ("wino_chain_kernel",), "can_chain"),
    Route("wino stages", "wino_stages", dict(c=12, k=20, h=17, w=23, batch=3), (WINO_U, W_IN, GEMM, W_OUT_ST), "f63"),
    Route("wino stages n = 90", "wino_stages", dict(c=12, k=20, h=17, w=23, batch=90), (W_IN, GEMM, W_OUT_ST), "column_blocks"),
    # ---- layers (feather_net.h) -------------------------------------------------------------------------------------------------------------------
    Route("relu odd", "relu", dict(n=100003), ("relu_kernel",), "none"),
    Route("add odd", "add", dict(n=100001, relu=0, inplace=False), ("add_kernel",), "none"),
    Route("add relu odd", "add", dict(n=99999, relu=1, inplace=False), ("add_kernel",), "none"),
    Route("add in place", "add", dict(n=100003, relu=1, inplace=True), ("add_kernel",), "none"),
    Route("affine vec", "affine", dict(batch=3, c=7, hw=16, relu=1), ("affine_kernel",), "none"),
    Route("affine scalar", "affine", dict(batch=3, c=7, hw=13, relu=0), ("affine_kernel",), "none"),
    Route("pooling generic max", "pooling", dict(batch=2, c=5, h=13, w=13, k=3, s=2, pad=1, avg=0, glob=0), ("pooling_kernel",), "none"),
    Route("pooling generic avg", "pooling", dict(batch=2, c=5, h=13, w=15, k=3, s=1, pad=0, avg=1, glob=0), ("pooling_kernel",), "none"),
    Route("pooling 3x3 s2 fast", "pooling", dict(batch=2, c=6, h=28, w=28, k=3, s=2, pad=0, avg=0, glob=0), ("maxpool3s2_kernel",), "none"),
    Route("pooling global small", "pooling", dict(batch=3, c=37, h=7, w=7, k=7, s=1, pad=0, avg=1, glob=1), ("plane_reduce_small_kernel",), "none"),
    Route("pooling global wave", "pooling", dict(batch=2, c=9, h=14, w=14, k=14, s=1, pad=0, avg=0, glob=1), ("plane_reduce_kernel",), "none"),
    Route("softmax", "softmax", dict(batch=3, n=1001), ("softmax_kernel",), "none"),
]
