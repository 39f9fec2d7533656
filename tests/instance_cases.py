"""One sweep case (or more) per kernel instantiation of the shipped library (tests/kernel_instances.py).

A case is an entry point (`kind`: the C-ABI call, the fused or chained forms, the layers, pixels), its geometry and batch, and the
instantiations it is meant to run (`targets`, normalised names).  tests/instance_sweep.py builds each case with scaled inputs and compares it
with an fp64 reference; tests/test_instance_sweep_gpu.py runs the whole table under a kernel trace and checks that every case ran its targets
and that the cases together ran every instantiation but those in EXCLUDED.  tests/test_kernel_instances_cpu.py checks, without a GPU, that the
table and the library agree.

Geometries come from the tests that own a route where they reach the target (tests/contract_routes.py and the route tests it imports);
new ones sit on an edge: a ragged last tile, an odd plane, the last image of a batch.  `cus256` marks a geometry cut for 256 CUs (row split,
persistent output transform): on another CU count the case runs a different instantiation and its trace check is skipped loudly.
"""
from __future__ import annotations

from dataclasses import dataclass

import contract_routes as CR

NAIVE, IM2COL, DEPTHWISE, WINO = CR.NAIVE, CR.IM2COL, CR.DEPTHWISE, CR.WINO

EXCLUDED = {"mfma_calibration_kernel": "measurement only (fhip_calibrate_mfma_f32): no tensor operands to compare"}


@dataclass
class Case:
    name: str
    kind: str      # conv | residual | maxpool2 | dw_pw | siblings | chained | first | relu | add | affine | pooling | softmax | pixels
    args: dict
    targets: tuple
    cus256: bool = False


def _b(v):
    return "true" if v else "false"


# ---- instantiation names ----------------------------------------------------------------------------------------------------------------------
def stream(d, bias, relu, ragged):
    return f"fhip::stream_gemm_kernel<{d}, {_b(bias)}, {_b(relu)}, {_b(ragged)}>"


_SHAPE = {"big": "fhip::GemmShape<128, 64, 16, 2, 2, 4>", "small": "fhip::GemmShape<64, 128, 16, 1, 4, 4>",
          "narrow": "fhip::GemmShape<64, 32, 16, 2, 1, 8>", "fused": "fhip::GemmShape<128, 64, 16, 2, 2, 3>"}


def gemm(shape, mode, twin=False):
    return f"fhip::gemm_mfma_kernel<{_SHAPE[shape]}, fhip::ConvGemmPolicy<{mode}, {_b(twin)}> >"


def wgemm(shape, nt):
    return f"fhip::gemm_mfma_kernel<{_SHAPE[shape]}, fhip::WinoGemmPolicyT<{nt}> >"


def glds(nt, split):
    return f"fhip::wino_gemm_glds_kernel<2, 16, 6, {nt}, {_b(split)}>"


def glds96(nt):
    return f"fhip::wino_gemm_glds96_kernel<{nt}>"


def out_staged(bias, relu, pool):
    return f"fhip::wino_output_transform_staged_kernel<{_b(bias)}, {_b(relu)}, {_b(pool)}>"


def out_persist(bias, relu, pool):
    return f"fhip::wino_output_transform_persist_kernel<{_b(bias)}, {_b(relu)}, {_b(pool)}>"


def out_oneshot(bias, relu):
    return f"fhip::wino_output_transform_kernel<{_b(bias)}, {_b(relu)}>"


def out43(bias, relu):
    return f"fhip::wino43_output_transform_kernel<{_b(bias)}, {_b(relu)}>"


def chain(bias, relu, pool, multi):
    return f"fhip::wino_chain_kernel<{_b(bias)}, {_b(relu)}, {_b(pool)}, {_b(multi)}>"


def staged_in(nv):
    return f"fhip::wino_input_staged_kernel<{nv}>"


def first_direct(c):
    return f"fhip::wino_input_from_first_kernel<{c}>"


def first_staged(c, share):
    return f"fhip::wino_input_from_first_staged_kernel<{c}, {_b(share)}, 16, true, 4, true>"


_FLAT_UNR = {(5, 1): 3, (6, 1): 3, (6, 2): 3, (7, 1): 2, (8, 1): 4, (8, 2): 4, (9, 1): 3, (10, 1): 4, (10, 2): 4, (12, 1): 3, (12, 2): 4,
             (14, 1): 3, (14, 2): 4, (16, 1): 3, (16, 2): 4, (18, 1): 3, (18, 2): 4, (20, 1): 3, (20, 2): 4, (24, 1): 3, (24, 2): 4,
             (28, 1): 4, (28, 2): 4, (32, 1): 3, (32, 2): 3, (36, 1): 3, (36, 2): 4}


def dw_flat(h, s):
    return f"fhip::depthwise3x3_flat_kernel<{h}, {s}, {_FLAT_UNR[(h, s)]}>"


_BAND = {144: (12, 2), 128: (16, 3), 112: (16, 2), 96: (16, 2), 80: (20, 2), 72: (24, 2), 64: (32, 3), 56: (28, 2), 48: (24, 2), 40: (40, 2)}


def dw_band(w):
    return f"fhip::depthwise3x3_band_kernel<{w}, {_BAND[w][0]}, {_BAND[w][1]}>"


def dw_direct(s, vx):
    return f"fhip::depthwise3x3_direct_kernel<{s}, {vx}, {4 if s == 1 else 2}>"


def smallc(tm, passes):
    return f"fhip::conv_smallc_kernel<{tm}, {passes}>"


def affine(relu, vec, src="PlaneSrc"):
    return f"fhip::affine_kernel<{_b(relu)}, {_b(vec)}, fhip::{src}>"


W_U, W43_U, W_IN, W43_IN = ("fhip::wino_filter_transform_kernel", "fhip::wino43_filter_transform_kernel", "fhip::wino_input_transform_kernel",
                            "fhip::wino43_input_transform_kernel")
IG_PACK, DW_PACK, RED = "fhip::igemm_pack_weights_kernel", "fhip::depthwise_pack12_kernel", "fhip::igemm_splitk_reduce_kernel"
DWPW_BAND = "fhip::dwpw_band_kernel<fhip::DwPwBandShape<112, 1, 2, 32, 8, 2, 4, 2> >"


# ---- case constructors ------------------------------------------------------------------------------------------------------------------------
def conv(name, c, k, h, ks, s, p, group, batch, algo, targets, w=None, bias=True, relu=True, cus256=False):
    return Case(name, "conv", dict(c=c, k=k, h=h, w=h if w is None else w, ks=ks, s=s, p=p, group=group, batch=batch, algo=algo, bias=bias,
                                   relu=relu), tuple(targets), cus256)


def wino(name, c, k, h, batch, targets, w=None, bias=True, relu=True, cus256=False, p=1):
    return conv(name, c, k, h, 3, 1, p, 1, batch, WINO, targets, w=w, bias=bias, relu=relu, cus256=cus256)


def dw(name, c, h, s, batch, targets, ks=3, p=1, bias=True, relu=True):
    return conv(name, c, c, h, ks, s, p, c, batch, DEPTHWISE, targets, bias=bias, relu=relu)


def chained(name, batch, c, h, w, layers, targets, pad0=1):
    """layers: [(out_channels, pool after it, bias, relu)]: layer i's flags pick the chained transform that feeds layer i + 1."""
    return Case(name, "chained", dict(batch=batch, c=c, h=h, w=w, layers=layers, pad0=pad0), tuple(targets))


def _mis(name, algo, targets, **kw):
    _, c, k, h, ks, s, p, g, batch = CR._mis(name)
    return conv("mis: " + name, c, k, h, ks, s, p, g, batch, algo, targets, **kw)


def _stream(name, targets):
    _, c, k, h, w, batch, bias, relu = next(r for r in CR.test_stream_gemm_gpu.ON_ROUTE if r[0] == name)
    return conv("stream " + name, c, k, h, 1, 1, 0, 1, batch, IM2COL, targets, w=w, bias=bias, relu=relu)


_RS = CR._RS
_FIRST = CR._FIRST

CASES = [
    # ---- stream_gemm_kernel<D, BIAS, RELU, RAGGED>: D = 16 where 32 divides C, RAGGED where 4 does not divide Ho*Wo --------------------------
    _stream("r50_res3x_2a_b8", (stream(16, 1, 1, 0), "fhip::stream_pack_weights_kernel", IG_PACK)),
    _stream("no_bias", (stream(16, 0, 1, 0),)),
    _stream("no_relu", (stream(16, 1, 0, 0),)),
    conv("stream 16 plain", 256, 128, 16, 1, 1, 0, 1, 17, IM2COL, (stream(16, 0, 0, 0),), bias=False, relu=False),
    _stream("ragged_54", (stream(16, 1, 1, 1),)),
    _stream("ragged_27_no_bias", (stream(16, 0, 0, 1),)),
    conv("stream 16 ragged no bias", 512, 128, 5, 1, 1, 0, 1, 171, IM2COL, (stream(16, 0, 1, 1),), bias=False),
    conv("stream 16 ragged no relu", 256, 160, 7, 1, 1, 0, 1, 90, IM2COL, (stream(16, 1, 0, 1),), relu=False),
    _stream("ring_depth_8", (stream(8, 1, 1, 0),)),
    conv("stream 8 no relu", 272, 160, 10, 1, 1, 0, 1, 43, IM2COL, (stream(8, 1, 0, 0),), relu=False),
    conv("stream 8 no bias", 272, 128, 12, 1, 1, 0, 1, 31, IM2COL, (stream(8, 0, 1, 0),), bias=False),
    conv("stream 8 plain", 336, 128, 8, 1, 1, 0, 1, 67, IM2COL, (stream(8, 0, 0, 0),), bias=False, relu=False),
    _stream("ragged_ring_8", (stream(8, 1, 1, 1),)),
    conv("stream 8 ragged no relu", 272, 192, 5, 1, 1, 0, 1, 170, IM2COL, (stream(8, 1, 0, 1),), relu=False),
    conv("stream 8 ragged no bias", 304, 128, 7, 1, 1, 0, 1, 87, IM2COL, (stream(8, 0, 1, 1),), bias=False),
    conv("stream 8 ragged plain", 272, 256, 3, 1, 1, 0, 1, 457, IM2COL, (stream(8, 0, 0, 1),), bias=False, relu=False),
    # ---- gemm_mfma_kernel<ConvShape*, ConvGemmPolicy<MODE, TWIN>> -------------------------------------------------------------------------------
    _mis("1x1 aligned planes", IM2COL, (gemm("big", 2), IG_PACK)),
    _mis("1x1 stride 2", IM2COL, (gemm("big", 1),)),
    _mis("1x1 ragged planes", IM2COL, (gemm("big", 5),)),
    conv("3x3 mode 0 Big", 16, 128, 12, 3, 1, 1, 1, 2, IM2COL, (gemm("big", 0),)),
    conv("1x1 mode 2 SmallM", 64, 64, 28, 1, 1, 0, 1, 2, IM2COL, (gemm("small", 2),), relu=False),
    conv("1x1 s2 mode 1 SmallM", 32, 48, 20, 1, 2, 0, 1, 2, IM2COL, (gemm("small", 1),), bias=False),
    conv("3x3 mode 0 SmallM", 16, 64, 12, 3, 1, 1, 1, 2, IM2COL, (gemm("small", 0),)),
    conv("1x1 mode 5 SmallM", 48, 40, 7, 1, 1, 0, 1, 5, IM2COL, (gemm("small", 5),)),
    conv("1x1 mode 2 Narrow", 128, 128, 4, 1, 1, 0, 1, 1, IM2COL, (gemm("narrow", 2),)),
    conv("1x1 s2 mode 1 Narrow", 64, 128, 8, 1, 2, 0, 1, 1, IM2COL, (gemm("narrow", 1),), relu=False),
    conv("5x5 s2 mode 0 Narrow", 5, 7, 9, 5, 2, 2, 1, 1, IM2COL, (gemm("narrow", 0),)),
    conv("NAIVE", 16, 32, 18, 3, 1, 1, 1, 2, NAIVE, (gemm("small", 0),), relu=False),
    conv("split-K mode 0 Big", 32, 128, 12, 3, 1, 1, 1, 2, IM2COL, (gemm("big", 0), RED)),
    conv("split-K mode 5 slots", 2048, 64, 7, 1, 1, 0, 1, 8, IM2COL, (gemm("small", 5), RED)),
    Case("siblings s2 (twin, mode 1)", "siblings", dict(c=64, ka=128, kb=32, h=28, s=2, batch=12), (gemm("big", 1, True),)),
    Case("siblings 14 px (twin, mode 2)", "siblings", dict(c=64, ka=128, kb=64, h=14, s=1, batch=24), (gemm("big", 2, True),)),
    Case("residual aligned", "residual", dict(c=64, k=256, h=28, w=28, batch=2), (gemm("big", 2),)),
    Case("residual ragged", "residual", dict(c=64, k=96, h=7, w=7, batch=9), (gemm("big", 5),)),
    Case("dw_pw s1", "dw_pw", dict(c=16, k=72, h=16, w=16, s=1, batch=3), (gemm("fused", 3),)),
    Case("dw_pw s2", "dw_pw", dict(c=8, k=200, h=24, w=16, s=2, batch=2), (gemm("fused", 4),)),
    Case("dw_pw band", "dw_pw", dict(c=32, k=64, h=37, w=112, s=1, batch=3), (DWPW_BAND,)),
    conv("ip stream padded octet", 1028, 300, 1, 1, 1, 0, 1, 7, IM2COL, ("fhip::ip_pack_input_kernel", "fhip::ip_stream_kernel<4>",
                                                                         "fhip::ip_reduce_kernel", "fhip::ip_pack_weights_kernel")),
    # ---- conv_smallc_kernel<TM, PASSES>: TM = 1 for K <= 32; PASSES buckets of ceil(patch / 256) ----------------------------------------------
    conv("smallc 3x3 c3 k32", 3, 32, 28, 3, 1, 1, 1, 2, IM2COL, (smallc(1, 3),)),
    conv("smallc 3x3 c3 k64", 3, 64, 28, 3, 1, 1, 1, 2, IM2COL, (smallc(2, 3),), bias=False),
    conv("smallc 3x3 c8 k24 (32-wide tile)", 8, 24, 32, 3, 1, 1, 1, 2, IM2COL, (smallc(1, 7),), relu=False),
    conv("smallc 3x3 c8 k48 (32-wide tile)", 8, 48, 32, 3, 1, 1, 1, 2, IM2COL, (smallc(2, 7),)),
    conv("smallc 7x7 s2 c3 k16", 3, 16, 40, 7, 2, 3, 1, 2, IM2COL, (smallc(1, 11),)),
    _mis("first 7x7 s2", IM2COL, (smallc(2, 11),)),
    # ---- Winograd F(6,3): tile GEMM by K (small M <= 64), depth (k_tiles >= 8 -> glds), columns and the size of M ------------------------------
    wino("wino plain input, SmallM gemm", 8, 8, 31, 3, (W_IN, wgemm("small", 1), out_staged(1, 1, 0), W_U), w=17),
    wino("wino big-M SmallM gemm", 16, 64, 24, 640, (wgemm("small", 3),), relu=False),
    wino("wino gemm_mfma Big", 48, 192, 13, 5, (wgemm("big", 0),)),
    wino("wino gemm_mfma Big, one row tile", 48, 128, 13, 5, (wgemm("big", 1),), bias=False),
    wino("wino big-M gemm_mfma Big", 48, 192, 24, 224, (wgemm("big", 2),)),
    wino("wino big-M gemm_mfma Big, one row tile", 48, 128, 24, 320, (wgemm("big", 3),)),
    wino("wino glds", 128, 128, 14, 2, (glds(0, False),)),
    wino("wino glds96 P = 90", 128, 128, 14, 10, (glds96(0),)),
    wino("wino big-M glds", 128, 128, 24, 320, (glds(2, False),)),
    wino("wino big-M glds96", 128, 128, 30, 195, (glds96(2),)),
    wino("wino row split 4", *_RS[3][:3], _RS[3][3], (glds(0, True),), cus256=True),
    wino("wino row split 2", *_RS[4][:3], _RS[4][3], (glds(0, True),), cus256=True),
    # staged input transform: NV vectors per lane = ceil(planes per block * H * W / 4 / threads); 16 x 16 planes (64 float4 each), 4 planes a vector
    *[wino(f"wino staged input nv {nv}", 2 * nv, 8, 16, 2, (staged_in(nv),)) for nv in range(1, 8)],
    # output transforms: staged (one block per row band), persistent (more items than resident blocks), one-shot (more than 256 tile columns)
    wino("wino output staged, no bias", 16, 32, 20, 2, (out_staged(0, 1, 0),), bias=False),
    wino("wino output staged, linear", 16, 32, 20, 2, (out_staged(1, 0, 0),), relu=False),
    wino("wino output staged, plain", 16, 32, 20, 2, (out_staged(0, 0, 0),), bias=False, relu=False),
    *[Case(f"maxpool2 staged bias={b} relu={r}", "maxpool2", dict(c=16, k=32, h=20, w=20, batch=2, bias=b, relu=r), (out_staged(b, r, 1),))
      for b in (0, 1) for r in (0, 1)],
    *[wino(f"wino persistent output bias={b} relu={r}", 16, 1024, 12, 1, (out_persist(b, r, 0),), bias=b, relu=r, cus256=True)
      for b in (0, 1) for r in (0, 1)],
    *[Case(f"maxpool2 persistent bias={b} relu={r}", "maxpool2", dict(c=16, k=1024, h=12, w=12, batch=1, bias=b, relu=r), (out_persist(b, r, 1),),
           cus256=True) for b in (0, 1) for r in (0, 1)],
    *[wino(f"wino one-shot output bias={b} relu={r}", 16, 16, 4, 1, (out_oneshot(b, r),), w=1560, bias=b, relu=r) for b in (0, 1) for r in (0, 1)],
    # F(4,3) on 7 / 8-pixel planes
    _mis("winograd f43", WINO, (W43_IN, out43(1, 1), W43_U)),
    *[wino(f"winograd f43 8px bias={b} relu={r}", 64, 64, 8, 4, (out43(b, r),), bias=b, relu=r) for b, r in ((0, 0), (0, 1), (1, 0))],
    # ---- chained transforms: layer i's output transform writes layer i + 1's V (wino_chain_kernel<BIAS, RELU, POOL, MULTI>) ---------------------
    *[chained(f"chain bias={b} relu={r}", 2, 8, 20, 26, [(16, 0, b, r), (8, 0, 1, 1)], (chain(b, r, 0, 0),)) for b in (0, 1) for r in (0, 1)],
    *[chained(f"chain pooled bias={b} relu={r}", 3, 8, 28, 22, [(12, 1, b, r), (8, 0, 1, 0)], (chain(b, r, 1, 0),)) for b in (0, 1) for r in (0, 1)],
    *[chained(f"chain pooled 224 px bias={b} relu={r}", 2, 3, 224, 224, [(4, 1, b, r), (4, 0, 1, 1)], (chain(b, r, 1, 1),))
      for b in (0, 1) for r in (0, 1)],
    chained("chain, no pooling, staged input", 2, 16, 28, 28, [(16, 0, 0, 0), (8, 0, 0, 0)], (staged_in(7),)),
    # ---- the first layer inside the next layer's input transform: staged form (shared columns where 6 TX - 1 >= W) or direct form -------------
    *[Case(f"first staged c={c} shared", "first", dict(batch=2, c=c, h=64, w=64, k=24, bias=True, relu=c != 3, pool=False),
           (first_staged(c, True),)) for c in (2, 3, 4)],
    *[Case(f"first staged c={c} unshared", "first", dict(batch=2, c=c, h=40, w=42, k=9, bias=c != 4, relu=True, pool=False),
           (first_staged(c, False),)) for c in (2, 3, 4)],
    *[Case(f"first direct c={c}", "first", dict(batch=18, c=c, h=40, w=14, k=6, bias=True, relu=True, pool=c == 2), (first_direct(c),))
      for c in (2, 3, 4)],
    # ---- depthwise ------------------------------------------------------------------------------------------------------------------------------
    *[dw(f"dw flat {h} s1", 8, h, 1, 3, (dw_flat(h, 1), DW_PACK)) for h in (5, 6, 7, 8, 9, 10, 12, 14, 16, 18, 20, 24, 28, 32, 36)],
    *[dw(f"dw flat {h} s2", 8, h, 2, 3, (dw_flat(h, 2),), relu=h % 4 != 0) for h in (6, 8, 10, 12, 14, 16, 18, 20, 24, 28, 32, 36)],
    *[dw(f"dw band {h}", 4, h, 1, 2, (dw_band(h),), bias=h != 56) for h in (40, 48, 56, 64, 72, 80, 96, 112, 128, 144)],
    dw("dw direct s1 vx4", 8, 44, 1, 2, (dw_direct(1, 4),)),
    dw("dw direct s1 vx2", 8, 30, 1, 2, (dw_direct(1, 2),), relu=False),
    dw("dw direct s1 vx1", 8, 31, 1, 2, (dw_direct(1, 1),)),
    dw("dw direct s2 vx4", 8, 40, 2, 2, (dw_direct(2, 4),)),
    dw("dw direct s2 vx2", 8, 44, 2, 2, (dw_direct(2, 2),), bias=False),
    dw("dw direct s2 vx1", 8, 41, 2, 2, (dw_direct(2, 1),)),
    _mis("dw chunk 7 s2", DEPTHWISE, ("fhip::depthwise3x3_chunk_kernel<2>",)),
    conv("dw 5x5 lds_scalar", 8, 8, 16, 5, 1, 2, 8, 2, DEPTHWISE, ("fhip::depthwise_lds_scalar_kernel",)),
    conv("dw 5x5 64px generic", 4, 4, 64, 5, 1, 2, 4, 1, DEPTHWISE, ("fhip::depthwise_generic_kernel",)),
    # ---- layers (feather_net.h) ------------------------------------------------------------------------------------------------------------------
    Case("relu odd", "relu", dict(n=(1 << 20) + 3), ("fhip::relu_kernel",)),
    Case("add odd", "add", dict(n=100001, relu=0), ("fhip::add_kernel<false>",)),
    Case("add relu odd", "add", dict(n=99999, relu=1), ("fhip::add_kernel<true>",)),
    Case("affine vec relu", "affine", dict(batch=3, c=7, hw=16, relu=1), (affine(1, 1),)),
    Case("affine vec", "affine", dict(batch=3, c=7, hw=20, relu=0), (affine(0, 1),)),
    Case("affine scalar relu", "affine", dict(batch=3, c=7, hw=13, relu=1), (affine(1, 0),)),
    Case("affine scalar", "affine", dict(batch=3, c=7, hw=15, relu=0), (affine(0, 0),)),
    Case("pixels vec", "pixels", dict(batch=3, type="RGB2BGR", w=33, h=21, tw=16, th=12), (affine(0, 1, "PixelSrc"),)),
    Case("pixels scalar", "pixels", dict(batch=3, type="RGBA2BGR", w=20, h=15, tw=13, th=9), (affine(0, 0, "PixelSrc"),)),
    Case("pooling generic max", "pooling", dict(batch=2, c=5, h=13, w=13, k=3, s=2, pad=1, avg=0, glob=0), ("fhip::pooling_kernel",)),
    Case("pooling generic avg", "pooling", dict(batch=2, c=5, h=13, w=15, k=3, s=1, pad=0, avg=1, glob=0), ("fhip::pooling_kernel",)),
    Case("pooling 3x3 s2 fast", "pooling", dict(batch=2, c=6, h=28, w=28, k=3, s=2, pad=0, avg=0, glob=0), ("fhip::maxpool3s2_kernel",)),
    Case("pooling global small avg", "pooling", dict(batch=3, c=37, h=7, w=7, k=7, s=1, pad=0, avg=1, glob=1),
         ("fhip::plane_reduce_small_kernel<true>",)),
    Case("pooling global small max", "pooling", dict(batch=3, c=37, h=5, w=5, k=5, s=1, pad=0, avg=0, glob=1),
         ("fhip::plane_reduce_small_kernel<false>",)),
    Case("pooling global wave avg", "pooling", dict(batch=2, c=9, h=14, w=14, k=14, s=1, pad=0, avg=1, glob=1), ("fhip::plane_reduce_kernel<true>",)),
    Case("pooling global wave max", "pooling", dict(batch=2, c=9, h=13, w=11, k=13, s=1, pad=0, avg=0, glob=1), ("fhip::plane_reduce_kernel<false>",)),
    Case("softmax", "softmax", dict(batch=3, n=1001), ("fhip::softmax_kernel",)),
]
