"""The size limits the sources state, one row each (tests/test_limits_cpu.py calls every row; INTEGRATION.md "Size limits" lists them).

A row names the entry point, the quantity that is limited, the largest value the library accepts (`max_ok`; the first refused value is
max_ok + 1, or the next value the dimensions can form: `step`), the words its refusal must contain, and two argument sets: `refuse` puts the
quantity exactly at the first refused value, `accept` one step below.  `measure` computes the quantity from an argument set in Python
integers, so the table checks itself.  Dimensions are absurd on purpose (2^20 images of a 2048-pixel plane): nothing is allocated, the
pointers are made up, and a refusal never reaches the device.

`queries`: the launch-free calls that must agree with the entry point on both sides of the boundary.
`code`: FHIP_E_BADARG for a refusal; FHIP_E_UNSUPPORTED where the boundary is between two routes and the caller is expected to take the other
one (the query says which).
`shadowed`: the limit sits behind another one and no argument set reaches it; the row states why, and has no argument sets.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Callable, Optional

BADARG, UNSUPPORTED = -2, -1
NAIVE, IM2COL, DEPTHWISE, WINO = 0, 1, 3, 4
I31 = 2 ** 31 - 1          # 0x7fffffff
COLS = 0x7fffff00          # the implicit GEMM's and the Winograd plan's column limit
ATROUS_MFMA = "fhip::gemm_mfma_kernel<fhip::GemmShape<128, 64, 16, 2, 2, 4>, fhip::AtrousGemmPolicy<false, false> >"


@dataclass(frozen=True)
class Limit:
    name: str
    lib: str                       # main | gate | inorm | shuffle | deconv | gconv | atrous | canvas | pixout
    entry: str                     # the entry point; tests/test_limits_cpu.py has a caller of the same name
    quantity: str
    max_ok: int
    word: str
    measure: Optional[Callable] = None
    refuse: Optional[dict] = None
    accept: Optional[dict] = None
    step: int = 1
    queries: tuple = ()
    code: int = BADARG
    shadowed: str = ""
    source: str = ""               # where the limit is written down


def shape(n, c, h, w, **kw):
    return dict(n=n, c=c, h=h, w=w, **kw)


def conv(c, k, h, w, kh=1, kw=1, s=1, pads=(0, 0, 0, 0), group=1, batch=1, **extra):
    """A convolution-style argument set: pads are (left, right, top, bottom); `extra` carries dilation, output padding, algo, route."""
    return dict(c=c, k=k, h=h, w=w, kh=kh, kw=kw, s=s, pads=pads, group=group, batch=batch, **extra)


def out_hw(a):
    """Output size of a `conv` argument set: the convolution's, the dilated one's (dil) or the transposed one's (deconv=True)."""
    pl, pr, pt, pb = a["pads"]
    s = a["s"]
    if a.get("deconv"):
        return (a["h"] - 1) * s + a["kh"] - pt - pb, (a["w"] - 1) * s + a["kw"] - pl - pr
    d = a.get("dil", 1)
    return (a["h"] + pt + pb - (d * (a["kh"] - 1) + 1)) // s + 1, (a["w"] + pl + pr - (d * (a["kw"] - 1) + 1)) // s + 1


def _elements(a):
    return a["n"] * a["c"] * a["h"] * a["w"]


def _conv_elements(a):
    oh, ow = out_hw(a)
    return max(a["batch"] * a["c"] * a["h"] * a["w"], a["batch"] * a["k"] * oh * ow)


def _columns(a):
    oh, ow = out_hw(a)
    return a["batch"] * oh * ow


def _slots(a):  # ConvGemmPolicy<5>: four pixel slots per group of a ragged plane
    oh, ow = out_hw(a)
    return a["batch"] * 4 * ((oh * ow + 3) // 4)


def _wino_tiles(a):
    pl, pr, pt, pb = a["pads"]
    return a["batch"] * ((a["h"] + pt + pb + 3) // 6) * ((a["w"] + pl + pr + 3) // 6)


def _blocks(lanes):
    return (lanes + 255) // 256


def _generic_packed(a):  # group * chunks of 4 output channels * Cg * taps * 4
    cg, kg = a["c"] // a["group"], a["k"] // a["group"]
    return a["group"] * ((kg + 3) // 4) * cg * a["kh"] * a["kw"] * 4


def _chunks(a):
    return a["group"] * ((a["k"] // a["group"] + 3) // 4)


def _ew_lanes(a):  # fhip_relu / fhip_add: a lane per float4 and one per leftover float; unaligned pointers take no float4
    n4 = a["count"] // 4 if a["aligned"] else 0
    return n4 + a["count"] - 4 * n4


_E = "2^31 elements"
_ONE_BELOW = shape(I31, 1, 1, 1)            # 2^31 - 1 is prime: one image of one pixel per channel
_AT = shape(2 ** 20, 1, 32, 64)             # 2^20 images of a 2048-pixel plane: 2^31 elements


def _side(lib, entry, queries=(), at=_AT, below=_ONE_BELOW, source=""):
    return Limit(f"{entry}: elements", lib, entry, "elements of one tensor (n * c * h * w)", I31, _E, _elements, at, below, queries=queries,
                 source=source)


LIMITS = [
    # ---- libfeather_gate.so ---------------------------------------------------------------------------------------------------------------------
    _side("gate", "fhip_channel_gate_forward", ("fhip_gate_route",), source="gate.hip check_shape; gate_apply_kernel's unsigned i ... i * 4u"),
    _side("gate", "fhip_squeeze_forward", ("fhip_squeeze_get_buffer_size", "fhip_gate_route"), source="gate.hip check_shape"),
    _side("gate", "fhip_gate_activation_forward", source="gate.hip check_shape; gate_activation_kernel's unsigned grid-stride loop"),
    Limit("fhip_excite_forward: n * c", "gate", "fhip_excite_forward", "elements of the mean / gate tensors (n * c)", I31, _E,
          lambda a: a["n"] * a["c"], dict(n=2 ** 15, c=2 ** 16, r=1), dict(n=1, c=I31, r=1), source="gate.hip excite_launch"),
    Limit("fhip_excite_forward: c * r", "gate", "fhip_excite_forward", "elements of a weight matrix (c * r)", I31, _E,
          lambda a: a["c"] * a["r"], dict(n=1, c=2 ** 16, r=2 ** 15), dict(n=1, c=I31, r=1), source="gate.hip excite_launch"),
    Limit("fhip_excite_forward: n", "gate", "fhip_excite_forward", "images (the grid's y dimension)", 65535, "65535",
          lambda a: a["n"], dict(n=65536, c=1, r=1), dict(n=65535, c=1, r=1), source="gate.hip excite_launch"),
    # ---- libfeather_inorm.so --------------------------------------------------------------------------------------------------------------------
    _side("inorm", "fhip_instance_norm_forward", ("fhip_instance_norm_get_buffer_size", "fhip_instance_norm_route"),
          source="inorm.hip check_shape; (unsigned)planes * nchunks"),
    _side("inorm", "fhip_instance_norm_forward_route", source="inorm.hip check_shape"),
    _side("inorm", "fhip_activation_forward", source="inorm.hip check_shape; activation_kernel's unsigned i ... i * 4u"),
    # ---- libfeather_shuffle.so ------------------------------------------------------------------------------------------------------------------
    _side("shuffle", "fhip_channel_shuffle_forward", ("fhip_channel_map_supported",),
          source="shuffle.hip check_shape; channel_map_kernel: base + 3 * stride < 2^31 + 2^21"),
    _side("shuffle", "fhip_channel_slice_forward", ("fhip_channel_map_supported",), source="shuffle.hip check_shape"),
    Limit("fhip_channel_map_create: rows", "shuffle", "fhip_channel_map_create", "output channels of all outputs together", 2 ** 24 - 1, "2^24",
          lambda a: sum(a["out_c"]), dict(out_c=(2 ** 22,) * 4), dict(out_c=(2 ** 22,) * 3 + (2 ** 22 - 1,)), source="shuffle.hip fhip_channel_map_create"),
    # ---- libfeather_deconv.so -------------------------------------------------------------------------------------------------------------------
    Limit("fhip_deconv_forward: elements", "deconv", "fhip_deconv_forward", "elements of the input or the output tensor", I31, _E, _conv_elements,
          conv(1, 1, 32, 64, batch=2 ** 20, deconv=True), conv(1, 1, 1, 1, batch=I31, deconv=True), source="deconv.hip fhip_deconv_forward"),
    Limit("fhip_deconv_forward: GEMM columns", "deconv", "fhip_deconv_forward", "GEMM columns of the MFMA route (batch * Hq * Wq)", 2 ** 30 - 1, "2^30",
          shadowed="the MFMA route needs 48 GEMM rows (24 output channels with paired phases), so the output has at least 48 elements per column "
                   "and the element limit refuses first: columns <= 2^31 / 48", source="deconv.hip fhip_deconv_forward"),
    Limit("fhip_deconv_init: packed floats", "deconv", "fhip_deconv_init", "floats of the packed filters", I31, "2^31 packed floats", _generic_packed,
          conv(2 ** 15, 2 ** 17, 1, 1, group=2, deconv=True), conv(2 ** 15, 2 ** 17 - 8, 1, 1, group=2, deconv=True), step=2 ** 17,
          source="deconv.hip fhip_deconv_init"),
    Limit("fhip_deconv_forward: channel chunks", "deconv", "fhip_deconv_forward", "chunks of 4 output channels over all groups (the grid's y dimension)",
          65535, "65535", _chunks, conv(1, 4 * 65536, 1, 1, deconv=True), conv(1, 4 * 65535, 1, 1, deconv=True), source="deconv.hip fhip_deconv_forward"),
    Limit("fhip_deconv_assign_output_dim: side", "deconv", "fhip_deconv_assign_output_dim", "output height or width", I31, "2^31",
          lambda a: max(out_hw(a)), conv(1, 1, 2 ** 30, 1, kh=2, kw=1, s=2, deconv=True), conv(1, 1, 2 ** 30, 1, kh=1, kw=1, s=2, deconv=True),
          queries=("fhip_deconv_supported",), source="deconv.hip check_geometry"),
    # ---- libfeather_gconv.so --------------------------------------------------------------------------------------------------------------------
    Limit("fhip_gconv_forward: lanes", "gconv", "fhip_gconv_forward", "lanes (batch * Ho * strips of the output row)", I31, "2^31 lanes", _columns,
          conv(4, 2, 32, 64, group=2, batch=2 ** 20), conv(4, 2, 1, 1, group=2, batch=I31), source="gconv.hip fhip_gconv_forward"),
    Limit("fhip_gconv_forward: channel chunks", "gconv", "fhip_gconv_forward", "chunks of output channels over all groups (the grid's y dimension)", 65535,
          "65535", _chunks, conv(4, 2 ** 18, 1, 1, group=2), conv(4, 2 ** 18 - 8, 1, 1, group=2), step=2, source="gconv.hip fhip_gconv_forward"),
    Limit("fhip_gconv_init: packed floats", "gconv", "fhip_gconv_init", "floats of the packed filters", I31, "2^31 packed floats", _generic_packed,
          conv(2 ** 15, 2 ** 17, 1, 1, group=2), conv(2 ** 15, 2 ** 17 - 8, 1, 1, group=2), step=2 ** 17, source="gconv.hip fhip_gconv_init"),
    # ---- libfeather_atrous.so -------------------------------------------------------------------------------------------------------------------
    Limit("fhip_atrous_supported: elements of one image", "atrous", "fhip_atrous_forward", "elements of one image of the input or the output (c * h * w)",
          I31, _E, _conv_elements, conv(2 ** 15, 1, 256, 256, dil=2), conv(I31, 1, 1, 1, dil=2),
          queries=("fhip_atrous_supported", "fhip_atrous_route", "fhip_atrous_get_buffer_size"), source="atrous.hip check_geometry"),
    Limit("fhip_atrous_forward: elements", "atrous", "fhip_atrous_forward", "elements of the input or the output tensor", I31, _E, _conv_elements,
          conv(1, 1, 32, 64, kh=3, kw=3, pads=(2, 2, 2, 2), dil=2, batch=2 ** 20), conv(1, 1, 1, 1, dil=2, batch=I31), source="atrous.hip do_forward"),
    Limit("fhip_atrous_forward_route: GEMM columns", "atrous", "fhip_atrous_forward_route", "GEMM columns of the MFMA route (batch * Ho * Wo)", 2 ** 30 - 1,
          "2^30", _columns, conv(16, 1, 1, 1, pads=(511, 512, 0, 0), dil=2, batch=2 ** 20, route=ATROUS_MFMA),
          conv(16, 1, 1, 1, pads=(511, 512, 0, 0), dil=2, batch=2 ** 20 - 1, route=ATROUS_MFMA), step=1024,
          source="atrous.hip do_forward (reached by name with fewer than 48 output channels; selected routes have 48 and the element limit refuses first)"),
    Limit("fhip_atrous_init: packed floats", "atrous", "fhip_atrous_init", "floats of the packed filters", I31, "2^31 packed floats", _generic_packed,
          conv(2 ** 15, 2 ** 17, 1, 1, group=2, dil=2), conv(2 ** 15, 2 ** 17 - 8, 1, 1, group=2, dil=2), step=2 ** 17, source="atrous.hip do_init"),
    Limit("fhip_atrous_forward: channel chunks", "atrous", "fhip_atrous_forward", "chunks of 4 output channels over all groups (the grid's y dimension)", 65535,
          "65535", _chunks, conv(1, 4 * 65536, 1, 1, dil=2), conv(1, 4 * 65535, 1, 1, dil=2), source="atrous.hip do_forward, generic route"),
    Limit("fhip_atrous_forward: depthwise plane", "atrous", "fhip_atrous_forward", "blocks of 256 lanes per output plane (Ho * ceil(Wo / 4) lanes)", 65535,
          "65535 blocks", lambda a: _blocks(out_hw(a)[0] * ((out_hw(a)[1] + 3) // 4)),
          conv(2, 2, 65535 * 256 + 1, 4, kh=3, kw=3, pads=(2, 2, 2, 2), dil=2, group=2), conv(2, 2, 65535 * 256, 4, kh=3, kw=3, pads=(2, 2, 2, 2), dil=2, group=2),
          source="atrous.hip do_forward, depthwise routes"),
    Limit("fhip_atrous_assign_output_dim: side", "atrous", "fhip_atrous_assign_output_dim", "output height or width", I31, "2^31",
          lambda a: max(out_hw(a)), conv(1, 1, 2 ** 30, 1, pads=(0, 0, 2 ** 30, 0), dil=2), conv(1, 1, 2 ** 30, 1, pads=(0, 0, 2 ** 30 - 1, 0), dil=2),
          source="atrous.hip fhip_atrous_assign_output_dim"),
    # ---- libfeather_canvas.so -------------------------------------------------------------------------------------------------------------------
    Limit("fhip_canvas_output_to_next_input: planes", "canvas", "fhip_canvas_output_to_next_input", "canvas planes (batch / 4 * output channels)", I31,
          "2^31 canvas planes", lambda a: a["batch"] // 4 * a["k"], dict(k=8, batch=2 ** 30), dict(k=7, batch=2 ** 30), step=2 ** 28,
          source="canvas.hip canvas_chain"),
    Limit("fhip_canvas_output_transform: output channels", "canvas", "fhip_canvas_output_transform", "output channels (the grid's y dimension)", 65535,
          "65535 output channels", lambda a: a["k"], dict(k=65536, batch=4), dict(k=65535, batch=4), code=UNSUPPORTED, source="canvas.hip canvas_output"),
    # ---- libfeather_pixout.so -------------------------------------------------------------------------------------------------------------------
    Limit("fhip_float_to_pixels: blocks", "pixout", "fhip_float_to_pixels", "blocks of 256 lanes (batch * target_h * lanes per row)", I31, "2^31 blocks",
          lambda a: _blocks(a["batch"] * a["h"] * a["w"]), dict(batch=2 ** 20, h=2 ** 19, w=1), dict(batch=2 ** 20, h=2 ** 19 - 1, w=1), step=4096,
          source="pixout.hip launch"),
    # ---- libfeather_hip.so: convolution routes ----------------------------------------------------------------------------------------------------
    Limit("fhip_conv_forward IM2COL: GEMM columns", "main", "fhip_conv_forward", "GEMM columns (batch * Ho * Wo), FHIP_IM2COL", COLS, "0x7fffff00", _columns,
          conv(4, 8, 1, 1, kh=3, kw=3, pads=(1, 1, 1, 1), batch=COLS + 1, algo=IM2COL), conv(4, 8, 1, 1, kh=3, kw=3, pads=(1, 1, 1, 1), batch=COLS, algo=IM2COL),
          queries=("fhip_conv_get_buffer_size",), source="implicit_gemm.hip igemm_forward: ntot > 0x7fffff00"),
    Limit("fhip_conv_forward NAIVE: GEMM columns", "main", "fhip_conv_forward", "GEMM columns (batch * Ho * Wo), FHIP_NAIVE", COLS, "0x7fffff00", _columns,
          conv(4, 8, 1, 1, kh=3, kw=3, pads=(1, 1, 1, 1), batch=COLS + 1, algo=NAIVE), conv(4, 8, 1, 1, kh=3, kw=3, pads=(1, 1, 1, 1), batch=COLS, algo=NAIVE),
          queries=("fhip_conv_get_buffer_size",), source="implicit_gemm.hip igemm_forward"),
    Limit("fhip_conv_forward IM2COL: pixel slots of a ragged 1x1", "main", "fhip_conv_forward", "GEMM columns as pixel slots (batch * 4 * ceil(Ho * Wo / 4))",
          COLS, "0x7fffff00", _slots, conv(8, 8, 1, 5, batch=(COLS + 8) // 8, algo=IM2COL), conv(8, 8, 1, 5, batch=COLS // 8, algo=IM2COL), step=8,
          queries=("fhip_conv_get_buffer_size",), source="implicit_gemm.hip igemm_forward: slots > 0x7fffff00"),
    Limit("fhip_conv_forward IM2COL: small-C tiles", "main", "fhip_conv_forward", "output tiles of the small-C kernel", I31, "2^31 output tiles",
          shadowed="a tile holds at least 4 outputs (rows are a multiple of 4 wide), so tiles <= columns / 4 < 2^29 once the column limit has passed",
          source="implicit_gemm.hip smallc_forward"),
    Limit("fhip_conv_forward_dw_pw: band work items", "main", "fhip_conv_forward_dw_pw", "work items of the band kernel (batch * row groups * channel blocks)",
          I31, "2^31 work items", shadowed="items <= batch * Ho <= columns / 112, and fhip_conv_can_fuse_dw_pw stops at 0x7fffff00 columns",
          source="implicit_gemm.hip dwpw_band_launch"),
    Limit("fhip_conv_can_fuse_dw_pw: GEMM columns", "main", "fhip_conv_forward_dw_pw", "GEMM columns of the pointwise layer (batch * Ho * Wo)", COLS,
          "0x7fffff00 GEMM columns", _columns, conv(16, 72, 64, 4, batch=2 ** 23), conv(16, 72, 64, 4, batch=2 ** 23 - 1), step=256, code=UNSUPPORTED,
          queries=("fhip_conv_can_fuse_dw_pw",), source="implicit_gemm.hip dwpw_applicable"),
    Limit("fhip_conv_can_fuse_siblings: GEMM columns", "main", "fhip_conv_forward_siblings", "GEMM columns of the two layers (batch * Ho * Wo)", COLS,
          "0x7fffff00 GEMM columns", _columns, conv(64, 128, 16, 16, batch=2 ** 23), conv(64, 128, 16, 16, batch=2 ** 23 - 1), step=256, code=UNSUPPORTED,
          queries=("fhip_conv_can_fuse_siblings",), source="implicit_gemm.hip igemm_twin_applicable"),
    Limit("fhip_conv_forward DEPTHWISE: planes", "main", "fhip_conv_forward", "planes (batch * channels)", I31, "2^31 planes", lambda a: a["batch"] * a["c"],
          conv(2, 2, 3, 3, kh=3, kw=3, pads=(1, 1, 1, 1), group=2, batch=2 ** 30, algo=DEPTHWISE),
          conv(1, 1, 3, 3, kh=3, kw=3, pads=(1, 1, 1, 1), group=1, batch=I31, algo=DEPTHWISE), queries=("fhip_conv_get_buffer_size",),
          source="depthwise.hip depthwise_forward"),
    Limit("fhip_conv_forward DEPTHWISE: chunks of planes", "main", "fhip_conv_forward", "chunks of small stride-2 planes", I31, "2^31 chunks",
          shadowed="a chunk holds at least one plane, and 2^31 planes are refused first", source="depthwise.hip depthwise_forward"),
    Limit("fhip_winograd_f63_plan: tiles", "main", "fhip_conv_forward", "Winograd tiles = GEMM columns (batch * tiles per image)", COLS, "0x7fffff00", _wino_tiles,
          conv(4, 4, 4, 4, kh=3, kw=3, pads=(1, 1, 1, 1), batch=COLS + 1, algo=WINO), conv(4, 4, 4, 4, kh=3, kw=3, pads=(1, 1, 1, 1), batch=COLS, algo=WINO),
          queries=("fhip_winograd_f63_plan", "fhip_conv_get_buffer_size"), source="winograd_f63.hip winograd_plan"),
    Limit("fhip_winograd_f63_input_transform: tiles", "main", "fhip_winograd_f63_input_transform", "Winograd tiles", COLS, "0x7fffff00", _wino_tiles,
          conv(4, 4, 4, 4, kh=3, kw=3, pads=(1, 1, 1, 1), batch=COLS + 1), conv(4, 4, 4, 4, kh=3, kw=3, pads=(1, 1, 1, 1), batch=COLS),
          source="winograd_f63.hip winograd_plan"),
    Limit("fhip_winograd_f63_tile_gemm: tiles", "main", "fhip_winograd_f63_tile_gemm", "Winograd tiles", COLS, "0x7fffff00", _wino_tiles,
          conv(4, 4, 4, 4, kh=3, kw=3, pads=(1, 1, 1, 1), batch=COLS + 1), conv(4, 4, 4, 4, kh=3, kw=3, pads=(1, 1, 1, 1), batch=COLS),
          source="winograd_f63.hip winograd_plan"),
    Limit("fhip_winograd_f63_output_transform: tiles", "main", "fhip_winograd_f63_output_transform", "Winograd tiles", COLS, "0x7fffff00", _wino_tiles,
          conv(4, 4, 4, 4, kh=3, kw=3, pads=(1, 1, 1, 1), batch=COLS + 1), conv(4, 4, 4, 4, kh=3, kw=3, pads=(1, 1, 1, 1), batch=COLS),
          source="winograd_f63.hip winograd_plan"),
    Limit("fhip_winograd_f63_input_transform: grid", "main", "fhip_winograd_f63_input_transform", "blocks of 256 (channel, tile) pairs", I31, "2^31 blocks",
          lambda a: _blocks(a["c"] * _wino_tiles(a)), conv(512, 4, 4, 4, kh=3, kw=3, pads=(1, 1, 1, 1), batch=2 ** 30),
          conv(512, 4, 4, 4, kh=3, kw=3, pads=(1, 1, 1, 1), batch=2 ** 30 - 1), step=2, source="winograd_f63.hip winograd_input_transform"),
    Limit("fhip_winograd_f63_output_to_next_input: planes", "main", "fhip_winograd_f63_output_to_next_input", "planes (batch * output channels)", I31,
          "2^31 planes", lambda a: a["batch"] * a["k"], conv(4, 2, 4, 4, kh=3, kw=3, pads=(1, 1, 1, 1), batch=2 ** 30),
          conv(4, 1, 4, 4, kh=3, kw=3, pads=(1, 1, 1, 1), batch=2 ** 30), step=2 ** 30, source="winograd_f63.hip winograd_output_to_next_input"),
    Limit("fhip_conv_can_fuse_first_winograd: input bytes", "main", "fhip_winograd_f63_input_from_first", "bytes of the RGB input (4 * batch * c * h * w)",
          2 ** 30 - 1, "2^30 input bytes", lambda a: 4 * a["batch"] * a["c"] * a["h"] * a["w"],
          conv(3, 64, 224, 224, kh=3, kw=3, pads=(1, 1, 1, 1), batch=1784), conv(3, 64, 224, 224, kh=3, kw=3, pads=(1, 1, 1, 1), batch=1783), step=4 * 3 * 224 * 224,
          code=UNSUPPORTED, queries=("fhip_conv_can_fuse_first_winograd",), source="winograd_f63.hip winograd_can_fuse_first: in_bytes < kWinoFirstOob (wino_first.h)"),
    Limit("fhip_conv_can_fuse_first_winograd: output channels", "main", "fhip_winograd_f63_input_from_first", "output channels of the first layer (the grid's y dimension)",
          65535, "65535 output channels", lambda a: a["k"], conv(3, 65536, 12, 12, kh=3, kw=3, pads=(1, 1, 1, 1), batch=1),
          conv(3, 65535, 12, 12, kh=3, kw=3, pads=(1, 1, 1, 1), batch=1), code=UNSUPPORTED, queries=("fhip_conv_can_fuse_first_winograd",),
          source="winograd_f63.hip winograd_can_fuse_first"),
    # route choices on 32-bit quantities: no refusal and no query -- past the value another kernel form runs, which computes the same
    Limit("winograd staged input: planes", "main", "fhip_winograd_f63_input_transform", "planes of the staged input transform (batch * input channels)", I31,
          "(route choice)", shadowed="not a refusal: from 2^31 planes on the direct input transform runs instead of the staged one; no query reports it, and no test runs either side",
          source="winograd_f63.hip winograd_input_staged: planes > 0x7fffffff"),
    Limit("first layer staged form: blocks", "main", "fhip_winograd_f63_input_from_first", "blocks of the staged form (blocks per image * batch)", I31,
          "(route choice)", shadowed="not a refusal: from 2^31 blocks on the direct form runs; unreachable below 2^30 input bytes (a block reads at least one "
                                     "image row): untested", source="winograd_f63.hip winograd_input_from_first: bpi * batch <= 0x7fffffff"),
    Limit("winograd persistent output: items", "main", "fhip_winograd_f63_output_transform", "work items of the persistent output transform", I31,
          "(route choice)", shadowed="not a refusal: from 2^31 items on the one-launch staged kernel runs instead of the persistent one; no query reports it, and no test runs either side",
          source="winograd_f63.hip winograd_output_transform: items <= 0x7fffffff"),
    Limit("depthwise band kernel: planes * 12", "main", "fhip_conv_forward", "floats of the 12-float filter copies the band kernel indexes (planes * 12)", I31,
          "(route choice)", shadowed="not a refusal: from 2^31 / 12 planes on the direct kernel runs instead of the band kernel.  Untested on both sides: the band kernel takes "
                                     "56- and 112-pixel planes only, and 1.8e8 of those are more than 2 TB",
          source="depthwise.hip depthwise_forward: planes * 12 <= 0x7fffffff"),
    # ---- libfeather_hip.so: layers ----------------------------------------------------------------------------------------------------------------
    Limit("fhip_relu: blocks, 4-byte aligned", "main", "fhip_relu", "blocks of 256 lanes (a lane per float)", I31, "2^31 blocks", lambda a: _blocks(_ew_lanes(a)),
          dict(count=I31 * 256 + 1, aligned=False), dict(count=I31 * 256, aligned=False), source="layers.hip ew_grid"),
    Limit("fhip_relu: blocks, 16-byte aligned", "main", "fhip_relu", "blocks of 256 lanes (a lane per float4)", I31, "2^31 blocks", lambda a: _blocks(_ew_lanes(a)),
          dict(count=4 * (I31 * 256 + 1), aligned=True), dict(count=4 * I31 * 256, aligned=True), source="layers.hip ew_grid"),
    Limit("fhip_add: blocks", "main", "fhip_add", "blocks of 256 lanes (a lane per float)", I31, "2^31 blocks", lambda a: _blocks(_ew_lanes(a)),
          dict(count=I31 * 256 + 1, aligned=False), dict(count=I31 * 256, aligned=False), source="layers.hip ew_grid"),
    Limit("fhip_affine: blocks", "main", "fhip_affine", "blocks of 256 lanes (batch * channels * hw floats, or float4s)", I31, "2^31 blocks",
          lambda a: _blocks(a["batch"] * a["c"] * a["hw"]), dict(batch=2 ** 20, c=2 ** 19, hw=1), dict(batch=2 ** 20, c=2 ** 19 - 1, hw=1), step=4096,
          source="layers.hip fhip_affine"),
    Limit("fhip_pixels_to_float: blocks", "main", "fhip_pixels_to_float", "blocks of 256 lanes (batch * channels * target_h * target_w floats, or float4s)", I31,
          "2^31 blocks", lambda a: _blocks(a["batch"] * a["h"] * a["w"]), dict(batch=2 ** 20, h=2 ** 19, w=1), dict(batch=2 ** 20, h=2 ** 19 - 1, w=1), step=4096,
          source="layers.hip launch_pixels"),
    Limit("fhip_pixel_images_plan: row bytes", "main", "fhip_pixel_images_plan", "bytes of one source row (w * channels)", I31, "2 GiB",
          lambda a: a["w"] * 4, dict(w=2 ** 29), dict(w=2 ** 29 - 1), step=4, source="layers.hip fhip_pixel_images_plan"),
    Limit("fhip_pooling: planes", "main", "fhip_pooling", "planes (batch * channels)", COLS, "0x7fffff00 planes", lambda a: a["batch"] * a["c"],
          dict(batch=COLS + 1, c=1, h=2, w=2), dict(batch=COLS, c=1, h=2, w=2),
          source="layers.hip fhip_pooling: the kernels' int planes, and grids that round the plane count up in int"),
    Limit("fhip_pooling: output plane", "main", "fhip_pooling", "elements of one output plane (oh * ow; padding can make it larger than the input's)", I31,
          "output plane too large: 2^31", lambda a: (a["h"] + 2 * a["pad"] - 1) * (a["w"] + 2 * a["pad"] - 1),
          dict(batch=1, c=1, h=2, w=2, pad=23170, k=2, s=1), dict(batch=1, c=1, h=1, w=2, pad=23170, k=2, s=1), step=46341,
          source="layers.hip fhip_pooling"),
    Limit("fhip_pooling: plane", "main", "fhip_pooling", "elements of one plane (h * w)", I31, "2^31 elements", lambda a: a["h"] * a["w"],
          dict(batch=1, c=1, h=2 ** 16, w=2 ** 15), dict(batch=1, c=1, h=I31, w=1), source="layers.hip fhip_pooling: yy * W + xx and H * W in int"),
]

LIMIT_IDS = [r.name for r in LIMITS]


def table():
    """(entry point, quantity, first refused value) of every row: what INTEGRATION.md lists."""
    return [(r.entry, r.quantity, r.max_ok + 1) for r in LIMITS]
