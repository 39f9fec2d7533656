"""Every size limit of tests/limit_cases.py, without a GPU: the entry point refuses the first value past its limit with its code and a message
that names the limit, before any device access (the pointers are made up and this test runs on a machine without a device); the launch-free
queries of the entry point accept one step below and refuse at the limit; the table's own arithmetic puts the two argument sets where it
says; the first-layer fusion of VGG-16's conv1_1 changes form and stops where the sources say; and INTEGRATION.md lists every row."""
import ctypes
import os
import re

import pytest

import limit_cases as LC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V = ctypes.c_void_p
OUT, IN, PACKED, BUF, BIAS, AUX = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000  # made-up device addresses, 16-byte aligned
GRAY, RGBA2RGB = 1 << 2, (1 << 3) | (1 << 16)
CALLABLE = [r for r in LC.LIMITS if not r.shadowed]


@pytest.fixture(scope="module")
def libs():
    from feathercnn_amd import _lib as L
    return {"main": (L.load_library(), "fhip_last_error"), "gate": (L.load_gate_library(), "fhip_gate_last_error"),
            "inorm": (L.load_inorm_library(), "fhip_inorm_last_error"), "shuffle": (L.load_shuffle_library(), "fhip_shuffle_last_error"),
            "deconv": (L.load_deconv_library(), "fhip_deconv_last_error"), "gconv": (L.load_gconv_library(), "fhip_gconv_last_error"),
            "atrous": (L.load_atrous_library(), "fhip_atrous_last_error"), "canvas": (L.load_canvas_library(), "fhip_canvas_last_error"),
            "pixout": (L.load_pixout_library(), "fhip_pixout_last_error")}


def _fit(v):
    return min(v, LC.I31)  # a side past int never reaches a struct: the checks compute it themselves


def _param(a, cls=None, **extra):
    from feathercnn_amd import _lib as L
    oh, ow = LC.out_hw(a)
    pl, pr, pt, pb = a["pads"]
    return (cls or L.fhip_conv_param)(output_channels=a["k"], input_channels=a["c"], input_h=a["h"], input_w=a["w"], kernel_h=a["kh"], kernel_w=a["kw"],
                                      output_h=_fit(oh), output_w=_fit(ow), stride_h=a["s"], stride_w=a["s"], pad_left=pl, pad_bottom=pb, pad_right=pr,
                                      pad_top=pt, group=a["group"], bias_term=0, activation=0, **extra)


def _deconv(a):
    from feathercnn_amd import _lib as L
    return _param(a, L.fhip_deconv_param, output_pad_right=0, output_pad_bottom=0)


def _atrous(a):
    from feathercnn_amd import _lib as L
    return _param(a, L.fhip_atrous_param, dilation_h=a["dil"], dilation_w=a["dil"])


def _pair(a):
    """(3x3 / pad-1 first layer, the 3x3 / pad-1 layer behind it) of an argument set: a["c"] -> a["k"] -> 8 channels."""
    nxt = LC.conv(a["k"], 8, a["h"], a["w"], kh=3, kw=3, pads=(1, 1, 1, 1))
    return _param(a), _param(nxt)


def _dw_pw(a):
    dw = LC.conv(a["c"], a["c"], a["h"], a["w"], kh=3, kw=3, pads=(1, 1, 1, 1), group=a["c"])
    return _param(dw), _param(a)


def _siblings(a):
    return _param(a), _param(dict(a, k=32))


def _canvas_plan(columns):
    from feathercnn_amd import _lib as L
    return L.fhip_winograd_plan(tiles_x=1, tiles_y=1, tiles_per_image=1, columns=columns, columns_padded=columns, column_block=columns, frequency_points=64,
                                tile_outputs=6)


def _pool(a):
    from feathercnn_amd import _lib as L
    pad, s = a.get("pad", 0), a.get("s", 2)
    return L.fhip_pool_param(channels=a["c"], input_h=a["h"], input_w=a["w"], kernel_h=2, kernel_w=2, stride_h=s, stride_w=s, pad_left=pad, pad_right=pad,
                             pad_top=pad, pad_bottom=pad, pooling_type=0, global_pooling=0)


def _image(a):
    from feathercnn_amd import _lib as L
    return L.fhip_pixel_image(data=IN, w=a["w"], h=2, stride=0)


def _sizes():
    return ctypes.byref(ctypes.c_size_t()), ctypes.byref(ctypes.c_size_t())


B = ctypes.byref
_EW = lambda a: (OUT, IN) if a["aligned"] else (OUT + 4, IN + 4)  # noqa: E731

# entry point -> the call, with made-up addresses
CALL = {
    "fhip_channel_gate_forward": lambda l, a: l.fhip_channel_gate_forward(a["n"], a["c"], a["h"], a["w"], V(OUT), V(IN), V(AUX), None, 0, None),
    "fhip_squeeze_forward": lambda l, a: l.fhip_squeeze_forward(a["n"], a["c"], a["h"], a["w"], V(OUT), V(IN), V(BUF), None),
    "fhip_gate_activation_forward": lambda l, a: l.fhip_gate_activation_forward(0, V(OUT), V(IN), a["n"], a["c"], a["h"] * a["w"], 0.0, 0.0, None),
    "fhip_excite_forward": lambda l, a: l.fhip_excite_forward(a["n"], a["c"], a["r"], V(OUT), V(IN), V(PACKED), None, V(AUX), None, 1, 0, 0.0, 0.0, None),
    "fhip_instance_norm_forward": lambda l, a: l.fhip_instance_norm_forward(a["n"], a["c"], a["h"], a["w"], V(OUT), V(IN), None, None, 1e-5, 0, 0.0, V(BUF), None),
    "fhip_instance_norm_forward_route": lambda l, a: l.fhip_instance_norm_forward_route(3, a["n"], a["c"], a["h"], a["w"], V(OUT), V(IN), None, None, 1e-5, 0, 0.0,
                                                                                       V(BUF), None),
    "fhip_activation_forward": lambda l, a: l.fhip_activation_forward(1, V(OUT), V(IN), a["n"], a["c"], a["h"] * a["w"], 0.1, 0.0, V(AUX), None),
    "fhip_channel_shuffle_forward": lambda l, a: l.fhip_channel_shuffle_forward(V(OUT), V(IN), a["n"], a["c"], a["h"], a["w"], 1, 0, None),
    "fhip_channel_slice_forward": lambda l, a: l.fhip_channel_slice_forward((V * 1)(OUT), V(IN), a["n"], a["c"], a["h"], a["w"], (ctypes.c_int * 1)(-233), 1, None),
    "fhip_channel_map_create": lambda l, a: l.fhip_channel_map_create(B(V()), (ctypes.c_int * 1)(1), 1, (ctypes.c_int * 4)(*a["out_c"]), 4, (ctypes.c_int * 2)(0, 0)),
    "fhip_deconv_forward": lambda l, a: l.fhip_deconv_forward(B(_deconv(a)), a["batch"], V(OUT), V(IN), V(PACKED), None, None, None),
    "fhip_deconv_init": lambda l, a: l.fhip_deconv_init(B(_deconv(a)), V(PACKED), V(IN), None),
    "fhip_deconv_assign_output_dim": lambda l, a: l.fhip_deconv_assign_output_dim(B(_deconv(a))),
    "fhip_gconv_forward": lambda l, a: l.fhip_gconv_forward(B(_param(a)), a["batch"], V(OUT), V(IN), V(PACKED), None, None, None),
    "fhip_gconv_init": lambda l, a: l.fhip_gconv_init(B(_param(a)), V(PACKED), V(IN), None),
    "fhip_atrous_forward": lambda l, a: l.fhip_atrous_forward(B(_atrous(a)), a["batch"], V(OUT), V(IN), V(PACKED), None, None, None),
    "fhip_atrous_forward_route": lambda l, a: l.fhip_atrous_forward_route(B(_atrous(a)), a["batch"], V(OUT), V(IN), V(PACKED), None, None, None, a["route"].encode()),
    "fhip_atrous_init": lambda l, a: l.fhip_atrous_init(B(_atrous(a)), V(PACKED), V(IN), None),
    "fhip_atrous_assign_output_dim": lambda l, a: l.fhip_atrous_assign_output_dim(B(_atrous(a))),
    "fhip_canvas_output_to_next_input": lambda l, a: l.fhip_canvas_output_to_next_input(
        2, B(_param(LC.conv(8, a["k"], 2, 2, kh=3, kw=3, pads=(1, 1, 1, 1)))), B(_param(LC.conv(a["k"], 8, 2, 2, kh=3, kw=3, pads=(1, 1, 1, 1)))), a["batch"],
        B(_canvas_plan(a["batch"] // 4)), B(_canvas_plan(a["batch"] // 4)), V(OUT), V(IN), None, None),
    "fhip_canvas_output_transform": lambda l, a: l.fhip_canvas_output_transform(
        B(_param(LC.conv(8, a["k"], 2, 2, kh=3, kw=3, pads=(1, 1, 1, 1)))), a["batch"], B(_canvas_plan(a["batch"] // 4)), V(OUT), V(IN), None, 0, None),
    "fhip_float_to_pixels": lambda l, a: l.fhip_float_to_pixels(V(OUT + 1), 0, V(IN), a["batch"], GRAY, a["w"], a["h"], a["w"], a["h"], None, None, None),
    "fhip_conv_forward": lambda l, a: l.fhip_conv_forward(B(_param(a)), a["algo"], a["batch"], V(OUT), V(IN), V(PACKED), V(BUF), None, None),
    "fhip_conv_forward_dw_pw": lambda l, a: l.fhip_conv_forward_dw_pw(B(_dw_pw(a)[0]), B(_dw_pw(a)[1]), a["batch"], V(OUT), V(IN), V(PACKED), None, V(AUX), None, None),
    "fhip_conv_forward_siblings": lambda l, a: l.fhip_conv_forward_siblings(B(_siblings(a)[0]), B(_siblings(a)[1]), a["batch"], V(OUT), V(BUF), V(IN), V(PACKED), None,
                                                                           None),
    "fhip_winograd_f63_input_transform": lambda l, a: l.fhip_winograd_f63_input_transform(B(_param(a)), a["batch"], V(BUF), V(IN), None),
    "fhip_winograd_f63_tile_gemm": lambda l, a: l.fhip_winograd_f63_tile_gemm(B(_param(a)), a["batch"], V(BUF), V(PACKED), V(IN), None),
    "fhip_winograd_f63_output_transform": lambda l, a: l.fhip_winograd_f63_output_transform(B(_param(a)), a["batch"], V(OUT), V(BUF), None, None),
    "fhip_winograd_f63_output_to_next_input": lambda l, a: l.fhip_winograd_f63_output_to_next_input(
        B(_param(a)), B(_param(LC.conv(a["k"], 4, a["h"], a["w"], kh=3, kw=3, pads=(1, 1, 1, 1)))), a["batch"], V(OUT), V(BUF), None, 0, None),
    "fhip_winograd_f63_input_from_first": lambda l, a: l.fhip_winograd_f63_input_from_first(B(_pair(a)[0]), B(_pair(a)[1]), a["batch"], V(BUF), V(IN), V(PACKED), None,
                                                                                           None),
    "fhip_relu": lambda l, a: l.fhip_relu(V(_EW(a)[0]), V(_EW(a)[1]), a["count"], None),
    "fhip_add": lambda l, a: l.fhip_add(V(_EW(a)[0]), V(_EW(a)[1]), V(_EW(a)[1]), a["count"], 1, None),
    "fhip_affine": lambda l, a: l.fhip_affine(V(OUT), V(IN), V(AUX), V(BIAS), a["batch"], a["c"], a["hw"], 0, None),
    "fhip_pixels_to_float": lambda l, a: l.fhip_pixels_to_float(V(OUT), V(IN), a["batch"], GRAY, a["w"], a["h"], a["w"], a["h"], None, None, None),
    "fhip_pixel_images_plan": lambda l, a: l.fhip_pixel_images_plan(B(_image(a)), 1, RGBA2RGB, 2, 2, None, B(ctypes.c_size_t())),
    "fhip_pooling": lambda l, a: l.fhip_pooling(B(_pool(a)), a["batch"], V(OUT), V(IN), None),
}
HOST_ONLY = {"fhip_deconv_assign_output_dim", "fhip_atrous_assign_output_dim", "fhip_pixel_images_plan"}  # launch-free themselves: called on both sides

_NAME = lambda: ctypes.create_string_buffer(200)  # noqa: E731
# query -> True when it accepts the argument set
QUERY = {
    "fhip_gate_route": lambda l, a: l.fhip_gate_route(0, a["n"], a["c"], a["h"], a["w"], V(OUT), V(IN), None, _NAME(), 200) == 0,
    "fhip_squeeze_get_buffer_size": lambda l, a: l.fhip_squeeze_get_buffer_size(a["n"], a["c"], a["h"], a["w"], _sizes()[0]) == 0,
    "fhip_instance_norm_get_buffer_size": lambda l, a: l.fhip_instance_norm_get_buffer_size(a["n"], a["c"], a["h"], a["w"], _sizes()[0]) == 0,
    "fhip_instance_norm_route": lambda l, a: l.fhip_instance_norm_route(a["n"], a["c"], a["h"], a["w"], V(OUT), V(IN), _NAME(), 200) == 0,
    "fhip_channel_map_supported": lambda l, a: l.fhip_channel_map_supported(a["n"], a["c"], a["h"], a["w"]) == 0,
    "fhip_deconv_supported": lambda l, a: l.fhip_deconv_supported(B(_deconv(a))) == 1,
    "fhip_atrous_supported": lambda l, a: l.fhip_atrous_supported(B(_atrous(a))) == 1,
    "fhip_atrous_route": lambda l, a: l.fhip_atrous_route(B(_atrous(a)), _NAME(), 200) == 0,
    "fhip_atrous_get_buffer_size": lambda l, a: l.fhip_atrous_get_buffer_size(B(_atrous(a)), a["batch"], *_sizes()) == 0,
    "fhip_conv_get_buffer_size": lambda l, a: l.fhip_conv_get_buffer_size(B(_param(a)), a["algo"], a["batch"], *_sizes()) == 0,
    "fhip_winograd_f63_plan": lambda l, a: l.fhip_winograd_f63_plan(B(_param(a)), a["batch"], B(_plan_struct())) == 0,
    "fhip_conv_can_fuse_dw_pw": lambda l, a: l.fhip_conv_can_fuse_dw_pw(B(_dw_pw(a)[0]), B(_dw_pw(a)[1]), a["batch"]) == 1,
    "fhip_conv_can_fuse_siblings": lambda l, a: l.fhip_conv_can_fuse_siblings(B(_siblings(a)[0]), LC.IM2COL, B(_siblings(a)[1]), LC.IM2COL, a["batch"]) == 1,
    "fhip_conv_can_fuse_first_winograd": lambda l, a: l.fhip_conv_can_fuse_first_winograd(B(_pair(a)[0]), B(_pair(a)[1]), LC.WINO, a["batch"]) == 1,
}


def _plan_struct():
    from feathercnn_amd import _lib as L
    return L.fhip_winograd_plan()


def test_the_table_puts_its_argument_sets_where_it_says():
    """Python integers, no library: `refuse` is the first value past the limit the dimensions can form, `accept` is within it."""
    assert len(set(LC.LIMIT_IDS)) == len(LC.LIMITS) >= 50
    for r in LC.LIMITS:
        assert r.source and r.word and r.quantity, r.name
        if r.shadowed:
            assert r.refuse is None and r.accept is None, r.name
            continue
        assert r.entry in CALL, r.name
        at, below = r.measure(r.refuse), r.measure(r.accept)
        assert below <= r.max_ok < at and at - r.step <= r.max_ok, (r.name, below, at)
        if r.step == 1:
            assert at == r.max_ok + 1, (r.name, at)
        assert all(q in QUERY for q in r.queries), r.name


@pytest.mark.parametrize("row", CALLABLE, ids=[r.name for r in CALLABLE])
def test_refused_at_the_limit_before_any_device_access(libs, row):
    lib, last_error = libs[row.lib]
    err = lambda: getattr(lib, last_error)().decode()  # noqa: E731
    rc = CALL[row.entry](lib, row.refuse)
    assert rc == row.code, (rc, err())
    assert row.word in err(), err()
    if row.entry in HOST_ONLY:
        assert CALL[row.entry](lib, row.accept) == 0, err()
    for q in row.queries:
        assert QUERY[q](lib, row.accept), (q, "refuses one step below the limit", err())
        assert not QUERY[q](lib, row.refuse), (q, "accepts what the entry point refuses")


def test_first_layer_fusion_boundaries_of_vgg16(libs):
    """conv1_1 inside conv1_2's input transform (wino_first.h) at 3 x 224 x 224: it fuses while the input stays below 2^30 bytes (which is what
    lets q.in_bytes be an unsigned), and V passes 2 GiB, where the shared-column form's buffer stores give way to plain stores, between batch 90
    and 91 -- the two batches tests/test_large_routes_gpu.py runs.  An image is 4 * 3 * 224 * 224 = 602 112 bytes, so batch 1782 (1 072 963 584
    bytes) and batch 1783 (1 073 565 696 bytes) are both below 2^30 = 1 073 741 824 and fuse; batch 1784 (1 074 167 808 bytes) is the first that
    does not."""
    from feathercnn_amd import _lib as L
    lib = libs["main"][0]
    a = LC.conv(3, 64, 224, 224, kh=3, kw=3, pads=(1, 1, 1, 1))
    first, nxt = _param(a), _param(LC.conv(64, 64, 224, 224, kh=3, kw=3, pads=(1, 1, 1, 1)))
    fuse = lambda n: lib.fhip_conv_can_fuse_first_winograd(B(first), B(nxt), LC.WINO, n)  # noqa: E731
    last = (2 ** 30 - 1) // (4 * 3 * 224 * 224)  # the last batch whose input is below 2^30 bytes
    assert last == 1783 and 4 * last * 3 * 224 * 224 < 2 ** 30 <= 4 * (last + 1) * 3 * 224 * 224
    assert (fuse(1), fuse(1782), fuse(last), fuse(last + 1)) == (1, 1, 1, 0)
    v = {}
    for n in (90, 91):
        pl = L.fhip_winograd_plan()
        assert lib.fhip_winograd_f63_plan(B(nxt), n, B(pl)) == 0
        v[n] = pl.v_bytes
        assert pl.tiles_per_image == 38 * 38 and pl.v_bytes == 64 * 64 * 4 * pl.columns_padded
    assert v[90] <= 2 ** 31 < v[91], v  # <= 0x80000000 shares columns through buffer stores; above it the plain-store form


def test_integration_md_lists_every_row():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    section = text[text.index("## Size limits"):]
    section = section[:section.index("\n## ", 5)] if "\n## " in section[5:] else section
    rows = [tuple(c.strip() for c in line.strip().strip("|").split("|")) for line in section.splitlines() if line.startswith("| `")]
    want = [(f"`{e}`", q, str(v)) for e, q, v in LC.table()]
    assert [r[:3] for r in rows] == want
    # each header states the limit next to the function
    heads = {n: open(os.path.join(ROOT, "include", "feather_hip", n)).read() for n in os.listdir(os.path.join(ROOT, "include", "feather_hip"))}
    for r in LC.LIMITS:
        assert any(re.search(r"\b" + r.entry + r"\b", h) for h in heads.values()), r.entry
    for name, word in (("feather_gate.h", "2^31 elements"), ("feather_inorm.h", "2^31 elements"), ("feather_shuffle.h", "2^31 elements"),
                       ("feather_deconv.h", "2^31 elements"), ("feather_gconv.h", "2^31 lanes"), ("feather_atrous.h", "2^30 GEMM columns"),
                       ("feather_canvas.h", "2^31 canvas planes"), ("feather_pixout.h", "2^31 blocks"), ("feather_hip.h", "0x7fffff00"),
                       ("feather_net.h", "2^31 planes"), ("feather_net.h", "2^31 blocks")):
        assert word in heads[name], (name, word)
