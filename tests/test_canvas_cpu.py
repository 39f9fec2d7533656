"""libfeather_canvas.so without a GPU: it exports exactly what include/feather_hip/feather_canvas.h declares and feathercnn_amd/_lib.py binds, shares no
symbol with the other libraries, and the canvas plan (libfeather_hip.so, host arithmetic only) counts tiles per canvas."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "feather_hip", "feather_canvas.h")


def _built():
    from feathercnn_amd import _lib
    if not os.path.exists(_lib.canvas_path()):
        import __graft_entry__
        __graft_entry__.build()
    return _lib


def test_header_exports_and_bindings_agree():
    _lib = _built()
    declared = sorted(set(re.findall(r"FHIP_CANVAS_API\s+[\w\s\*]+?\b(fhip_\w+)\s*\(", open(HEADER).read())))
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.canvas_path()], capture_output=True, text=True, check=True).stdout
    exported = sorted(set(re.findall(r" T (fhip_\w+)", out)))
    assert declared and declared == exported == sorted(_lib.CANVAS_SIGNATURES)
    others = (set(_lib.SIGNATURES) | set(_lib.PIXOUT_SIGNATURES) | set(_lib.GCONV_SIGNATURES) | set(_lib.DECONV_SIGNATURES) | set(_lib.INORM_SIGNATURES)
              | set(_lib.SHUFFLE_SIGNATURES))
    assert not set(declared) & others  # an application may load all seven
    lib = _lib.load_canvas_library()
    assert lib.fhip_canvas_last_error() == b""
    assert lib.fhip_canvas_output_transform(None, 4, None, None, None, None, 0, None) == -2  # FHIP_E_BADARG, no device call
    assert b"bad argument" in lib.fhip_canvas_last_error()


def test_canvas_plan_counts_tiles_per_canvas():
    _lib = _built()
    from feathercnn_amd import ConvParam
    lib = _lib.load_library()
    for h, tiles, plain in ((14, 5, 3), (56, 19, 10)):
        prm = ConvParam(output_channels=512, input_channels=512, input_h=h, input_w=h, kernel_h=3, kernel_w=3, stride_h=1, stride_w=1, pad_left=1,
                        pad_right=1, pad_top=1, pad_bottom=1, group=1, bias_term=True, activation=1)
        prm.AssignOutputDim()
        c, pl, q = prm._c(), _lib.fhip_winograd_plan(), _lib.fhip_conv_param()
        assert lib.fhip_winograd_f63_plan_canvas(ctypes.byref(c), 32, 2, ctypes.byref(pl)) == 0
        assert (pl.tiles_x, pl.tiles_y, pl.tiles_per_image, pl.columns) == (tiles, tiles, tiles * tiles, 8 * tiles * tiles)
        assert lib.fhip_winograd_f63_plan_canvas(ctypes.byref(c), 32, 1, ctypes.byref(pl)) == 0 and pl.columns == 32 * plain * plain
        assert lib.fhip_winograd_f63_canvas_param(ctypes.byref(c), 32, ctypes.byref(q)) == 0
        assert (q.input_h, q.input_w, q.output_h, q.output_w, q.input_channels, q.pad_left) == (2 * h + 2, 2 * h + 2, 2 * h + 2, 2 * h + 2, 512, 1)
        for n in (5, 6, 30):
            assert lib.fhip_winograd_f63_plan_canvas(ctypes.byref(c), n, 2, ctypes.byref(pl)) == -1  # FHIP_E_UNSUPPORTED
        assert lib.fhip_winograd_f63_plan_canvas(ctypes.byref(c), 32, 3, ctypes.byref(pl)) == -2
    for h in (28, 112, 224, 8, 13, 26, 38, 50):
        prm = ConvParam(output_channels=8, input_channels=8, input_h=h, input_w=h, kernel_h=3, kernel_w=3, stride_h=1, stride_w=1, pad_left=1,
                        pad_right=1, pad_top=1, pad_bottom=1, group=1, bias_term=True, activation=1)
        prm.AssignOutputDim()
        c, pl = prm._c(), _lib.fhip_winograd_plan()
        assert lib.fhip_winograd_f63_plan_canvas(ctypes.byref(c), 32, 2, ctypes.byref(pl)) == -1, h
