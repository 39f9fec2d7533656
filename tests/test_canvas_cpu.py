"""The canvas plan without a GPU (libfeather_hip.so, host arithmetic only): it counts tiles per canvas.  What libfeather_canvas.so shares with
the other run-time libraries is in tests/test_side_contract_cpu.py."""
import ctypes
import os



def _built():
    from feathercnn_amd import _lib
    if not os.path.exists(_lib.canvas_path()):
        import __graft_entry__
        __graft_entry__.build()
    return _lib


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
