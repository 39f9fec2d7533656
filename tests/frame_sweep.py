"""One way to run the entry points of libfeather_frame.so on the device with every tensor between guards (tests/guarded.py): window() and
pixel_shuffle(), which tests/test_frame_gpu.py compares with tests/frame_ref.py, and sweep(), which walks the tables of tests/frame_cases.py so
that every instantiation of frame_cases.targets() is launched -- tests/frame_trace_child.py runs it under the kernel trace."""
import ctypes

import numpy as np

import frame_cases as C
import frame_ref as R
import side_contract
from guarded import Guarded, describe

F = np.float32
V = ctypes.c_void_p


def route(lib, what, a=0, w=0, b=0, out_w=0, aligned16=1):
    name = ctypes.create_string_buffer(128)
    assert lib.fhip_frame_route(what, a, w, b, out_w, aligned16, name, 128) == 0, lib.fhip_frame_last_error()
    return name.value.decode()


def _finish(buffers, out, shape):
    import torch
    torch.cuda.synchronize()
    for g in buffers:
        assert g.guards_intact() is None, describe(g.guards_intact())
    bits = out.bits().cpu().numpy().view(np.uint32).reshape(shape)  # read as words: a float copy could quiet a NaN
    return bits.view(F)


def window(lib, x, type_=0, value=0.0, per_channel=None, front=0, behind=0, top=0, bottom=0, left=0, right=0, offset=0):
    """-> the window of x from guarded buffers; the output starts as a pattern no case writes (a canary NaN), so every element is written
    iff it differs from it afterwards -- checked by the comparison with the restatement, which holds no such pattern."""
    n, c, h, w = x.shape
    oc, oh, ow = R.window_output_dim(c, h, w, front, behind, top, bottom, left, right)
    src, out = Guarded(x.size, x, offset), Guarded(n * oc * oh * ow, "poison", offset)
    pc = None if per_channel is None else Guarded(c, per_channel, offset)
    rc = lib.fhip_frame_window_forward(type_, ctypes.c_float(value), None if pc is None else V(pc.ptr), n, c, h, w, front, behind, top, bottom, left, right,
                                       V(out.ptr), V(src.ptr), side_contract.stream())
    assert rc == 0, lib.fhip_frame_last_error()
    got = _finish([src, out] + ([pc] if pc else []), out, (n, oc, oh, ow))
    assert out.unwritten() == 0, out.unwritten()
    return got


def pixel_shuffle(lib, x, r, mode=0, relu=0, slope=0.0, offset=0):
    n, c, h, w = x.shape
    C_, oh, ow = R.pixel_shuffle_output_dim(r, c, h, w)
    src, out = Guarded(x.size, x, offset), Guarded(x.size, "poison", offset)
    rc = lib.fhip_pixel_shuffle_forward(r, mode, relu, ctypes.c_float(slope), n, c, h, w, V(out.ptr), V(src.ptr), side_contract.stream())
    assert rc == 0, lib.fhip_frame_last_error()
    got = _finish([src, out], out, (n, C_, oh, ow))
    assert out.unwritten() == 0, out.unwritten()
    return got


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


# the cases the sweep walks: one per window instantiation (16-byte aligned buffers), and both PixelShuffle kernels
SWEEP_WINDOWS = ("const_3x5_left1", "const_1x1_all_sides", "rep_1x1_larger_than_plane", "rep_3x5_larger_than_plane", "ref_7x9_left1", "ref_3x5_dim_minus_1",
                 "crop_8x8_aligned", "crop_to_1x1")
SWEEP_SHUFFLES = ((4, 2, 0, (8, 8)), (2, 1, 1, (2, C.TILE // 2 + 1)))


def sweep(lib, seen):
    """Launches every instantiation once on small data, compared with the restatement as it goes; seen(route name) for each launch, in launch
    order."""
    for name in SWEEP_WINDOWS:
        x, kw, want = C.window_case(name)
        assert same_bits(window(lib, x, **kw), want), name
        seen(route(lib, C.WINDOW, kw["type_"], 0, int(C.window_pads(name)), want.shape[3], 1))
    for case in SWEEP_SHUFFLES:
        r, _, mode, (h, w) = case
        x = C.shuffle_input(case)
        assert same_bits(pixel_shuffle(lib, x, r, mode), R.pixel_shuffle(x, r, mode)), case
        seen(route(lib, C.SHUFFLE, r, w, h))
