"""The tables of the framing-layer tests (tests/test_frame_cpu.py, tests/test_frame_gpu.py, tests/test_frame_contract_cpu.py): the kernel
instantiations of libfeather_frame.so, the window and PixelShuffle cases and the inputs of the net-level tests.

Shapes are the smallest at which the kernels can still go wrong.  A window lane owns 4 output pixels of a row: rows of 1, 5, 9 and 13
pixels end in a ragged lane and take scalar stores, rows of 8 and 12 take the vector store; left margins of 0, 1 and 4 make the source run
of an interior lane aligned and misaligned.  n = 2 and c = 3 everywhere, so every index has more than one image and plane behind it.
tests/test_frame_cpu.py holds the restatement to np.pad / torch on exactly these inputs; the GPU tests compare bit patterns with it."""
import functools
import os

import numpy as np

import frame_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "feathercnn_amd", "libfeather_frame.so")
F = np.float32
TILE, TILE_MIN = R.TILE, 1024  # FHIP_FRAME_TILE, FHIP_FRAME_TILE_MIN
WINDOW, SHUFFLE = 0, 1  # fhip_frame_op
NAN_PAYLOAD = 0x7FC12345  # a quiet NaN with a payload: `value` travels as bits

KERNELS = {"window_kernel", "pixel_shuffle_tile_kernel", "pixel_shuffle_direct_kernel"}


def window_target(type_, pad, out_w, aligned16=True):
    """The name fhip_frame_route gives a window: T is the type where some margin is positive, else 3; V where the row is a multiple of 4 and
    `out` 16-byte aligned."""
    return "fhip::window_kernel<%d, %d>" % (type_ if pad else 3, 1 if out_w % 4 == 0 and aligned16 else 0)


def targets():
    """Every instantiation of the library, by the names fhip_frame_route reports."""
    return {"fhip::window_kernel<%d, %d>" % (t, v) for t in range(4) for v in range(2)} | {"fhip::pixel_shuffle_tile_kernel", "fhip::pixel_shuffle_direct_kernel"}


def planted(shape, seed):
    """U(-1, 1) with a few NaN (one with a payload), inf and -0.0 elements planted: a bit copy must carry them."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1, 1, shape).astype(F)
    flat = x.reshape(-1).view(np.uint32)
    spots = rng.choice(flat.size, size=min(5, flat.size), replace=False)
    for k, bits in zip(spots, (0x7FC00000, NAN_PAYLOAD, 0x7F800000, 0xFF800000, 0x80000000)):
        flat[k] = bits
    return x


# name -> ((h, w), type, (front, behind, top, bottom, left, right), value bits or None, per-channel?)   -- n = 2, c = 3
def _w(plane, type_, margins, value=None, per_channel=False):
    return (plane, type_, margins, value, per_channel)


ZERO, HALF, MINUS_ZERO = 0x00000000, 0x3F000000, 0x80000000
WINDOWS = {
    # constant
    "const_1x1_all_sides": _w((1, 1), 0, (0, 0, 1, 2, 3, 1), HALF),                  # a plane of one pixel, a row of 5
    "const_3x5_left1": _w((3, 5), 0, (0, 0, 1, 1, 1, 2), ZERO),                       # row of 8: vector stores, misaligned source runs
    "const_7x9_left0_right_only": _w((7, 9), 0, (0, 0, 0, 2, 0, 3), MINUS_ZERO),      # margins on some sides only; row of 12, value -0.0
    "const_8x8_left4": _w((8, 8), 0, (0, 0, 2, 0, 4, 0), NAN_PAYLOAD),                # aligned source runs, value NaN with a payload; row of 12
    "const_4x12_left1_scalar": _w((4, 12), 0, (0, 0, 0, 1, 1, 0), HALF),              # row of 13: scalar stores
    "const_channels": _w((3, 5), 0, (1, 2, 0, 0, 0, 0), HALF),                        # channel pad alone
    "const_channels_per_channel": _w((7, 9), 0, (1, 2, 1, 0, 2, 1), HALF, True),      # channel pad + per-channel values; row of 12
    "const_per_channel": _w((8, 8), 0, (0, 0, 1, 1, 1, 0), ZERO, True),               # row of 9
    "const_pad_left_crop_right": _w((8, 8), 0, (0, 0, 2, -3, 3, -3), HALF),           # one side padded, the opposite cropped; row of 8
    "const_crop_channel_pad_rows": _w((4, 12), 0, (-1, 0, 1, 1, -4, 0), HALF),        # a cropped channel, padded rows; row of 8
    # replicate
    "rep_1x1_larger_than_plane": _w((1, 1), 1, (0, 0, 3, 2, 4, 3)),                   # every output pixel is the one input pixel; row of 8
    "rep_3x5_larger_than_plane": _w((3, 5), 1, (0, 0, 5, 4, 7, 6)),                   # row of 18
    "rep_7x9_left1": _w((7, 9), 1, (0, 0, 0, 1, 1, 2)),                               # row of 12
    "rep_8x8_left4": _w((8, 8), 1, (0, 0, 1, 0, 4, 1)),                               # row of 13
    "rep_pad_top_crop_bottom": _w((8, 8), 1, (0, 0, 2, -5, -1, 1)),                   # row of 8
    # reflect
    "ref_3x5_dim_minus_1": _w((3, 5), 2, (0, 0, 2, 2, 4, 4)),                         # the largest reflect pad; row of 13
    "ref_7x9_left1": _w((7, 9), 2, (0, 0, 3, 0, 1, 2)),                               # row of 12
    "ref_8x8_left4": _w((8, 8), 2, (0, 0, 0, 7, 4, 0)),                               # row of 12, aligned runs
    "ref_4x12_left0": _w((4, 12), 2, (0, 0, 1, 1, 0, 3)),                             # row of 15
    "ref_pad_left_crop_right": _w((8, 8), 2, (-1, -1, 1, 1, 5, -5)),                  # a single channel left; row of 8
    # crop only: no border, whatever the type says
    "crop_to_1x1": _w((7, 9), 0, (-1, -1, -3, -3, -4, -4)),
    "crop_8x8_aligned": _w((8, 8), 1, (0, 0, -2, -1, -4, 0)),                         # row of 4: vector stores and loads
    "crop_4x12_left1": _w((4, 12), 2, (0, -1, 0, -1, -1, -3)),                        # row of 8: vector stores, misaligned loads
    "crop_4x12_scalar": _w((4, 12), 0, (0, 0, -1, 0, -2, -1)),                        # row of 9
    "copy_3x5": _w((3, 5), 0, (0, 0, 0, 0, 0, 0)),                                    # all margins 0 through the C-ABI: a copy
}


@functools.lru_cache(maxsize=None)
def window_case(name):
    """-> (x, kwargs of R.window, want) of a case; per_channel values and the value's bits included."""
    (h, w), type_, (f, b, t, bo, l, r), value, pc = WINDOWS[name]
    seed = sorted(WINDOWS).index(name)
    x = planted((2, 3, h, w), 100 + seed)
    kw = dict(type_=type_, value=np.asarray([value or 0], np.uint32).view(F)[0], front=f, behind=b, top=t, bottom=bo, left=l, right=r)
    if pc:
        kw["per_channel"] = planted((3,), 300 + seed)
    want = R.window(x, **kw)
    want.setflags(write=False)
    return x, kw, want


def window_pads(name):
    return any(m > 0 for m in WINDOWS[name][2])


# (r, C, mode, (h, w)): the small planes, both modes; then the tile's edge at h = 2 -- r * w just under, at and just over FHIP_FRAME_TILE
SHUFFLES = [(r, C, mode, plane) for r in (2, 3, 4) for C in (1, 2) for mode in (0, 1) for plane in ((1, 1), (3, 5), (8, 8))] + \
           [(2, 1, 0, (2, TILE // 2 - 1)), (2, 2, 1, (2, TILE // 2)), (2, 1, 1, (2, TILE // 2 + 1)), (3, 1, 0, (2, TILE // 3)), (3, 1, 1, (2, TILE // 3 + 1)),
            (4, 1, 0, (2, TILE // 4)), (4, 1, 1, (2, TILE // 4 + 1)), (1, 3, 0, (3, 5)), (2, 2, 0, (40, 300))]
RELUS = [(R.RELU_NONE, 0.0), (R.RELU_SLOPE, 0.0), (R.RELU_SLOPE, 0.2), (R.RELU_PLAIN, 0.0)]


def shuffle_id(c):
    return "r%d-C%d-mode%d-%dx%d" % (c[0], c[1], c[2], c[3][0], c[3][1])


@functools.lru_cache(maxsize=None)
def shuffle_input(case):
    r, C, mode, (h, w) = case
    return planted((2, C * r * r, h, w), 500 + SHUFFLES.index(case))  # shared among the tests, which leave it unchanged


def shuffle_target(r, w, h):
    """The tile kernel where an output row fits the tile and a block moves TILE_MIN elements or more (feather_frame.h)."""
    tiled = r > 1 and r * w <= TILE and min(h * r, TILE // (r * w)) * r * w >= TILE_MIN
    return "fhip::pixel_shuffle_tile_kernel" if tiled else "fhip::pixel_shuffle_direct_kernel"


# ---- net level -------------------------------------------------------------------------------------------------------------------------
FRAME_TOPS = ("pad_reflect", "pad_same", "ps0", "pad_rep", "crop_one", "pad_pc", "ps1", "crop_b", "pad_ch", "crop_ref")


@functools.lru_cache(maxsize=None)
def net_model():
    """-> ((param, bin, input, output), the trace for model_zoo.numpy_forward) of tiny_frame."""
    from feathercnn_amd import model_zoo
    trace = []
    return model_zoo.tiny_frame(trace=trace), trace


@functools.lru_cache(maxsize=None)
def net_input(batch=3):
    """-> (x, every blob of the numpy forward)."""
    from feathercnn_amd import model_zoo
    (p, b, i, o), trace = net_model()
    x = np.random.default_rng(4000 + batch).uniform(-1, 1, (batch, 3, 8, 10)).astype(F)
    return x, model_zoo.numpy_forward(trace, i, x)
