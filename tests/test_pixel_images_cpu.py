"""Mixed-size / cropped image batches without a GPU: fhip_pixel_images_plan refuses every bad descriptor on the host (with the image's
index in the message) and reports the size it writes; fhip_pixels_to_float_images and fhip_net_feed_pixel_images refuse a bad plan or
batch before any device call; a C++ application using feather::Net::FeedPixelImages compiles against include/."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import pixels_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOGUS = 0x2001  # never dereferenced: the plan builder is host-only


@pytest.fixture(scope="module")
def lib():
    import feathercnn_amd
    from feathercnn_amd import _lib
    if not os.path.exists(_lib.lib_path()):
        import __graft_entry__
        __graft_entry__.build()
    return feathercnn_amd.load_library()


def _descs(specs):
    from feathercnn_amd import _lib
    arr = (_lib.fhip_pixel_image * len(specs))()
    for d, s in zip(arr, specs):
        d.data, d.w, d.h, d.stride, d.roi_x, d.roi_y, d.roi_w, d.roi_h = s
    return arr


GOOD = (BOGUS, 40, 30, 0, 0, 0, 0, 0)


def _plan(lib, specs, t=R.PIXEL_BGR2RGB, tw=16, th=12, buf=None):
    size = ctypes.c_size_t(0 if buf is None else buf.nbytes)
    rc = lib.fhip_pixel_images_plan(_descs(specs), len(specs), t, tw, th, None if buf is None else buf.ctypes.data_as(ctypes.c_void_p),
                                    ctypes.byref(size))
    return rc, size.value


BAD = [  # (what, descriptor at index 2 of an otherwise good batch)
    ("null data", (0, 40, 30, 0, 0, 0, 0, 0)),
    ("w < 1", (BOGUS, 0, 30, 0, 0, 0, 0, 0)),
    ("h < 1", (BOGUS, 40, 0, 0, 0, 0, 0, 0)),
    ("stride below w * cin", (BOGUS, 40, 30, 119, 0, 0, 0, 0)),
    ("ROI left of the image", (BOGUS, 40, 30, 0, -1, 0, 10, 10)),
    ("ROI above the image", (BOGUS, 40, 30, 0, 0, -1, 10, 10)),
    ("ROI past the right edge", (BOGUS, 40, 30, 0, 31, 0, 10, 10)),
    ("ROI past the bottom edge", (BOGUS, 40, 30, 0, 0, 21, 10, 10)),
    ("ROI of width 0 with a height", (BOGUS, 40, 30, 0, 0, 0, 0, 10)),
    ("1-pixel-wide ROI that must be resized", (BOGUS, 40, 30, 0, 5, 5, 1, 10)),
    ("1-pixel-high ROI that must be resized", (BOGUS, 40, 30, 0, 5, 5, 10, 1)),
    ("1-pixel-wide image that must be resized", (BOGUS, 1, 30, 0, 0, 0, 0, 0)),
]


@pytest.mark.parametrize("what,bad", BAD, ids=[b[0] for b in BAD])
def test_plan_refuses_each_bad_descriptor(lib, what, bad):
    buf = np.zeros(4096, np.uint8)
    rc, _ = _plan(lib, [GOOD, GOOD, bad, GOOD])
    assert rc == -2, what
    assert b"image 2" in lib.fhip_last_error(), lib.fhip_last_error()
    rc, _ = _plan(lib, [GOOD, GOOD, bad, GOOD], buf=buf)
    assert rc == -2 and not buf.any(), f"{what}: the plan was written"


def test_plan_edges_that_are_valid(lib):
    """ROIs touching each edge, a 2-pixel axis, a padded pitch, and a 1-pixel axis kept at its size are all accepted."""
    specs = [(BOGUS, 40, 30, 0, 30, 20, 10, 10), (BOGUS, 40, 30, 0, 0, 0, 40, 30), (BOGUS, 40, 30, 0, 38, 28, 2, 2),
             (BOGUS, 40, 30, 128, 0, 0, 0, 0), (BOGUS, 16, 1, 0, 0, 0, 0, 0)]
    assert _plan(lib, specs[:4])[0] == 0
    assert _plan(lib, [specs[4]], tw=16, th=1)[0] == 0  # no resize: a 1-pixel axis is fine
    assert _plan(lib, [(BOGUS, 16, 12, 0, 4, 0, 1, 12)], tw=1, th=12)[0] == 0


def test_plan_refuses_bad_batch_type_and_target(lib):
    for t in (0, 3, 16, R.PIXEL_RGB | (R.PIXEL_RGBA << 16), -1):
        assert _plan(lib, [GOOD], t=t)[0] == -2, hex(t)
    assert _plan(lib, [GOOD], tw=0)[0] == -2 and _plan(lib, [GOOD], th=0)[0] == -2
    size = ctypes.c_size_t(0)
    assert lib.fhip_pixel_images_plan(_descs([GOOD]), 0, R.PIXEL_RGB, 8, 8, None, ctypes.byref(size)) == -2
    assert lib.fhip_pixel_images_plan(None, 1, R.PIXEL_RGB, 8, 8, None, ctypes.byref(size)) == -2
    assert lib.fhip_pixel_images_plan(_descs([GOOD]), 1, R.PIXEL_RGB, 8, 8, None, None) == -2


def test_size_query_matches_written_size(lib):
    for n in (1, 2, 7, 64):
        rc, need = _plan(lib, [GOOD] * n)
        assert rc == 0 and need > 0
        buf = np.zeros(need + 64, np.uint8)
        rc, wrote = _plan(lib, [GOOD] * n, buf=buf)
        assert rc == 0 and wrote == need and not buf[need:].any()
        small = np.zeros(need - 8, np.uint8)
        assert _plan(lib, [GOOD] * n, buf=small)[0] == -2  # capacity below the size
    _, one = _plan(lib, [GOOD])
    _, two = _plan(lib, [GOOD] * 2)
    assert (two - one) % 16 == 0 and two > one


def test_launch_refuses_a_plan_the_builder_did_not_write(lib):
    """Checked on the host before any device call: output and device plan here are addresses no call may touch."""
    f = lib.fhip_pixels_to_float_images
    _, need = _plan(lib, [GOOD] * 3)
    good = np.zeros(need, np.uint8)
    assert _plan(lib, [GOOD] * 3, buf=good)[0] == 0
    out, dev = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x3000)
    p = lambda b: b.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    assert f(out, p(np.zeros(need, np.uint8)), dev, None, None, None) == -2  # zeros
    for i in range(0, 48, 4):  # any header word changed
        bad = good.copy()
        bad[i] ^= 1
        assert f(out, p(bad), dev, None, None, None) == -2, f"header byte {i}"
    assert f(None, p(good), dev, None, None, None) == -2
    assert f(out, None, dev, None, None, None) == -2
    assert f(out, p(good), None, None, None, None) == -2
    assert f(ctypes.c_void_p(0x1002), p(good), dev, None, None, None) == -2  # output not 4-byte aligned
    assert f(out, p(good), ctypes.c_void_p(0x3004), None, None, None) == -2  # device plan not 8-byte aligned


def test_net_entry_refuses_before_any_device_call(lib):
    h = ctypes.c_void_p()
    assert lib.fhip_net_create(ctypes.byref(h)) == 0
    try:
        px = (ctypes.c_ubyte * (40 * 30 * 3))()
        ok = _descs([(ctypes.addressof(px), 40, 30, 0, 0, 0, 0, 0)])
        bad = _descs([(ctypes.addressof(px), 40, 30, 0, 0, 0, 0, 0), (ctypes.addressof(px), 40, 30, 0, 35, 0, 10, 10)])
        f = lib.fhip_net_feed_pixel_images
        assert f(h, b"data", 2, bad, R.PIXEL_BGR2RGB, 16, 16, None, None, 0) == -2
        assert b"image 1" in lib.fhip_last_error()
        assert f(h, b"data", 0, ok, R.PIXEL_BGR2RGB, 16, 16, None, None, 0) == -2
        assert f(h, b"data", 1, ok, 0, 16, 16, None, None, 0) == -2
        assert f(h, None, 1, ok, R.PIXEL_BGR2RGB, 16, 16, None, None, 0) == -2
        assert f(h, b"nope", 1, ok, R.PIXEL_BGR2RGB, 16, 16, None, None, 0) == -1  # NET_E_IO, as FeedInput
        assert b"nope" in lib.fhip_last_error()
    finally:
        lib.fhip_net_destroy(h)


def test_python_descriptors_keep_strided_views_in_place():
    """A crop img[y0:y1, x0:x1] is passed without a copy, its row stride as the pitch; a view with strided pixels is copied."""
    from feathercnn_amd.pixels import _image_descs
    img = np.random.default_rng(0).integers(0, 256, (30, 40, 3), dtype=np.uint8)
    crop = img[5:25, 8:30]
    d, dev, keep = _image_descs([img, crop], R.PIXEL_BGR2RGB, [None, (1, 2, 10, 12)])
    assert dev == 0 and d[1].data == crop.ctypes.data and d[1].stride == 120 and (d[1].w, d[1].h) == (22, 20)
    assert (d[1].roi_x, d[1].roi_y, d[1].roi_w, d[1].roi_h) == (1, 2, 10, 12) and (d[0].roi_w, d[0].roi_h) == (0, 0)
    d, _, keep = _image_descs([img[:, ::2]], R.PIXEL_BGR2RGB, None)
    assert d[0].stride == 20 * 3 and keep[0].flags["C_CONTIGUOUS"]


def test_cpp_pixel_images_application_compiles(lib, tmp_path):
    """tests/cpp/pixel_images_app_main.cpp: dense ROI copies + Mat::from_pixels_resize + FeedInput, then feather::Net::FeedPixelImages;
    compiles against include/ and links against the product library (tests/test_pixel_images_gpu.py runs it)."""
    from feathercnn_amd import _lib
    libdir = os.path.dirname(_lib.lib_path())
    inc = os.path.join(ROOT, "include")
    exe = str(tmp_path / "pixel_images_app_main")
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-I" + inc, "-I" + os.path.join(inc, "feather"),
                    os.path.join(ROOT, "tests", "cpp", "pixel_images_app_main.cpp"), "-o", exe, "-L" + libdir, "-lfeather_hip",
                    "-Wl,-rpath," + libdir], check=True, capture_output=True, text=True)
    assert os.path.exists(exe)
