"""The uint8 image input path without a GPU: the numpy restatement (tests/pixels_ref.py) and the host code of include/ncnn/mat.h equal
the reference's own from_pixels_resize on every recorded fixture (tests/golden/pixel_golden.npz), the C-ABI refuses bad arguments before
any device call, and a reference-style application that prepares its input with ncnn::Mat::from_pixels_resize compiles against include/."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import pixels_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "pixel_golden.npz")
MEAN = np.array([104.0, 116.67, 122.68, 0.5], np.float32)  # tests/cpp/pixel_mat_main.cpp's values
NORM = np.array([0.017, 1.0 / 58.8, 0.0175, -2.0], np.float32)


def golden_cases():
    g = np.load(GOLDEN)
    for name, (t, w, h, tw, th) in zip(g["names"], g["cases"]):
        cin, _ = R.channels(int(t))
        yield (str(name), int(t), int(w), int(h), int(tw), int(th), g[f"in_c{cin}_{w}x{h}"],
               g[f"out_{name}_{w}x{h}_{tw}x{th}"].astype(np.float32))


@pytest.fixture(scope="module")
def lib():
    import feathercnn_amd
    from feathercnn_amd import _lib
    if not os.path.exists(_lib.lib_path()):
        import __graft_entry__
        __graft_entry__.build()
    return feathercnn_amd.load_library()


def test_fixture_covers_every_type_and_shape_class():
    cases = list(golden_cases())
    assert {c[1] for c in cases} == set(R.TYPES.values())
    shapes = {(w, h, tw, th) for _, _, w, h, tw, th, _, _ in cases}
    assert any(tw < w and th < h for w, h, tw, th in shapes) and any(tw > w and th > h for w, h, tw, th in shapes)
    assert any((w, h) == (tw, th) for w, h, tw, th in shapes) and any(min(w, h) == 2 for w, h, _, _ in shapes)
    assert any(max(w / h, h / w) > 20 for w, h, _, _ in shapes)
    assert os.path.getsize(GOLDEN) < 1 << 20


def test_restatement_equals_reference_fixtures():
    n = 0
    for name, t, w, h, tw, th, px, want in golden_cases():
        got = R.from_pixels_resize(px, t, tw, th)[0]
        assert got.dtype == np.float32 and np.array_equal(got.view(np.int32), want.view(np.int32)), f"{name} {w}x{h}->{tw}x{th}"
        n += 1
    assert n >= 13 * 5


def test_restatement_refuses_one_pixel_axis():
    px = np.zeros((1, 4, 1, 3), np.uint8)
    with pytest.raises(ValueError):
        R.from_pixels_resize(px, R.PIXEL_RGB, 3, 3)
    assert R.from_pixels_resize(px, R.PIXEL_RGB, 1, 4).shape == (1, 3, 4, 1)


def test_mean_norm_forms():
    x = np.arange(256, dtype=np.float32).reshape(1, 1, 16, 16).repeat(3, axis=1)
    m, s = MEAN[:3], NORM[:3]
    assert np.array_equal(R.mean_norm(x, m, None), x - m.reshape(1, 3, 1, 1))
    assert np.array_equal(R.mean_norm(x, None, s), x * s.reshape(1, 3, 1, 1))
    both = R.mean_norm(x, m, s)
    assert np.array_equal(both, (x * s.reshape(1, 3, 1, 1)) + (-(m * s)).reshape(1, 3, 1, 1))
    assert np.array_equal(R.mean_norm(x), x)


def _mat_driver(tmp_path):
    exe = str(tmp_path / "pixel_mat_main")
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "pixel_mat_main.cpp"), "-o", exe], check=True, capture_output=True, text=True)
    return exe


def test_header_from_pixels_resize_equals_reference_fixtures(tmp_path):
    """ncnn::Mat::from_pixels[_resize] of include/ncnn/mat.h, built with g++, bit for bit against every fixture; substract_mean_normalize's
    four forms against the restatement."""
    exe = _mat_driver(tmp_path)
    cases = list(golden_cases())
    stdin, want = b"", []
    for name, t, w, h, tw, th, px, out in cases:
        cin, cout = R.channels(t)
        for form in range(4):
            stdin += f"{t} {w} {h} {tw} {th} {cin} {form}\n".encode() + px.tobytes()
            mean = MEAN[:cout] if form & 1 else None
            norm = NORM[:cout] if form & 2 else None
            want.append((f"{name} {w}x{h}->{tw}x{th} form {form}", R.mean_norm(out[None], mean, norm)[0]))
    proc = subprocess.run([exe], input=stdin, capture_output=True, timeout=120)
    assert proc.returncode == 0, proc.stderr
    got = np.frombuffer(proc.stdout, np.float32)
    pos = 0
    for what, w in want:
        g = got[pos:pos + w.size].reshape(w.shape)
        pos += w.size
        assert np.array_equal(g.view(np.int32), w.view(np.int32)), what
    assert pos == got.size


def test_c_abi_refuses_bad_arguments_before_any_device_call(lib):
    """Every argument error is answered on the host: these calls name no valid device memory at all."""
    bogus_out, bogus_px = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x2001)
    f = lib.fhip_pixels_to_float
    ok_type = R.PIXEL_BGR2RGB
    for t in (0, 3, 16, R.PIXEL_RGB | (R.PIXEL_RGBA << 16), R.PIXEL_RGB | (R.PIXEL_RGB << 16), R.PIXEL_GRAY | (5 << 16), -1):
        assert f(bogus_out, bogus_px, 1, t, 8, 8, 4, 4, None, None, None) == -2, hex(t)
    for args in ((1, 0, 8, 4, 4), (1, 8, 0, 4, 4), (1, 8, 8, 0, 4), (1, 8, 8, 4, 0), (0, 8, 8, 4, 4), (1, 1, 8, 4, 4), (1, 8, 1, 4, 4)):
        n, w, h, tw, th = args
        assert f(bogus_out, bogus_px, n, ok_type, w, h, tw, th, None, None, None) == -2, args
    assert f(None, bogus_px, 1, ok_type, 8, 8, 4, 4, None, None, None) == -2
    assert f(bogus_out, None, 1, ok_type, 8, 8, 4, 4, None, None, None) == -2
    assert f(ctypes.c_void_p(0x1002), bogus_px, 1, ok_type, 8, 8, 4, 4, None, None, None) == -2  # output not 4-byte aligned
    assert b"pixel" in lib.fhip_last_error() or b"aligned" in lib.fhip_last_error()
    # the Net entry: bad type / sizes / no such blob, answered before the upload
    h = ctypes.c_void_p()
    assert lib.fhip_net_create(ctypes.byref(h)) == 0
    try:
        px = (ctypes.c_ubyte * 48)()
        assert lib.fhip_net_feed_pixels(h, b"data", 1, px, 0, 4, 4, 2, 2, None, None, 0) == -2
        assert lib.fhip_net_feed_pixels(h, b"data", 0, px, R.PIXEL_RGB, 4, 4, 2, 2, None, None, 0) == -2
        assert lib.fhip_net_feed_pixels(h, b"data", 1, px, R.PIXEL_RGB, 1, 4, 2, 2, None, None, 0) == -2
        assert lib.fhip_net_feed_pixels(h, b"data", 1, None, R.PIXEL_RGB, 4, 4, 2, 2, None, None, 0) == -2
        assert lib.fhip_net_feed_pixels(h, b"nope", 1, px, R.PIXEL_RGB, 4, 4, 2, 2, None, None, 0) == -1  # NET_E_IO, as FeedInput
        assert b"nope" in lib.fhip_last_error()
    finally:
        lib.fhip_net_destroy(h)


def test_python_constants_match_ncnn_values():
    import feathercnn_amd as F
    for name, v in R.TYPES.items():
        assert getattr(F, "PIXEL_" + name) == v
    assert (F.PIXEL_RGB, F.PIXEL_BGR, F.PIXEL_GRAY, F.PIXEL_RGBA) == (1, 2, 4, 8)
    assert F.PIXEL_BGR2RGB == 2 | (1 << 16) and F.PIXEL_RGBA2GRAY == 8 | (4 << 16)


def test_reference_style_pixel_application_compiles(lib, tmp_path):
    """Mat::PIXEL_* + Mat::from_pixels_resize + substract_mean_normalize + feather::Net::FeedInput, as ncnn programs write it, plus
    feather::Net::FeedPixels: compiles against include/ and links against the product library (tests/test_pixels_gpu.py runs it)."""
    from feathercnn_amd import _lib
    libdir = os.path.dirname(_lib.lib_path())
    inc = os.path.join(ROOT, "include")
    exe = str(tmp_path / "pixel_app_main")
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-I" + inc, "-I" + os.path.join(inc, "feather"),
                    os.path.join(ROOT, "tests", "cpp", "pixel_app_main.cpp"), "-o", exe, "-L" + libdir, "-lfeather_hip", "-Wl,-rpath," + libdir],
                   check=True, capture_output=True, text=True)
    assert os.path.exists(exe)
