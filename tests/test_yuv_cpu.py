"""NV21 (yuv420sp) input without a GPU: the numpy restatement (tests/yuv_ref.py) and the host code of include/ncnn/mat.h equal the
reference's own functions on every recorded fixture (tests/golden/yuv_golden.npz: both chains, resize_bilinear_c2,
resize_bilinear_yuv420sp, to_pixels, to_pixels_resize); the C-ABI refuses bad arguments before any device call; a reference-style
application that feeds a camera frame compiles against include/."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import pixels_ref as R
import yuv_ref as Y

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "yuv_golden.npz")
NAMES = {v: k for k, v in Y.TYPES.items()}


def chain_cases():
    g = np.load(GOLDEN)
    for t, w, h, tw, th, rf in g["cases"]:
        t, w, h, tw, th, rf = (int(v) for v in (t, w, h, tw, th, rf))
        yield t, w, h, tw, th, rf, g[f"in_{w}x{h}"], g[f"out_{NAMES[t]}_{w}x{h}_{tw}x{th}_rf{rf}"]


@pytest.fixture(scope="module")
def lib():
    import feathercnn_amd
    from feathercnn_amd import _lib
    if not os.path.exists(_lib.lib_path()):
        import __graft_entry__
        __graft_entry__.build()
    return feathercnn_amd.load_library()


def test_fixture_covers_chains_types_and_shape_classes():
    cases = list(chain_cases())
    assert {(c[0], c[5]) for c in cases} == {(t, rf) for t in Y.TYPES.values() for rf in (0, 1)}
    for rf in (0, 1):
        shapes = {(w, h, tw, th) for t, w, h, tw, th, r, _, _ in cases if r == rf}
        assert any(tw < w and th < h for w, h, tw, th in shapes) and any(tw > w and th > h for w, h, tw, th in shapes)
        assert any((w, h) == (tw, th) for w, h, tw, th in shapes) and any(max(w / h, h / w) >= 40 for w, h, _, _ in shapes)
        assert any(min(w, h) == 4 for w, h, _, _ in shapes)
        assert any(tw % 4 == 0 for _, _, tw, _ in shapes) and any(tw % 4 for _, _, tw, _ in shapes)
    assert any(tw % 2 for _, _, _, tw, _, rf, _, _ in cases if rf == 0)
    assert os.path.getsize(GOLDEN) < os.path.getsize(os.path.join(ROOT, "tests", "golden", "pixel_golden.npz")) // 4


def test_restatement_equals_reference_fixtures():
    n = 0
    for t, w, h, tw, th, rf, yuv, want in chain_cases():
        got = Y.yuv420sp_to_float(yuv, t, tw, th, bool(rf))[0]
        assert got.dtype == np.float32 and np.array_equal(got, want.astype(np.float32)), f"{NAMES[t]} {w}x{h}->{tw}x{th} rf{rf}"
        n += 1
    assert n >= 60
    g = np.load(GOLDEN)
    for sw, sh, dw, dh in g["c2"]:
        assert np.array_equal(R.resize_bilinear(g[f"c2in_{sw}x{sh}"][None], int(dw), int(dh))[0], g[f"c2_{sw}x{sh}_{dw}x{dh}"])
    for sw, sh, dw, dh in g["yuvresize"]:
        got = Y.resize_bilinear_yuv420sp(g[f"in_{sw}x{sh}"][None], int(dw), int(dh))[0]
        assert np.array_equal(got, g[f"yuvresize_{sw}x{sh}_{dw}x{dh}"])
    for t, w, h, c, tw, th in g["topixels"]:
        got = Y.to_pixels_resize(g[f"mat_{w}x{h}x{c}"], int(t), int(tw), int(th))
        assert np.array_equal(got, g[f"topix_{t}_{w}x{h}x{c}_{tw}x{th}"]), (t, w, h, c, tw, th)


def test_equal_size_chains_agree():
    """At equal size resize_bilinear_yuv420sp is the identity, so both chains give the same floats."""
    f = np.random.default_rng(3).integers(0, 256, (2, 18, 16), dtype=np.uint8)
    for t in Y.TYPES.values():
        assert np.array_equal(Y.yuv420sp_to_float(f, t, 16, 12, True), Y.yuv420sp_to_float(f, t, 16, 12, False))
    assert np.array_equal(Y.resize_bilinear_yuv420sp(f, 16, 12), f)


def test_restatement_refusals():
    f = np.zeros((6, 4), np.uint8)  # a 4x4 frame
    for args in ((R.PIXEL_BGR, 4, 4, True), (R.PIXEL_BGR, 4, 4, False), (R.PIXEL_RGB, 5, 4, True), (R.PIXEL_RGB, 4, 3, True)):
        t, tw, th, rf = args
        with pytest.raises(ValueError):
            Y.yuv420sp_to_float(f, t, tw, th, rf)
    assert Y.yuv420sp_to_float(f, R.PIXEL_RGB, 5, 3, False).shape == (1, 3, 3, 5)  # chain 0 takes an odd target
    with pytest.raises(ValueError):
        Y.yuv420sp_to_float(np.zeros((6, 5), np.uint8), R.PIXEL_RGB, 4, 4, False)  # odd frame width
    with pytest.raises(ValueError):
        Y.yuv420sp_to_float(np.zeros((3, 2), np.uint8), R.PIXEL_RGB, 2, 2, True)  # 2x2: VU plane 1 pair wide
    assert Y.yuv420sp_to_float(np.zeros((3, 2), np.uint8), R.PIXEL_RGB, 3, 5, False).shape == (1, 3, 5, 3)


def _run_mat_driver(exe, stdin):
    proc = subprocess.run([exe], input=stdin, capture_output=True, timeout=120)
    assert proc.returncode == 0, (proc.returncode, proc.stderr)
    return proc.stdout


def test_header_functions_equal_reference_fixtures(tmp_path):
    """tests/cpp/yuv_mat_main.cpp over include/ncnn/mat.h (yuv420sp2rgb, resize_bilinear_c1..c4, resize_bilinear_yuv420sp,
    Mat::to_pixels, Mat::to_pixels_resize), built with g++, bit for bit against every fixture."""
    exe = str(tmp_path / "yuv_mat_main")
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "yuv_mat_main.cpp"), "-o", exe], check=True, capture_output=True, text=True)
    g = np.load(GOLDEN)
    stdin, want = b"", []
    for t, w, h, tw, th, rf, yuv, out in chain_cases():
        stdin += f"C {t} {w} {h} {tw} {th} {rf}\n".encode() + yuv.tobytes()
        want.append((f"{NAMES[t]} {w}x{h}->{tw}x{th} rf{rf}", out))
    for sw, sh, dw, dh in g["c2"]:
        stdin += f"R2 {sw} {sh} {dw} {dh}\n".encode() + g[f"c2in_{sw}x{sh}"].tobytes()
        want.append((f"c2 {sw}x{sh}->{dw}x{dh}", g[f"c2_{sw}x{sh}_{dw}x{dh}"]))
    for sw, sh, dw, dh in g["yuvresize"]:
        stdin += f"RY {sw} {sh} {dw} {dh}\n".encode() + g[f"in_{sw}x{sh}"].tobytes()
        want.append((f"yuv420sp {sw}x{sh}->{dw}x{dh}", g[f"yuvresize_{sw}x{sh}_{dw}x{dh}"]))
    for t, w, h, c, tw, th in g["topixels"]:
        stdin += f"P {t} {w} {h} {c} {tw} {th}\n".encode() + g[f"mat_{w}x{h}x{c}"].tobytes()
        want.append((f"to_pixels {t:#x} {w}x{h}x{c}->{tw}x{th}", g[f"topix_{t}_{w}x{h}x{c}_{tw}x{th}"]))
    got = _run_mat_driver(exe, stdin)
    pos = 0
    for what, w in want:
        assert np.array_equal(np.frombuffer(got[pos:pos + w.size], np.uint8).reshape(w.shape), w), what
        pos += w.size
    assert pos == len(got)


def test_c_abi_refuses_bad_arguments_before_any_device_call(lib):
    """Every argument error is answered on the host: these calls name no valid device memory at all."""
    bogus_out, bogus_px = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x2001)
    f = lib.fhip_yuv420sp_to_float
    for t in (0, R.PIXEL_BGR, R.PIXEL_GRAY, R.PIXEL_RGBA, R.PIXEL_BGR2RGB, R.PIXEL_BGR2GRAY, R.PIXEL_RGBA2RGB, -1):
        assert f(bogus_out, bogus_px, 1, t, 8, 8, 4, 4, 1, None, None, None) == -2, hex(t)
        assert f(bogus_out, bogus_px, 1, t, 8, 8, 4, 4, 0, None, None, None) == -2, hex(t)
    ok = R.PIXEL_RGB2BGR
    bad = [  # (batch, w, h, tw, th, resize_first)
        (1, 7, 8, 4, 4, 0), (1, 8, 7, 4, 4, 0), (1, 7, 8, 4, 4, 1), (1, 8, 7, 4, 4, 1),  # odd frame size
        (1, 8, 8, 5, 4, 1), (1, 8, 8, 4, 5, 1),  # resize_first, odd target
        (1, 2, 8, 4, 4, 1), (1, 8, 2, 4, 4, 1), (1, 2, 2, 2, 2, 1), (1, 2, 8, 2, 8, 1),  # resize_first below 4 px, equal size included
        (0, 8, 8, 4, 4, 0), (-1, 8, 8, 4, 4, 1), (1, 0, 8, 4, 4, 0), (1, 8, 0, 4, 4, 0), (1, 8, 8, 0, 4, 0), (1, 8, 8, 4, 0, 0),
        (1, -2, 8, 4, 4, 0), (1, 8, 8, -4, 4, 1)]
    for n, w, h, tw, th, rf in bad:
        assert f(bogus_out, bogus_px, n, ok, w, h, tw, th, rf, None, None, None) == -2, (n, w, h, tw, th, rf)
    assert f(None, bogus_px, 1, ok, 8, 8, 4, 4, 1, None, None, None) == -2
    assert f(bogus_out, None, 1, ok, 8, 8, 4, 4, 1, None, None, None) == -2
    assert f(ctypes.c_void_p(0x1002), bogus_px, 1, ok, 8, 8, 4, 4, 1, None, None, None) == -2  # output not 4-byte aligned
    assert b"aligned" in lib.fhip_last_error()
    # the Net entry: the same refusals, and no such blob, answered before the upload
    h = ctypes.c_void_p()
    assert lib.fhip_net_create(ctypes.byref(h)) == 0
    try:
        px = (ctypes.c_ubyte * 96)()
        g = lib.fhip_net_feed_yuv420sp
        assert g(h, b"data", 1, px, 8, 8, 4, 4, R.PIXEL_BGR, 1, None, None, 0) == -2
        for n, w, hh, tw, th, rf in bad:
            assert g(h, b"data", n, px, w, hh, tw, th, ok, rf, None, None, 0) == -2, (n, w, hh, tw, th, rf)
        assert g(h, b"data", 1, None, 8, 8, 4, 4, ok, 1, None, None, 0) == -2
        assert g(h, None, 1, px, 8, 8, 4, 4, ok, 1, None, None, 0) == -2
        assert g(None, b"data", 1, px, 8, 8, 4, 4, ok, 1, None, None, 0) == -2
        assert g(h, b"nope", 1, px, 8, 8, 4, 4, ok, 1, None, None, 0) == -1  # NET_E_IO, as FeedInput
        assert b"nope" in lib.fhip_last_error()
    finally:
        lib.fhip_net_destroy(h)


def test_python_refuses_before_the_call():
    from feathercnn_amd import FeatherHipError
    from feathercnn_amd.pixels import _frames
    with pytest.raises(FeatherHipError):
        _frames(np.zeros((6, 4), np.uint8), R.PIXEL_BGR)
    with pytest.raises(FeatherHipError):
        _frames(np.zeros((5, 4), np.uint8), R.PIXEL_RGB)  # rows not h*3/2
    with pytest.raises(FeatherHipError):
        _frames(np.zeros((6, 4), np.float32), R.PIXEL_RGB)
    n, w, h, cout, _, dev, _ = _frames(np.zeros((3, 12, 10), np.uint8), R.PIXEL_RGB2GRAY)
    assert (n, w, h, cout, dev) == (3, 10, 8, 1, 0)


def test_reference_style_yuv_application_compiles(lib, tmp_path):
    """ncnn::resize_bilinear_yuv420sp -> ncnn::yuv420sp2rgb -> Mat::from_pixels -> FeedInput, as ncnn programs write it, plus
    feather::Net::FeedYUV420sp: compiles against include/ and links against the product library (tests/test_yuv_gpu.py runs it)."""
    from feathercnn_amd import _lib
    libdir = os.path.dirname(_lib.lib_path())
    inc = os.path.join(ROOT, "include")
    exe = str(tmp_path / "yuv_app_main")
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-I" + inc, "-I" + os.path.join(inc, "feather"),
                    os.path.join(ROOT, "tests", "cpp", "yuv_app_main.cpp"), "-o", exe, "-L" + libdir, "-lfeather_hip", "-Wl,-rpath," + libdir],
                   check=True, capture_output=True, text=True)
    assert os.path.exists(exe)
