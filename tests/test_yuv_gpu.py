"""NV21 (yuv420sp) input on the MI355X: fhip_yuv420sp_to_float (affine_kernel over PixelSrc in its NV21 modes) bit-exact against the
reference's own chains (tests/golden/yuv_golden.npz) and the numpy restatement (tests/yuv_ref.py) over a seeded sweep that includes
batches of 1920x1080 -> 224x224 and 1280x720 -> 300x300; the mean / norm forms; the guarded-buffer contract; hipGraph capture; equal-size
chain 1 equal to chain 0; Net.FeedYUV420sp + Forward equal to FeedInput(the restated floats) + Forward at fusion 0 / 3, with the graph,
with sub-batch replicas, from host and device memory and across a change of target size; the reference-style C++ application."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import pixels_ref as R
import side_contract
import yuv_ref as Y
from guarded import Guarded

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "yuv_golden.npz")
TYPES = list(Y.TYPES.values())
NAMES = {v: k for k, v in Y.TYPES.items()}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _convert(f, t, tw, th, rf, mean=None, norm=None):
    import torch

    from feathercnn_amd import yuv420sp_to_float
    out = yuv420sp_to_float(torch.from_numpy(np.ascontiguousarray(f)).cuda(), t, (tw, th), rf, mean, norm)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _want(f, t, tw, th, rf, mean=None, norm=None):
    """The restatement, frame by frame (a batch of full-HD frames in int64 at once would need gigabytes)."""
    return np.concatenate([Y.yuv420sp_to_float(f[i:i + 1], t, tw, th, rf, mean, norm) for i in range(f.shape[0])])


def _frames(rng, n, w, h):
    return rng.integers(0, 256, (n, h * 3 // 2, w), dtype=np.uint8)


_stream = side_contract.stream


def test_every_fixture_bit_exact_in_a_batch(cuda):
    """Each fixture frame in the middle of a batch of three different frames: every frame is converted on its own."""
    g = np.load(GOLDEN)
    rng = np.random.default_rng(11)
    n = 0
    for t, w, h, tw, th, rf in g["cases"]:
        t, w, h, tw, th, rf = (int(v) for v in (t, w, h, tw, th, rf))
        f = g[f"in_{w}x{h}"]
        batch = np.stack([_frames(rng, 1, w, h)[0], f, _frames(rng, 1, w, h)[0]])
        got = _convert(batch, t, tw, th, bool(rf))
        want = g[f"out_{NAMES[t]}_{w}x{h}_{tw}x{th}_rf{rf}"].astype(np.float32)
        what = f"{NAMES[t]} {w}x{h}->{tw}x{th} resize_first={rf}"
        assert np.array_equal(_bits(got[1]), _bits(want)), f"{what}: differs from the reference"
        assert np.array_equal(_bits(got), _bits(_want(batch, t, tw, th, bool(rf)))), f"{what}: batch neighbours"
        n += 1
    assert n == len(g["cases"]) >= 60


def _sweep_cases():
    rng = np.random.default_rng(2031)
    cases = []
    for rf in (1, 0):
        cases += [(R.PIXEL_RGB2BGR, 1920, 1080, 224, 224, rf, 8), (R.PIXEL_RGB, 1280, 720, 300, 300, rf, 8),
                  (R.PIXEL_RGB2GRAY, 640, 480, 224, 224, rf, 2), (R.PIXEL_RGB, 4, 4, 2, 2, rf, 3), (R.PIXEL_RGB2BGR, 8, 6, 64, 40, rf, 2)]
    while len(cases) < 80:
        t = TYPES[int(rng.integers(len(TYPES)))]
        rf = int(rng.integers(2))
        w, h = 2 * int(rng.integers(2 if rf else 1, 90)), 2 * int(rng.integers(2 if rf else 1, 90))
        mode = int(rng.integers(3))
        if mode == 0:  # down
            tw, th = max(2, w // int(rng.integers(2, 9))), max(2, h // int(rng.integers(2, 9)))
        elif mode == 1:  # up
            tw, th = w * int(rng.integers(2, 5)) + int(rng.integers(0, 3)), h * int(rng.integers(2, 5)) + int(rng.integers(0, 3))
        else:  # anything
            tw, th = int(rng.integers(1, 150)), int(rng.integers(1, 150))
        if rf:
            tw, th = max(2, tw & ~1), max(2, th & ~1)
        cases.append((t, w, h, tw, th, rf, int(rng.integers(1, 4))))
    return cases


SWEEP = _sweep_cases()


def test_seeded_sweep_bit_exact(cuda):
    rng = np.random.default_rng(5)
    assert any(tw % 4 == 0 for _, _, _, tw, _, _, _ in SWEEP) and any(tw % 4 for _, _, _, tw, _, _, _ in SWEEP)
    assert any(tw % 2 for _, _, _, tw, _, rf, _ in SWEEP if rf == 0)
    for t, w, h, tw, th, rf, n in SWEEP:
        f = _frames(rng, n, w, h)
        got = _convert(f, t, tw, th, bool(rf))
        assert np.array_equal(_bits(got), _bits(_want(f, t, tw, th, bool(rf)))), f"type {t:#x} {n}x {w}x{h} -> {tw}x{th} rf{rf}"


@pytest.mark.parametrize("form", ["none", "mean", "norm", "both"])
@pytest.mark.parametrize("t,w,h,tw,th,rf", [(R.PIXEL_RGB2BGR, 64, 48, 32, 24, 1), (R.PIXEL_RGB, 40, 30, 21, 19, 0),
                                            (R.PIXEL_RGB2GRAY, 20, 18, 40, 30, 1)])
def test_mean_norm_forms(cuda, form, t, w, h, tw, th, rf):
    cout = 1 if t == R.PIXEL_RGB2GRAY else 3
    f = _frames(np.random.default_rng(9), 2, w, h)
    rng = np.random.default_rng(3)
    mean = rng.uniform(0, 255, cout).astype(np.float32) if form in ("mean", "both") else None
    norm = rng.uniform(-0.1, 0.1, cout).astype(np.float32) if form in ("norm", "both") else None
    if form == "both":
        mean[0], norm[0] = np.float32(127.5), np.float32(1 / 127.5)
    got = _convert(f, t, tw, th, bool(rf), mean, norm)
    assert np.array_equal(_bits(got), _bits(_want(f, t, tw, th, bool(rf), mean, norm))), form


def test_equal_size_chains_agree(cuda):
    f = _frames(np.random.default_rng(12), 3, 36, 20)
    for t in TYPES:
        a, b = _convert(f, t, 36, 20, True), _convert(f, t, 36, 20, False)
        assert np.array_equal(_bits(a), _bits(b)) and np.array_equal(_bits(a), _bits(_want(f, t, 36, 20, False)))


def _guarded_source(raw: np.ndarray, byte_offset: int):
    import torch
    raw = raw.reshape(-1)
    nf = (raw.size + byte_offset + 3) // 4 + 1
    g = Guarded(nf, np.zeros(nf, np.float32))
    body = g.raw.view(torch.uint8)[4 * g.lo:4 * (g.lo + nf)]
    body[byte_offset:byte_offset + raw.size].copy_(torch.from_numpy(raw))
    return g, g.ptr + byte_offset


@pytest.mark.parametrize("t,w,h,tw,th,rf", [(R.PIXEL_RGB2BGR, 38, 30, 24, 16, 1), (R.PIXEL_RGB, 14, 8, 14, 8, 0),
                                            (R.PIXEL_RGB2GRAY, 10, 12, 23, 5, 0), (R.PIXEL_RGB, 4, 4, 8, 40, 1), (R.PIXEL_RGB, 30, 2, 9, 7, 0)])
def test_guarded_contract(cuda, t, w, h, tw, th, rf):
    """Guards intact, every output word written, the source unchanged; a second call bit-identical; the source at byte offsets 0-3 and
    the output 4 bytes past a 16-byte boundary (the scalar-store form) give the same bits."""
    import torch

    from feathercnn_amd import load_library
    lib = load_library()
    cout = 1 if t == R.PIXEL_RGB2GRAY else 3
    n = 3
    f = _frames(np.random.default_rng(1), n, w, h)
    want = _want(f, t, tw, th, bool(rf))
    count = n * cout * th * tw
    for boff in range(4):
        src, sp = _guarded_source(f, boff)
        before = src.snapshot()
        for ooff in (0, 1):
            out = Guarded(count, "poison", ooff)
            for rep in range(2):
                assert lib.fhip_yuv420sp_to_float(ctypes.c_void_p(out.ptr), ctypes.c_void_p(sp), n, t, w, h, tw, th, rf, None, None,
                                                  _stream()) == 0
                torch.cuda.synchronize()
                assert out.guards_intact() is None, f"offset {boff}/{ooff}: wrote outside the output: {out.guards_intact()}"
                assert out.unwritten() == 0, f"offset {boff}/{ooff}: {out.unwritten()} of {count} output words unwritten"
                assert src.unchanged(before), f"offset {boff}: the source changed"
                got = out.body.cpu().numpy().reshape(want.shape)
                assert np.array_equal(_bits(got), _bits(want)), f"byte offset {boff}, output offset {ooff}, call {rep + 1}"


@pytest.mark.parametrize("rf", [1, 0])
def test_graph_capture(cuda, rf):
    """Stream-capturable: mean / norm are read at the call, nothing is allocated or copied; a replay converts whatever the source holds."""
    import torch

    from feathercnn_amd import yuv420sp_to_float
    t, w, h, tw, th = R.PIXEL_RGB2BGR, 64, 48, 32, 32
    mean, norm = np.array([104, 117, 123], np.float32), np.array([0.017, 0.017, 0.017], np.float32)
    rng = np.random.default_rng(4)
    a, b = _frames(rng, 2, w, h), _frames(rng, 2, w, h)
    src = torch.from_numpy(a).cuda()
    out = torch.empty((2, 3, th, tw), device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        yuv420sp_to_float(src, t, (tw, th), rf, mean, norm, out=out)  # warm-up outside capture
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        yuv420sp_to_float(src, t, (tw, th), rf, mean, norm, out=out)
    mean[:] = 0  # the captured call keeps the values it was given
    for f in (a, b):
        src.copy_(torch.from_numpy(f))
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        want = _want(f, t, tw, th, bool(rf), np.array([104, 117, 123], np.float32), norm)
        assert np.array_equal(_bits(out.cpu().numpy()), _bits(want))


# ---- Net level -----------------------------------------------------------------------------------------------------------------------

def _net(model, fusion, graph=False, sub_batches=1):
    from feathercnn_amd.net import Net
    p, b, i, o = model
    net = Net(fusion=fusion, tuned=fusion == 3, graph=graph, sub_batches=sub_batches)
    net.LoadParam(p)
    net.LoadWeights(b)
    return net, i, o


def _forward(net, out, twice=False):
    net.Forward()
    if twice:
        net.Forward()
    return net.Extract(out)


NET_CASES = [  # model, fusion, graph, sub_batches, batch, frame (w, h), targets (chain 1 / chain 0 alternate)
    ("tiny", 0, False, 1, 2, (38, 30), [(20, 20), (24, 16)]),
    ("tiny", 3, True, 1, 3, (42, 18), [(20, 20), (28, 28)]),
    ("tiny", 1, False, 2, 5, (34, 36), [(20, 20), (16, 24)]),
    ("mobilenet", 0, False, 1, 2, (320, 240), [(224, 224)]),
    ("mobilenet", 3, True, 1, 2, (320, 240), [(224, 224)]),
    ("mobilenet", 3, True, 2, 5, (256, 256), [(224, 224)]),
]


@pytest.mark.parametrize("on_device", [0, 1], ids=["host", "device"])
@pytest.mark.parametrize("case", NET_CASES, ids=[f"{c[0]}-f{c[1]}{'-graph' if c[2] else ''}-sb{c[3]}-n{c[4]}" for c in NET_CASES])
def test_net_feed_yuv420sp_equals_feed_input(cuda, case, on_device):
    """FeedYUV420sp + Forward is bit-identical to FeedInput(the restated floats) + Forward on the same net, for both chains and across a
    change of target size (the blob is reshaped, the graph dropped and re-recorded)."""
    import torch

    from feathercnn_amd import model_zoo
    name, fusion, graph, sub, n, (w, h), targets = case
    model = model_zoo.tiny_allsorts() if name == "tiny" else model_zoo.mobilenet_v1()
    net, i, o = _net(model, fusion, graph, sub)
    t = R.PIXEL_RGB2BGR
    mean, norm = np.array([104, 117, 123], np.float32), np.array([0.017, 0.018, 0.019], np.float32)
    f = _frames(np.random.default_rng(8), n, w, h)
    for rf in (1, 0):
        for tw, th in targets:
            x = _want(f, t, tw, th, bool(rf), mean, norm)
            net.FeedInput(i, x)
            want = _forward(net, o, twice=graph)
            src = torch.from_numpy(f).cuda() if on_device else f
            net.FeedYUV420sp(i, src, t, (tw, th), bool(rf), mean, norm)
            if fusion == 0:
                assert np.array_equal(_bits(net.Extract(i)), _bits(x)), "the input blob differs from the restated floats"
            got = _forward(net, o, twice=graph)
            assert got.shape == want.shape and got.shape[0] == n
            assert np.array_equal(_bits(got), _bits(want)), f"{name} {tw}x{th} rf{rf}: FeedYUV420sp + Forward != FeedInput + Forward"
    net.close()


def test_net_feed_yuv420sp_single_frame_and_gray(cuda):
    """A single [h*3/2][w] frame: RGB + Forward equal to FeedInput + Forward; RGB2GRAY gives a 1-channel blob of the restated floats."""
    from feathercnn_amd import model_zoo
    net, i, o = _net(model_zoo.tiny_allsorts(), 0)
    f = _frames(np.random.default_rng(2), 1, 30, 26)[0]
    x = Y.yuv420sp_to_float(f, R.PIXEL_RGB, 20, 20, True)
    net.FeedInput(i, x)
    want = _forward(net, o)
    net.FeedYUV420sp(i, f, R.PIXEL_RGB, (20, 20), True)
    assert np.array_equal(_bits(_forward(net, o)), _bits(want))
    net.FeedYUV420sp(i, f, R.PIXEL_RGB2GRAY, (20, 20), False)
    assert np.array_equal(_bits(net.Extract(i)), _bits(Y.yuv420sp_to_float(f, R.PIXEL_RGB2GRAY, 20, 20, False)))
    net.close()


def test_cpp_yuv_application_end_to_end(cuda, tmp_path):
    """tests/cpp/yuv_app_main.cpp: resize_bilinear_yuv420sp + yuv420sp2rgb + from_pixels + substract_mean_normalize + FeedInput, then
    Net::FeedYUV420sp, on MobileNet-V1 -- same logits both ways, and equal to Net.FeedYUV420sp from Python."""
    from feathercnn_amd import _lib as L
    from feathercnn_amd import model_zoo
    p, b, i, o = model_zoo.mobilenet_v1()
    (tmp_path / "m.param").write_bytes(p)
    (tmp_path / "m.bin").write_bytes(b)
    w, h = 320, 240
    f = _frames(np.random.default_rng(6), 1, w, h)[0]
    (tmp_path / "frame.nv21").write_bytes(f.tobytes())
    libdir = os.path.dirname(L.lib_path())
    inc = os.path.join(ROOT, "include")
    exe = str(tmp_path / "yuv_app_main")
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-ffp-contract=off", "-I" + inc, "-I" + os.path.join(inc, "feather"),
                    os.path.join(ROOT, "tests", "cpp", "yuv_app_main.cpp"), "-o", exe, "-L" + libdir, "-lfeather_hip",
                    "-Wl,-rpath," + libdir], check=True, capture_output=True, text=True)
    a, c = str(tmp_path / "mat.f32"), str(tmp_path / "yuv.f32")
    run = subprocess.run([exe, str(tmp_path / "m.param"), str(tmp_path / "m.bin"), str(tmp_path / "frame.nv21"), str(w), str(h), "224",
                          "224", i, o, a, c], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "yuv app ok" in run.stdout, run.stdout + run.stderr
    from_mat, from_yuv = np.fromfile(a, np.float32), np.fromfile(c, np.float32)
    assert from_mat.size == 1000 and np.array_equal(_bits(from_mat), _bits(from_yuv))
    net, _, _ = _net((p, b, i, o), 1)
    net.FeedYUV420sp(i, f, R.PIXEL_RGB2BGR, (224, 224), True, np.array([104, 117, 123], np.float32), np.array([0.017] * 3, np.float32))
    assert np.array_equal(_bits(_forward(net, o).reshape(-1)), _bits(from_yuv))
    net.close()
