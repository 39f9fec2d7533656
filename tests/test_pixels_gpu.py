"""The uint8 image input path on the MI355X: fhip_pixels_to_float (affine_kernel over PixelSrc) bit-exact against the reference's own
from_pixels_resize (tests/golden/pixel_golden.npz) and the numpy restatement (tests/pixels_ref.py) over a seeded sweep; the mean / norm
forms; the guarded-buffer contract the other C-ABI routes keep (tests/test_contract_gpu.py); hipGraph capture; and Net.FeedPixels +
Forward equal to FeedInput(the restated floats) + Forward at fusion 0 / 3, with the graph, with sub-batch replicas, from host and
device memory and across a change of target size; the reference-style C++ application end to end."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import pixels_ref as R
import side_contract
from guarded import Guarded

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "pixel_golden.npz")
TYPES = list(R.TYPES.values())


def _bits(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    return a.view(np.int32)


def _convert(px, t, tw, th, mean=None, norm=None):
    import torch

    from feathercnn_amd import pixels_to_float
    out = pixels_to_float(torch.from_numpy(np.ascontiguousarray(px)).cuda(), t, (tw, th), mean, norm)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _lib():
    from feathercnn_amd import load_library
    return load_library()


_stream = side_contract.stream


def test_every_fixture_bit_exact_in_a_batch(cuda):
    """Each fixture image in the middle of a batch of three different images: every image is resized and converted on its own."""
    g = np.load(GOLDEN)
    rng = np.random.default_rng(11)
    n = 0
    for name, (t, w, h, tw, th) in zip(g["names"], g["cases"]):
        t, w, h, tw, th = int(t), int(w), int(h), int(tw), int(th)
        cin, _ = R.channels(t)
        img = g[f"in_c{cin}_{w}x{h}"]
        batch = np.stack([rng.integers(0, 256, img.shape, dtype=np.uint8), img, rng.integers(0, 256, img.shape, dtype=np.uint8)])
        got = _convert(batch, t, tw, th)
        want = g[f"out_{name}_{w}x{h}_{tw}x{th}"].astype(np.float32)
        assert np.array_equal(_bits(got[1]), _bits(want)), f"{name} {w}x{h}->{tw}x{th}: differs from the reference's from_pixels_resize"
        assert np.array_equal(_bits(got), _bits(R.from_pixels_resize(batch, t, tw, th))), f"{name} {w}x{h}->{tw}x{th}: batch neighbours"
        n += 1
    assert n == len(g["cases"]) >= 13 * 5


def _sweep_cases():
    rng = np.random.default_rng(2027)
    cases = [(R.PIXEL_BGR2RGB, 1920, 1080, 224, 224, 4), (R.PIXEL_RGB, 200, 160, 50, 40, 2), (R.PIXEL_RGBA2BGR, 20, 15, 80, 60, 2),
             (R.PIXEL_GRAY, 33, 17, 1, 9, 1), (R.PIXEL_RGB2GRAY, 31, 23, 13, 1, 2), (R.PIXEL_BGR2GRAY, 9, 5, 1, 1, 3),
             (R.PIXEL_GRAY2BGR, 640, 480, 224, 224, 1), (R.PIXEL_RGBA2GRAY, 257, 131, 1027, 65, 1)]
    while len(cases) < 120:
        t = TYPES[int(rng.integers(len(TYPES)))]
        w, h = int(rng.integers(2, 160)), int(rng.integers(2, 160))
        mode = int(rng.integers(4))
        if mode == 0:  # >= 4x down
            tw, th = max(1, w // int(rng.integers(4, 9))), max(1, h // int(rng.integers(4, 9)))
        elif mode == 1:  # >= 4x up
            tw, th = w * int(rng.integers(4, 7)) + int(rng.integers(0, 3)), h * int(rng.integers(4, 7))
        elif mode == 2:  # anything, odd widths included
            tw, th = int(rng.integers(1, 200)) | 1, int(rng.integers(1, 200))
        else:  # one axis kept
            tw, th = (w, int(rng.integers(1, 120))) if rng.integers(2) else (int(rng.integers(1, 120)), h)
        cases.append((t, w, h, tw, th, int(rng.integers(1, 4))))
    return cases


SWEEP = _sweep_cases()


def test_seeded_sweep_bit_exact(cuda):
    rng = np.random.default_rng(5)
    assert len(SWEEP) >= 100
    assert any(w >= 4 * tw and h >= 4 * th for _, w, h, tw, th, _ in SWEEP) and any(tw >= 4 * w and th >= 4 * h for _, w, h, tw, th, _ in SWEEP)
    assert any(tw == 1 for _, _, _, tw, _, _ in SWEEP) and any(th == 1 for _, _, _, _, th, _ in SWEEP)
    assert any(tw % 2 for _, _, _, tw, _, _ in SWEEP) and any(w % 2 for _, w, _, _, _, _ in SWEEP)
    for t, w, h, tw, th, n in SWEEP:
        cin, _ = R.channels(t)
        px = rng.integers(0, 256, (n, h, w, cin), dtype=np.uint8)
        got = _convert(px, t, tw, th)
        assert np.array_equal(_bits(got), _bits(R.from_pixels_resize(px, t, tw, th))), f"type {t:#x} {n}x {w}x{h} -> {tw}x{th}"


@pytest.mark.parametrize("form", ["none", "mean", "norm", "both"])
@pytest.mark.parametrize("t,w,h,tw,th", [(R.PIXEL_BGR2RGB, 64, 48, 32, 24), (R.PIXEL_RGBA, 17, 9, 17, 9), (R.PIXEL_RGB2GRAY, 40, 30, 21, 19)])
def test_mean_norm_forms(cuda, form, t, w, h, tw, th):
    cin, cout = R.channels(t)
    px = np.random.default_rng(9).integers(0, 256, (2, h, w, cin), dtype=np.uint8)
    rng = np.random.default_rng(3)
    mean = (rng.uniform(0, 255, cout).astype(np.float32) if form in ("mean", "both") else None)
    norm = (rng.uniform(-0.1, 0.1, cout).astype(np.float32) if form in ("norm", "both") else None)
    if form == "both":
        mean[0], norm[0] = np.float32(127.5), np.float32(1 / 127.5)  # the usual [-1, 1] scaling
    got = _convert(px, t, tw, th, mean, norm)
    want = R.from_pixels_resize(px, t, tw, th, mean, norm)
    assert np.array_equal(_bits(got), _bits(want)), form
    if form == "mean":  # the one-sided forms are the exact IEEE operation
        assert np.array_equal(got, (R.from_pixels_resize(px, t, tw, th) - mean.reshape(1, -1, 1, 1)).astype(np.float32))


def _guarded_source(px: np.ndarray, byte_offset: int):
    """The uint8 images at `byte_offset` into the body of a guarded region; returns (Guarded, device pointer)."""
    import torch
    raw = px.reshape(-1)
    nf = (raw.size + byte_offset + 3) // 4 + 1
    g = Guarded(nf, np.zeros(nf, np.float32))
    body = g.raw.view(torch.uint8)[4 * g.lo:4 * (g.lo + nf)]
    body[byte_offset:byte_offset + raw.size].copy_(torch.from_numpy(raw))
    return g, g.ptr + byte_offset


@pytest.mark.parametrize("t,w,h,tw,th", [(R.PIXEL_BGR2RGB, 37, 29, 24, 16), (R.PIXEL_GRAY, 13, 7, 13, 7), (R.PIXEL_RGBA2GRAY, 9, 11, 23, 5),
                                         (R.PIXEL_RGB, 31, 3, 8, 40)])
def test_guarded_contract(cuda, t, w, h, tw, th):
    """Guards intact, every output word written, the source unchanged; a second call bit-identical; the source at byte offsets 0-3 and
    the output 4 bytes past a 16-byte boundary (the scalar-store form) give the same bits."""
    import torch
    lib = _lib()
    cin, cout = R.channels(t)
    n = 3
    px = np.random.default_rng(1).integers(0, 256, (n, h, w, cin), dtype=np.uint8)
    want = R.from_pixels_resize(px, t, tw, th)
    count = n * cout * th * tw
    for boff in range(4):
        src, sp = _guarded_source(px, boff)
        before = src.snapshot()
        for ooff in (0, 1):
            out = Guarded(count, "poison", ooff)
            for rep in range(2):
                assert lib.fhip_pixels_to_float(ctypes.c_void_p(out.ptr), ctypes.c_void_p(sp), n, t, w, h, tw, th, None, None, _stream()) == 0
                torch.cuda.synchronize()
                assert out.guards_intact() is None, f"offset {boff}/{ooff}: wrote outside the output: {out.guards_intact()}"
                assert out.unwritten() == 0, f"offset {boff}/{ooff}: {out.unwritten()} of {count} output words unwritten"
                assert src.unchanged(before), f"offset {boff}: the source changed"
                got = out.body.cpu().numpy().reshape(want.shape)
                assert np.array_equal(_bits(got), _bits(want)), f"byte offset {boff}, output offset {ooff}, call {rep + 1}"


def test_graph_capture(cuda):
    """fhip_pixels_to_float is stream-capturable: mean / norm are read at the call, nothing is allocated or copied; a replay converts
    whatever the source buffer holds then."""
    import torch

    from feathercnn_amd import pixels_to_float
    t, w, h, tw, th = R.PIXEL_BGR2RGB, 64, 48, 32, 32
    mean, norm = np.array([104, 117, 123], np.float32), np.array([0.017, 0.017, 0.017], np.float32)
    rng = np.random.default_rng(4)
    a, b = (rng.integers(0, 256, (2, h, w, 3), dtype=np.uint8) for _ in range(2))
    src = torch.from_numpy(a).cuda()
    out = torch.empty((2, 3, th, tw), device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        pixels_to_float(src, t, (tw, th), mean, norm, out=out)  # warm-up outside capture
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        pixels_to_float(src, t, (tw, th), mean, norm, out=out)
    mean[:] = 0  # the captured call keeps the values it was given
    for img in (a, b):
        src.copy_(torch.from_numpy(img))
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        want = R.from_pixels_resize(img, t, tw, th, np.array([104, 117, 123], np.float32), norm)
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


NET_CASES = [  # model, fusion, graph, sub_batches, batch, source (w, h), targets
    ("tiny", 0, False, 1, 2, (37, 29), [(20, 20), (24, 16)]),
    ("tiny", 3, True, 1, 3, (41, 17), [(20, 20), (28, 28)]),
    ("tiny", 1, False, 2, 5, (33, 35), [(20, 20), (16, 24)]),
    ("mobilenet", 0, False, 1, 2, (300, 200), [(224, 224)]),
    ("mobilenet", 3, True, 1, 2, (300, 200), [(224, 224)]),
    ("mobilenet", 3, True, 2, 5, (256, 256), [(224, 224)]),
]


@pytest.mark.parametrize("on_device", [0, 1], ids=["host", "device"])
@pytest.mark.parametrize("case", NET_CASES, ids=[f"{c[0]}-f{c[1]}{'-graph' if c[2] else ''}-sb{c[3]}-n{c[4]}" for c in NET_CASES])
def test_net_feed_pixels_equals_feed_input(cuda, case, on_device):
    """FeedPixels + Forward is bit-identical to FeedInput(the restated floats) + Forward on the same net, across a change of target
    size (the blob is reshaped, the graph dropped and re-recorded)."""
    import torch

    from feathercnn_amd import model_zoo
    name, fusion, graph, sub, n, (w, h), targets = case
    model = model_zoo.tiny_allsorts() if name == "tiny" else model_zoo.mobilenet_v1()
    net, i, o = _net(model, fusion, graph, sub)
    t = R.PIXEL_BGR2RGB
    mean, norm = np.array([104, 117, 123], np.float32), np.array([0.017, 0.018, 0.019], np.float32)
    px = np.random.default_rng(8).integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    for tw, th in targets:
        x = R.from_pixels_resize(px, t, tw, th, mean, norm)
        net.FeedInput(i, x)
        want = _forward(net, o, twice=graph)
        if fusion == 0:
            assert np.array_equal(_bits(net.Extract(i)), _bits(x))
        src = torch.from_numpy(px).cuda() if on_device else px
        net.FeedPixels(i, src, t, (tw, th), mean, norm)
        if fusion == 0:
            assert np.array_equal(_bits(net.Extract(i)), _bits(x)), "the input blob differs from the restated floats"
        got = _forward(net, o, twice=graph)
        assert got.shape == want.shape == (n,) + want.shape[1:]
        assert np.array_equal(_bits(got), _bits(want)), f"{name} {tw}x{th}: FeedPixels + Forward != FeedInput + Forward"
    net.close()


def test_net_feed_pixels_single_image_and_gray(cuda):
    """A single [H][W][C] image, gray source replicated into the net's 3 channels (GRAY2RGB)."""
    from feathercnn_amd import model_zoo
    net, i, o = _net(model_zoo.tiny_allsorts(), 1)
    px = np.random.default_rng(2).integers(0, 256, (30, 25, 1), dtype=np.uint8)
    x = R.from_pixels_resize(px, R.PIXEL_GRAY2RGB, 20, 20)
    net.FeedInput(i, x)
    want = _forward(net, o)
    net.FeedPixels(i, px, R.PIXEL_GRAY2RGB, (20, 20))
    assert np.array_equal(_bits(_forward(net, o)), _bits(want))
    net.close()


def test_cpp_pixel_application_end_to_end(cuda, tmp_path):
    """tests/cpp/pixel_app_main.cpp: Mat::from_pixels_resize + substract_mean_normalize + FeedInput, then FeedPixels, on MobileNet-V1 --
    same logits both ways, and equal to Net.FeedPixels from Python."""
    from feathercnn_amd import _lib as L
    from feathercnn_amd import model_zoo
    p, b, i, o = model_zoo.mobilenet_v1()
    (tmp_path / "m.param").write_bytes(p)
    (tmp_path / "m.bin").write_bytes(b)
    w, h = 320, 240
    px = np.random.default_rng(6).integers(0, 256, (h, w, 3), dtype=np.uint8)
    (tmp_path / "img.u8").write_bytes(px.tobytes())
    libdir = os.path.dirname(L.lib_path())
    inc = os.path.join(ROOT, "include")
    exe = str(tmp_path / "pixel_app_main")
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-ffp-contract=off", "-I" + inc, "-I" + os.path.join(inc, "feather"),
                    os.path.join(ROOT, "tests", "cpp", "pixel_app_main.cpp"), "-o", exe, "-L" + libdir, "-lfeather_hip",
                    "-Wl,-rpath," + libdir], check=True, capture_output=True, text=True)
    a, c = str(tmp_path / "mat.f32"), str(tmp_path / "pix.f32")
    run = subprocess.run([exe, str(tmp_path / "m.param"), str(tmp_path / "m.bin"), str(tmp_path / "img.u8"), str(w), str(h), "224", "224",
                          i, o, a, c], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "pixel app ok" in run.stdout, run.stdout + run.stderr
    from_mat, from_pixels = np.fromfile(a, np.float32), np.fromfile(c, np.float32)
    assert from_mat.size == 1000 and np.array_equal(_bits(from_mat), _bits(from_pixels))
    net, _, _ = _net((p, b, i, o), 1)
    net.FeedPixels(i, px, R.PIXEL_BGR2RGB, (224, 224), np.array([104, 117, 123], np.float32), np.array([0.017] * 3, np.float32))
    assert np.array_equal(_bits(_forward(net, o).reshape(-1)), _bits(from_pixels))
    net.close()
