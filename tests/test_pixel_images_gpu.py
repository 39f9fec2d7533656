"""Mixed-size / cropped image batches on the MI355X: fhip_pixels_to_float_images (affine_kernel over a planned PixelSrc) bit-exact against
from_pixels_resize of a dense copy of each ROI (tests/pixels_ref.py) over all 13 pixel types and the size classes that matter; equal to
fhip_pixels_to_float on an equal-size batch; the guarded-buffer contract with poison around every ROI; graph capture; Net.FeedPixelImages
from host and device memory equal to FeedInput of the restated batch, with sub-batch replicas and across a target-size change; and the
C++ application end to end."""
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
TYPES = list(R.TYPES.values())
MEAN = np.array([104.0, 116.67, 122.68, 0.5], np.float32)
NORM = np.array([0.017, 1.0 / 58.8, 0.0175, -2.0], np.float32)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _lib():
    from feathercnn_amd import load_library
    return load_library()


_stream = side_contract.stream


def _want(img, roi, t, tw, th, mean=None, norm=None):
    """from_pixels_resize of a dense copy of the ROI, then mean / norm: the reference's result for one image."""
    x, y, w, h = roi if roi is not None else (0, 0, img.shape[1], img.shape[0])
    return R.from_pixels_resize(np.ascontiguousarray(img[y:y + h, x:x + w])[None], t, tw, th, mean, norm)[0]


def _mixed_batch(rng, t, tw, th):
    """(images [H][W][C] numpy, pitched views included, rois) covering the size classes: down / up / identity, extreme aspect ratios,
    2-pixel ROI axes, ROIs touching each edge, pitched sources."""
    cin, _ = R.channels(t)

    def img(h, w, pad=0):
        a = rng.integers(0, 256, (h, w + pad, cin), dtype=np.uint8)
        return a[:, :w] if pad else a  # pad: a row-strided view (pitch > w * cin)

    items = [
        (img(150, 200), None),                     # down
        (img(7, 9), None),                         # up
        (img(th + 6, tw + 5), (3, 2, tw, th)),     # identity size: no resize, read as it is
        (img(4, 300), None),                       # extreme aspect ratios
        (img(200, 3), None),
        (img(30, 40), (17, 9, 2, 2)),              # 2-pixel ROI axes
        (img(30, 40), (5, 3, 2, 25)),
        (img(30, 40), (0, 4, 12, 11)),             # ROI touching the left edge
        (img(30, 40), (6, 0, 12, 11)),             # top
        (img(30, 40), (28, 7, 12, 11)),            # right
        (img(30, 40), (3, 19, 12, 11)),            # bottom
        (img(33, 27, pad=13), None),               # pitched, whole image
        (img(64, 48, pad=5), (7, 5, 31, 50)),      # pitched, with a ROI
        (img(th, tw), None),                       # identity, whole image
    ]
    return [a for a, _ in items], [r for _, r in items]


def _is_view(a):
    return a.base is not None and a.base.ndim == 3 and a.base.shape[0] == a.shape[0] and a.base.shape[2] == a.shape[2]


@pytest.mark.parametrize("t", TYPES, ids=list(R.TYPES))
def test_mixed_batch_bit_exact(cuda, t):
    import torch

    from feathercnn_amd import pixels_images_to_float
    rng = np.random.default_rng(1000 + t % 997)
    _, cout = R.channels(t)
    for k, (tw, th, aligned) in enumerate([(24, 20, True), (23, 17, True), (24, 20, False)]):
        imgs, rois = _mixed_batch(rng, t, tw, th)
        mean, norm = (MEAN[:cout], NORM[:cout]) if (k + t) % 2 else (None, None)
        # odd images as dense copies, even ones with the host array's layout (a pitched view stays a pitched view)
        dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda() if i % 2 or not _is_view(a) else torch.from_numpy(a.base).cuda()[:, :a.shape[1]]
               for i, a in enumerate(imgs)]
        assert any(d.stride(0) > d.shape[1] * d.shape[2] for d in dev), "no pitched source in the batch"
        count = len(imgs) * cout * th * tw
        flat = torch.empty(count + 4, device="cuda")
        out = flat[(0 if aligned else 1):][:count].view(len(imgs), cout, th, tw)
        out.fill_(float("nan"))
        pixels_images_to_float(dev, t, (tw, th), rois, mean, norm, out=out)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        for i, (a, r) in enumerate(zip(imgs, rois)):
            want = _want(a, r, t, tw, th, mean, norm)
            assert np.array_equal(_bits(got[i]), _bits(want)), f"type {t:#x} image {i} roi {r} of {a.shape} -> {tw}x{th} aligned={aligned}"


def test_equal_size_batch_equals_pixels_to_float(cuda):
    import torch

    from feathercnn_amd import pixels_images_to_float, pixels_to_float
    for t, w, h, tw, th in [(R.PIXEL_BGR2RGB, 64, 48, 32, 24), (R.PIXEL_RGBA2GRAY, 37, 29, 23, 31), (R.PIXEL_GRAY2RGB, 20, 20, 20, 20)]:
        cin, cout = R.channels(t)
        px = torch.randint(0, 256, (5, h, w, cin), dtype=torch.uint8, device="cuda")
        mean, norm = MEAN[:cout], NORM[:cout]
        a = pixels_to_float(px, t, (tw, th), mean, norm)
        b = pixels_images_to_float([px[i] for i in range(5)], t, (tw, th), None, mean, norm)
        torch.cuda.synchronize()
        assert np.array_equal(_bits(a.cpu().numpy()), _bits(b.cpu().numpy())), hex(t)


def _plan(descs, t, tw, th):
    from feathercnn_amd.pixels import _plan as plan
    return plan(descs, t, tw, th)


def test_guarded_contract(cuda):
    """Every image in one guarded region, poison bytes around each ROI and in the pitch padding, the last image's ROI ending at the
    region's last byte; the output 0 or 1 float past a 16-byte boundary.  Guards intact, every output word written, the source unchanged,
    and the output equal to the unguarded run and the reference."""
    import torch

    from feathercnn_amd import _lib as L
    from feathercnn_amd import pixels_images_to_float
    lib = _lib()
    t, tw, th = R.PIXEL_BGR2RGB, 20, 16
    cin, cout = R.channels(t)
    rng = np.random.default_rng(77)
    specs = [(31, 23, 31 * 3 + 7, (4, 3, 17, 12)), (40, 12, 40 * 3, (0, 0, 40, 12)), (9, 30, 9 * 3 + 1, (7, 28, 2, 2)),
             (25, 25, 25 * 3 + 3, (20, 0, 5, 25)), (50, 40, 50 * 3 + 9, (13, 21, 37, 19))]
    offs, pos = [], 5
    for w, h, pitch, _ in specs:
        offs.append(pos)
        pos += h * pitch + 11  # poison between images
    w, h, pitch, (rx, ry, rw, rh) = specs[-1]
    end_of_roi = (ry + rh - 1) * pitch + (rx + rw) * cin
    body_bytes = (offs[-1] + end_of_roi + 3) // 4 * 4
    offs[-1] = body_bytes - end_of_roi  # the last ROI's last byte is the region's last byte
    body = np.full(body_bytes, 0x5A, np.uint8)
    imgs = []
    for (w, h, pitch, (rx, ry, rw, rh)), off in zip(specs, offs):
        a = rng.integers(0, 256, (h, w, cin), dtype=np.uint8)
        imgs.append(a)
        for y in range(ry, ry + rh):  # only the ROI's bytes: the rest of the image stays poison
            o = off + y * pitch + rx * cin
            body[o:o + rw * cin] = a[y, rx:rx + rw].reshape(-1)
    src = Guarded(body_bytes // 4, body.view(np.float32))
    before = src.snapshot()
    descs = (L.fhip_pixel_image * len(specs))()
    for d, (w, h, pitch, roi), off in zip(descs, specs, offs):
        d.data, d.w, d.h, d.stride = src.ptr + off, w, h, pitch
        d.roi_x, d.roi_y, d.roi_w, d.roi_h = roi
    plan = _plan(descs, t, tw, th)
    plan_dev = torch.from_numpy(plan).cuda()
    want = np.stack([_want(a, s[3], t, tw, th, MEAN[:3], NORM[:3]) for a, s in zip(imgs, specs)])
    dense = [torch.from_numpy(np.ascontiguousarray(a[s[3][1]:s[3][1] + s[3][3], s[3][0]:s[3][0] + s[3][2]])).cuda() for a, s in zip(imgs, specs)]
    plain = pixels_images_to_float(dense, t, (tw, th), None, MEAN[:3], NORM[:3]).cpu().numpy()
    assert np.array_equal(_bits(plain), _bits(want))
    m, s = np.ascontiguousarray(MEAN[:3]), np.ascontiguousarray(NORM[:3])
    for ooff in (0, 1):
        out = Guarded(want.size, "poison", ooff)
        for rep in range(2):
            rc = lib.fhip_pixels_to_float_images(ctypes.c_void_p(out.ptr), plan.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(plan_dev.data_ptr()),
                                                 m.ctypes.data_as(ctypes.c_void_p), s.ctypes.data_as(ctypes.c_void_p), _stream())
            assert rc == 0
            torch.cuda.synchronize()
            assert out.guards_intact() is None, f"output offset {ooff}: wrote outside the output: {out.guards_intact()}"
            assert out.unwritten() == 0, f"output offset {ooff}: {out.unwritten()} output words unwritten"
            assert src.guards_intact() is None and src.unchanged(before), "the source changed"
            got = out.body.cpu().numpy().reshape(want.shape)
            assert np.array_equal(_bits(got), _bits(want)), f"output offset {ooff}, call {rep + 1}"


def test_graph_capture(cuda):
    """fhip_pixels_to_float_images captured into a graph: a replay after the source bytes change equals an eager run on the new bytes."""
    import torch

    from feathercnn_amd import pixels_images_to_float
    from feathercnn_amd.pixels import _image_descs
    lib = _lib()
    t, tw, th = R.PIXEL_BGR2RGB, 32, 24
    rng = np.random.default_rng(4)
    shapes = [(48, 64), (20, 30), (24, 32), (90, 17)]
    rois = [(8, 4, 40, 30), None, None, (2, 10, 12, 70)]
    srcs = [torch.from_numpy(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).cuda() for h, w in shapes]
    descs, _, keep = _image_descs(srcs, t, rois)
    plan = _plan(descs, t, tw, th)
    plan_dev = torch.from_numpy(plan).cuda()
    mean, norm = np.array([104, 117, 123], np.float32), np.array([0.017, 0.018, 0.019], np.float32)
    out = torch.empty((len(srcs), 3, th, tw), device="cuda")

    def call():
        assert lib.fhip_pixels_to_float_images(ctypes.c_void_p(out.data_ptr()), plan.ctypes.data_as(ctypes.c_void_p),
                                               ctypes.c_void_p(plan_dev.data_ptr()), mean.ctypes.data_as(ctypes.c_void_p),
                                               norm.ctypes.data_as(ctypes.c_void_p), _stream()) == 0
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()  # warm-up outside capture
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    mean_at_capture = mean.copy()
    mean[:] = 0  # the captured call keeps the values it was given
    for _ in range(2):
        for x in srcs:
            x.copy_(torch.from_numpy(rng.integers(0, 256, tuple(x.shape), dtype=np.uint8)))
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        eager = pixels_images_to_float(srcs, t, (tw, th), rois, mean_at_capture, norm)
        torch.cuda.synchronize()
        assert np.array_equal(_bits(out.cpu().numpy()), _bits(eager.cpu().numpy()))
        want = np.stack([_want(x.cpu().numpy(), r, t, tw, th, mean_at_capture, norm) for x, r in zip(srcs, rois)])
        assert np.array_equal(_bits(out.cpu().numpy()), _bits(want))
    del keep


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


NET_CASES = [  # fusion, graph, sub_batches, batch
    (0, False, 2, 5),
    (0, False, 1, 3),
    (3, True, 2, 5),
]


@pytest.mark.parametrize("on_device", [0, 1], ids=["host", "device"])
@pytest.mark.parametrize("case", NET_CASES, ids=[f"f{c[0]}{'-graph' if c[1] else ''}-sb{c[2]}-n{c[3]}" for c in NET_CASES])
def test_net_feed_pixel_images_equals_feed_input(cuda, case, on_device):
    """FeedPixelImages + Forward is bit-identical to FeedInput(the restated batch) + Forward on tiny_allsorts, across a change of target
    size; the input blob (fusion 0) equals the restated floats."""
    import torch

    from feathercnn_amd import model_zoo
    fusion, graph, sub, n = case
    net, i, o = _net(model_zoo.tiny_allsorts(), fusion, graph, sub)
    t = R.PIXEL_BGR2RGB
    mean, norm = np.array([104, 117, 123], np.float32), np.array([0.017, 0.018, 0.019], np.float32)
    rng = np.random.default_rng(8 + n)
    sizes = [(37, 29), (64, 48), (20, 20), (9, 40), (120, 33), (31, 31), (50, 18)][:n]
    full = [rng.integers(0, 256, (h, w + 3, 3), dtype=np.uint8) for w, h in sizes]
    imgs = [a[:, :w] for a, (w, h) in zip(full, sizes)]  # pitched views
    rois = [None if k % 2 else (1, 2, max(2, w - 3), max(2, h - 4)) for k, (w, h) in enumerate(sizes)]
    for tw, th in [(20, 20), (24, 16)]:
        x = np.stack([_want(a, r, t, tw, th, mean, norm) for a, r in zip(imgs, rois)])
        net.FeedInput(i, x)
        want = _forward(net, o, twice=graph)
        src = [torch.from_numpy(a).cuda()[:, :w] for a, (w, h) in zip(full, sizes)] if on_device else imgs
        net.FeedPixelImages(i, src, t, (tw, th), rois, mean, norm)
        if fusion == 0:
            assert np.array_equal(_bits(net.Extract(i)), _bits(x)), "the input blob differs from the restated floats"
        got = _forward(net, o, twice=graph)
        assert got.shape == want.shape and got.shape[0] == n
        assert np.array_equal(_bits(got), _bits(want)), f"{tw}x{th}: FeedPixelImages + Forward != FeedInput + Forward"
    net.close()


def test_cpp_pixel_images_application_end_to_end(cuda, tmp_path):
    """tests/cpp/pixel_images_app_main.cpp: dense ROI copies + Mat::from_pixels_resize + substract_mean_normalize + FeedInput, then
    FeedPixelImages, on tiny_allsorts -- same output both ways, and equal to Net.FeedPixelImages from Python."""
    from feathercnn_amd import _lib as L
    from feathercnn_amd import model_zoo
    p, b, i, o = model_zoo.tiny_allsorts()
    (tmp_path / "m.param").write_bytes(p)
    (tmp_path / "m.bin").write_bytes(b)
    rng = np.random.default_rng(6)
    specs = [(64, 48, 64 * 3 + 4, (10, 4, 40, 40)), (30, 22, 90, (0, 0, 30, 22)), (200, 20, 600, (150, 3, 50, 17))]
    blob, lines, imgs = b"", [], []
    for w, h, pitch, (rx, ry, rw, rh) in specs:
        a = rng.integers(0, 256, (h, pitch), dtype=np.uint8)
        blob += a.tobytes()
        imgs.append(a[:, :w * 3].reshape(h, w, 3))
        lines.append(f"{w} {h} {pitch} {rx} {ry} {rw} {rh}")
    (tmp_path / "img.u8").write_bytes(blob)
    libdir = os.path.dirname(L.lib_path())
    inc = os.path.join(ROOT, "include")
    exe = str(tmp_path / "pixel_images_app_main")
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-ffp-contract=off", "-I" + inc, "-I" + os.path.join(inc, "feather"),
                    os.path.join(ROOT, "tests", "cpp", "pixel_images_app_main.cpp"), "-o", exe, "-L" + libdir, "-lfeather_hip",
                    "-Wl,-rpath," + libdir], check=True, capture_output=True, text=True)
    a, c = str(tmp_path / "mat.f32"), str(tmp_path / "img.f32")
    run = subprocess.run([exe, str(tmp_path / "m.param"), str(tmp_path / "m.bin"), str(tmp_path / "img.u8"), "20", "20", i, o, a, c],
                         input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "pixel images app ok" in run.stdout, run.stdout + run.stderr
    from_mat, from_images = np.fromfile(a, np.float32), np.fromfile(c, np.float32)
    assert from_mat.size > 0 and np.array_equal(_bits(from_mat), _bits(from_images))
    net, _, _ = _net((p, b, i, o), 1)
    net.FeedPixelImages(i, imgs, R.PIXEL_BGR2RGB, (20, 20), [s[3] for s in specs], np.array([104, 117, 123], np.float32),
                        np.array([0.017] * 3, np.float32))
    assert np.array_equal(_bits(_forward(net, o).reshape(-1)), _bits(from_images))
    net.close()
