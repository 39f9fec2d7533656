"""The image output path on the MI355X: fhip_float_to_pixels (libfeather_pixout.so, float_to_pixels_kernel) byte for byte against the
reference's own Mat::to_pixels / to_pixels_resize results (tests/golden/yuv_golden.npz, topix_*) and against the numpy restatement
(tests/yuv_ref.py, tests/pixels_ref.py) over the whole case table of tests/pixout_cases.py -- every case compared, 0 differing bytes --;
guarded output buffers at every byte offset and odd pitches, 4-byte-aligned-only inputs; hipGraph capture; the values outside the
reference's domain; Net.FeedPixels -> Forward -> ExtractPixels against the restatement of what Extract returns, at fusion 1 and 3, with
sub-batch replicas and under hipGraph replay of the forward; the reference-style C++ application end to end."""
import collections
import concurrent.futures
import ctypes
import os
import subprocess

import numpy as np
import pytest

import pixels_ref as R
import pixout_cases as PC
import side_contract
import yuv_ref as Y
from guarded import Guarded

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "yuv_golden.npz")
FILL = 0xCD  # pitch gaps of the sweep's padded outputs


def _restate(x, t, tw, th, mean=None, norm=None):
    """[N][C][h][w] float32 -> [N][th][tw][cn] uint8: substract_mean_normalize, then to_pixels_resize per image."""
    v = R.mean_norm(x, mean, norm)
    return np.stack([Y.to_pixels_resize(v[i], t, tw, th) for i in range(v.shape[0])])


def _convert(x, t, tw, th, mean=None, norm=None):
    import torch

    from feathercnn_amd import float_to_pixels
    out = float_to_pixels(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda(), t, (tw, th), mean, norm)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _pitched(n, th, tw, cn, pitch):
    """(flat uint8 CUDA buffer filled with FILL, its [n][th][tw][cn] view with rows `pitch` bytes apart)."""
    import torch
    buf = torch.full((n * th * pitch,), FILL, dtype=torch.uint8, device="cuda")
    return buf, buf.as_strided((n, th, tw, cn), (th * pitch, pitch, cn, 1))


def _gaps_untouched(buf, n, th, tw, cn, pitch):
    rows = buf.view(n * th, pitch)
    return bool((rows[:, tw * cn:] == FILL).all())


def test_every_recorded_reference_result(cuda):
    """Each topix_* fixture as a batch of 1, and in the middle of a batch of distinct images of its shape."""
    g = np.load(GOLDEN)
    rng = np.random.default_rng(21)
    assert len(g["topixels"]) >= 10
    for t, w, h, c, tw, th in (tuple(int(v) for v in row) for row in g["topixels"]):
        m = g[f"mat_{w}x{h}x{c}"]
        want = g[f"topix_{t}_{w}x{h}x{c}_{tw}x{th}"]
        got = _convert(m[None], t, tw, th)
        assert got.shape == (1, th, tw, c) and np.array_equal(got[0], want), f"{t:#x} {w}x{h}x{c}->{tw}x{th}: differs from the reference"
        batch = np.stack([rng.uniform(-60, 320, m.shape).astype(np.float32), m, rng.uniform(-60, 320, m.shape).astype(np.float32),
                          m[:, ::-1].copy()])
        got = _convert(batch, t, tw, th)
        assert np.array_equal(got[1], want), f"{t:#x} {w}x{h}x{c}->{tw}x{th}: differs inside a batch"
        assert np.array_equal(got, _restate(batch, t, tw, th)), f"{t:#x} {w}x{h}x{c}->{tw}x{th}: batch neighbours"


def _pool_of(combo):
    """The inputs of one (type, geometry, mean / norm) and their restated result, with what the sweep asserts of its inputs."""
    index, (tn, t, gn, (w, h, tw, th), form) = combo
    cn = PC.CHANNELS[t]
    mean, norm = PC.mean_norm(form, cn)
    x = PC.make_input(1000 + index, PC.POOL, cn, h, w, mean, norm)
    v = R.mean_norm(x, mean, norm)
    # both clamps and truncation (not rounding) are exercised, inside the domain where the reference's cast is defined
    assert (v < 0).any() and (v > 255).any() and (v != np.trunc(v)).any() and np.abs(v).max() < 2.0 ** 31, (tn, gn, form)
    want = np.stack([Y.to_pixels_resize(v[i], t, tw, th) for i in range(PC.POOL)])
    return x, want


def test_sweep_every_case_bit_exact(cuda):
    """All six types x every geometry x batch {1, 3, 32} x the four mean / norm forms x {dense, pitched}: 0 differing bytes in every
    case, the pitch gaps untouched.  The restatement of a (type, geometry, form) is computed once for a pool of 32 distinct images
    (on worker threads, a few ahead of the device); the batches are windows of that pool."""
    import torch

    from feathercnn_amd import float_to_pixels
    combos = list(enumerate(PC.combos()))
    compared = collections.Counter()
    failures = []
    with concurrent.futures.ThreadPoolExecutor(8) as pool:
        pending = collections.deque()
        todo = iter(combos)

        def refill():
            while len(pending) < 12:
                c = next(todo, None)
                if c is None:
                    return
                pending.append((c, pool.submit(_pool_of, c)))

        refill()
        while pending:
            (index, (tn, t, gn, (w, h, tw, th), form)), fut = pending.popleft()
            x, want = fut.result()
            refill()
            cn = PC.CHANNELS[t]
            mean, norm = PC.mean_norm(form, cn)
            xd = torch.from_numpy(x).cuda()
            for batch in PC.BATCHES:
                win = PC.window(batch)
                xb = xd[win]
                for pitched in (False, True):
                    pitch = PC.pitch_of(tw, cn, pitched)
                    if pitched:
                        buf, view = _pitched(batch, th, tw, cn, pitch)
                        got = float_to_pixels(xb, t, (tw, th), mean, norm, out=view)
                    else:
                        got = float_to_pixels(xb, t, (tw, th), mean, norm)
                    torch.cuda.synchronize()
                    differing = int((got.cpu().numpy() != want[win]).sum())
                    print(f"pixout sweep {tn} {gn} {w}x{h}->{tw}x{th} {form} n={batch} pitch={pitch}: {differing} differing bytes")
                    compared[(tn, gn, form, batch, pitched)] += 1
                    if differing or (pitched and not _gaps_untouched(buf, batch, th, tw, cn, pitch)):
                        failures.append((tn, gn, form, batch, pitch, differing))
            del xd
    assert not failures, f"{len(failures)} cases differ (type, geometry, form, batch, pitch, bytes): {failures[:20]}"
    # every case of the table ran exactly once: nothing skipped, nothing filtered
    assert set(compared) == {(tn, gn, f, b, p) for tn, _, gn, _, f, b, p in PC.cases()} and set(compared.values()) == {1}
    assert len(compared) == 6 * len(PC.GEOMETRIES) * 3 * 4 * 2


GUARDED = [  # type, (w, h, tw, th), batch, byte offset of the output, pitch - row bytes, input offset in floats
    (R.PIXEL_GRAY, (36, 20, 36, 20), 3, 0, 0, 0), (R.PIXEL_GRAY, (36, 20, 36, 20), 3, 1, 0, 1), (R.PIXEL_GRAY, (37, 29, 37, 29), 2, 0, 3, 1),
    (R.PIXEL_GRAY, (17, 13, 42, 31), 3, 2, 2, 1), (R.PIXEL_GRAY, (45, 33, 24, 18), 2, 0, 8, 0),
    (R.PIXEL_RGB, (36, 20, 36, 20), 3, 0, 0, 1), (R.PIXEL_RGB, (36, 20, 36, 20), 2, 3, 0, 0), (R.PIXEL_BGR2RGB, (37, 29, 37, 29), 3, 0, 0, 1),
    (R.PIXEL_RGB2BGR, (37, 29, 37, 29), 2, 0, 17, 0), (R.PIXEL_BGR, (37, 29, 37, 29), 2, 0, 5, 1), (R.PIXEL_RGB, (17, 13, 42, 31), 3, 1, 7, 1),
    (R.PIXEL_BGR, (200, 3, 7, 150), 2, 0, 3, 0), (R.PIXEL_RGB2BGR, (45, 33, 24, 18), 3, 2, 0, 1),
    (R.PIXEL_RGBA, (36, 20, 36, 20), 3, 0, 0, 1), (R.PIXEL_RGBA, (36, 20, 36, 20), 2, 4, 0, 0), (R.PIXEL_RGBA, (37, 29, 37, 29), 2, 0, 12, 1),
    (R.PIXEL_RGBA, (37, 29, 37, 29), 2, 8, 4, 0), (R.PIXEL_RGBA, (17, 13, 42, 31), 3, 3, 1, 1), (R.PIXEL_RGBA, (45, 33, 24, 18), 2, 0, 16, 1),
]


@pytest.mark.parametrize("case", GUARDED, ids=[f"t{c[0]:#x}-{c[1][0]}x{c[1][1]}to{c[1][2]}x{c[1][3]}-n{c[2]}-at{c[3]}-gap{c[4]}-in{c[5]}" for c in GUARDED])
def test_guarded_buffers_and_misaligned_pointers(cuda, case):
    """The output is a guarded region (tests/guarded.py) entered at any byte offset, with dense rows and with pitches that leave the rows
    misaligned; the input a guarded region that may be only 4-byte aligned.  Every byte of [N][th][row span] is the restated value, no
    other byte of the allocation changes (guards, pitch gaps, the bytes before the first row and after the last), the input is intact."""
    import torch

    from feathercnn_amd import _lib
    t, (w, h, tw, th), n, at, gap, xoff = case
    cn = PC.CHANNELS[t]
    mean, norm = PC.mean_norm("both", cn)
    x = PC.make_input(77, n, cn, h, w, mean, norm)
    want = _restate(x, t, tw, th, mean, norm)
    row = tw * cn
    pitch = row + gap
    span = (n * th - 1) * pitch + row  # what the call may write: feather_pixout.h
    gin = Guarded(x.size, x, offset=xoff)
    gout = Guarded((at + span + 3) // 4 + 1, "poison")
    before = gout.snapshot().view(torch.uint8)
    lib = _lib.load_pixout_library()
    m = mean.ctypes.data_as(ctypes.c_void_p)
    s = norm.ctypes.data_as(ctypes.c_void_p)
    rc = lib.fhip_float_to_pixels(ctypes.c_void_p(gout.ptr + at), 0 if gap == 0 else pitch, ctypes.c_void_p(gin.ptr), n, t, w, h, tw, th, m, s,
                                  ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.fhip_pixout_last_error()
    torch.cuda.synchronize()
    assert gout.guards_intact() is None and gin.guards_intact() is None
    assert np.array_equal(gin.body.cpu().numpy().view(np.int32), x.reshape(-1).view(np.int32))
    after = gout.raw.view(torch.uint8)
    first = 4 * gout.lo + at
    body = after[first:first + span].cpu().numpy()
    rows = np.lib.stride_tricks.as_strided(body, (n * th, row), (pitch, 1))
    assert np.array_equal(rows.reshape(n, th, tw, cn), want)
    live = torch.zeros_like(after, dtype=torch.bool)
    inside = torch.from_numpy(np.add.outer(np.arange(n * th) * pitch, np.arange(row)).reshape(-1) + first).cuda()
    live[inside] = True
    changed = (after != before) & ~live
    assert not bool(changed.any()), f"{int(changed.sum())} bytes written outside [N][th][row span]"


def test_graph_capture(cuda):
    """One launch, nothing allocated or copied: the call is captured and replayed; mean / norm travel by value."""
    import torch

    from feathercnn_amd import float_to_pixels
    t, (w, h, tw, th), n = R.PIXEL_RGB2BGR, (37, 29, 48, 20), 3
    mean, norm = (a.copy() for a in PC.mean_norm("both", 3))
    x = PC.make_input(5, n, 3, h, w, mean, norm)
    x2 = PC.make_input(6, n, 3, h, w, mean, norm)
    want, want2 = _restate(x, t, tw, th, mean, norm), _restate(x2, t, tw, th, mean, norm)
    src = torch.from_numpy(x).cuda()
    out = torch.zeros((n, th, tw, 3), dtype=torch.uint8, device="cuda")
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        float_to_pixels(src, t, (tw, th), mean, norm, out=out)  # warm-up outside capture
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        float_to_pixels(src, t, (tw, th), mean, norm, out=out)
    mean[:] = 0  # the captured call keeps the values it was given
    for data, expect in ((x, want), (x2, want2)):
        src.copy_(torch.from_numpy(data))
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), expect)


def test_outside_the_domain_is_deterministic(cuda):
    """NaN -> 0, -inf and huge negative values -> 0, +inf and huge values -> 255 (the reference's cast is undefined there: documented in
    feather_pixout.h, not compared with it), at equal size and through the resize, whose neighbours are converted first."""
    x = np.zeros((1, 1, 4, 8), np.float32)
    x[0, 0, 0] = [np.nan, -np.inf, np.inf, -3e9, 3e9, 2.0 ** 31, -2.0 ** 31, 1e38]
    x[0, 0, 1] = [-0.0, -0.99, 0.99, 254.99, 255.0, 255.5, 256.0, 1.5]
    got = _convert(x, R.PIXEL_GRAY, 8, 4)
    assert got[0, 0, :, 0].tolist() == [0, 0, 255, 0, 255, 255, 0, 255]
    assert got[0, 1, :, 0].tolist() == [0, 0, 0, 254, 255, 255, 255, 1]
    bytes_ = got[0, :, :, 0][None]  # the byte image the resize works on
    up = _convert(x, R.PIXEL_GRAY, 13, 9)
    assert np.array_equal(up[0, :, :, 0], R.resize_bilinear(bytes_[..., None], 13, 9)[0, :, :, 0])


def _image_net():
    """3 -> 8 -> 3 channels, 3x3 / stride 1 / pad 1, no activation: a net whose output is an image of the input's size."""
    from feathercnn_amd import model_zoo
    b = model_zoo.GraphBuilder(seed=31)
    top = b.input("data", 3, 32, 40)
    top = b.conv("conv1", top, 3, 8, 3, 1, 1)
    top = b.conv("conv2", top, 8, 3, 3, 1, 1)
    param, weights = b.finish()
    return param, weights, "data", top


NET_CASES = [(1, False, 1), (3, False, 1), (1, False, 2), (3, False, 2), (1, True, 1), (3, True, 1), (3, True, 2)]  # fusion, graph, sub-batches


@pytest.mark.parametrize("fusion,graph,sub", NET_CASES, ids=[f"f{f}{'-graph' if g else ''}-sb{s}" for f, g, s in NET_CASES])
def test_net_round_trip(cuda, fusion, graph, sub):
    """FeedPixels -> Forward -> ExtractPixels equals to_pixels_resize(mean_norm(Extract)) of the same blob, with a mean / norm that spreads
    the net's output over about -60..320, at the blob's size and resized, for every output type of 3 channels."""
    from feathercnn_amd.net import Net
    param, weights, i, o = _image_net()
    net = Net(fusion=fusion, tuned=fusion == 3, graph=graph, sub_batches=sub)
    net.LoadParam(param)
    net.LoadWeights(weights)
    n, (w, h), (tw, th) = 5, (53, 47), (40, 32)
    px = np.random.default_rng(9).integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    net.FeedPixels(i, px, R.PIXEL_RGB, (tw, th), [104.0, 117.0, 123.0], [0.017, 0.017, 0.017])
    net.Forward()
    if graph:
        net.Forward()  # the replay
    f = net.Extract(o)
    assert f.shape == (n, 3, th, tw)
    lo, hi = f.min(axis=(0, 2, 3)), f.max(axis=(0, 2, 3))
    norm = (380.0 / (hi - lo)).astype(np.float32)
    mean = (lo + 60.0 / norm).astype(np.float32)
    v = R.mean_norm(f, mean, norm)
    assert v.min() < -50 and v.max() > 310 and (v < 0).any() and (v > 255).any() and (v != np.trunc(v)).any()
    for t in (R.PIXEL_RGB, R.PIXEL_BGR, R.PIXEL_RGB2BGR, R.PIXEL_BGR2RGB):
        for target in (None, (64, 27), (23, 50)):
            ow, oh = target or (tw, th)
            got = net.ExtractPixels(o, t, target, mean, norm)
            assert got.dtype == np.uint8 and got.shape == (n, oh, ow, 3)
            assert np.array_equal(got, _restate(f, t, ow, oh, mean, norm)), (t, target)
    assert np.array_equal(net.ExtractPixels(o, R.PIXEL_RGB), _restate(f, R.PIXEL_RGB, tw, th))  # no mean / norm
    assert np.array_equal(net.Extract(o).view(np.int32), f.view(np.int32))  # the blob is read, not changed
    from feathercnn_amd import FeatherHipError
    with pytest.raises(FeatherHipError, match="channels"):
        net.ExtractPixels(o, R.PIXEL_GRAY)
    with pytest.raises(FeatherHipError, match="not an output type"):
        net.ExtractPixels(o, R.PIXEL_RGB2GRAY)
    if fusion == 3 and net.chains(raw=True):
        with pytest.raises(FeatherHipError):  # a blob a fusion removed: the error Extract gives
            net.ExtractPixels("conv1", R.PIXEL_RGB)
    net.close()


def test_cpp_output_application_end_to_end(cuda, tmp_path):
    """tests/cpp/pixout_app_main.cpp: Extract + Mat::substract_mean_normalize + Mat::to_pixels_resize on the host against
    feather::Net::ExtractPixels and ExtractPixelsDevice -- the same bytes all three ways, and what Net.ExtractPixels gives from Python."""
    param, weights, i, o = _image_net()
    (tmp_path / "m.param").write_bytes(param)
    (tmp_path / "m.bin").write_bytes(weights)
    w, h, tw, th = 96, 72, 133, 50
    px = np.random.default_rng(12).integers(0, 256, (h, w, 3), dtype=np.uint8)
    (tmp_path / "img.u8").write_bytes(px.tobytes())
    from feathercnn_amd.net import Net
    net = Net(fusion=1)
    net.LoadParam(param)
    net.LoadWeights(weights)
    net.FeedPixels(i, px, R.PIXEL_RGB, None, [104.0, 117.0, 123.0], [0.017, 0.017, 0.017])
    net.Forward()
    f = net.Extract(o)
    lo, hi = f.min(axis=(0, 2, 3)), f.max(axis=(0, 2, 3))
    norm = (380.0 / (hi - lo)).astype(np.float32)  # the net's output spread over about -60..320
    mean = (lo + 60.0 / norm).astype(np.float32)
    exe = side_contract.build_app("pixout", tmp_path)
    outs = [str(tmp_path / f"{k}.u8") for k in ("mat", "host", "device")]
    run = subprocess.run([exe, str(tmp_path / "m.param"), str(tmp_path / "m.bin"), str(tmp_path / "img.u8"), str(w), str(h), str(tw), str(th),
                          i, o] + outs + [float(v).hex() for v in mean] + [float(v).hex() for v in norm],
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "pixout app ok" in run.stdout, run.stdout + run.stderr
    mat, host, device = (np.fromfile(p, np.uint8) for p in outs)
    assert mat.size == tw * th * 3 and np.array_equal(mat, host) and np.array_equal(mat, device)
    assert len(np.unique(mat)) > 100  # an image, not a constant
    got = net.ExtractPixels(o, R.PIXEL_RGB2BGR, (tw, th), mean, norm)
    assert np.array_equal(got.reshape(-1), mat)
    assert np.array_equal(got, _restate(f, R.PIXEL_RGB2BGR, tw, th, mean, norm))
    net.close()
