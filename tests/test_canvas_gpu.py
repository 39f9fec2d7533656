"""Chained Winograd runs on 2x2 image canvases (include/feather_hip/feather_canvas.h, libfeather_canvas.so).

The oracle is inside the project: the canvases are assembled on the host (N / 4 images of (2H + 2)^2 pixels, zero seam), the existing PLAIN
stage kernels run on them as ordinary images of that size (fhip_winograd_f63_input_transform / _tile_gemm / _output_transform), and the seam is
zeroed between layers.  The canvas run's V, its M and its final activation must equal that EXACTLY: same butterflies, same values, same order.
V, M and the output are filled with NaN before every canvas run, so an unmasked seam or a column nobody wrote shows up in the result.
Then the compiled reference per image, the net-level choice on VGG-16, and the GEMM grids in a kernel trace."""
import os

import numpy as np
import pytest

import ktrace
from oracle import conv_geom, nerr

pytestmark = pytest.mark.gpu
WINO = 4  # FHIP_WINOGRADF63
TOL = 1e-4  # tests/test_net_gpu.py's
HERE = os.path.dirname(os.path.abspath(__file__))


def _layer(cuda, ic, oc, h, bias=True, relu=True, seed=0):
    import torch

    from feathercnn_amd import ConvLayer, ConvParam
    rng = np.random.default_rng(seed)
    wt = (rng.standard_normal((oc, ic, 3, 3)) / np.sqrt(9 * ic)).astype(np.float32)
    b = rng.uniform(-0.5, 0.5, oc).astype(np.float32) if bias else None
    prm = ConvParam(output_channels=oc, input_channels=ic, input_h=h, input_w=h, kernel_h=3, kernel_w=3, stride_h=1, stride_w=1, pad_left=1,
                    pad_right=1, pad_top=1, pad_bottom=1, group=1, bias_term=bias, activation=1 if relu else 0)
    return ConvLayer(prm, torch.from_numpy(wt).to(cuda), None if b is None else torch.from_numpy(b).to(cuda), algo=WINO), wt, b


def _to_canvas(x, h):
    """[N][C][h][h] -> [N/4][C][2h+2][2h+2], image n = quadrant n % 4 (row (n % 4) // 2, column n % 2) of canvas n // 4, zero seam."""
    import torch
    n, c = x.shape[:2]
    cv = torch.zeros((n // 4, c, 2 * h + 2, 2 * h + 2), dtype=x.dtype, device=x.device)
    for q in range(4):
        oy, ox = (q >> 1) * (h + 2), (q & 1) * (h + 2)
        cv[:, :, oy:oy + h, ox:ox + h] = x[q::4]
    return cv


def _from_canvas(cv, h, pitch):
    import torch
    nc, c = cv.shape[:2]
    x = torch.empty((4 * nc, c, h, h), dtype=cv.dtype, device=cv.device)
    for q in range(4):
        oy, ox = (q >> 1) * pitch, (q & 1) * pitch
        x[q::4] = cv[:, :, oy:oy + h, ox:ox + h]
    return x


def _stage(lib, param_c, batch, x, layer, plan):
    """The plain stage kernels on `x` as an ordinary batch of images -> (V, M, Y before pooling)."""
    import ctypes

    import torch

    from feathercnn_amd.booster import _check, _ptr, _stream
    v = torch.zeros(plan.v_bytes // 4, dtype=torch.float32, device=x.device)
    m = torch.zeros(plan.m_bytes // 4, dtype=torch.float32, device=x.device)
    y = torch.empty((batch, param_c.output_channels, param_c.output_h, param_c.output_w), dtype=torch.float32, device=x.device)
    _check(lib.fhip_winograd_f63_input_transform(ctypes.byref(param_c), batch, _ptr(v), _ptr(x.contiguous()), _stream()), "input_transform")
    _check(lib.fhip_winograd_f63_tile_gemm(ctypes.byref(param_c), batch, _ptr(m), _ptr(layer.packed), _ptr(v), _stream()), "tile_gemm")
    _check(lib.fhip_winograd_f63_output_transform(ctypes.byref(param_c), batch, _ptr(y), _ptr(m), _ptr(layer.bias), _stream()), "output_transform")
    return v, m, y


def _same(got, want, plan, rows, what):
    """bit equality of the columns a plan holds (the padding columns of V are nobody's)"""
    import torch

    from feathercnn_amd.booster import winograd_rows
    g, w = winograd_rows(got, plan, rows)[:, :, :plan.columns], winograd_rows(want, plan, rows)[:, :, :plan.columns]
    assert not torch.isnan(g).any(), f"{what}: NaN (a column or a seam nobody wrote)"
    assert torch.equal(g, w), f"{what}: max diff {(g - w).abs().max().item():.3e}"


# name, H of the canvas layers, batch, channels [c0, c1, ...] (layer i: c[i] -> c[i + 1]), bias, relu, pooling behind the LAST layer, exit
# exit=False: plain 2H (pool) -> canvas H -> canvas H [-> pool] -> output        (ENTRY, INSIDE, canvas output transform)
# exit=True:  plain 2H (pool) -> canvas H -> canvas H -> pool -> plain H/2       (ENTRY, INSIDE, EXIT)
RUNS = [
    ("h14_n4_c64", 14, 4, [64, 64, 64, 64], True, True, True, False),
    ("h14_n8_plain_epilogue", 14, 8, [64, 64, 64, 64], False, False, False, False),
    ("h14_n32_vgg", 14, 32, [64, 512, 512, 512], True, True, True, False),
    ("h14_n8_bias_only", 14, 8, [16, 24, 40, 8], True, False, False, False),
    ("h56_n4_c64_exit", 56, 4, [64, 64, 64, 64, 64], True, True, False, True),
    ("h56_n8_vgg_exit", 56, 8, [64, 128, 256, 256, 64], True, True, False, True),
    ("h56_n32_c64_exit", 56, 32, [16, 64, 64, 64, 16], True, True, False, True),
    ("h56_n4_no_bias_relu_exit", 56, 4, [8, 16, 24, 16, 8], False, True, False, True),
    ("h56_n4_output_unpooled", 56, 4, [8, 64, 64, 16], False, False, False, False),
    ("h56_n8_output_pooled", 56, 8, [8, 16, 64, 64], True, True, True, False),
]


def _build(cuda, run):
    name, h, batch, ch, bias, relu, last_pool, exit_ = run
    sizes = [2 * h, h, h] + ([h // 2] if exit_ else [])
    layers, host = [], []
    for i, s in enumerate(sizes):
        l, w, b = _layer(cuda, ch[i], ch[i + 1], s, bias=bias, relu=relu, seed=200 + i)
        l.param.batch = batch
        layers.append(l)
        host.append((w, b))
    pools = [True, False, True, False] if exit_ else [True, False, last_pool]
    canvas = [False, True, True, False] if exit_ else [False, True, True]
    return layers, host, pools, canvas


@pytest.mark.parametrize("run", RUNS, ids=[r[0] for r in RUNS])
def test_canvas_run_equals_plain_kernels_on_assembled_canvases(cuda, run):
    import torch

    from feathercnn_amd import _lib
    from feathercnn_amd.booster import winograd_plan
    from feathercnn_amd.canvas import canvas_param, forward_chained_canvas, plan_canvas
    name, h, batch, ch, bias, relu, last_pool, exit_ = run
    layers, _, pools, canvas = _build(cuda, run)
    lib = _lib.load_library()
    x = torch.from_numpy(np.random.default_rng(7).uniform(-1, 1, (batch, ch[0], 2 * h, 2 * h)).astype(np.float32)).to(cuda)
    out, kept = forward_chained_canvas(layers, x, pools, canvas, fill=float("nan"), keep=True)
    torch.cuda.synchronize()
    assert not torch.isnan(out).any(), "NaN reached the output"

    # ---- the oracle: plain kernels, host-assembled canvases
    p0 = layers[0].param._c()
    _, _, y0 = _stage(lib, p0, batch, x, layers[0], winograd_plan(layers[0].param))
    act = _to_canvas(torch.nn.functional.max_pool2d(y0, 2, 2), h)
    for i in (1, 2):
        cp = canvas_param(layers[i].param, batch)
        assert cp is not None and cp.input_h == 2 * h + 2
        pl = plan_canvas(layers[i].param, batch, True)
        assert pl.tiles_x == pl.tiles_y == (2 * h + 2) // 6 and pl.columns == (batch // 4) * pl.tiles_per_image
        v, m, y = _stage(lib, cp, batch // 4, act, layers[i], pl)
        _same(kept[i][0], v, pl, ch[i], f"{name}: V of canvas layer {i}")
        _same(kept[i][1], m, pl, ch[i + 1], f"{name}: M of canvas layer {i}")
        act = y.clone()
        act[:, :, h:h + 2, :] = 0  # the seam: junk of the convolution, zero before the next layer sees it
        act[:, :, :, h:h + 2] = 0
    if exit_:
        images = _from_canvas(torch.nn.functional.max_pool2d(y, 2, 2), h // 2, h // 2 + 1)  # pooled canvas: images h/2, one seam pixel
        p3, pl3 = layers[3].param._c(), winograd_plan(layers[3].param)
        v, m, want = _stage(lib, p3, batch, images, layers[3], pl3)
        _same(kept[3][0], v, pl3, ch[3], f"{name}: V of the plain layer behind the exit")
        _same(kept[3][1], m, pl3, ch[4], f"{name}: M of the plain layer behind the exit")
    elif last_pool:
        want = _from_canvas(torch.nn.functional.max_pool2d(y, 2, 2), h // 2, h // 2 + 1)
    else:
        want = _from_canvas(y, h, h + 2)
    assert out.shape == want.shape
    assert torch.equal(out, want), f"{name}: output max diff {(out - want).abs().max().item():.3e}"


@pytest.mark.parametrize("run", [("ref_h14", 14, 8, [8, 16, 24, 8], True, True, True, False), ("ref_h56_exit", 56, 4, [4, 8, 12, 8, 4], True, True, False, True)],
                         ids=["h14", "h56_exit"])
def test_canvas_run_against_the_reference_per_image(cuda, checker, run):
    """Every image, the three non-origin quadrants included, against the checker (the compiled reference where it is built); bias and ReLU
    on every layer, as conv_geom's defaults have them."""
    import torch

    from feathercnn_amd.canvas import forward_chained_canvas
    name, h, batch, ch, bias, relu, last_pool, exit_ = run
    layers, host, pools, canvas = _build(cuda, run)
    x = np.random.default_rng(9).uniform(-1, 1, (batch, ch[0], 2 * h, 2 * h)).astype(np.float32)
    got = forward_chained_canvas(layers, torch.from_numpy(x).to(cuda), pools, canvas, fill=float("nan")).cpu().numpy()
    ref = x
    for l, (w, b), pool in zip(layers, host, pools):
        ref = checker.forward(conv_geom(l.param.input_channels, l.param.output_channels, l.param.input_h, 3, 1, 1), ref, w, b)
        if pool:
            ref = ref.reshape(ref.shape[0], ref.shape[1], ref.shape[2] // 2, 2, ref.shape[3] // 2, 2).max(axis=(3, 5))
    assert got.shape == ref.shape and np.isfinite(got).all()
    for k in range(batch):
        assert nerr(got[k:k + 1], ref[k:k + 1]) <= TOL, (name, k)


def test_plan_and_refusals(cuda):
    from feathercnn_amd.booster import winograd_plan
    from feathercnn_amd.canvas import canvas_param, plan_canvas
    for h, tiles, plain in ((14, 5, 3), (56, 19, 10)):
        l, _, _ = _layer(cuda, 8, 8, h)
        l.param.batch = 8
        pl, pp = plan_canvas(l.param, 8, True), plan_canvas(l.param, 8, False)
        assert (pl.tiles_x, pl.tiles_y, pl.tiles_per_image, pl.columns) == (tiles, tiles, tiles * tiles, 2 * tiles * tiles)
        p0 = winograd_plan(l.param)
        assert (pp.tiles_x, pp.columns, pp.v_bytes, pp.m_bytes) == (plain, 8 * plain * plain, p0.v_bytes, p0.m_bytes) == (p0.tiles_x, p0.columns, p0.v_bytes, p0.m_bytes)
        for n in (5, 6, 1, 2):
            assert canvas_param(l.param, n) is None  # a batch that is not a multiple of 4 stays plain
    # no gain, not whole tiles, F(4x4,3x3) planes, odd, more LDS than a block has; 26 / 38 / 50 are whole tiles as canvases but leave through
    # boundaries nobody measured (26 -> pool -> 13): the rule is on for 14 and 56 only
    for h in (28, 112, 224, 7, 8, 13, 62, 26, 38, 50):
        l, _, _ = _layer(cuda, 8, 8, h)
        assert canvas_param(l.param, 8) is None, h


def _vgg(batch, fusion=3):
    from feathercnn_amd import model_zoo
    from feathercnn_amd.net import Net
    p, b, i, o = model_zoo.vgg16()
    x = np.random.default_rng(2025).uniform(-1, 1, (batch, 3, 224, 224)).astype(np.float32)
    net = Net(fusion=fusion, graph=True, tuned=True, concurrency=True)
    net.LoadParam(p)
    net.LoadWeights(b)
    net.FeedInput(i, x)
    for _ in range(3):
        net.Forward()
    return (p, b, i, o), x, net


@pytest.mark.parametrize("batch", [32, 4])
def test_vgg16_net_runs_conv3_and_conv5_on_canvases_and_matches_the_reference(cuda, batch):
    from oracle import netcheck
    (p, b, i, o), x, net = _vgg(batch)
    names = [net.layers()[k][1] for k in net.canvases()]
    assert names == ["conv3_1", "conv3_2", "conv3_3", "conv5_1", "conv5_2", "conv5_3"], names
    prob, logits = net.Extract(o), net.Extract("fc8")
    assert np.isfinite(prob).all()
    picks = list(range(batch))
    if netcheck.have_ref_net():
        ref = netcheck.RefNet(p, b)
        want = [ref.run_blobs(i, x[k], (o, "fc8")) for k in picks]
        ref.close()
    else:
        picks = picks[:1]
        blobs = netcheck.PortNet(p, b).run(i, x[:1], o, keep=True)
        want = [(blobs[o], blobs["fc8"])]
    for k, (wp, wl) in zip(picks, want):
        assert nerr(logits[k:k + 1], wl) <= TOL, k
        assert nerr(prob[k:k + 1], wp) <= TOL, k
        assert int(prob[k].reshape(-1).argmax()) == int(wp.reshape(-1).argmax())


def test_other_plane_sizes_stay_plain_and_keep_running(cuda):
    """52 -> pool -> 26 -> 26 -> pool -> 13 at batch 4: 26-pixel planes would be whole tiles as canvases (54 = 9 tiles) but leave through a pooled
    boundary to an odd plane, a form nobody measured or tested: the run chains as before, has no canvas layer, and gives what level 1 gives."""
    from feathercnn_amd import model_zoo
    from feathercnn_amd.net import Net
    g = model_zoo.GraphBuilder(13)
    x = g.input("data", 16, 52, 52)
    x = g.pool("p1", g.relu("r1", g.conv("c1", x, 16, 32, 3, 1, 1)), 2, 2)
    x = g.relu("r2", g.conv("c2", x, 32, 32, 3, 1, 1))
    x = g.pool("p3", g.relu("r3", g.conv("c3", x, 32, 32, 3, 1, 1)), 2, 2)
    x = g.relu("r4", g.conv("c4", x, 32, 16, 3, 1, 1))
    p, b = g.finish()
    img = np.random.default_rng(11).uniform(-1, 1, (4, 16, 52, 52)).astype(np.float32)
    outs = []
    for level in (1, 3):
        net = Net(fusion=level, tuned=True)
        net.LoadParam(p)
        net.LoadWeights(b)
        net.FeedInput("data", img)
        net.Forward()
        assert net.canvases() == []
        outs.append(net.Extract("r4"))
    names = {net.layers()[k][1]: v for k, v in net.chains().items()}
    assert names.get("c2") == (True, True) and names.get("c3") == (True, True) and names.get("c4") == (True, False), names
    assert outs[1].shape == (4, 16, 13, 13) and nerr(outs[1], outs[0]) <= 1e-5


@pytest.mark.parametrize("batch", [5, 6])
def test_a_batch_that_is_not_a_multiple_of_4_takes_the_plain_path(cuda, batch):
    """No canvas layer, and the logits equal, bit for bit, what the commit before the canvases computed for the same seeded images and weights
    (tests/golden/canvas_plain_vgg16.npz, recorded from that commit's build on an MI355X with the same Net configuration)."""
    (p, b, i, o), x, net = _vgg(batch)
    assert net.canvases() == []
    want = np.load(os.path.join(HERE, "golden", "canvas_plain_vgg16.npz"))[f"fc8_b{batch}"]
    got = net.Extract("fc8").reshape(want.shape)
    assert np.array_equal(got, want), float(np.abs(got - want).max())


def test_kernel_trace_shows_the_canvas_gemm_grids(cuda, tmp_path):
    """Once, under rocprofv3 --kernel-trace (no counters): VGG-16 b32's conv3_x tile GEMMs run on 2888 columns and conv5_x's on 200."""
    _, rows, _ = ktrace.trace("canvas_trace_child.py", [], tmp_path, 300, stats=True)
    launches = [(name, gx, wx) for _, name, gx, wx in rows]  # (kernel name, grid, workgroup) per launch

    def count(target):
        # GEMM launches of `target` blocks.  The tool reports work-items (target * workgroup) or blocks; a tile-GEMM grid is a multiple of 64
        # blocks of 256 lanes, so in work-items it is at least 16384 and no target below can be mistaken for one
        return sum(1 for k, gx, wx in launches if ("wino_gemm_glds" in k or "gemm_mfma_kernel" in k) and (gx == target * wx or gx == target))

    forwards = 2  # tests/canvas_trace_child.py
    # 64 frequency points x (K / 128 row tiles) x ceil(columns / 64) column tiles of the 128 x 64 kernel: conv3_1 .. conv3_3 on 2888 columns
    # (46 tiles), conv5_1 .. conv5_3 on 200 (4 tiles) -- three launches each per forward, and none of the plain forms' 3200 columns (50 tiles
    # of 64) or 288 (3 tiles of 96)
    assert count(64 * 2 * 46) == 3 * forwards and count(64 * 4 * 4) == 3 * forwards, (count(64 * 2 * 46), count(64 * 4 * 4))
    assert count(64 * 2 * 50) == 0 and count(64 * 4 * 3) == 0
    names = {k for k, _, _ in launches}
    assert any("canvas_chain_kernel" in k for k in names) and any("canvas_output_kernel" in k for k in names), sorted(names)
