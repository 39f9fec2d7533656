"""The transposed-convolution route (libfeather_deconv.so) on the MI355X.

* the sweep: every case of tests/deconv_cases.py -- every kernel instantiation of the library -- against the fp64 definition
  (tests/deconv_ref.py), all four epilogues, batch 1 and 3, between guarded buffers (tests/guarded.py): output and packed weights between
  poisoned guards, inputs between NaN guards, so nothing outside is written and nothing outside reaches a result; the library's own route
  report (fhip_deconv_route, the selection function fhip_deconv_forward launches with) names the instantiation the case targets;
* the reference's recorded results on the zero-stuffed input with the flipped kernel (tests/golden/deconv_golden.npz);
* run-to-run bit identity, idempotent init and capture into a hipGraph;
* feather::Net with deconvolution layers: tiny_deconv at fusion levels 0 - 3, with sub-batches, concurrency and the graph, Extract of a
  deconvolution's top; style_transfer and unet_k4 at batch 4; FeedPixels -> style_transfer -> ExtractPixels (the missing library:
  tests/test_side_contract_gpu.py); a reference-style C++ application.
Bound everywhere: max|y - ref| / max|ref| <= 1e-4.  Measured on the MI355X: MFMA sweep 5.7e-7, generic sweep 3.4e-7, fixtures
5.3e-6 against the recorded reference and 3.5e-7 against fp64, tiny_deconv 5.0e-7, unet_k4 b4 8.2e-7, style_transfer b4 1.1e-5
(DESIGN.md 3.13); each test prints its own figures."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import deconv_cases as DC
import deconv_ref as R
import side_contract
from guarded import Guarded, describe

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-4
WORST = {}


def _note(family, e):
    WORST[family] = max(WORST.get(family, 0.0), e)


lib = side_contract.fixture("deconv", gpu=True)


def _param(case, bias, act, batch):
    from feathercnn_amd import DeconvParam
    _, c, k, group, h, w, kh, kw, s, (pl, pr, pt, pb), (opr, opb), _ = case
    sh, sw = DC.strides(s)
    p = DeconvParam(output_channels=k, input_channels=c, input_h=h, input_w=w, kernel_h=kh, kernel_w=kw, stride_h=sh, stride_w=sw, pad_left=pl,
                    pad_right=pr, pad_top=pt, pad_bottom=pb, group=group, bias_term=bool(bias), activation=act, output_pad_right=opr,
                    output_pad_bottom=opb, batch=batch)
    p.AssignOutputDim()
    return p


_stream = side_contract.stream


@pytest.mark.parametrize("case", DC.CASES, ids=[c[0] for c in DC.CASES])
def test_sweep_between_guards(lib, case):
    import torch
    name, c, k, group, h, w, kh, kw, s, pads, out_pads, offset = case
    sh, sw = DC.strides(s)
    ho, wo = DC.out_dims(case)
    worst = 0.0
    for batch in DC.BATCHES:
        x, wt, b = R.synth(c, k, h, w, kh, kw, group, batch, seed=2000 + len(name) + batch, sh=sh, sw=sw)
        for bias, act in DC.EPILOGUES:
            p = _param(case, bias, act, batch)
            assert (p.output_h, p.output_w) == (ho, wo)
            cp = p._c()
            sb, pk = ctypes.c_size_t(), ctypes.c_size_t()
            assert lib.fhip_deconv_get_buffer_size(ctypes.byref(cp), batch, ctypes.byref(sb), ctypes.byref(pk)) == 0
            assert sb.value == 0
            gx, gw = Guarded(x.size, x, offset), Guarded(wt.size, wt, 0)
            gb = Guarded(k, b if bias else "nan", 0)  # without bias_term the bias must not be read: a NaN body
            gy, gp, gs = Guarded(batch * k * ho * wo, "poison", offset), Guarded(pk.value // 4, "poison", 0), Guarded(0, "poison", 0)
            snaps = [g.snapshot() for g in (gx, gw, gb)]
            route = ctypes.create_string_buffer(160)
            assert lib.fhip_deconv_route(ctypes.byref(cp), route, 160) == 0
            assert route.value.decode() == DC.instance(case), (name, route.value)
            v = ctypes.c_void_p
            rc = lib.fhip_deconv_init(ctypes.byref(cp), v(gp.ptr), v(gw.ptr), _stream())
            assert rc == 0, lib.fhip_deconv_last_error()
            rc = lib.fhip_deconv_forward(ctypes.byref(cp), batch, v(gy.ptr), v(gx.ptr), v(gp.ptr), v(gs.ptr), v(gb.ptr), _stream())
            assert rc == 0, lib.fhip_deconv_last_error()
            torch.cuda.synchronize()
            for what, g in (("output", gy), ("packed weights", gp), ("scratch", gs), ("input", gx), ("weights", gw), ("bias", gb)):
                assert g.guards_intact() is None, f"{name}: {what} guard: {describe(g.guards_intact())}"
            assert gy.unwritten() == 0 and gp.unwritten() == 0, (name, gy.unwritten(), gp.unwritten())
            for g, snap in zip((gx, gw, gb), snaps):
                assert g.unchanged(snap), (name, g.first_change(snap))
            y = gy.values().reshape(batch, k, ho, wo)
            assert np.isfinite(y).all(), f"{name}: a value from outside a tensor reached the result"
            want = R.deconv(x, wt, b if bias else None, group, (sh, sw), pads, out_pads, bool(act))
            e = R.nerr(y, want)
            worst = max(worst, e)
            assert e <= TOL, (name, batch, bias, act, e)
            if act:
                assert (y >= 0).all()
    family = "generic" if DC.instance(case) == DC.GENERIC else "MFMA"
    _note(family, worst)
    print(f"deconv sweep {name}: {DC.instance(case)} worst normalised error vs fp64 {worst:.2e} ({family} so far {WORST[family]:.2e})")


def test_sweep_reaches_every_instantiation():
    import kernel_instances as KI
    assert set(KI.instances(DC.LIB)) == DC.targets()


def test_recorded_reference_fixtures(lib):
    import torch
    from feathercnn_amd import DeconvLayer, DeconvParam
    g = np.load(os.path.join(ROOT, "tests", "golden", "deconv_golden.npz"))
    worst_ref = worst_64 = 0.0
    routes = set()
    for n in (str(v) for v in g["names"]):
        c, k, h, w, ks, s, pd, op, bias, relu, batch = (int(v) for v in g[n + "/geom"])
        p = DeconvParam.make(c, k, h, ks, s, pd, op, bias=bias, act=relu, w=w, batch=batch)
        x, wt, b = g[n + "/x"], g[n + "/w"], g[n + "/b"]
        layer = DeconvLayer(p, torch.from_numpy(wt).cuda(), torch.from_numpy(b).cuda() if bias else None)
        routes.add(layer.deconv.Route(p))
        y = layer.Forward(torch.from_numpy(x).cuda()).cpu().numpy()
        e_ref = R.nerr(y, g[n + "/y"])
        e_64 = R.nerr(y, R.deconv(x, wt, b if bias else None, 1, (s, s), (pd,) * 4, (op, op), bool(relu)))
        print(f"deconv fixture {n}: vs recorded reference {e_ref:.2e}, vs fp64 {e_64:.2e}")
        worst_ref, worst_64 = max(worst_ref, e_ref), max(worst_64, e_64)
        assert e_ref <= TOL and e_64 <= TOL, (n, e_ref, e_64)
    print(f"deconv fixtures: worst vs recorded reference {worst_ref:.2e}, vs fp64 {worst_64:.2e}")
    assert DC.GENERIC in routes and len(routes) >= 3, routes


def test_forward_is_bit_identical_and_graph_capturable(lib):
    import torch
    from feathercnn_amd import DeconvLayer, DeconvParam
    # the paired MFMA route, the one-phase MFMA route, the generic kernel (depthwise)
    for c, k, group, h, ks, s, pd, op in ((64, 64, 1, 16, 4, 2, 1, 0), (32, 96, 1, 9, 3, 1, 1, 0), (64, 32, 1, 11, 3, 2, 1, 1), (21, 21, 21, 15, 4, 2, 1, 0)):
        p = DeconvParam.make(c, k, h, ks, s, pd, op, group=group, batch=5)
        x, wt, b = R.synth(c, k, h, h, ks, ks, group, 5, seed=77, sh=s, sw=s)
        layer = DeconvLayer(p, torch.from_numpy(wt).cuda(), torch.from_numpy(b).cuda())
        xd = torch.from_numpy(x).cuda()
        first = layer.Forward(xd).clone()
        assert R.nerr(first.cpu().numpy(), R.deconv(x, wt, b, group, (s, s), (pd,) * 4, (op, op), True)) <= TOL
        for _ in range(3):
            assert torch.equal(layer.Forward(xd), first)
        packed = layer.packed.clone()
        layer.deconv.Init(p, layer.packed, torch.from_numpy(wt).cuda())  # idempotent
        assert torch.equal(packed, layer.packed)
        out = torch.full_like(first, float("nan"))
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(graph, stream=side):
                layer.Forward(xd, out=out)
        assert torch.isnan(out).all()  # captured, not run
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, first)
        xd.copy_(torch.from_numpy(x[::-1].copy()).cuda())
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, layer.Forward(xd))


# ---- feather::Net --------------------------------------------------------------------------------------------------------------------
def _run(model, x, blob=None, **kw):
    from feathercnn_amd.net import Net
    p, b, i, o = model
    net = Net(**kw)
    net.LoadParam(p)
    net.LoadWeights(b)
    net.FeedInput(i, x)
    net.Forward()
    y = net.Extract(blob or o)
    if kw.get("graph"):  # a second forward replays the captured graph
        net.FeedInput(i, x)
        net.Forward()
        assert np.array_equal(net.Extract(blob or o), y)
    layers = net.layers()
    net.close()
    return y, layers


def test_tiny_deconv_net_at_every_fusion_level(cuda):
    from feathercnn_amd import model_zoo
    model = model_zoo.tiny_deconv()
    x = np.random.default_rng(3).uniform(-1, 1, (5, 3, 16, 16)).astype(np.float32)
    ref = R.Net(model[0], model[1])
    want = ref.run(model[2], x, model[3])
    assert want.shape == (5, 8, 16, 16)
    outs = {}
    for level in (0, 1, 2, 3):
        y, layers = _run(model, x, fusion=level, tuned=(level == 3))
        e = R.nerr(y, want)
        print(f"tiny_deconv fusion {level}: {len(layers)} layers, normalised error vs the restatement {e:.2e}")
        assert e <= TOL, (level, e)
        outs[level] = y
        routes = {nm: a for _, nm, a in layers}
        assert all(routes[nm] == "DECONV" for nm in model_zoo.DECONV_LAYERS["tiny_deconv"]), routes
        names = [nm for _, nm, _ in layers]
        if level == 0:
            assert len(layers) == 21, names
        if level == 1:
            # Deconvolution + ReLU only; BatchNorm and Scale stay (and compose with each other and the ReLU behind them, as they always did)
            assert not {"relu_d1", "relu_gd", "relu_d3"} & set(names) and "d2_bn" in names, names
        if level >= 2:
            assert not {"relu_d1", "d2_bn", "d2_scale", "d2_relu", "relu_gd", "relu_d3"} & set(names), names
            assert {"split1", "cat", "d1", "d2", "dw_up", "gd", "d3", "d4"} <= set(names), names  # nothing else absorbs or is absorbed
    for level in (1, 2, 3):
        assert R.nerr(outs[level], outs[0]) <= 1e-5, level
    # sub-batch replicas, branch concurrency and the captured graph
    for kw in ({"sub_batches": 2}, {"graph": True}, {"sub_batches": 2, "graph": True, "concurrency": True}, {"concurrency": True}):
        y, _ = _run(model, x, fusion=2, **kw)
        assert R.nerr(y, outs[2]) <= 1e-5 and R.nerr(y, want) <= TOL, kw
    # a deconvolution's top can be extracted, per layer against the restatement
    blobs = ref.run(model[2], x, model[3], keep=True)
    for blob in ("d1", "d2", "dw_up", "gd", "d3"):
        y, _ = _run(model, x, blob=blob, fusion=0)
        e = R.nerr(y, blobs[blob])
        print(f"tiny_deconv blob {blob} {y.shape}: {e:.2e}")
        assert y.shape == blobs[blob].shape and e <= TOL, (blob, e)


@pytest.mark.parametrize("name", ["style_transfer", "unet_k4"])
def test_image_nets_batch4(cuda, name):
    from feathercnn_amd import model_zoo
    model = model_zoo.MODELS[name]()
    x = np.random.default_rng(4).uniform(-1, 1, (4, 3, 256, 256)).astype(np.float32)
    want = R.Net(model[0], model[1]).run(model[2], x, model[3])
    assert want.shape == (4, 3, 256, 256)
    for kw in ({"fusion": 1}, {"fusion": 3, "tuned": True, "graph": True}):
        y, layers = _run(model, x, **kw)
        e = R.nerr(y, want)
        routes = [a for _, _, a in layers]
        print(f"{name} b4 {kw}: {len(layers)} layers, routes {sorted(set(r for r in routes if r))}, normalised error {e:.2e}")
        assert routes.count("DECONV") == len(model_zoo.DECONV_LAYERS[name])
        if name == "style_transfer" and kw["fusion"] == 3:
            assert routes.count("WINOGRADF63") >= 10  # the residual blocks keep their Winograd route
        assert e <= TOL, (kw, e)


def test_pixels_through_style_transfer_to_pixels(cuda):
    """FeedPixels -> style_transfer -> ExtractPixels against the host restatements of the three stages.  The uint8 images must equal the
    restatement's except where the fp64 pre-quantisation value lies within the parity bound (1e-4 of the blob's max |value|, times norm) of
    an integer, the quantisation boundaries of to_pixels; there one level of difference is allowed, nowhere else, and never more."""
    import pixels_ref as P
    import yuv_ref as Y
    from feathercnn_amd import model_zoo
    from feathercnn_amd.net import Net
    param, weights, i, o = model_zoo.style_transfer()
    n, (w, h), size = 2, (90, 70), 64
    px = np.random.default_rng(9).integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    mean_in, norm_in = [104.0, 117.0, 123.0], [0.017, 0.017, 0.017]
    x = P.from_pixels_resize(px, P.PIXEL_RGB, size, size, mean_in, norm_in)
    want = R.Net(param, weights).run(i, x, o)
    peak = float(np.abs(want).max())
    lo, hi = want.min(axis=(0, 2, 3)), want.max(axis=(0, 2, 3))
    norm = (300.0 / (hi - lo)).astype(np.float32)
    mean = (lo + 20.0 / norm).astype(np.float32)  # spreads the output over about -20 .. 280: both clamps are exercised
    pre = (want.astype(np.float64) - mean.astype(np.float64).reshape(1, 3, 1, 1)) * norm.astype(np.float64).reshape(1, 3, 1, 1)
    bound = TOL * peak * float(norm.max())
    near = (np.abs(pre - np.rint(pre)) <= bound).transpose(0, 2, 3, 1)  # [N][h][w][C] like the images
    expect = np.stack([Y.to_pixels_resize(v, P.PIXEL_RGB, size, size) for v in P.mean_norm(want, mean, norm)])
    for kw in ({"fusion": 1}, {"fusion": 3, "tuned": True, "graph": True}):
        net = Net(**kw)
        net.LoadParam(param)
        net.LoadWeights(weights)
        net.FeedPixels(i, px, P.PIXEL_RGB, (size, size), mean_in, norm_in)
        net.Forward()
        e = R.nerr(net.Extract(o), want)
        got = net.ExtractPixels(o, P.PIXEL_RGB, None, mean, norm)
        net.close()
        assert got.shape == expect.shape == (n, size, size, 3) and got.dtype == np.uint8
        diff = np.abs(got.astype(np.int32) - expect.astype(np.int32))
        print(f"style_transfer pixels {kw}: blob error {e:.2e}; {int(near.sum())} of {near.size} values within {bound:.2e} of a quantisation "
              f"boundary, {int((diff != 0).sum())} bytes differ (all by {int(diff.max())})")
        assert e <= TOL
        assert diff.max() <= 1 and not (diff != 0)[~near].any()
        assert expect.min() == 0 and expect.max() == 255


def test_reference_style_application_runs(lib, tmp_path):
    from feathercnn_amd import model_zoo
    exe = side_contract.build_app("deconv", tmp_path)
    p, b, i, o = model_zoo.tiny_deconv()
    x = np.random.default_rng(9).uniform(-1, 1, (2, 3, 16, 16)).astype(np.float32)
    lx, lw, lb = R.synth(32, 40, 5, 7, 4, 4, 1, 2, seed=10, sh=2, sw=2)
    paths = {n: str(tmp_path / n) for n in ("m.param", "m.bin", "in.f32", "net.f32", "x.f32", "w.f32", "b.f32", "layer.f32")}
    open(paths["m.param"], "wb").write(p)
    open(paths["m.bin"], "wb").write(b)
    for n, a in (("in.f32", x), ("x.f32", lx), ("w.f32", lw), ("b.f32", lb)):
        a.tofile(paths[n])
    r = subprocess.run([exe, paths["m.param"], paths["m.bin"], paths["in.f32"], "2", "3", "16", "16", i, o, paths["net.f32"], paths["x.f32"],
                        paths["w.f32"], paths["b.f32"], paths["layer.f32"]], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr)
    want = R.Net(p, b).run(i, x, o)
    assert R.nerr(np.fromfile(paths["net.f32"], np.float32).reshape(want.shape), want) <= TOL
    lay = R.deconv(lx, lw, lb, 1, (2, 2), (1, 1, 1, 1), (0, 0), True)
    assert R.nerr(np.fromfile(paths["layer.f32"], np.float32).reshape(lay.shape), lay) <= TOL
