"""The grouped-convolution route (1 < group < C, libfeather_gconv.so) on the MI355X.

* the sweep: every case of tests/gconv_cases.py -- every kernel instantiation of the library -- against the fp64 definition
  (tests/gconv_ref.py), all four epilogues, batch 1 and 3, between guarded buffers (tests/guarded.py): output and packed weights between
  poisoned guards, inputs between NaN guards, so nothing outside is written and nothing outside reaches a result; the library's own route
  report (fhip_gconv_route, the selection function fhip_gconv_forward launches with) names the instantiation the case targets;
* the reference's recorded results on slices (tests/golden/gconv_golden.npz);
* run-to-run bit identity and capture into a hipGraph;
* feather::Net with grouped layers: tiny_grouped at fusion levels 0 - 3, with sub-batches, with the graph; ResNeXt-50 (32x4d) at batch 8;
  Extract of a grouped layer's top (the missing library: tests/test_side_contract_gpu.py).
Bound everywhere: max|y - ref| / max|ref| <= 1e-4.  Measured on the MI355X: tuned sweep 7.9e-7, generic sweep 2.9e-7, fixtures
3.9e-6 against the recorded reference, ResNeXt-50 logits 3.5e-7; each test prints its own figures."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import gconv_cases as GC
import gconv_ref as R
import side_contract
from guarded import Guarded, describe

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-4
WORST = {}


def _note(family, e):
    WORST[family] = max(WORST.get(family, 0.0), e)


lib = side_contract.fixture("gconv", gpu=True)


def _param(case, bias, act, batch):
    from feathercnn_amd import ConvParam
    _, c, k, group, h, w, kh, kw, s, (pl, pr, pt, pb), _ = case
    sh, sw = GC.strides(s)
    p = ConvParam(output_channels=k, input_channels=c, input_h=h, input_w=w, kernel_h=kh, kernel_w=kw, stride_h=sh, stride_w=sw, pad_left=pl,
                  pad_right=pr, pad_top=pt, pad_bottom=pb, group=group, bias_term=bool(bias), activation=act, batch=batch)
    p.AssignOutputDim()
    return p


_stream = side_contract.stream


@pytest.mark.parametrize("case", GC.CASES, ids=[c[0] for c in GC.CASES])
def test_sweep_between_guards(lib, case):
    import torch
    name, c, k, group, h, w, kh, kw, s, pads, offset = case
    ho, wo = GC.out_dims(case)
    worst = 0.0
    for batch in GC.BATCHES:
        x, wt, b = R.synth(c, k, h, w, kh, kw, group, batch, seed=1000 + len(name) + batch)
        for bias, act in GC.EPILOGUES:
            p = _param(case, bias, act, batch)
            assert (p.output_h, p.output_w, p.output_channels) == (ho, wo, k)
            cp = p._c()
            sb, pk = ctypes.c_size_t(), ctypes.c_size_t()
            assert lib.fhip_gconv_get_buffer_size(ctypes.byref(cp), batch, ctypes.byref(sb), ctypes.byref(pk)) == 0
            gx, gw = Guarded(x.size, x, offset), Guarded(wt.size, wt, 0)
            gb = Guarded(k, b if bias else "nan", 0)  # without bias_term the bias must not be read: a NaN body
            gy, gp, gs = Guarded(batch * k * ho * wo, "poison", offset), Guarded(pk.value // 4, "poison", 0), Guarded(sb.value // 4, "poison", 0)
            snaps = [g.snapshot() for g in (gx, gw, gb)]
            route = ctypes.create_string_buffer(96)
            assert lib.fhip_gconv_route(ctypes.byref(cp), ctypes.c_void_p(gy.ptr), ctypes.c_void_p(gx.ptr), route, 96) == 0
            assert route.value.decode() == GC.instance(case, gx.ptr, gy.ptr) == GC.instance(case), (name, route.value)
            v = ctypes.c_void_p
            rc = lib.fhip_gconv_init(ctypes.byref(cp), v(gp.ptr), v(gw.ptr), _stream())
            assert rc == 0, lib.fhip_gconv_last_error()
            rc = lib.fhip_gconv_forward(ctypes.byref(cp), batch, v(gy.ptr), v(gx.ptr), v(gp.ptr), v(gs.ptr), v(gb.ptr), _stream())
            assert rc == 0, lib.fhip_gconv_last_error()
            torch.cuda.synchronize()
            for what, g in (("output", gy), ("packed weights", gp), ("scratch", gs), ("input", gx), ("weights", gw), ("bias", gb)):
                assert g.guards_intact() is None, f"{name}: {what} guard: {describe(g.guards_intact())}"
            assert gy.unwritten() == 0 and gp.unwritten() == 0, (name, gy.unwritten(), gp.unwritten())
            for g, snap in zip((gx, gw, gb), snaps):
                assert g.unchanged(snap), (name, g.first_change(snap))
            y = gy.values().reshape(batch, k, ho, wo)
            assert np.isfinite(y).all(), f"{name}: a value from outside a tensor reached the result"
            want = R.conv(x, wt, b if bias else None, group, GC.strides(s), pads, bool(act))
            e = R.nerr(y, want)
            worst = max(worst, e)
            assert e <= TOL, (name, batch, bias, act, e)
            if act:
                assert (y >= 0).all()
    family = "tuned 3x3" if GC.instance(case) != GC.GENERIC else "generic"
    _note(family, worst)
    print(f"gconv sweep {name}: {GC.instance(case)} worst normalised error vs fp64 {worst:.2e} ({family} so far {WORST[family]:.2e})")


def test_sweep_reaches_every_instantiation():
    import kernel_instances as KI
    assert set(KI.instances(GC.LIB)) == GC.targets()


def test_recorded_reference_fixtures(lib):
    import torch
    from feathercnn_amd import ConvParam, GroupedConvLayer
    g = np.load(os.path.join(ROOT, "tests", "golden", "gconv_golden.npz"))
    worst_ref = worst_64 = 0.0
    for n in (str(v) for v in g["names"]):
        c, k, group, h, w, kh, kw, sh, sw, pl, pr, pt, pb, bias, relu, batch = (int(v) for v in g[n + "/geom"])
        p = ConvParam(output_channels=k, input_channels=c, input_h=h, input_w=w, kernel_h=kh, kernel_w=kw, stride_h=sh, stride_w=sw,
                      pad_left=pl, pad_right=pr, pad_top=pt, pad_bottom=pb, group=group, bias_term=bool(bias), activation=relu, batch=batch)
        x, wt, b = g[n + "/x"], g[n + "/w"], g[n + "/b"]
        layer = GroupedConvLayer(p, torch.from_numpy(wt).cuda(), torch.from_numpy(b).cuda() if bias else None)
        y = layer.Forward(torch.from_numpy(x).cuda()).cpu().numpy()
        e_ref = R.nerr(y, g[n + "/y"])
        e_64 = R.nerr(y, R.conv(x, wt, b if bias else None, group, (sh, sw), (pl, pr, pt, pb), bool(relu)))
        print(f"gconv fixture {n}: vs recorded reference {e_ref:.2e}, vs fp64 {e_64:.2e}")
        worst_ref, worst_64 = max(worst_ref, e_ref), max(worst_64, e_64)
        assert e_ref <= TOL and e_64 <= TOL, (n, e_ref, e_64)
    print(f"gconv fixtures: worst vs recorded reference {worst_ref:.2e}, vs fp64 {worst_64:.2e}")


def test_forward_is_bit_identical_and_graph_capturable(lib):
    import torch
    from feathercnn_amd import ConvParam, GroupedConvLayer
    for c, k, group, h, s in ((128, 128, 32, 28, 1), (64, 64, 2, 15, 2), (32, 24, 4, 9, 1)):
        kk = 3 if k != 24 else 1
        p = ConvParam.make(c, k, h, kk, s, kk // 2, group=group, batch=5)
        x, wt, b = R.synth(c, k, h, h, kk, kk, group, 5, seed=77)
        layer = GroupedConvLayer(p, torch.from_numpy(wt).cuda(), torch.from_numpy(b).cuda())
        xd = torch.from_numpy(x).cuda()
        first = layer.Forward(xd).clone()
        for _ in range(3):
            assert torch.equal(layer.Forward(xd), first)
        packed = layer.packed.clone()
        layer.conv.Init(p, layer.packed, torch.from_numpy(wt).cuda())  # idempotent
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


def test_tiny_grouped_net_at_every_fusion_level(cuda):
    from feathercnn_amd import model_zoo
    model = model_zoo.tiny_grouped()
    x = np.random.default_rng(3).uniform(-1, 1, (5, 3, 21, 21)).astype(np.float32)
    ref = R.Net(model[0], model[1])
    want = ref.run(model[2], x, model[3])
    outs = {}
    for level in (0, 1, 2, 3):
        y, layers = _run(model, x, fusion=level, tuned=(level == 3))
        e = R.nerr(y, want)
        print(f"tiny_grouped fusion {level}: {len(layers)} layers, normalised error vs the restatement {e:.2e}")
        assert e <= TOL, (level, e)
        outs[level] = y
        routes = {nm: a for _, nm, a in layers}
        assert all(routes[nm] == "GCONV" for nm in model_zoo.GROUPED_LAYERS["tiny_grouped"]), routes
        names = [nm for _, nm, _ in layers]
        if level == 0:
            assert len(layers) == 19
        if level == 1:
            assert "relu_g1" not in names and "relu_g4" not in names and "g2_bn" in names, names  # Conv + ReLU only, as the reference
        if level >= 2:
            # ReLU and BatchNorm + Scale + ReLU are folded into the grouped layers; the Eltwise sum and the pooling behind one are declined
            assert not {"relu_g1", "g2_bn", "g2_scale", "g2_relu", "relu_g4"} & set(names), names
            assert {"sum", "pool1"} <= set(names), names
    for level in (1, 2, 3):
        assert R.nerr(outs[level], outs[0]) <= 1e-5, level
    # sub-batch replicas, branch concurrency and the captured graph
    for kw in ({"sub_batches": 2}, {"graph": True}, {"sub_batches": 2, "graph": True, "concurrency": True}, {"concurrency": True}):
        y, _ = _run(model, x, fusion=2, **kw)
        assert R.nerr(y, outs[2]) <= 1e-5 and R.nerr(y, want) <= TOL, kw
    # a grouped layer's top can be extracted, per layer against the restatement
    blobs = ref.run(model[2], x, model[3], keep=True)
    for blob in ("g1", "g2", "g3", "g4"):
        y, _ = _run(model, x, blob=blob, fusion=0)
        e = R.nerr(y, blobs[blob])
        print(f"tiny_grouped blob {blob} {y.shape}: {e:.2e}")
        assert y.shape == blobs[blob].shape and e <= TOL, (blob, e)


def test_resnext50_batch8(cuda):
    from feathercnn_amd import model_zoo
    model = model_zoo.resnext50_32x4d()
    x = np.random.default_rng(4).uniform(-1, 1, (8, 3, 224, 224)).astype(np.float32)
    want = R.Net(model[0], model[1]).run(model[2], x, model[3], keep=True)
    for kw in ({"fusion": 1}, {"fusion": 3, "tuned": True, "graph": True}):
        y, layers = _run(model, x, blob="fc1000", **kw)
        e = R.nerr(y, want["fc1000"])
        print(f"resnext50_32x4d b8 {kw}: {len(layers)} layers, logits normalised error {e:.2e}")
        assert sum(a == "GCONV" for _, _, a in layers) == 16
        assert e <= TOL, (kw, e)
        assert (y.reshape(8, -1).argmax(1) == want["fc1000"].reshape(8, -1).argmax(1)).all()


def test_reference_style_application_runs(lib, tmp_path):
    from feathercnn_amd import model_zoo
    exe = side_contract.build_app("gconv", tmp_path)
    p, b, i, o = model_zoo.tiny_grouped()
    x = np.random.default_rng(9).uniform(-1, 1, (2, 3, 21, 21)).astype(np.float32)
    lx, lw, lb = R.synth(16, 16, 9, 13, 3, 3, 4, 2, seed=10)
    paths = {n: str(tmp_path / n) for n in ("m.param", "m.bin", "in.f32", "net.f32", "x.f32", "w.f32", "b.f32", "layer.f32")}
    open(paths["m.param"], "wb").write(p)
    open(paths["m.bin"], "wb").write(b)
    for n, a in (("in.f32", x), ("x.f32", lx), ("w.f32", lw), ("b.f32", lb)):
        a.tofile(paths[n])
    r = subprocess.run([exe, paths["m.param"], paths["m.bin"], paths["in.f32"], "2", "3", "21", "21", i, o, paths["net.f32"], paths["x.f32"],
                        paths["w.f32"], paths["b.f32"], paths["layer.f32"]], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr)
    want = R.Net(p, b).run(i, x, o)
    assert R.nerr(np.fromfile(paths["net.f32"], np.float32).reshape(want.shape), want) <= TOL
    lay = R.conv(lx, lw, lb, 4, (1, 1), (1, 1, 1, 1), True)
    assert R.nerr(np.fromfile(paths["layer.f32"], np.float32).reshape(lay.shape), lay) <= TOL
