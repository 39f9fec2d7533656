"""The dilated-convolution route (libfeather_atrous.so) on the MI355X.

* the sweep: every case of tests/atrous_cases.py -- every kernel instantiation of the library -- against the fp64 definition
  (tests/atrous_ref.py), all four epilogues, batch 1 and 3, between guarded buffers (tests/guarded.py): output and packed weights between
  poisoned guards, inputs between NaN guards, so nothing outside is written and nothing outside reaches a result; the library's own route
  report (fhip_atrous_route, the selection function fhip_atrous_forward launches with) names the instantiation the case targets; the
  forms that run by name only (ROW4, tap skipping against the selection) go through the same guarded run with fhip_atrous_*_route;
* fhip_atrous_forward_route: every route that accepts a case (ROW4 and scalar, tap skipping on and off, both tiles, the depthwise forms,
  the generic kernel) gives the same result within the bound;
* the reference's recorded results with the zero-stuffed kernel (tests/golden/atrous_golden.npz);
* run-to-run bit identity, idempotent init and capture into a hipGraph;
* feather::Net with dilated layers (Net.SetDilated): tiny_dilated at fusion levels 0 - 3, with sub-batches, concurrency and the graph,
  Extract of a dilated layer's top; deeplab_largefov and deeplab_v2_aspp at 65 pixels, batch 2 (the missing library:
  tests/test_side_contract_gpu.py); a kernel trace of tiny_dilated in a process of its own; a reference-style C++ application.
Bound everywhere: max|y - ref| / max|ref| <= 1e-4; fusion levels among themselves 1e-5.  Each test prints its own
figures; the measured worst cases are recorded in DESIGN.md 3.17."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import atrous_cases as AC
import atrous_ref as R
import kernel_instances as KI
import ktrace
import side_contract
from guarded import Guarded, describe

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-4
WORST = {}


def _note(family, e):
    WORST[family] = max(WORST.get(family, 0.0), e)


def _family(inst):
    return "generic" if inst == AC.GENERIC else "depthwise" if "dw3x3" in inst else "MFMA"


lib = side_contract.fixture("atrous", gpu=True)


def _param(case, bias, act, batch):
    from feathercnn_amd import AtrousParam
    _, c, k, group, h, w, kh, kw, s, (pl, pr, pt, pb), (dh, dw), _ = case
    sh, sw = AC.strides(s)
    p = AtrousParam(output_channels=k, input_channels=c, input_h=h, input_w=w, kernel_h=kh, kernel_w=kw, stride_h=sh, stride_w=sw, pad_left=pl,
                    pad_right=pr, pad_top=pt, pad_bottom=pb, group=group, bias_term=bool(bias), activation=act, dilation_h=dh, dilation_w=dw,
                    batch=batch)
    p.AssignOutputDim()
    return p


_stream = side_contract.stream


def _want(case, x, wt, b, act):
    _, c, k, group, h, w, kh, kw, s, pads, dil, _ = case
    return R.atrous(x, wt, b, group, AC.strides(s), pads, dil, bool(act))


@pytest.mark.parametrize("case", AC.CASES, ids=[c[0] for c in AC.CASES])
def test_sweep_between_guards(lib, case):
    import torch
    name, c, k, group, h, w, kh, kw, s, pads, dil, offset = case
    ho, wo = AC.out_dims(case)
    worst = 0.0
    for batch in AC.BATCHES:
        x, wt, b = R.synth(c, k, h, w, kh, kw, group, batch, seed=3000 + len(name) + batch)
        # the selected route with every epilogue; the variants that run by name only (ROW4, tap skipping on / off) with bias + ReLU
        for route, bias, act in [(None, bi, ac) for bi, ac in AC.EPILOGUES] + [(r, 1, 1) for r in AC.sweep_routes(case)[1:]]:
            p = _param(case, bias, act, batch)
            assert (p.output_h, p.output_w) == (ho, wo)
            cp = p._c()
            sb, pk = ctypes.c_size_t(), ctypes.c_size_t()
            named = route.encode() if route else AC.instance(case).encode()  # the *_route calls under the selected name equal the plain ones
            assert lib.fhip_atrous_get_buffer_size_route(ctypes.byref(cp), batch, named, ctypes.byref(sb), ctypes.byref(pk)) == 0
            assert sb.value == 0
            if route is None:
                pk2 = ctypes.c_size_t()
                assert lib.fhip_atrous_get_buffer_size(ctypes.byref(cp), batch, ctypes.byref(sb), ctypes.byref(pk2)) == 0 and pk2.value == pk.value
            gx, gw = Guarded(x.size, x, offset), Guarded(wt.size, wt, 0)
            gb = Guarded(k, b if bias else "nan", 0)  # without bias_term the bias must not be read: a NaN body
            gy, gp, gs = Guarded(batch * k * ho * wo, "poison", offset), Guarded(pk.value // 4, "poison", 0), Guarded(0, "poison", 0)
            snaps = [g.snapshot() for g in (gx, gw, gb)]
            told = ctypes.create_string_buffer(160)
            assert lib.fhip_atrous_route(ctypes.byref(cp), told, 160) == 0
            assert told.value.decode() == AC.instance(case), (name, told.value)
            v = ctypes.c_void_p
            if route is None:
                rc = lib.fhip_atrous_init(ctypes.byref(cp), v(gp.ptr), v(gw.ptr), _stream())
                assert rc == 0, lib.fhip_atrous_last_error()
                rc = lib.fhip_atrous_forward(ctypes.byref(cp), batch, v(gy.ptr), v(gx.ptr), v(gp.ptr), v(gs.ptr), v(gb.ptr), _stream())
            else:
                rc = lib.fhip_atrous_init_route(ctypes.byref(cp), v(gp.ptr), v(gw.ptr), _stream(), named)
                assert rc == 0, lib.fhip_atrous_last_error()
                rc = lib.fhip_atrous_forward_route(ctypes.byref(cp), batch, v(gy.ptr), v(gx.ptr), v(gp.ptr), v(gs.ptr), v(gb.ptr), _stream(), named)
            assert rc == 0, lib.fhip_atrous_last_error()
            torch.cuda.synchronize()
            for what, g in (("output", gy), ("packed weights", gp), ("scratch", gs), ("input", gx), ("weights", gw), ("bias", gb)):
                assert g.guards_intact() is None, f"{name}: {what} guard: {describe(g.guards_intact())}"
            assert gy.unwritten() == 0 and gp.unwritten() == 0, (name, gy.unwritten(), gp.unwritten())
            for g, snap in zip((gx, gw, gb), snaps):
                assert g.unchanged(snap), (name, g.first_change(snap))
            y = gy.values().reshape(batch, k, ho, wo)
            assert np.isfinite(y).all(), f"{name}: a value from outside a tensor reached the result"
            e = R.nerr(y, _want(case, x, wt, b if bias else None, act))
            worst = max(worst, e)
            assert e <= TOL, (name, route, batch, bias, act, e)
            if act:
                assert (y >= 0).all()
    family = _family(AC.instance(case))
    _note(family, worst)
    print(f"atrous sweep {name}: {AC.instance(case)} worst normalised error vs fp64 {worst:.2e} ({family} so far {WORST[family]:.2e})")


def test_sweep_reaches_every_instantiation():
    assert set(KI.instances(AC.LIB)) == AC.targets()


@pytest.mark.parametrize("case", AC.CASES, ids=[c[0] for c in AC.CASES])
def test_every_accepting_route_agrees(lib, case):
    """fhip_atrous_forward_route on every route that accepts the case, packed by fhip_atrous_init_route under the same name; a route that
    does not accept it answers FHIP_E_UNSUPPORTED on the host."""
    import torch
    from feathercnn_amd import AtrousLayer, FeatherHipError
    name, c, k, group, h, w, kh, kw, s, pads, dil, _ = case
    batch = 3
    x, wt, b = R.synth(c, k, h, w, kh, kw, group, batch, seed=4000 + len(name))
    want = _want(case, x, wt, b, 1)
    xd, wd, bd = (torch.from_numpy(a).cuda() for a in (x, wt, b))
    routes = AC.accepted_routes(case)
    assert AC.instance(case) in routes
    worst, outs = 0.0, {}
    for route in routes:
        y = AtrousLayer(_param(case, 1, 1, batch), wd, bd, route=route).Forward(xd).cpu().numpy()
        e = R.nerr(y, want)
        worst = max(worst, e)
        assert e <= TOL, (name, route, e)
        outs[route] = y
    for route, y in outs.items():  # tap skipping drops exact zeros only: on and off are the same sum in the same order
        twin = route.replace("true> >", "false> >")
        if twin != route and twin in outs:
            assert np.array_equal(y, outs[twin]), (name, route)
    every = {AC.GENERIC} | {AC.dw(st, v) for st in (1, 2) for v in (False, True)} | {AC.mfma(sh, r, k_) for sh in (AC.BIG, AC.SMALLM) for r in (False, True) for k_ in (False, True)}
    for route in sorted(every - set(routes)):
        with pytest.raises(FeatherHipError) as err:
            AtrousLayer(_param(case, 1, 1, batch), wd, bd, route=route)
        assert "code -1" in str(err.value), (name, route, str(err.value))
    with pytest.raises(FeatherHipError):
        AtrousLayer(_param(case, 1, 1, batch), wd, bd, route="fhip::no_such_kernel")
    _note("routes", worst)
    print(f"atrous routes {name}: {len(routes)} routes agree, worst normalised error vs fp64 {worst:.2e}")


def test_recorded_reference_fixtures(lib):
    import torch
    from feathercnn_amd import AtrousLayer, AtrousParam
    g = np.load(os.path.join(ROOT, "tests", "golden", "atrous_golden.npz"))
    worst_ref = worst_64 = 0.0
    routes = set()
    for n in (str(v) for v in g["names"]):
        c, k, h, w, ks, s, pd, d, bias, relu, batch = (int(v) for v in g[n + "/geom"])
        p = AtrousParam.make(c, k, h, ks, s, d, pd, bias=bias, act=relu, w=w, batch=batch)
        x, wt, b = g[n + "/x"], g[n + "/w"], g[n + "/b"]
        layer = AtrousLayer(p, torch.from_numpy(wt).cuda(), torch.from_numpy(b).cuda() if bias else None)
        routes.add(layer.conv.Route(p))
        y = layer.Forward(torch.from_numpy(x).cuda()).cpu().numpy()
        e_ref = R.nerr(y, g[n + "/y"])
        e_64 = R.nerr(y, R.atrous(x, wt, b if bias else None, 1, (s, s), (pd,) * 4, (d, d), bool(relu)))
        print(f"atrous fixture {n}: vs recorded reference {e_ref:.2e}, vs fp64 {e_64:.2e}")
        worst_ref, worst_64 = max(worst_ref, e_ref), max(worst_64, e_64)
        assert e_ref <= TOL and e_64 <= TOL, (n, e_ref, e_64)
    print(f"atrous fixtures: worst vs recorded reference {worst_ref:.2e}, vs fp64 {worst_64:.2e}")
    assert AC.GENERIC in routes and any("AtrousGemmPolicy" in r for r in routes), routes  # both families of the fixtures' group-1 layers


def test_forward_is_bit_identical_and_graph_capturable(lib):
    import torch
    from feathercnn_amd import AtrousLayer, AtrousParam
    # ROW4 with tap skipping, the scalar form, the depthwise kernel, the generic kernel (grouped)
    for c, k, group, h, s, d in ((32, 96, 1, 12, 1, 12), (16, 64, 1, 11, 2, 2), (24, 24, 24, 12, 1, 2), (16, 24, 4, 9, 1, 3)):
        p = AtrousParam.make(c, k, h, 3, s, d, group=group, batch=5)
        x, wt, b = R.synth(c, k, h, h, 3, 3, group, 5, seed=77)
        layer = AtrousLayer(p, torch.from_numpy(wt).cuda(), torch.from_numpy(b).cuda())
        xd = torch.from_numpy(x).cuda()
        first = layer.Forward(xd).clone()
        assert R.nerr(first.cpu().numpy(), R.atrous(x, wt, b, group, (s, s), (d,) * 4, (d, d), True)) <= TOL
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
    net.SetDilated(True)
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


def test_tiny_dilated_net_at_every_fusion_level(cuda):
    from feathercnn_amd import model_zoo
    model = model_zoo.tiny_dilated()
    dilated = model_zoo.DILATED_LAYERS["tiny_dilated"]
    x = np.random.default_rng(3).uniform(-1, 1, (5, 3, 16, 16)).astype(np.float32)
    ref = R.Net(model[0], model[1])
    want = ref.run(model[2], x, model[3])
    assert want.shape == (5, 8, 4, 4)
    outs = {}
    for level in (0, 1, 2, 3):
        y, layers = _run(model, x, fusion=level, tuned=(level == 3))
        e = R.nerr(y, want)
        print(f"tiny_dilated fusion {level}: {len(layers)} layers, normalised error vs the restatement {e:.2e}")
        assert e <= TOL, (level, e)
        outs[level] = y
        routes = {nm: a for _, nm, a in layers}
        assert all(routes[nm] == "ATROUS" for nm in dilated), routes
        assert sum(a == "ATROUS" for a in routes.values()) == len(dilated)
        names = [nm for _, nm, _ in layers]
        if level == 0:
            assert len(layers) == 21, names
        if level == 1:
            # Convolution + ReLU only; BatchNorm and Scale stay (and compose with each other and the ReLU behind them, as they always did)
            assert not {"relu_a1", "relu_dw", "relu_g", "relu_far"} & set(names) and "a3_bn" in names, names
        if level >= 2:
            assert not {"relu_a1", "a3_bn", "a3_scale", "a3_relu", "relu_dw", "relu_g", "relu_far"} & set(names), names
            # the residual sum, the pooling and the pointwise head stay layers of their own: no other fusion takes a dilated layer
            assert {"split1", "sum", "pool1", "head", *dilated} <= set(names), names
    for level in (1, 2, 3):
        assert R.nerr(outs[level], outs[0]) <= 1e-5, level
    # sub-batch replicas, branch concurrency and the captured graph
    for kw in ({"sub_batches": 2}, {"graph": True}, {"sub_batches": 2, "graph": True, "concurrency": True}, {"concurrency": True}):
        y, _ = _run(model, x, fusion=2, **kw)
        assert R.nerr(y, outs[2]) <= 1e-5 and R.nerr(y, want) <= TOL, kw
    # a dilated layer's top can be extracted, per layer against the restatement
    blobs = ref.run(model[2], x, model[3], keep=True)
    for blob in dilated:
        y, _ = _run(model, x, blob=blob, fusion=0)
        e = R.nerr(y, blobs[blob])
        print(f"tiny_dilated blob {blob} {y.shape}: {e:.2e}")
        assert y.shape == blobs[blob].shape and e <= TOL, (blob, e)


@pytest.mark.parametrize("name", ["deeplab_largefov", "deeplab_v2_aspp"])
def test_deeplab_nets_65px_batch2(cuda, name):
    from feathercnn_amd import model_zoo
    model = model_zoo.MODELS[name](size=65)
    x = np.random.default_rng(4).uniform(-1, 1, (2, 3, 65, 65)).astype(np.float32)
    want = R.Net(model[0], model[1]).run(model[2], x, model[3])
    assert want.shape == (2, 21, 9, 9)
    for kw in ({"fusion": 1}, {"fusion": 3, "tuned": True, "graph": True}):
        y, layers = _run(model, x, **kw)
        e = R.nerr(y, want)
        routes = [a for _, _, a in layers]
        print(f"{name} 65 px b2 {kw}: {len(layers)} layers, routes {sorted(set(r for r in routes if r))}, normalised error {e:.2e}")
        assert routes.count("ATROUS") == len(model_zoo.DILATED_LAYERS[name])
        assert e <= TOL, (kw, e)


def test_kernel_trace_of_tiny_dilated(cuda, tmp_path):
    """One child under rocprofv3 --kernel-trace (tests/atrous_trace_child.py, a run of its own): tiny_dilated launches the kernels the routes
    of its dilated layers report -- MFMA instantiations on both tiles, the depthwise and the generic kernel."""
    text, rows, _ = ktrace.trace("atrous_trace_child.py", [], tmp_path, 240)
    want = [ln.split(" ", 1)[1] for ln in text.splitlines() if ln.startswith("ROUTE ")]
    assert len(want) == 6, text
    launched = {KI.normalise(name) for _, name, *_ in rows}
    assert launched, "the trace holds no kernel"
    missing = [w for w in want if w not in launched]
    assert not missing, (missing, sorted(n for n in launched if "trous" in n))
    kinds = {"mfma 128-row": any(AC.BIG in w for w in want), "mfma 64-row": any(AC.SMALLM in w for w in want),
             "depthwise": any("dw3x3" in w for w in want), "generic": AC.GENERIC in want}
    assert all(kinds.values()), kinds
    print(f"tiny_dilated trace: {sorted(set(want))} all launched")


def test_reference_style_application_runs(lib, tmp_path):
    """tests/cpp/atrous_app_main.cpp executed: feather::Net::SetDilated + tiny_dilated, and booster::AtrousConv Init / Forward on one layer,
    both against the fp64 restatement."""
    from feathercnn_amd import model_zoo
    exe = side_contract.build_app("atrous", tmp_path)
    p, b, i, o = model_zoo.tiny_dilated()
    x = np.random.default_rng(9).uniform(-1, 1, (2, 3, 16, 16)).astype(np.float32)
    lx, lw, lb = R.synth(32, 64, 5, 8, 3, 3, 1, 2, seed=10)
    paths = {n: str(tmp_path / n) for n in ("m.param", "m.bin", "in.f32", "net.f32", "x.f32", "w.f32", "b.f32", "layer.f32")}
    open(paths["m.param"], "wb").write(p)
    open(paths["m.bin"], "wb").write(b)
    for n, a in (("in.f32", x), ("x.f32", lx), ("w.f32", lw), ("b.f32", lb)):
        a.tofile(paths[n])
    r = subprocess.run(["timeout", "-k", "10", "240", exe, paths["m.param"], paths["m.bin"], paths["in.f32"], "2", "3", "16", "16", i, o, paths["net.f32"],
                        paths["x.f32"], paths["w.f32"], paths["b.f32"], paths["layer.f32"]], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr)
    want = R.Net(p, b).run(i, x, o)
    e_net = R.nerr(np.fromfile(paths["net.f32"], np.float32).reshape(want.shape), want)
    lay = R.atrous(lx, lw, lb, 1, (1, 1), (2, 2, 2, 2), (2, 2), True)
    e_lay = R.nerr(np.fromfile(paths["layer.f32"], np.float32).reshape(lay.shape), lay)
    print(f"atrous C++ application: net {e_net:.2e}, layer {e_lay:.2e}")
    assert e_net <= TOL and e_lay <= TOL
