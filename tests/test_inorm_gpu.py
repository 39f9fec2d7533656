"""libfeather_inorm.so (InstanceNorm and the activations of generative nets) on the MI355X.

* the sweep: every case of tests/inorm_cases.py -- every kernel instantiation of the library -- against the fp64 definition
  (tests/inorm_ref.py) per plane, with and without gamma / beta, all three epilogues, a distinct power-of-two scale per image, between
  guarded buffers (tests/guarded.py); the library's own route report names the instantiation the case targets;
* offset planes N(+-100, 1), where a variance computed as E[x^2] - E[x]^2 misses the bound by 10 x; constant planes; eps = 0;
* run-to-run bit identity of every case and capture into a hipGraph (an allocation in Forward would fail the capture);
* the activations over [-20, 20], +-0 and +-88; a ReLU without a slope through the Net is fhip_relu bit for bit;
* feather::Net: tiny_generative at fusion levels 0 - 3 with the expected layer lists, style_transfer_in and pix2pix_unet at batch 4,
  FeedPixels -> style_transfer_in -> ExtractPixels, refusals at Reshape (the missing library: tests/test_side_contract_gpu.py).
Bound everywhere: max|y - ref| / max|ref| <= 1e-4, per plane for the layer itself.  Each test prints its own figures."""
import ctypes

import numpy as np
import pytest

import inorm_cases as IC
import inorm_ref as R
import side_contract
from guarded import Guarded, describe

pytestmark = pytest.mark.gpu
TOL = 1e-4
ACT_CODE = {None: 0, "relu": 1, "leaky_relu": 2}


lib = side_contract.fixture("inorm", gpu=True)


_stream = side_contract.stream


def _synth(case, seed):
    """Input N(0.3, 1) times a distinct power of two per image, gamma U(0.5, 1.5) with alternating sign, beta U(-0.5, 0.5)."""
    _, n, c, h, w, _ = case
    rng = np.random.default_rng(seed)
    x = rng.normal(0.3, 1.0, (n, c, h, w)).astype(np.float32)
    x *= np.float32(2.0) ** np.arange(-2, n - 2, dtype=np.float32).reshape(n, 1, 1, 1)
    gamma = (rng.uniform(0.5, 1.5, c) * np.where(np.arange(c) % 2, -1, 1)).astype(np.float32)
    beta = rng.uniform(-0.5, 0.5, c).astype(np.float32)
    return x, gamma, beta


def _forward(lib, case, gx, gy, gg, gb, gs, eps, act, slope):
    _, n, c, h, w, _ = case
    v = ctypes.c_void_p
    rc = lib.fhip_instance_norm_forward(n, c, h, w, v(gy.ptr), v(gx.ptr), v(gg.ptr) if gg else None, v(gb.ptr) if gb else None, eps, ACT_CODE[act],
                                        slope, v(gs.ptr), _stream())
    assert rc == 0, lib.fhip_inorm_last_error()


@pytest.mark.parametrize("case", IC.CASES, ids=[c[0] for c in IC.CASES])
def test_sweep_between_guards(lib, case):
    import torch
    name, n, c, h, w, offset = case
    x, gamma, beta = _synth(case, 3000 + len(name))
    sb = ctypes.c_size_t()
    assert lib.fhip_instance_norm_get_buffer_size(n, c, h, w, ctypes.byref(sb)) == 0 and sb.value == IC.scratch_bytes(case)
    gx, gy = Guarded(x.size, x, offset), Guarded(x.size, "poison", offset)
    gs = Guarded(sb.value // 4, "poison", 0)
    route = ctypes.create_string_buffer(96)
    assert lib.fhip_instance_norm_route(n, c, h, w, ctypes.c_void_p(gy.ptr), ctypes.c_void_p(gx.ptr), route, 96) == 0
    assert route.value.decode() == IC.instance(case), (name, route.value)
    worst = 0.0
    for affine in (True, False):
        gg, gb = (Guarded(c, gamma, 0), Guarded(c, beta, 1)) if affine else (None, None)
        for act, slope in IC.EPILOGUES:
            eps = 1e-3 if act != "relu" else 1e-5
            gy.fill("poison")
            gs.fill("poison")
            snaps = [g.snapshot() for g in (gx, gg, gb) if g]
            _forward(lib, case, gx, gy, gg, gb, gs, eps, act, slope)
            torch.cuda.synchronize()
            for what, g in (("output", gy), ("scratch", gs), ("input", gx), ("gamma", gg), ("beta", gb)):
                assert g is None or g.guards_intact() is None, f"{name}: {what} guard: {describe(g.guards_intact())}"
            assert gy.unwritten() == 0 and gs.unwritten() == 0, (name, gy.unwritten(), gs.unwritten())
            for g, snap in zip([g for g in (gx, gg, gb) if g], snaps):
                assert g.unchanged(snap), (name, g.first_change(snap))
            y = gy.values().reshape(n, c, h, w)
            assert np.isfinite(y).all(), f"{name}: a value from outside a tensor reached the result"
            want = R.instance_norm(x, gamma if affine else None, beta if affine else None, np.float32(eps), act, np.float32(slope))
            e = R.plane_nerr(y, want)
            worst = max(worst, e)
            assert e <= TOL, (name, affine, act, e)
            if act == "relu":
                assert (y >= 0).all()
            first = gy.bits().clone()
            _forward(lib, case, gx, gy, gg, gb, gs, eps, act, slope)  # a second forward: bit-identical
            torch.cuda.synchronize()
            assert torch.equal(gy.bits(), first), name
    print(f"inorm sweep {name}: {' + '.join(IC.instances(case))} worst per-plane normalised error vs fp64 {worst:.2e}")


def test_sweep_reaches_every_instantiation():
    import kernel_instances as KI
    assert set(KI.instances(IC.LIB)) == IC.targets()


OFFSET_SHAPES = [(3, 5, 7, 7), (3, 5, 64, 64), (3, 2, 256, 256), (3, 5, 128, 128), (3, 86, 128, 128), (3, 2, 129, 127)]


@pytest.mark.parametrize("shape", OFFSET_SHAPES, ids=["x".join(map(str, s)) for s in OFFSET_SHAPES])
def test_offset_planes(cuda, shape):
    """x ~ N(+-100, 1): a two-pass variance in fp32 has 10 x margin to the bound, E[x^2] - E[x]^2 misses it by 10 x (tests/test_inorm_cpu.py)."""
    import torch
    from feathercnn_amd import instance_norm, instance_norm_route
    rng = np.random.default_rng(4)
    for mean in (100.0, -100.0):
        x = rng.normal(mean, 1.0, shape).astype(np.float32)
        gamma, beta = rng.uniform(0.5, 1.5, shape[1]).astype(np.float32), rng.uniform(-0.5, 0.5, shape[1]).astype(np.float32)
        xd = torch.from_numpy(x).cuda()
        y = instance_norm(xd, torch.from_numpy(gamma).cuda(), torch.from_numpy(beta).cuda(), 1e-3).cpu().numpy()
        e = R.plane_nerr(y, R.instance_norm(x, gamma, beta, np.float32(1e-3)))
        print(f"offset planes {shape} mean {mean:+.0f} ({instance_norm_route(xd)}): per-plane normalised error {e:.2e}")
        assert e <= TOL, (shape, mean, e)


def test_every_route_that_holds_a_plane_gives_the_same_result(cuda):
    """fhip_instance_norm_forward_route: a plane that fits several routes (tools/inorm_bench.py --routes times them against each other to
    place the thresholds) is normalised by each of them to the bound, and the grid-strided plane kernels agree with themselves."""
    import torch
    from feathercnn_amd import instance_norm
    rng = np.random.default_rng(12)
    for shape, routes in (((3, 5, 16, 16), ("wave", "block256", "block1024", "split")), ((3, 5, 31, 33), ("wave", "block256", "block1024", "split")),
                          ((3, 5, 64, 64), ("block256", "block1024", "split")), ((3, 5, 90, 90), ("block1024", "split"))):
        x = rng.normal(0.5, 1.0, shape).astype(np.float32)
        gamma, beta = rng.uniform(0.5, 1.5, shape[1]).astype(np.float32), rng.uniform(-0.5, 0.5, shape[1]).astype(np.float32)
        want = R.instance_norm(x, gamma, beta, np.float32(1e-3), "leaky_relu", np.float32(0.2))
        for route in routes:
            y = instance_norm(torch.from_numpy(x).cuda(), torch.from_numpy(gamma).cuda(), torch.from_numpy(beta).cuda(), 1e-3, "leaky_relu", 0.2,
                              route=route).cpu().numpy()
            e = R.plane_nerr(y, want)
            print(f"forced route {route} on {shape}: per-plane normalised error {e:.2e}")
            assert e <= TOL, (shape, route, e)


def test_constant_planes_and_eps_zero(cuda):
    import torch
    from feathercnn_amd import instance_norm, instance_norm_route
    rng = np.random.default_rng(5)
    routes = set()
    for shape in ((3, 6, 7, 7), (3, 6, 1, 1), (3, 6, 32, 32), (3, 6, 50, 50), (3, 6, 33, 33), (3, 6, 64, 64), (3, 90, 72, 72), (3, 3, 100, 130), (3, 2, 129, 127)):
        n, c = shape[:2]
        vals = rng.uniform(-1, 1, (n, c, 1, 1)).astype(np.float32)
        vals[0, 0], vals[0, 1] = 0.0, 1.0
        x = np.broadcast_to(vals, shape).copy()
        gamma, beta = rng.uniform(-2, 2, c).astype(np.float32), rng.uniform(-0.5, 0.5, c).astype(np.float32)
        xd = torch.from_numpy(x).cuda()
        routes.add(instance_norm_route(xd))
        y = instance_norm(xd, torch.from_numpy(gamma).cuda(), torch.from_numpy(beta).cuda(), 1e-3).cpu().numpy()
        assert np.isfinite(y).all(), shape
        d = float(np.abs(y - beta.reshape(1, c, 1, 1)).max())
        print(f"constant planes {shape}: max |y - beta| = {d:.2e}")
        assert d <= 1e-6, (shape, d)
        # eps = 0 on planes that are not constant: accepted, and the definition's result
        x = rng.normal(0, 1, shape).astype(np.float32) if shape[2] * shape[3] > 1 else None
        if x is not None:
            y = instance_norm(torch.from_numpy(x).cuda(), torch.from_numpy(gamma).cuda(), torch.from_numpy(beta).cuda(), 0.0).cpu().numpy()
            assert R.plane_nerr(y, R.instance_norm(x, gamma, beta, 0.0)) <= TOL, shape
    assert len(routes) == 7, routes  # every route, all but one in both access widths


def test_graph_capture_replays_the_eager_result(cuda):
    """Each route captured into a hipGraph and replayed: bit-identical to the eager forward.  Forward allocates nothing -- a hipMalloc
    inside the captured region would invalidate the capture."""
    import torch
    from feathercnn_amd import activation, instance_norm
    from feathercnn_amd.inorm import scratch_bytes
    rng = np.random.default_rng(6)
    for shape in ((5, 6, 13, 13), (5, 6, 64, 64), (3, 90, 72, 72), (3, 2, 256, 256), (3, 2, 129, 127)):
        c = shape[1]
        x = torch.from_numpy(rng.normal(0, 1, shape).astype(np.float32)).cuda()
        gamma, beta = torch.from_numpy(rng.uniform(0.5, 1.5, c).astype(np.float32)).cuda(), torch.from_numpy(rng.uniform(-1, 1, c).astype(np.float32)).cuda()
        scratch = torch.empty(max(scratch_bytes(shape) // 4, 1), dtype=torch.float32, device="cuda")
        eager = instance_norm(x, gamma, beta, 1e-3, "leaky_relu", 0.2, scratch=scratch).clone()
        eager_t = activation(eager, "tanh")
        out, out_t = torch.full_like(x, float("nan")), torch.full_like(x, float("nan"))
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(graph, stream=side):
                instance_norm(x, gamma, beta, 1e-3, "leaky_relu", 0.2, out=out, scratch=scratch)
                activation(out, "tanh", out=out_t)
        assert torch.isnan(out).all()  # captured, not run
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager) and torch.equal(out_t, eager_t), shape
        x.copy_(x.flip(0))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, instance_norm(x, gamma, beta, 1e-3, "leaky_relu", 0.2, scratch=scratch)), shape


# ---- activations ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", IC.ACT_CASES, ids=[c[0] for c in IC.ACT_CASES])
def test_activations_between_guards(lib, case):
    import torch
    name, n, c, hw, offset = case
    rng = np.random.default_rng(7000 + len(name))
    x = rng.uniform(-20, 20, (n, c, hw)).astype(np.float32)
    x.reshape(-1)[:8] = [0.0, -0.0, 88.0, -88.0, 20.0, -20.0, 1e-30, -1e-30]
    slopes = rng.uniform(0.05, 0.35, c).astype(np.float32)
    gx, gy, gs = Guarded(x.size, x, offset), Guarded(x.size, "poison", offset), Guarded(c, slopes, 1)
    v = ctypes.c_void_p
    for kind in IC.KINDS:
        code = {"leaky_relu": 0, "prelu_shared": 1, "prelu": 1, "sigmoid": 2, "tanh": 3, "clip": 4}[kind]
        p0, p1 = {"leaky_relu": (0.2, 0.0), "prelu_shared": (0.25, 0.0), "clip": (-3.5, 6.0)}.get(kind, (0.0, 0.0))
        gy.fill("poison")
        snap = gx.snapshot()
        rc = lib.fhip_activation_forward(code, v(gy.ptr), v(gx.ptr), n, c, hw, p0, p1, v(gs.ptr) if kind == "prelu" else None, _stream())
        assert rc == 0, lib.fhip_inorm_last_error()
        torch.cuda.synchronize()
        assert gy.guards_intact() is None and gx.unchanged(snap) and gs.guards_intact() is None, (name, kind)
        y = gy.values().reshape(n, c, hw)
        assert np.isfinite(y).all() and gy.unwritten() == 0, (name, kind)
        want = {"leaky_relu": lambda: R.activation(x, "leaky_relu", np.float32(0.2)), "prelu_shared": lambda: R.activation(x, "prelu", np.float32(0.25)),
                "prelu": lambda: R.activation(x, "prelu", slopes=slopes), "sigmoid": lambda: R.activation(x, "sigmoid"),
                "tanh": lambda: R.activation(x, "tanh"), "clip": lambda: R.activation(x, "clip", lo=-3.5, hi=6.0)}[kind]()
        e = R.nerr(y, want)
        print(f"activation {name} {kind}: normalised error {e:.2e}")
        assert e <= TOL, (name, kind, e)
        f = y.reshape(-1)
        if kind == "sigmoid":
            assert f[2] == 1.0 and 0.0 <= f[3] <= 1e-37 and f[0] == 0.5 and f[1] == 0.5
        if kind == "tanh":
            assert f[2] == 1.0 and f[3] == -1.0 and f[0] == 0.0 and f[1] == 0.0
    # in place
    rc = lib.fhip_activation_forward(3, v(gx.ptr), v(gx.ptr), n, c, hw, 0.0, 0.0, None, _stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert R.nerr(gx.values().reshape(n, c, hw), R.activation(x, "tanh")) <= TOL and gx.guards_intact() is None


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


def _one(line, c=8):
    return f"7767517\n2 2\nInput data 0 1 data 0=8 1=8 2={c}\n{line}\n".encode()


def test_plain_relu_through_the_net_is_fhip_relu(cuda):
    import torch
    from feathercnn_amd import _lib
    x = np.random.default_rng(8).normal(0, 1, (3, 8, 8, 8)).astype(np.float32)
    x.reshape(-1)[:2] = [0.0, -0.0]
    xd = torch.from_numpy(x).cuda()
    want = torch.empty_like(xd)
    assert _lib.load_library().fhip_relu(ctypes.c_void_p(want.data_ptr()), ctypes.c_void_p(xd.data_ptr()), xd.numel(), _stream()) == 0
    torch.cuda.synchronize()
    for line in ("ReLU r 1 1 data r", "ReLU r 1 1 data r 0=0", "ReLU r 1 1 data r 0=0.0"):
        y, _ = _run((_one(line), b"", "data", "r"), x)
        assert np.array_equal(y.view(np.int32), want.cpu().numpy().view(np.int32)), line
    y, layers = _run((_one("ReLU r 1 1 data r 0=0.2"), b"", "data", "r"), x)
    assert layers[1][:2] == ("ReLU", "r") and R.nerr(y, R.activation(x, "leaky_relu", np.float32(0.2))) <= 1e-7 and (y[x < 0] < 0).all()


def test_reshape_refuses_mismatched_channels(cuda):
    from feathercnn_amd import FeatherHipError
    from feathercnn_amd.net import Net
    x = np.zeros((1, 8, 8, 8), np.float32)
    for line, weights in (("InstanceNorm n 1 1 data n 0=6", np.ones(12, np.float32).tobytes()), ("PReLU n 1 1 data n 0=3", np.ones(3, np.float32).tobytes())):
        net = Net()
        net.LoadParam(_one(line))
        net.LoadWeights(weights)
        with pytest.raises(FeatherHipError) as e:
            net.FeedInput("data", x)
            net.Forward()
        assert "code -300" in str(e.value), str(e.value)
        net.close()


def test_tiny_generative_net_at_every_fusion_level(cuda):
    from feathercnn_amd import model_zoo
    model = model_zoo.tiny_generative()
    x = np.random.default_rng(3).uniform(-1, 1, (5, 3, 24, 24)).astype(np.float32)
    ref = R.Net(model[0], model[1])
    blobs = ref.run(model[2], x, model[3], keep=True)
    want = blobs["out"]
    assert want.shape == (5, 3, 20, 20) and blobs["gate"].shape == (5, 32, 1, 1)
    all_names = [nm for _, nm, _, _, _ in ref.layers]
    outs = {}
    for level in (0, 1, 2, 3):
        y, layers = _run(model, x, fusion=level, tuned=(level == 3))
        e = R.nerr(y, want)
        gate, _ = _run(model, x, blob="gate", fusion=level, tuned=(level == 3))
        eg = R.nerr(gate, blobs["gate"])
        print(f"tiny_generative fusion {level}: {len(layers)} layers, normalised error vs the restatement {e:.2e} (out), {eg:.2e} (gate)")
        assert e <= TOL and eg <= TOL, (level, e, eg)
        outs[level] = y
        names = [nm for _, nm, _ in layers]
        routes = {nm: a for _, nm, a in layers}
        assert all(routes[nm] == "INORM" for nm in ("conv1_in", "in2", "in3", "in4", "d1_in")), routes
        # InstanceNorm + ReLU (leaky or plain) is one layer from level 1 on; nothing else about the new layers fuses at any level, and a
        # Convolution followed by a leaky ReLU stays two layers
        absorbed = [] if level == 0 else ["conv1_relu", "relu2", "d1_relu"]
        assert names == [nm for nm in all_names if nm not in absorbed], (level, names)
        assert "conv2" in names and "lrelu2" in names
    for level in (1, 2, 3):
        assert R.nerr(outs[level], outs[0]) <= 1e-5, level
    for kw in ({"sub_batches": 2}, {"graph": True}, {"sub_batches": 2, "graph": True, "concurrency": True}):
        y, _ = _run(model, x, fusion=2, **kw)
        assert R.nerr(y, outs[2]) <= 1e-5 and R.nerr(y, want) <= TOL, kw
    for blob in ("conv1_relu", "lrelu2", "relu2", "prelu3", "in4", "prelu4", "d1_relu", "clip"):
        y, _ = _run(model, x, blob=blob, fusion=0)
        e = R.nerr(y, blobs[blob])
        print(f"tiny_generative blob {blob} {y.shape}: {e:.2e}")
        assert y.shape == blobs[blob].shape and e <= TOL, (blob, e)


@pytest.mark.parametrize("name", ["style_transfer_in", "pix2pix_unet"])
def test_generative_nets_batch4(cuda, name):
    from feathercnn_amd import model_zoo
    model = model_zoo.MODELS[name]()
    x = np.random.default_rng(4).uniform(-1, 1, (4, 3, 256, 256)).astype(np.float32)
    want = R.Net(model[0], model[1]).run(model[2], x, model[3])
    assert want.shape == (4, 3, 256, 256)
    for kw in ({"fusion": 3, "tuned": True, "graph": True}, {"fusion": 3, "tuned": True, "graph": True, "sub_batches": 2}):
        y, layers = _run(model, x, **kw)
        e = R.nerr(y, want)
        routes = [a for _, _, a in layers]
        print(f"{name} b4 {kw}: {len(layers)} layers, {routes.count('INORM')} InstanceNorm, normalised error {e:.2e}")
        assert routes.count("INORM") == sum(t == "InstanceNorm" for t, *_ in R.gconv_ref.parse_param(model[0]))
        # every ReLU behind an InstanceNorm is absorbed; pix2pix's first encoder level (Convolution + leaky ReLU) keeps its own
        assert [nm for t, nm, _ in layers if t == "ReLU"] == ([] if name == "style_transfer_in" else ["e1_relu"])
        assert e <= TOL, (kw, e)


def test_pixels_through_style_transfer_in_to_pixels(cuda):
    """FeedPixels -> style_transfer_in -> ExtractPixels (mean -1, norm 127.5: TanH's [-1, 1] to [0, 255]) against the host composition of
    the repo's pixel restatements around inorm_ref.Net: equal in at least 99.5 % of the bytes, never off by more than 1."""
    import pixels_ref as P
    from feathercnn_amd import model_zoo
    from feathercnn_amd.net import Net
    param, weights, i, o = model_zoo.style_transfer_in()
    px, x = R.pixel_input()
    want = R.Net(param, weights).run(i, x, o)
    expect = R.pixel_output(want)
    for kw in ({"fusion": 1}, {"fusion": 3, "tuned": True, "graph": True}):
        net = Net(**kw)
        net.LoadParam(param)
        net.LoadWeights(weights)
        net.FeedPixels(i, px, P.PIXEL_RGB, (R.PIXEL_SIZE, R.PIXEL_SIZE), R.PIXEL_MEAN_IN, R.PIXEL_NORM_IN)
        net.Forward()
        e = R.nerr(net.Extract(o), want)
        got = net.ExtractPixels(o, P.PIXEL_RGB, None, np.float32(R.PIXEL_MEAN_OUT), np.float32(R.PIXEL_NORM_OUT))
        net.close()
        assert got.shape == expect.shape and got.dtype == np.uint8
        diff = np.abs(got.astype(np.int32) - expect.astype(np.int32))
        share = float((diff != 0).mean())
        print(f"style_transfer_in pixels {kw}: blob error {e:.2e}; {100 * share:.3f} % of {diff.size} bytes differ, by at most {int(diff.max())}")
        assert e <= TOL
        assert diff.max() <= 1 and share <= R.PIXEL_CAP
