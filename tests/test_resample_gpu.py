"""libfeather_resample.so (Interp: nearest / bilinear resize; HardSwish) on the MI355X.

* Interp: every row of tests/resample_cases.py -- both modes, both align_corner values, the size given and decided by a scale, 1 / 3 / 17
  channels, batches 1 / 3, pointers 0 / 4 / 8 / 12 bytes past a 16-byte boundary -- bit for bit (int32 views) against the float32
  restatement of tests/resample_ref.py, every tensor between guards (tests/guarded.py's canary and poison words): nothing outside the
  output is written, every output word is, no input changes, two runs give the same bits, and fhip_interp_route names the instantiation
  the header states for those pointers;
* Interp with a residual, and with a residual and ReLU, bit-identical to the resize followed by fhip_add; out aliasing the residual; out
  overlapping in refused;
* HardSwish bit for bit, with inputs planted at lower, upper, +-0 and their float32 neighbours, in place, sizes 1 / 3 / 4 / 1023 / 4097;
* feather::Net: tiny_resample at fusion levels 0 .. 3, with sub-batches, the graph and concurrency, against resample_ref.Net at the
  project's 1e-4 normalised; the collapsed upsample-add-ReLU bit-identical to the library applied to that run's own blobs; a second input
  size through the same net; mobilenet_v3_small / _large, fpn_resnet50, deeplab_largefov_full and unet_bilinear at small sizes; a net
  without these layers never maps the library; one collapsed upsample-add-ReLU is one launch by kernel trace.
Each test prints its own figures."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import ktrace
import resample_cases as RC
import resample_ref as R
from guarded import CANARY, POISON

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-4
GUARD = 1 << 14  # floats on each side
TRACE_TIMEOUT = 240


class Region:
    """[guard | body | guard] in one allocation, the body `offset` floats (0 .. 3) past a 16-byte boundary (tests/guarded.py's layout)."""

    def __init__(self, shape, fill="poison", offset=0):
        import torch
        self.shape, self.n = tuple(shape), int(np.prod(shape))
        self.raw = torch.full((2 * GUARD + 4 + self.n,), CANARY, dtype=torch.int32, device="cuda")
        self.lo = GUARD + offset
        self.body = self.raw.view(torch.float32)[self.lo:self.lo + self.n]
        if isinstance(fill, str):
            self.raw[self.lo:self.lo + self.n] = POISON
        else:
            self.body.copy_(torch.from_numpy(np.ascontiguousarray(fill, np.float32).reshape(-1)))
        assert self.raw.data_ptr() % 16 == 0
        self.tensor = self.body.view(self.shape)
        assert self.tensor.data_ptr() % 16 == 4 * offset
        self.snap = self.raw.clone()

    def guards_intact(self):
        return bool((self.raw[:self.lo] == CANARY).all()) and bool((self.raw[self.lo + self.n:] == CANARY).all())

    def unwritten(self):
        return int((self.raw[self.lo:self.lo + self.n] == POISON).sum())

    def unchanged(self):
        import torch
        return bool(torch.equal(self.raw, self.snap))

    def bits(self):
        return self.raw[self.lo:self.lo + self.n].cpu().numpy().reshape(self.shape)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _shapes():
    """(n, c, offsets): every offset on the smallest and the largest tensor of a row, offset 0 on the others."""
    for c in RC.CHANNELS:
        for n in RC.BATCHES:
            yield n, c, (RC.OFFSETS if (n, c) in ((1, 1), (3, 17)) else (0,))


def _variants(i, o):
    for mode, align, ii, oo, by in RC.cases():
        if (ii, oo) == (i, o):
            yield mode, align, by


# ---- Interp ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i,o", RC.PLANES, ids=[f"{i[0]}x{i[1]}-{o[0]}x{o[1]}" for i, o in RC.PLANES])
def test_interp_bit_for_bit_between_guards(cuda, i, o):
    from feathercnn_amd import interp
    from feathercnn_amd.resample import interp_route
    rng = np.random.default_rng(1000 * i[0] + 10 * i[1] + o[0])
    launches, routes = 0, set()
    for n, c, offsets in _shapes():
        x = rng.uniform(-2, 2, (n, c) + i).astype(np.float32)
        for mode, align, by in _variants(i, o):
            hs, ws = RC.by_scale(i, o) if by == "scale" else (0.0, 0.0)
            kw = {"scale": (hs, ws)} if by == "scale" else {"size": o}
            want = _bits(R.interp(x, mode, o[0], o[1], bool(align), hs, ws))
            for off in offsets:
                for in_off in ({off, 0} if off else {0}):  # both tensors off the boundary, and the output alone
                    xi, out = Region(x.shape, x, in_off), Region((n, c) + o, "poison", off)
                    interp(xi.tensor, mode, align_corner=bool(align), out=out.tensor, **kw)
                    route = interp_route(xi.tensor, mode, out=out.tensor, **kw)
                    assert route == RC.expected_route(mode, i, o, hs, ws, off, in_off), (n, c, mode, by, off, in_off, route)
                    routes.add(route)
                    launches += 1
                    assert out.guards_intact() and out.unwritten() == 0, (n, c, mode, align, by, off, in_off, route)
                    assert xi.unchanged(), (n, c, mode, align, by, off)
                    assert np.array_equal(out.bits(), want), (n, c, mode, align, by, off, in_off, route)
            again = Region((n, c) + o, "poison", 0)  # two runs give the same bits
            interp(Region(x.shape, x, 0).tensor, mode, align_corner=bool(align), out=again.tensor, **kw)
            assert np.array_equal(again.bits(), want)
    print(f"interp {i} -> {o}: {launches} launches bit-identical to the float32 restatement; routes {sorted(routes)}")


@pytest.mark.parametrize("i,o", RC.PLANES, ids=[f"{i[0]}x{i[1]}-{o[0]}x{o[1]}" for i, o in RC.PLANES])
def test_interp_with_residual_and_relu_equals_the_unfused_composition(cuda, i, o):
    """out = relu(interp(x) + r) in one launch against interp, then fhip_add (with its ReLU): the same bits, and the restatement's; out may
    be the residual."""
    from feathercnn_amd import FeatherHipError, interp
    from feathercnn_amd.net import add
    from feathercnn_amd.resample import interp_route
    rng = np.random.default_rng(77 * i[0] + o[1])
    routes = set()
    for n, c in ((1, 1), (3, 17)):
        x = rng.uniform(-2, 2, (n, c) + i).astype(np.float32)
        r = rng.uniform(-2, 2, (n, c) + o).astype(np.float32)
        for mode, align, by in _variants(i, o):
            if mode == R.BILINEAR and align:
                continue
            hs, ws = RC.by_scale(i, o) if by == "scale" else (0.0, 0.0)
            kw = {"scale": (hs, ws)} if by == "scale" else {"size": o}
            for off, res_off in ((0, 0), (1, 1), (0, 2)):
                xi, ri = Region(x.shape, x, 0), Region(r.shape, r, res_off)
                plain = interp(xi.tensor, mode, **kw)
                for relu in (False, True):
                    out = Region(r.shape, "poison", off)
                    interp(xi.tensor, mode, residual=ri.tensor, relu=relu, out=out.tensor, **kw)
                    route = interp_route(xi.tensor, mode, out=out.tensor, residual=ri.tensor, **kw)
                    assert route == RC.expected_route(mode, i, o, hs, ws, off, 0, res_off), (mode, by, off, res_off, route)
                    routes.add(route)
                    assert out.guards_intact() and out.unwritten() == 0 and xi.unchanged() and ri.unchanged(), (n, c, mode, by, off, relu)
                    two = add(plain, ri.tensor.clone(), relu=relu)
                    assert np.array_equal(out.bits(), two.cpu().numpy().view(np.int32)), (n, c, mode, by, off, res_off, relu)
                    assert np.array_equal(out.bits(), _bits(R.interp(x, mode, o[0], o[1], False, hs, ws, residual=r, relu=relu))), (n, c, mode, by, off, relu)
                want = out.bits()
                interp(xi.tensor, mode, residual=ri.tensor, relu=True, out=ri.tensor, **kw)  # out aliasing the residual
                assert ri.guards_intact() and np.array_equal(ri.bits(), want), (n, c, mode, by, res_off)
        with pytest.raises(FeatherHipError, match="overlap"):
            interp(xi.tensor, mode, size=i, out=xi.tensor)
        assert xi.unchanged()
    print(f"interp + residual (+ ReLU) {i} -> {o}: fused == two launches == restatement; routes {sorted(routes)}")


# ---- HardSwish -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha,beta", RC.HARDSWISH_PARAMS + ((0.7, -0.1), (-0.25, 0.5)))
def test_hard_swish_bit_for_bit(cuda, alpha, beta):
    from feathercnn_amd import hard_swish
    from feathercnn_amd.resample import hard_swish_route
    rng = np.random.default_rng(9)
    a32, b32 = np.float32(alpha), np.float32(beta)
    lower = -b32 / a32
    upper = np.float32(1) / a32 + lower
    planted = []
    for v in (lower, upper, np.float32(0.0), np.float32(-0.0)):
        planted += [v, np.nextafter(v, np.float32(np.inf), dtype=np.float32), np.nextafter(v, np.float32(-np.inf), dtype=np.float32)]
    routes = set()
    for size in RC.HARDSWISH_SIZES:
        x = rng.uniform(-8, 8, size).astype(np.float32)
        k = min(size, len(planted))
        x[:k] = planted[:k] if size > 4 else planted[3 * (size % 4):3 * (size % 4) + k]
        want = _bits(R.hard_swish(x, alpha, beta))
        for off in RC.OFFSETS:
            xi, out = Region((1, 1, size), x, off), Region((1, 1, size), "poison", off)
            hard_swish(xi.tensor, alpha, beta, out=out.tensor)
            route = hard_swish_route(xi.tensor, out.tensor)
            assert route == f"fhip::hardswish_kernel<{'true' if size % 4 == 0 and off == 0 else 'false'}>"
            routes.add(route)
            assert out.guards_intact() and out.unwritten() == 0 and xi.unchanged(), (size, off)
            assert np.array_equal(out.bits().reshape(-1), want), (size, off, alpha, beta)
            hard_swish(xi.tensor, alpha, beta, out=xi.tensor)  # in place
            assert xi.guards_intact() and np.array_equal(xi.bits().reshape(-1), want), (size, off)
    x = rng.uniform(-8, 8, (3, 17, 7, 12)).astype(np.float32)  # a tensor as a net hands it over
    got = hard_swish(Region(x.shape, x, 0).tensor, alpha, beta)
    assert np.array_equal(got.cpu().numpy().view(np.int32), _bits(R.hard_swish(x, alpha, beta)))
    assert routes == {"fhip::hardswish_kernel<true>", "fhip::hardswish_kernel<false>"}
    print(f"hard_swish({alpha:.4f}, {beta}): lower {lower}, upper {upper}; sizes {RC.HARDSWISH_SIZES} bit-identical at every offset, in place too")


# ---- feather::Net ----------------------------------------------------------------------------------------------------------------------
_REF = {}


def _reference(name, size, batch, seed):
    from feathercnn_amd import model_zoo
    key = (name, size, batch, seed)
    if key not in _REF:
        kw = {} if name == "tiny_resample" and size == 24 else {"size": size}
        model = model_zoo.MODELS[name](**kw)
        x = np.random.default_rng(seed).uniform(-1, 1, (batch, 3, size, size)).astype(np.float32)
        _REF[key] = (model, x, R.Net(model[0], model[1]).run(model[2], x, model[3], keep=True))
    return _REF[key]


def _net(model, x, level, dilated=False, **kw):
    from feathercnn_amd.net import Net
    net = Net(fusion=level, **kw)
    net.SetExtendedLayers(True)
    if dilated:
        net.SetDilated(True)
    net.LoadParam(model[0])
    net.LoadWeights(model[1])
    net.FeedInput(model[2], x)
    net.Forward()
    return net


TINY_BLOBS = ("sum1_relu", "sum2", "side", "shrink", "aligned", "to_ref", "down", "heads", "fc", "prob")


@pytest.mark.parametrize("level,kw", [(0, {}), (1, {}), (2, {}), (3, {}), (2, {"sub_batches": 2}), (2, {"graph": True}), (3, {"graph": True, "tuned": True}),
                                      (2, {"concurrency": True}), (2, {"concurrency": True, "graph": True})])
def test_tiny_resample_against_the_restatement(cuda, level, kw):
    model, x, blobs = _reference("tiny_resample", 24, 5, 21)
    net = _net(model, x, level, **kw)
    if kw.get("graph"):
        net.Forward()  # the replay
    worst = 0.0
    for name in TINY_BLOBS + (("hs1", "hs2", "up1", "up2") if level == 0 else ()):
        got = net.Extract(name)
        e = R.nerr(got, blobs[name])
        worst = max(worst, e)
        assert got.shape == blobs[name].shape and e <= TOL, (level, kw, name, e)
    routed = [nm for _, nm, a in net.layers() if a == "RESAMPLE"]
    assert sorted(routed) == sorted(["hs1", "hs2", "up1", "up2", "shrink", "aligned", "to_ref", "down"])
    names = [nm for _, nm, _ in net.layers()]
    assert ("sum1" in names) == (level < 2)
    print(f"tiny_resample level {level} {kw}: worst normalised error {worst:.2e}, {len(routed)} resample-route layers of {len(names)}")


@pytest.mark.parametrize("level", [2, 3])
def test_the_collapsed_layer_equals_the_library_on_its_own_blobs(cuda, level):
    """up1 -> sum1 -> sum1_relu as one layer: its output is, bit for bit, interp(residual, relu) of that run's own relu3 and lat; the blobs
    inside refuse Extract; at level 0 every Interp and HardSwish top is the library call on its bottom."""
    import torch
    from feathercnn_amd import FeatherHipError, hard_swish, interp
    model, x, _ = _reference("tiny_resample", 24, 5, 21)
    net = _net(model, x, level)
    t = lambda name: torch.from_numpy(net.Extract(name)).cuda()
    want = interp(t("relu3"), "nearest", scale=2.0, residual=t("lat"), relu=True)
    assert np.array_equal(_bits(net.Extract("sum1_relu")), want.cpu().numpy().view(np.int32))
    for name in ("up1", "sum1"):
        with pytest.raises(FeatherHipError, match="fused"):
            net.Extract(name)
    net.Extract("up2")  # the Interp with two readers keeps its blob
    lv0 = _net(model, x, 0)
    t = lambda name: torch.from_numpy(lv0.Extract(name)).cuda()
    for top, bottom, kw in (("up1", "relu3", {"mode": "nearest", "scale": 2.0}), ("up2", "split2_0", {"mode": "nearest", "scale": 2.0}),
                            ("shrink", "split1_2", {"mode": "bilinear", "scale": (np.float32(0.45), np.float32(0.6))}),
                            ("aligned", "split2_1", {"mode": "bilinear", "scale": (np.float32(0.75), np.float32(1.1)), "align_corner": True}),
                            ("to_ref", "q_relu", {"mode": "bilinear", "size": (9, 13)}), ("down", "split2_2", {"mode": "nearest", "size": (5, 5)})):
        assert np.array_equal(_bits(lv0.Extract(top)), interp(t(bottom), **kw).cpu().numpy().view(np.int32)), top
    assert np.array_equal(_bits(lv0.Extract("hs1")), hard_swish(t("conv1")).cpu().numpy().view(np.int32))
    assert np.array_equal(_bits(lv0.Extract("hs2")), hard_swish(t("conv2"), np.float32(0.166667), 0.5).cpu().numpy().view(np.int32))
    assert np.array_equal(_bits(lv0.Extract("sum1_relu")), _bits(net.Extract("sum1_relu")))  # one launch or three: the same bits


def test_a_second_input_size_and_reshape_refusals(cuda):
    from feathercnn_amd import FeatherHipError, model_zoo
    from feathercnn_amd.net import Net
    for level in (0, 2):
        model = model_zoo.tiny_resample()
        net = None
        for size, seed in ((24, 1), (20, 2), (24, 3)):  # the two-bottom Interp follows the input: 9 x 13, 7 x 11, 9 x 13
            x = np.random.default_rng(seed).uniform(-1, 1, (3, 3, size, size)).astype(np.float32)
            if net is None:
                net = _net(model, x, level)
            else:
                net.FeedInput(model[2], x)
                net.Forward()
            want = R.Net(model[0], model[1]).run(model[2], x, model[3], keep=True)
            for name in ("to_ref", "sum1_relu", "prob"):
                assert net.Extract(name).shape == want[name].shape and R.nerr(net.Extract(name), want[name]) <= TOL, (level, size, name)
        assert net.Extract("to_ref").shape[2:] == (9, 13)
    head = "7767517\n3 4\nInput data 0 1 data 0=8 1=8 2=8\n"
    for lines, word in (("ReLU p 1 1 data p\nInterp m 1 1 p m 0=2 1=0.1 2=1.0\n", "below 1"),  # int(8 * 0.1) = 0
                        ("Interp p 1 1 data p 0=1 1=2.0 2=2.0\nEltwise m 2 1 data p m 0=1\n", "Shape mismatch"),
                        ("ReLU p 1 1 data p\nInterp m 1 1 p m 0=2 3=40000 4=40000\n", "2^31")):
        net = Net(fusion=2)
        net.SetExtendedLayers(True)
        net.LoadParam((head + lines).encode())
        net.LoadWeights(b"")
        net.FeedInput("data", np.ones((2, 8, 8, 8), np.float32))
        with pytest.raises(FeatherHipError) as e:
            net.Forward()
        assert "code -100" in str(e.value) and word in str(e.value), (lines, str(e.value))


@pytest.mark.parametrize("name,size,batch,outputs", [("mobilenet_v3_small", 64, 2, ("fc2", "prob")), ("mobilenet_v3_large", 64, 2, ("fc2", "prob")),
                                                     ("fpn_resnet50", 64, 1, ("fpn_p2", "fpn_p3", "fpn_p4", "fpn_p5")),
                                                     ("deeplab_largefov_full", 65, 1, ("fc8", "fc8_interp")), ("unet_bilinear", 32, 2, ("d1",))])
def test_zoo_nets_against_the_restatement(cuda, name, size, batch, outputs):
    from feathercnn_amd import model_zoo
    model, x, blobs = _reference(name, size, batch, 33)
    for level in (0, 2):
        net = _net(model, x, level, dilated=name in model_zoo.DILATED_LAYERS, tuned=(level == 2))
        errs = {o: R.nerr(net.Extract(o), blobs[o]) for o in outputs}
        routed = sum(a == "RESAMPLE" for _, _, a in net.layers())
        print(f"{name} {size} px batch {batch}, level {level}: " + ", ".join(f"{o} {e:.2e}" for o, e in errs.items()) + f"; {routed} resample-route layers")
        assert all(net.Extract(o).shape == blobs[o].shape for o in outputs)
        assert all(e <= TOL for e in errs.values()), (name, level, errs)
        assert routed == sum(t in R.RESAMPLE_TYPES for t, *_ in R.shuffle_ref.parse_param(model[0]))
        if name == "fpn_resnet50":
            names = [nm for _, nm, _ in net.layers()]
            assert all((f"fpn_sum{k}" in names) == (level == 0) for k in (4, 3, 2))  # the top-down path: three launches at level 2


def test_a_net_without_these_layers_never_maps_the_library(cuda, tmp_path):
    """libfeather_hip.so alone in a directory: a net without the new layers runs, one with either of them fails at its first Reshape with a
    message that names the missing library; with the library in place, /proc/self/maps shows it only after a net that needs it."""
    from feathercnn_amd import _lib
    shutil.copy(_lib.lib_path(), tmp_path / "libfeather_hip.so")
    code = (
        "import numpy as np\n"
        "from feathercnn_amd import FeatherHipError\n"
        "from feathercnn_amd.net import Net\n"
        "head = '7767517\\n3 4\\nInput data 0 1 data 0=8 1=8 2=8\\n'\n"
        "mapped = lambda: 'libfeather_resample' in open('/proc/self/maps').read()\n"
        "for name, lines in (('plain', 'Pooling p 1 1 data p 0=1 1=2 2=2\\nReLU c 1 1 p c\\n'), ('interp', 'ReLU p 1 1 data p\\nInterp c 1 1 p c 0=2 1=2.0 2=2.0\\n'),\n"
        "                    ('hswish', 'ReLU p 1 1 data p\\nHardSwish c 1 1 p c\\n')):\n"
        "    net = Net(fusion=2); net.SetExtendedLayers(True); net.LoadParam((head + lines).encode()); net.LoadWeights(b'')\n"
        "    try:\n"
        "        net.FeedInput('data', np.zeros((1, 8, 8, 8), np.float32)); net.Forward(); net.Extract('c'); print(name, 'ran', 'mapped' if mapped() else 'unmapped')\n"
        "    except FeatherHipError as e:\n"
        "        print(name, 'refused:', e, 'mapped' if mapped() else 'unmapped')\n")
    for lib_dir, expect in ((tmp_path, "refused"), (None, "ran")):
        env = dict(os.environ, PYTHONPATH=ROOT)
        if lib_dir:
            env["FEATHER_HIP_LIB"] = str(tmp_path / "libfeather_hip.so")
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd=str(tmp_path), timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = {ln.split()[0]: ln for ln in r.stdout.splitlines() if ln.split() and ln.split()[0] in ("plain", "interp", "hswish")}
        assert "plain ran unmapped" in lines["plain"], r.stdout  # the switch alone opens nothing
        for name in ("interp", "hswish"):
            if expect == "refused":
                assert "refused" in lines[name] and "libfeather_resample.so" in lines[name] and "unmapped" in lines[name], r.stdout
            else:
                assert lines[name] == f"{name} ran mapped", r.stdout


def test_one_collapsed_upsample_add_relu_is_one_launch_by_kernel_trace(cuda, tmp_path):
    """Interp (nearest x2) -> Eltwise -> ReLU at fusion level 2, one Forward in a fresh child process under rocprofv3 (kernel trace only), cut
    at the two marker launches around the Forward: exactly one kernel, under the name fhip_interp_route reports."""
    text, rows, _ = ktrace.trace("resample_trace_child.py", [], tmp_path, TRACE_TIMEOUT)
    routes = [ln.split(" ", 1)[1] for ln in text.splitlines() if ln.startswith("route ")]
    assert routes == ["fhip::interp_nearest2x_kernel"], text[-3000:]
    window, = ktrace.between(rows, 2)  # the child brackets its Forward with two fhip_relu launches
    print("kernels of the collapsed upsample-add-ReLU:", window)
    assert len(window) == 1 and routes[0].replace(" ", "") in window[0].replace(" ", "").replace("void", ""), window
