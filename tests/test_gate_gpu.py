"""libfeather_gate.so (squeeze-and-excitation channel gating, Swish, HardSigmoid) on the MI355X.

* apply: bit for bit (int32 views) against numpy float32 x * g, x * g + r, max(x * g + r, 0) -- planes 1x1 .. 56x56, 1 .. 72 channels,
  batches 1 / 3 / 32, pointers 0 / 4 / 8 / 12 bytes past a 16-byte boundary, out aliasing in and residual, a gate plane of exact zeros and
  one of negative values; every tensor between guards (tests/guarded.py's canary and poison words): nothing outside an output is
  written, every output word is, no input changes;
* squeeze against the fp64 mean per plane (images scaled by 2^-6 .. 2^6), every route, two runs bit-identical; excite against fp64 for
  every (C, R) of the table, every activation, with and without biases; Swish against fp64, HardSigmoid bit for bit against numpy float32.
  The bound is the project's 1e-4 normalised; measured worst cases: DESIGN.md 3.18;
* feather::Net: tiny_se at fusion levels 0 .. 3 (sub-batches, graph) against the restatement; a collapsed block bit-identical to the
  library applied to that run's own blobs; level 0's BinaryOp / Scale tops bit-identical to the library call; Extract and Reshape
  refusals; a second input size; se_resnet50 and efficientnet_b0 at 64 px; a net without these layers never opens the library; the launches
  of one collapsed residual block by kernel trace.
Each test prints its own figures."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import gate_cases as GC
import gate_ref as R
import ktrace
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

    def values(self):
        return self.body.cpu().numpy().reshape(self.shape).copy()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _apply_shapes(h, w):
    for c in GC.APPLY_CHANNELS:
        for n in GC.APPLY_BATCHES:
            yield n, c


# ---- apply -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", GC.APPLY_PLANES)
def test_apply_bit_for_bit_between_guards(cuda, h, w):
    from feathercnn_amd import channel_gate
    from feathercnn_amd.gate import gate_route
    rng = np.random.default_rng(100 * h + w)
    launches, routes = 0, set()
    for n, c in _apply_shapes(h, w):
        x = rng.uniform(-2, 2, (n, c, h, w)).astype(np.float32)
        r = rng.uniform(-2, 2, (n, c, h, w)).astype(np.float32)
        g = rng.uniform(0.05, 1.0, (n, c)).astype(np.float32)
        g.reshape(-1)[0] = 0.0                 # a plane of exact zeros
        g.reshape(-1)[-1] = -1.5 if n * c > 1 else 0.0  # and one of negative values
        g4 = g.reshape(n, c, 1, 1)
        want = {"mul": x * g4, "add": x * g4 + r, "relu": np.maximum(x * g4 + r, np.float32(0))}
        for off in GC.OFFSETS:
            for mode in ("mul", "add", "relu"):
                xi, gi = Region(x.shape, x, off), Region(g.shape, g, (off + 1) % 4)
                ri = Region(r.shape, r, off) if mode != "mul" else None
                out = Region(x.shape, "poison", off)
                channel_gate(xi.tensor, gi.tensor, None if ri is None else ri.tensor, relu=(mode == "relu"), out=out.tensor)
                routes.add(gate_route("apply", xi.tensor, out.tensor, None if ri is None else ri.tensor))
                launches += 1
                assert out.guards_intact() and out.unwritten() == 0, (n, c, off, mode)
                assert xi.unchanged() and gi.unchanged() and (ri is None or ri.unchanged()), (n, c, off, mode)
                assert np.array_equal(out.bits(), _bits(want[mode])), (n, c, off, mode)
        # mixed alignment: only the residual is off the 16-byte boundary
        xi, gi, ri, out = Region(x.shape, x, 0), Region(g.shape, g, 0), Region(r.shape, r, 2), Region(x.shape, "poison", 0)
        channel_gate(xi.tensor, gi.tensor, ri.tensor, relu=True, out=out.tensor)
        assert gate_route("apply", xi.tensor, out.tensor, ri.tensor) == "fhip::gate_apply_kernel<false>"
        assert out.guards_intact() and out.unwritten() == 0 and np.array_equal(out.bits(), _bits(want["relu"])), (n, c)
    assert routes == ({"fhip::gate_apply_kernel<true>", "fhip::gate_apply_kernel<false>"} if (h * w) % 4 == 0 else {"fhip::gate_apply_kernel<false>"})
    print(f"apply {h}x{w}: {launches} launches bit-identical to numpy float32, routes {sorted(routes)}")


@pytest.mark.parametrize("h,w", GC.APPLY_PLANES)
def test_apply_aliasing(cuda, h, w):
    """out may be in, or residual, or (with in == residual) both."""
    from feathercnn_amd import channel_gate
    rng = np.random.default_rng(7 * h + w)
    n, c = 3, 24
    x = rng.uniform(-2, 2, (n, c, h, w)).astype(np.float32)
    r = rng.uniform(-2, 2, (n, c, h, w)).astype(np.float32)
    g = rng.uniform(-1, 1, (n, c)).astype(np.float32)
    g4 = g.reshape(n, c, 1, 1)
    for off in GC.OFFSETS:
        for relu in (False, True):
            act = (lambda y: np.maximum(y, np.float32(0))) if relu else (lambda y: y)
            gi = Region(g.shape, g, off)
            xi = Region(x.shape, x, off)  # out is in, no residual
            channel_gate(xi.tensor, gi.tensor, None, relu=relu, out=xi.tensor)
            assert xi.guards_intact() and np.array_equal(xi.bits(), _bits(act(x * g4))), ("out=in", off, relu)
            xi, ri = Region(x.shape, x, off), Region(r.shape, r, off)  # out is in, with a residual
            channel_gate(xi.tensor, gi.tensor, ri.tensor, relu=relu, out=xi.tensor)
            assert xi.guards_intact() and ri.unchanged() and np.array_equal(xi.bits(), _bits(act(x * g4 + r))), ("out=in+res", off, relu)
            xi, ri = Region(x.shape, x, off), Region(r.shape, r, off)  # out is residual
            channel_gate(xi.tensor, gi.tensor, ri.tensor, relu=relu, out=ri.tensor)
            assert ri.guards_intact() and xi.unchanged() and np.array_equal(ri.bits(), _bits(act(x * g4 + r))), ("out=res", off, relu)
            xi = Region(x.shape, x, off)  # out is in is residual
            channel_gate(xi.tensor, gi.tensor, xi.tensor, relu=relu, out=xi.tensor)
            assert xi.guards_intact() and gi.unchanged() and np.array_equal(xi.bits(), _bits(act(x * g4 + x))), ("out=in=res", off, relu)


def test_fused_apply_equals_multiply_then_fhip_add(cuda):
    """The rounding rule of the header: one call with a residual and ReLU is a multiply followed by fhip_add, bit for bit."""
    import torch
    from feathercnn_amd import channel_gate
    from feathercnn_amd.net import add
    x, r = (torch.randn((3, 24, 14, 14), device="cuda") for _ in range(2))
    g = torch.rand((3, 24), device="cuda")
    for relu in (False, True):
        assert torch.equal(channel_gate(x, g, r, relu=relu).view(torch.int32), add(channel_gate(x, g), r, relu=relu).view(torch.int32))


# ---- squeeze ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", GC.SQUEEZE_PLANES)
def test_squeeze_against_fp64(cuda, h, w):
    import torch
    from feathercnn_amd import squeeze
    from feathercnn_amd.gate import gate_route, squeeze_scratch_bytes
    rng = np.random.default_rng(h * 1000 + w)
    n, c = 13, 3
    x = (rng.uniform(-1, 1, (n, c, h, w)) + 0.5).astype(np.float32) * np.float32(2.0) ** np.arange(-6, 7, dtype=np.float32).reshape(n, 1, 1, 1)
    want = R.squeeze(x)
    worst = 0.0
    for off in (0, 1):
        xi, out = Region(x.shape, x, off), Region((n, c, 1, 1), "poison", off)
        need = squeeze_scratch_bytes(x.shape)
        assert (need > 0) == (h * w > GC.SPLIT_CHUNK)
        scratch = Region((max(need // 4, 1),), "poison", 0)
        assert gate_route("squeeze", xi.tensor) == GC.squeeze_route(h, w, off == 0)
        squeeze(xi.tensor, out=out.tensor, scratch=scratch.tensor if need else None)
        first = out.bits().copy()
        assert out.guards_intact() and out.unwritten() == 0 and xi.unchanged() and scratch.guards_intact(), (off,)
        assert not need or scratch.unwritten() == 0
        e = R.plane_nerr(out.values(), want)
        worst = max(worst, e)
        assert e <= TOL, (h, w, off, e)
        out2 = torch.empty((n, c, 1, 1), device="cuda")
        squeeze(xi.tensor, out=out2, scratch=scratch.tensor if need else None)
        assert np.array_equal(first, out2.cpu().numpy().view(np.int32))  # two runs are bit-identical
    print(f"squeeze {h}x{w} ({GC.squeeze_route(h, w)}{', split' if h * w > GC.SPLIT_CHUNK else ''}): worst per-plane error {worst:.2e}")


# ---- excite ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,r", GC.EXCITE)
def test_excite_against_fp64(cuda, c, r):
    import torch
    from feathercnn_amd import excite
    rng = np.random.default_rng(c * 7 + r)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()
    w1 = (rng.uniform(-1, 1, (r, c)) * np.sqrt(6.0 / c)).astype(np.float32)
    w2 = (rng.uniform(-1, 1, (c, r)) * np.sqrt(6.0 / r) * 4).astype(np.float32)  # wide enough for both clamps of HardSigmoid
    b1, b2 = rng.uniform(-0.5, 0.5, r).astype(np.float32), rng.uniform(-0.5, 0.5, c).astype(np.float32)
    dw1, dw2, db1, db2 = dev(w1), dev(w2), dev(b1), dev(b2)
    worst, clamps = 0.0, set()
    for n in GC.EXCITE_BATCHES:
        mean = rng.uniform(-1, 1, (n, c, 1, 1)).astype(np.float32)
        mi = Region(mean.shape, mean, n % 2)
        for mact in ("relu", "swish", None):
            for gact, alpha, beta in (("sigmoid", 0.2, 0.5), ("hard_sigmoid", 0.2, 0.5), ("hard_sigmoid", 1.0 / 6, 0.5)):
                for bias in (True, False):
                    want = R.excite(mean, w1, b1 if bias else None, w2, b2 if bias else None, mact, gact, alpha, beta)
                    out = Region((n, c, 1, 1), "poison", (n + 1) % 2)
                    excite(mi.tensor, dw1, db1 if bias else None, dw2, db2 if bias else None, mact, gact, alpha, beta, out=out.tensor)
                    assert out.guards_intact() and out.unwritten() == 0 and mi.unchanged(), (n, mact, gact, bias)
                    got = out.values()
                    e = R.nerr(got, want)
                    worst = max(worst, e)
                    assert e <= TOL, (c, r, n, mact, gact, bias, e)
                    if gact == "hard_sigmoid":
                        clamps |= {0.0} & set(got.reshape(-1).tolist()) | {1.0} & set(got.reshape(-1).tolist())
                    if (c >= 960 or r > 1024) and n == 3 and bias:  # an image's channels in one block or dealt out to several: the same bits
                        for slices in (1, 4):
                            sl = excite(mi.tensor, dw1, db1, dw2, db2, mact, gact, alpha, beta, slices=slices)
                            assert np.array_equal(sl.cpu().numpy().view(np.int32), out.bits()), slices
    assert c < 16 or clamps == {0.0, 1.0}, clamps  # the HardSigmoid cases reach both clamps
    print(f"excite C={c} R={r}: worst normalised error {worst:.2e}")


# ---- activations -----------------------------------------------------------------------------------------------------------------------
def test_activations(cuda):
    from feathercnn_amd import gate_activation
    rng = np.random.default_rng(5)
    worst = 0.0
    for shape, off in (((2, 3, 7, 7), 0), ((2, 3, 7, 7), 1), ((3, 24, 14, 14), 0), ((3, 24, 14, 14), 3), ((1, 1, 1, 1), 0)):
        # -100: exp(100) overflows float32 and Swish gives -0 where float64 gives -3.7e-42 -- invisible next to the other values
        x = np.concatenate([rng.uniform(-12, 12, int(np.prod(shape)) - 1), [-100.0 if np.prod(shape) > 1 else 0.75]]).astype(np.float32).reshape(shape)
        xi, out = Region(shape, x, off), Region(shape, "poison", off)
        gate_activation(xi.tensor, "swish", out=out.tensor)
        assert out.guards_intact() and out.unwritten() == 0 and xi.unchanged()
        e = R.nerr(out.values(), R.swish(x))
        worst = max(worst, e)
        assert e <= TOL, (shape, off, e)
        for alpha, beta in ((0.2, 0.5), (1.0 / 6, 0.5), (0.7, -0.1)):
            out = Region(shape, "poison", off)
            gate_activation(xi.tensor, "hard_sigmoid", alpha, beta, out=out.tensor)
            assert out.guards_intact() and out.unwritten() == 0 and xi.unchanged()
            assert R.nerr(out.values(), R.hard_sigmoid(x, np.float32(alpha), np.float32(beta))) <= TOL
            assert np.array_equal(out.bits(), _bits(R.hard_sigmoid(x, alpha, beta, np.float32))), (shape, off, alpha)  # bit for bit
        gate_activation(xi.tensor, "swish", out=xi.tensor)  # in place
        assert xi.guards_intact() and R.nerr(xi.values(), R.swish(x)) <= TOL
    print(f"swish: worst normalised error {worst:.2e}")


# ---- feather::Net ----------------------------------------------------------------------------------------------------------------------
_REF = {}


def _reference(name, size, batch, seed):
    from feathercnn_amd import model_zoo
    key = (name, size, batch, seed)
    if key not in _REF:
        kw = {} if name == "tiny_se" and size == 24 else {"size": size}
        model = model_zoo.MODELS[name](**kw)
        x = np.random.default_rng(seed).uniform(-1, 1, (batch, 3, size, size)).astype(np.float32)
        _REF[key] = (model, x, R.Net(model[0], model[1]).run(model[2], x, model[3], keep=True))
    return _REF[key]


def _net(model, x, level, **kw):
    from feathercnn_amd.net import Net
    net = Net(fusion=level, **kw)
    net.LoadParam(model[0])
    net.LoadWeights(model[1])
    net.FeedInput(model[2], x)
    net.Forward()
    return net


@pytest.mark.parametrize("level,kw", [(0, {}), (1, {}), (2, {}), (3, {}), (2, {"sub_batches": 2}), (2, {"graph": True}), (3, {"graph": True, "tuned": True})])
def test_tiny_se_against_the_restatement(cuda, level, kw):
    model, x, blobs = _reference("tiny_se", 24, 5, 21)
    net = _net(model, x, level, **kw)
    if kw.get("graph"):
        net.Forward()  # the replay
    worst = 0.0
    for name in ("res_relu", "b_mul", "c_mul", "d_scale", "aux", "fc", "prob"):
        e = R.nerr(net.Extract(name), blobs[name])
        worst = max(worst, e)
        assert e <= TOL, (level, kw, name, e)
    gates = sum(a == "GATE" for _, _, a in net.layers())
    assert gates == (7 if level < 2 else 5)
    print(f"tiny_se level {level} {kw}: worst normalised error {worst:.2e}, {gates} gate-route layers of {len(net.layers())}")


@pytest.mark.parametrize("level", [2, 3])
def test_collapsed_blocks_equal_the_library_on_their_own_blobs(cuda, level):
    """Block `a` (InnerProduct excite, Scale, Eltwise + ReLU), `b` (1x1 Convolution excite, Swish, BinaryOp) and `c` (no mact, HardSigmoid,
    gate first): the block's output is, bit for bit, squeeze -> excite -> channel_gate of that run's own x and shortcut with the weights of
    the file; the blobs inside refuse Extract."""
    import torch
    from feathercnn_amd import FeatherHipError, channel_gate, excite, squeeze
    model, x, _ = _reference("tiny_se", 24, 5, 21)
    w = R.Net(model[0], model[1]).w
    net = _net(model, x, level)
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32).reshape(a.shape[0], -1)).cuda()
    for xin, short, d1, d2, mact, gact, alpha, out, inner in (
            ("a_split_1", "res_split_0", "a_fc1", "a_fc2", "relu", "sigmoid", 0.2, "res_relu", ("a_gap", "a_fc1", "a_relu", "a_fc2", "a_sigmoid", "a_scale", "res")),
            ("b_split_1", None, "b_conv1", "b_conv2", "swish", "sigmoid", 0.2, "b_mul", ("b_gap", "b_conv1", "b_swish", "b_conv2", "b_sigmoid")),
            ("c_split_1", None, "c_conv1", "c_conv2", None, "hard_sigmoid", np.float32(0.166667), "c_mul", ("c_gap", "c_conv1", "c_conv2", "c_hsigmoid"))):
        xt = torch.from_numpy(net.Extract(xin)).cuda()
        gate = excite(squeeze(xt), dev(w[d1][0]), dev(w[d1][1]), dev(w[d2][0]), dev(w[d2][1]), mact, gact, float(alpha), 0.5)
        want = channel_gate(xt, gate, None if short is None else torch.from_numpy(net.Extract(short)).cuda(), relu=short is not None)
        assert np.array_equal(_bits(net.Extract(out)), want.cpu().numpy().view(np.int32)), (level, out)
        for name in inner:
            with pytest.raises(FeatherHipError, match="fused"):
                net.Extract(name)
    net.Extract("d_sigmoid")  # the block that did not collapse keeps its blobs
    assert np.array_equal(net.Extract("a_split_0"), net.Extract("a_split_1"))


def test_level_0_gate_layers_equal_the_library_call(cuda):
    import torch
    from feathercnn_amd import channel_gate, gate_activation
    model, x, _ = _reference("tiny_se", 24, 5, 21)
    net = _net(model, x, 0)
    t = lambda name: torch.from_numpy(net.Extract(name)).cuda()
    for top, xin, gate in (("a_scale", "a_split_0", "a_sigmoid"), ("b_mul", "b_split_0", "b_sigmoid"), ("c_mul", "c_split_0", "c_hsigmoid"),
                           ("d_scale", "d_split_0", "d_gate_split_0")):
        want = channel_gate(t(xin), t(gate).reshape(5, -1))
        assert np.array_equal(_bits(net.Extract(top)), want.cpu().numpy().view(np.int32)), top
    assert np.array_equal(_bits(net.Extract("conv3_swish")), gate_activation(t("conv3_scale"), "swish").cpu().numpy().view(np.int32))
    assert np.array_equal(_bits(net.Extract("c_hsigmoid")), gate_activation(t("c_conv2"), "hard_sigmoid", np.float32(0.166667), 0.5).cpu().numpy().view(np.int32))


def test_reshape_refusals_and_a_second_input_size(cuda):
    from feathercnn_amd import FeatherHipError, model_zoo
    from feathercnn_amd.net import Net
    head = "7767517\n3 4\nInput data 0 1 data 0=8 1=8 2=8\n"
    for lines, why in (("Pooling p 1 1 data p 0=1 1=2 2=2\nBinaryOp m 2 1 data p m 0=2\n", "a 4 x 4 second operand"),
                       ("Convolution p 1 1 data p 0=4 1=8 5=0 6=2048\nBinaryOp m 2 1 data p m 0=2\n", "a gate of 4 channels for 8"),
                       ("Pooling p 1 1 data p 0=1 4=1\nScale m 2 1 p data m 0=-233\n", "Scale with the gate first"),
                       ("ReLU p 1 1 data p\nBinaryOp m 2 1 data p m 0=2\n", "two full tensors")):
        net = Net(fusion=2)
        net.LoadParam((head + lines).encode())
        net.LoadWeights(np.zeros(2048 + 1, np.float32).tobytes() if "Convolution" in lines else b"")
        net.FeedInput("data", np.ones((2, 8, 8, 8), np.float32))
        with pytest.raises(FeatherHipError) as e:
            net.Forward()
        assert "code -100" in str(e.value) and "channel gate" in str(e.value), (why, str(e.value))
    for level in (0, 2):
        model = model_zoo.tiny_se()
        net = None
        for size, seed in ((24, 1), (32, 2), (24, 3)):
            x = np.random.default_rng(seed).uniform(-1, 1, (3, 3, size, size)).astype(np.float32)
            if net is None:
                net = _net(model, x, level)
            else:
                net.FeedInput(model[2], x)
                net.Forward()
            want = R.Net(model[0], model[1]).run(model[2], x, model[3], keep=True)
            for name in ("c_mul", "prob"):
                assert net.Extract(name).shape == want[name].shape and R.nerr(net.Extract(name), want[name]) <= TOL, (level, size, name)


def test_a_block_whose_hidden_width_outweighs_its_plane_runs_its_own_layers(cuda):
    """2 R > HW (here R = 8 on a 3 x 3 plane): the collapsed layer is still one Pooling layer on the GATE route whose inner blobs refuse
    Extract, but it runs the block's layers as written, so its output equals fusion level 0 bit for bit; on a 6 x 6 plane the same block
    runs its three kernels.  Both against the restatement."""
    from feathercnn_amd import FeatherHipError, model_zoo
    g = model_zoo.GraphBuilder(3)
    x = g.relu("relu0", g.conv("conv0", g.input("data", 3, 3, 3), 3, 16, 1))
    short, y = g.split("split", x)
    g.relu("out", g.eltwise("sum", short, g.se_block("se", y, 16, 8, "caffe")))
    param, weights = g.finish()
    model = (param, weights, "data", "out")
    for size in (3, 6):
        xin = np.random.default_rng(size).uniform(-1, 1, (5, 3, size, size)).astype(np.float32)
        want = R.Net(param, weights).run("data", xin, "out", keep=True)["out"]
        lv0, lv2 = _net(model, xin, 0), _net(model, xin, 2)
        assert [(t, a) for t, n, a in lv2.layers() if n == "se_gap"] == [("Pooling", "GATE")] and len(lv2.layers()) < len(lv0.layers()) - 6
        assert R.nerr(lv2.Extract("out"), want) <= TOL and R.nerr(lv0.Extract("out"), want) <= TOL
        if size == 3:
            assert np.array_equal(_bits(lv2.Extract("out")), _bits(lv0.Extract("out")))
        with pytest.raises(FeatherHipError, match="fused"):
            lv2.Extract("se_sigmoid")


@pytest.mark.parametrize("name,logits", [("se_resnet50", "fc1000"), ("efficientnet_b0", "fc")])
def test_large_nets_against_the_restatement(cuda, name, logits):
    model, x, blobs = _reference(name, 64, 2, 33)
    for level in (0, 2):
        net = _net(model, x, level, tuned=(level == 2))
        e, ep = R.nerr(net.Extract(logits), blobs[logits]), R.nerr(net.Extract("prob"), blobs["prob"])
        gates = sum(a == "GATE" and t == "Pooling" for t, _, a in net.layers())
        print(f"{name} 64 px batch 2, level {level}: logits {e:.2e}, prob {ep:.2e}; {gates} collapsed blocks")
        assert e <= TOL and ep <= TOL, (name, level, e, ep)
        assert gates == (0 if level == 0 else 16)


def test_a_net_without_these_layers_never_opens_the_library(cuda, tmp_path):
    """libfeather_hip.so alone in a directory: a net without the new layers runs, one with any of them fails at its first Reshape with a
    message that names the missing library; with the library in place, /proc/self/maps shows it only after a net that needs it."""
    from feathercnn_amd import _lib
    shutil.copy(_lib.lib_path(), tmp_path / "libfeather_hip.so")
    code = (
        "import numpy as np\n"
        "from feathercnn_amd import FeatherHipError\n"
        "from feathercnn_amd.net import Net\n"
        "head = '7767517\\n3 4\\nInput data 0 1 data 0=8 1=8 2=8\\n'\n"
        "mapped = lambda: 'libfeather_gate' in open('/proc/self/maps').read()\n"
        "for name, lines in (('plain', 'Pooling p 1 1 data p 0=1 4=1\\nReLU c 1 1 p c\\n'), ('mul', 'Pooling p 1 1 data p 0=1 4=1\\nBinaryOp c 2 1 data p c 0=2\\n'),\n"
        "                    ('scale', 'Pooling p 1 1 data p 0=1 4=1\\nScale c 2 1 data p c 0=-233\\n'), ('swish', 'ReLU p 1 1 data p\\nSwish c 1 1 p c\\n'),\n"
        "                    ('hsig', 'ReLU p 1 1 data p\\nHardSigmoid c 1 1 p c\\n')):\n"
        "    net = Net(fusion=2); net.LoadParam((head + lines).encode()); net.LoadWeights(b'')\n"
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
        lines = {ln.split()[0]: ln for ln in r.stdout.splitlines() if ln.split() and ln.split()[0] in ("plain", "mul", "scale", "swish", "hsig")}
        assert "plain ran unmapped" in lines["plain"], r.stdout
        for name in ("mul", "scale", "swish", "hsig"):
            if expect == "refused":
                assert "refused" in lines[name] and "libfeather_gate.so" in lines[name] and "unmapped" in lines[name], r.stdout
            else:
                assert lines[name] == f"{name} ran mapped", r.stdout


def test_one_collapsed_residual_block_is_three_launches_by_kernel_trace(cuda, tmp_path):
    """One residual SE block (Caffe spelling, 64 channels on 14 x 14, Eltwise + ReLU) at fusion level 2, one Forward in a fresh child process
    under rocprofv3 (kernel trace only), cut at the two marker launches around the Forward: squeeze, excite and apply, under the names
    fhip_gate_route reports, and nothing else."""
    text, rows, _ = ktrace.trace("gate_trace_child.py", [], tmp_path, TRACE_TIMEOUT)
    routes = [ln.split(" ", 1)[1] for ln in text.splitlines() if ln.startswith("route ")]
    assert len(routes) == 3, text[-3000:]
    window, = ktrace.between(rows, 2)  # the child brackets its Forward with two fhip_relu launches
    print("kernels of the collapsed block:", window)
    assert len(window) <= 3 and len(window) == len(routes), window
    for got, want in zip(window, routes):
        assert want.replace(" ", "") in got.replace(" ", "").replace("void", ""), (got, want)
