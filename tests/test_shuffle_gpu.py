"""libfeather_shuffle.so (ShuffleChannel, Slice and the channel map) on the MI355X.

The kernels only copy, so every comparison of a layer is bit for bit (int32 views), against tests/shuffle_ref.py:
* the sweep: planes 1x1 .. 56x56, channel counts that are and are not multiples of 4, groups 2 / 3 / 4 / 8, reverse, batches 1 / 3 / 32,
  pointers 0 / 4 / 8 / 12 bytes past a 16-byte boundary, unequal slices, a table reading three sources -- every tensor between guards
  (tests/guarded.py's canary and poison words): nothing outside an output is written, every output word is, no input changes;
* feather::Net: the shapes after Reshape, refusals at Reshape; fusion levels 0 / 1 against 2 / 3 bit for bit on a net that only copies,
  and on tiny_shuffle / shufflenet_v2_x1_0 every map blob still extractable bit-identical to the map of that run's own inputs (the
  convolutions between them round differently from level to level); collapsed blobs refuse Extract; the launch counts of one ShuffleNet v2
  unit boundary by kernel trace; whole nets against the restatement within the project's 1e-4 (measured worst case 5.3e-7, on the logits
  of shufflenet_v2_x1_0); a net without these layers never opens the library.
Each test prints its own figures."""
import ctypes
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import ktrace
import shuffle_cases as SC
import shuffle_ref as R
import side_contract
from guarded import CANARY, POISON

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-4
GUARD = 1 << 16  # floats on each side
TRACE_TIMEOUT = 240


class Region:
    """[guard | body | guard] in one allocation, the body `offset` floats (0 .. 3) past a 16-byte boundary: tests/guarded.py's layout with
    the two further offsets this library's alignment rule distinguishes."""

    def __init__(self, shape, fill, offset=0):
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
        self.ptr = self.raw.data_ptr() + 4 * self.lo
        self.tensor = self.body.view(self.shape)

    def guards_intact(self):
        return bool((self.raw[:self.lo] == CANARY).all()) and bool((self.raw[self.lo + self.n:] == CANARY).all())

    def unwritten(self):
        return int((self.raw[self.lo:self.lo + self.n] == POISON).sum())

    def bits(self):
        return self.raw[self.lo:self.lo + self.n].cpu().numpy().reshape(self.shape)


lib = side_contract.fixture("shuffle", gpu=True)


_stream = side_contract.stream


def _values(rng, shape):
    """Distinct bit patterns incl. -0.0, a subnormal, Inf and a NaN payload: a copy must keep every one."""
    x = rng.normal(0, 1, shape).astype(np.float32)
    f = x.reshape(-1)
    special = np.array([0x80000000, 0x00000001, 0x7F800000, 0x7FC12345], np.uint32).view(np.float32)
    f[:min(4, f.size)] = special[:min(4, f.size)]
    return x


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.int32), np.ascontiguousarray(b, np.float32).view(np.int32))


def _check_regions(what, ins, outs, snaps):
    import torch
    torch.cuda.synchronize()
    for r in ins + outs:
        assert r.guards_intact(), f"{what}: a guard word changed"
    for r in outs:
        assert r.unwritten() == 0, f"{what}: {r.unwritten()} output words were not written"
    for r, s in zip(ins, snaps):
        assert torch.equal(r.raw, s), f"{what}: an input changed"


@pytest.mark.parametrize("plane", SC.PLANES, ids=[f"{h}x{w}" for h, w in SC.PLANES])
def test_shuffle_sweep_between_guards(lib, plane):
    from feathercnn_amd.shuffle import channel_route
    h, w = plane
    rng = np.random.default_rng(100 + h * w)
    seen, count = set(), 0
    for ci, (c, group) in enumerate(SC.SHUFFLES):
        for bi, n in enumerate(SC.BATCHES):
            if n == 32 and h * w > 196 and ci % 3:  # the large planes at batch 32: every third channel count
                continue
            for reverse in (0, 1):
                off_in, off_out = SC.OFFSETS[(ci + bi + reverse) % 4], SC.OFFSETS[(ci + 2 * bi) % 4] if (ci + bi) % 2 else 0
                x = _values(rng, (n, c, h, w))
                gx, gy = Region(x.shape, x, off_in), Region(x.shape, "poison", off_out)
                snap = [gx.raw.clone()]
                rc = lib.fhip_channel_shuffle_forward(ctypes.c_void_p(gy.ptr), ctypes.c_void_p(gx.ptr), n, c, h, w, group, reverse, _stream())
                assert rc == 0, lib.fhip_shuffle_last_error()
                what = f"shuffle {n}x{c}x{h}x{w} group {group} reverse {reverse} offsets {off_in}/{off_out}"
                _check_regions(what, [gx], [gy], snap)
                assert _same(gy.bits().view(np.float32), R.channel_shuffle(x, group, bool(reverse))), what
                route = channel_route("shuffle", h, w, [gy.tensor, gx.tensor])
                assert route == SC.instance(1, h, w, [off_in, off_out]), what
                seen.add(route)
                count += 1
    print(f"shuffle sweep {h}x{w}: {count} cases bit-identical between guards; instantiations {sorted(seen)}")
    assert any("true" in s for s in seen) == ((h * w) % 4 == 0)


@pytest.mark.parametrize("plane", SC.PLANES, ids=[f"{h}x{w}" for h, w in SC.PLANES])
def test_slice_and_map_sweep_between_guards(lib, plane):
    from feathercnn_amd.shuffle import ChannelMap
    h, w = plane
    rng = np.random.default_rng(200 + h * w)
    count = 0
    for si, (c, sizes) in enumerate(SC.SLICES):
        for bi, n in enumerate(SC.BATCHES):
            resolved = R.slice_sizes(c, sizes)
            x = _values(rng, (n, c, h, w))
            gx = Region(x.shape, x, SC.OFFSETS[(si + bi) % 4])
            outs = [Region((n, s, h, w), "poison", SC.OFFSETS[(si + j) % 4] if bi else 0) for j, s in enumerate(resolved)]
            snap = [gx.raw.clone()]
            rc = lib.fhip_channel_slice_forward((ctypes.c_void_p * len(outs))(*[o.ptr for o in outs]), ctypes.c_void_p(gx.ptr), n, c, h, w,
                                                (ctypes.c_int * len(sizes))(*sizes), len(sizes), _stream())
            assert rc == 0, lib.fhip_shuffle_last_error()
            what = f"slice {n}x{c}x{h}x{w} sizes {sizes}"
            _check_regions(what, [gx], outs, snap)
            for o, want in zip(outs, R.channel_slice(x, sizes)):
                assert _same(o.bits().view(np.float32), want), what
            count += 1
    # tables: three sources into three outputs, and ShuffleNet v2's unit boundary (two sources, two outputs), both access widths forced
    for src_c, steps, outputs in (SC.THREE_SOURCES, SC.V2_BOUNDARY(58), SC.V2_BOUNDARY(3)):
        tables = R.compose(src_c, steps, outputs)
        m = ChannelMap(src_c, tables)
        for bi, n in enumerate(SC.BATCHES):
            for offs in ((0,) * 6, (1, 0, 2, 3, 0, 1)) if bi != 1 else ((2, 2, 2, 2, 2, 2),):
                xs = [_values(rng, (n, c, h, w)) for c in src_c]
                srcs = [Region(x.shape, x, offs[i]) for i, x in enumerate(xs)]
                outs = [Region((n, len(t), h, w), "poison", offs[3 + j]) for j, t in enumerate(tables)]
                snaps = [s.raw.clone() for s in srcs]
                routes = [None] + (["4b", "16b"] if SC.vec(h, w, offs) else ["4b"])
                for route in routes:
                    for o in outs:
                        o.raw[o.lo:o.lo + o.n] = POISON
                    m.forward([s.tensor for s in srcs], [o.tensor for o in outs], route)
                    what = f"map {len(src_c)} sources {n}x{src_c}x{h}x{w} offsets {offs} route {route}"
                    _check_regions(what, srcs, outs, snaps)
                    for o, want in zip(outs, R.apply_map(xs, tables)):
                        assert _same(o.bits().view(np.float32), want), what
                    count += 1
                if not SC.vec(h, w, offs):
                    from feathercnn_amd import FeatherHipError
                    with pytest.raises(FeatherHipError, match="16-byte"):
                        m.forward([s.tensor for s in srcs], [o.tensor for o in outs], "16b")
        m.close()
    print(f"slice / map sweep {h}x{w}: {count} cases bit-identical between guards")


def test_python_mirror_and_graph_capture(cuda):
    import torch
    from feathercnn_amd import channel_map, channel_shuffle, channel_slice
    from feathercnn_amd.shuffle import ChannelMap, channel_route
    rng = np.random.default_rng(5)
    x = torch.from_numpy(rng.normal(0, 1, (3, 24, 7, 7)).astype(np.float32)).cuda()
    assert _same(channel_shuffle(x, 4).cpu().numpy(), R.channel_shuffle(x.cpu().numpy(), 4))
    assert torch.equal(channel_shuffle(channel_shuffle(x, 4), 4, reverse=True), x)
    for got, want in zip(channel_slice(x, [5, -233, 9]), torch.split(x[:, :23], [5, 9, 9], dim=1)):  # the share is (24 - 5) // 2 = 9
        assert torch.equal(got, want)
    a, b = x[:, :12].contiguous(), x[:, 12:].contiguous()
    tables = R.compose(*SC.V2_BOUNDARY(12))
    keep, work = channel_map([a, b], tables)
    sh = channel_shuffle(torch.cat([a, b], 1), 2)
    assert torch.equal(keep, sh[:, :12]) and torch.equal(work, sh[:, 12:])
    assert channel_route("map", 7, 7, [a, b]) == "fhip::channel_map_kernel<0, false>" and channel_route("shuffle", 14, 14, [a]) == "fhip::channel_map_kernel<1, true>"
    # captured into a graph and replayed: Forward allocates nothing
    m = ChannelMap([12, 12], tables)
    outs = [torch.full_like(a, float("nan")), torch.full_like(a, float("nan"))]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            m.forward([a, b], outs)
    assert torch.isnan(outs[0]).all()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(outs[0], keep) and torch.equal(outs[1], work)
    m.close()


# ---- feather::Net --------------------------------------------------------------------------------------------------------------------
def _run(model, x, blobs=None, **kw):
    from feathercnn_amd.net import Net
    p, b, i, o = model
    net = Net(**kw)
    net.LoadParam(p)
    net.LoadWeights(b)
    net.FeedInput(i, x)
    net.Forward()
    out = {name: net.Extract(name) for name in (blobs or [o])}
    if kw.get("graph"):
        net.FeedInput(i, x)
        net.Forward()
        assert all(_same(net.Extract(name), y) for name, y in out.items())
    layers = net.layers()
    net.close()
    return out, layers


def _one(lines, c=8, hw=8):
    body = "\n".join(lines)
    tops = sum(int(ln.split()[3]) for ln in lines)
    return f"7767517\n{1 + len(lines)} {1 + tops}\nInput data 0 1 data 0={hw} 1={hw} 2={c}\n{body}\n".encode()


def test_shapes_after_reshape(cuda):
    x = np.random.default_rng(6).normal(0, 1, (3, 32, 7, 7)).astype(np.float32)
    param = _one(["ShuffleChannel s 1 1 data s 0=4", "Slice three 1 3 s a b c -23300=3,5,-233,14", "Slice two 1 2 a d e -23300=2,-233,-233",
                  "Slice part 1 2 c f g -23300=2,3,4", "ShuffleChannel r 1 1 b r 0=13 1=1"], c=32, hw=7)
    s = R.channel_shuffle(x, 4)
    a, b, c = R.channel_slice(s, [5, -233, 14])
    want = dict(zip("sabcdefg", [s, a, b, c] + R.channel_slice(a, [-233, -233]) + R.channel_slice(c, [3, 4])), r=R.channel_shuffle(b, 13, True))
    assert [want[k].shape[1] for k in "abcdefg"] == [5, 13, 14, 2, 3, 3, 4]  # -233 shares of 32 and of 5, and a slice that drops the rest
    for level in (0, 2):
        # level 2: s -> three -> two is the longest prefix of the run that fits one map (its tops are b, c, d, e); s and a are collapsed
        left = [k for k in "sabcdefgr" if level == 0 or k not in "sa"]
        out, layers = _run((param, b"", "data", "s"), x, blobs=left, fusion=level)
        for k in left:
            assert out[k].shape == want[k].shape and _same(out[k], want[k]), (level, k)
        print(f"shapes after Reshape, fusion {level}: {layers}")
        assert all(r == "SHUFFLE" for _, _, r in layers[1:])
        assert [nm for _, nm, _ in layers] == (["data", "s", "three", "two", "part", "r"] if level == 0 else ["data", "s", "part", "r"])


@pytest.mark.parametrize("lines,code,word", [(["ShuffleChannel s 1 1 data s 0=3"], -100, "divide"), (["Slice s 1 2 data a b -23300=2,5,4"], -100, "more than"),
                                             (["Slice s 1 2 data a b -23300=2,8,-233"], -100, "without a channel"),
                                             (["Slice s 1 2 data a b -23300=2,4,4", "ShuffleChannel r 1 1 a r 0=3"], -100, "divide")])
def test_reshape_refuses_with_the_documented_codes(cuda, lines, code, word):
    from feathercnn_amd import FeatherHipError
    from feathercnn_amd.net import Net
    for level in (0, 2):
        net = Net(fusion=level)
        net.LoadParam(_one(lines))
        net.LoadWeights(b"")
        with pytest.raises(FeatherHipError) as e:
            net.FeedInput("data", np.zeros((1, 8, 8, 8), np.float32))
            net.Forward()
        assert f"code {code}" in str(e.value) and word in str(e.value), str(e.value)
        net.close()


COLLAPSED = {"tiny_shuffle": ["u1_concat", "u1_shuffle", "u2_concat", "u2_shuffle", "cat3", "u3_concat"]}


@pytest.mark.parametrize("name,batch", [("tiny_shuffle", 3), ("shufflenet_v2_x1_0", 2)])
def test_every_map_blob_is_an_exact_copy_at_every_fusion_level(cuda, name, batch):
    """Other fusions (BatchNorm folded into a convolution, a depthwise + pointwise pair in one kernel) change the rounding of the
    convolution outputs between levels, so blobs are not compared ACROSS levels bit for bit here (the test below does that on a net that
    only copies).  Within each level every Concat / ShuffleChannel / Slice top that can still be extracted must be, bit for bit, the
    restatement applied to that run's own extractable inputs -- through the collapsed blobs, which refuse Extract with the level message."""
    from feathercnn_amd import FeatherHipError, model_zoo
    from feathercnn_amd.net import Net
    model = model_zoo.MODELS[name]()
    size = 28 if name == "tiny_shuffle" else 224
    x = np.random.default_rng(7).uniform(-1, 1, (batch, 3, size, size)).astype(np.float32)
    layers = R.parse_param(model[0])
    kinds = R.MAP_TYPES + ("Concat",)
    moved = [t for ty, _, _, tops, _ in layers if ty in kinds for t in tops]
    base = None
    for level, kw in ((0, {}), (1, {}), (2, {}), (3, {"tuned": True}), (2, {"graph": True}), (2, {"sub_batches": 2})):
        net = Net(fusion=level, **kw)
        net.LoadParam(model[0])
        net.LoadWeights(model[1])
        net.FeedInput(model[2], x)
        net.Forward()
        gone, val, checked = [], {}, 0
        for k in moved:
            try:
                val[k] = net.Extract(k)
            except FeatherHipError as e:
                assert "disable fusion to extract it" in str(e), str(e)
                gone.append(k)

        def get(blob):
            if blob not in val:
                try:
                    val[blob] = net.Extract(blob)
                except FeatherHipError:
                    val[blob] = None  # absorbed by another fusion
            return val[blob]
        for ty, nm, bottoms, tops, pd in layers:
            if ty not in kinds:
                continue
            ins = [get(b) for b in bottoms]
            if any(v is None for v in ins):
                continue
            if ty == "Concat":
                want = [np.concatenate(ins, axis=1)]
            elif ty == "ShuffleChannel":
                want = [R.channel_shuffle(ins[0], pd.get(0, 1), bool(pd.get(1, 0)))]
            else:
                want = R.channel_slice(ins[0], pd[-23300])
            for t, wv in zip(tops, want):
                if t in gone:
                    val[t] = wv  # feeds the next step of the collapsed run
                else:
                    assert _same(val[t], wv), (level, kw, nm, t)
                    checked += 1
        out = net.Extract(model[3])
        base = out if base is None else base
        e = R.nerr(out, base)
        got = net.layers()
        print(f"{name} fusion {level} {kw}: {len(got)} layers, {sum(r == 'SHUFFLE' for _, _, r in got)} channel-map launches, {len(gone)} collapsed blobs, "
              f"{checked} map blobs bit-identical to their inputs, output vs fusion 0 {e:.2e}")
        assert e <= TOL and checked >= (len(moved) - len(gone)) // 2
        if level < 2:
            assert not gone and checked == len(moved)
        elif name in COLLAPSED:
            assert gone == COLLAPSED[name], gone
        else:  # 13 Concat -> ShuffleChannel -> Slice runs lose two blobs each, the 3 Concat -> ShuffleChannel runs before a stride-2 unit / conv5 one
            assert len(gone) == 2 * 13 + 3, gone
        net.close()


def test_collapsed_run_equals_the_three_layers_bit_for_bit(cuda):
    """Two Input blobs -> Concat -> ShuffleChannel(2) -> Slice(2): nothing but copies, so fusion 0 / 1 against 2 / 3 is bit-identical on the
    blobs that are left, and the collapsed ones refuse Extract."""
    from feathercnn_amd import FeatherHipError
    from feathercnn_amd.net import Net
    rng = np.random.default_rng(8)
    for c, hw in ((58, 28), (116, 14), (232, 7), (3, 5)):
        param = (f"7767517\n5 6\nInput a 0 1 a 0={hw} 1={hw} 2={c}\nInput b 0 1 b 0={hw} 1={hw} 2={c}\nConcat cat 2 1 a b cat 0=0\n"
                 "ShuffleChannel sh 1 1 cat sh 0=2\nSlice sl 1 2 sh keep work -23300=2,-233,-233\n").encode()
        a, b = _values(rng, (3, c, hw, hw)), _values(rng, (3, c, hw, hw))
        got = {}
        for level in (0, 1, 2, 3):
            net = Net(fusion=level)
            net.LoadParam(param)
            net.LoadWeights(b"")
            net.FeedInput("a", a)
            net.FeedInput("b", b)
            net.Forward()
            got[level] = (net.Extract("keep"), net.Extract("work"))
            if level >= 2:
                assert [(t, nm, r) for t, nm, r in net.layers()][2:] == [("Concat", "cat", "SHUFFLE")]
                for blob in ("cat", "sh"):
                    with pytest.raises(FeatherHipError, match="disable fusion to extract it"):
                        net.Extract(blob)
            else:
                assert _same(net.Extract("sh"), R.channel_shuffle(np.concatenate([a, b], 1), 2))
            net.close()
        keep, work = R.channel_slice(R.channel_shuffle(np.concatenate([a, b], 1), 2), [-233, -233])
        for level in (0, 1, 2, 3):
            assert _same(got[level][0], keep) and _same(got[level][1], work), (c, hw, level)


def _trace(tmp_path, level):
    _, rows, copies = ktrace.trace("shuffle_trace_child.py", [level], tmp_path, TRACE_TIMEOUT, copies=True)
    (kernels,), (copied,) = ktrace.between(rows, 2, copies)  # the child brackets its Forward with two fhip_relu launches
    return kernels, copied


def test_launch_counts_of_one_v2_unit_by_kernel_trace(cuda, tmp_path):
    """Concat -> ShuffleChannel -> Slice between two Input blobs, one Forward in a fresh child process under rocprofv3 (kernel and memory-copy
    trace, no counters), cut at the two marker launches around the Forward: fusion 0 is Concat's two copies (copy-engine transfers or the
    runtime's copy kernels, whichever it chose) plus two channel-map kernels, fusion 2 exactly one channel-map kernel."""
    k0, c0 = _trace(tmp_path, 0)
    k2, c2 = _trace(tmp_path, 2)
    maps0, maps2 = [k for k in k0 if "channel_map_kernel" in k], [k for k in k2 if "channel_map_kernel" in k]
    other0, other2 = [k for k in k0 if "channel_map_kernel" not in k], [k for k in k2 if "channel_map_kernel" not in k]
    print(f"fusion 0: {len(maps0)} channel-map kernels, {c0} device-to-device copies, other kernels {other0}")
    print(f"fusion 2: {len(maps2)} channel-map kernels, {c2} device-to-device copies, other kernels {other2}")
    assert len(maps0) == 2 and c0 + len(other0) == 2  # a copy is a copy-engine transfer or a copy kernel of the runtime
    assert len(maps2) == 1 and c2 + len(other2) == 0
    assert "<0," in maps2[0].replace(" ", "")


@pytest.mark.parametrize("name", ["tiny_shuffle", "shufflenet_v2_x1_0", "shufflenet_v1_g3"])
def test_whole_nets_against_the_restatement(cuda, name):
    from feathercnn_amd import model_zoo
    model = model_zoo.MODELS[name]()
    size = 28 if name == "tiny_shuffle" else 224
    ref = R.Net(model[0], model[1])
    worst = 0.0
    for batch in (1, 4):
        x = np.random.default_rng(9 + batch).uniform(-1, 1, (batch, 3, size, size)).astype(np.float32)
        blobs = ref.run(model[2], x, model[3], keep=True)
        assert np.isfinite(blobs["fc"]).all()
        for kw in ({"fusion": 0}, {"fusion": 2}, {"fusion": 3, "tuned": True, "graph": True}):
            out, layers = _run(model, x, blobs=[model[3], "fc"], **kw)
            # the softmax of a deep net with random weights can saturate, where it would hide an error: the logits are compared as well
            e, ef = R.nerr(out[model[3]], blobs[model[3]]), R.nerr(out["fc"], blobs["fc"])
            worst = max(worst, e, ef)
            print(f"{name} b{batch} {kw}: {len(layers)} layers, {sum(r == 'SHUFFLE' for _, _, r in layers)} channel-map launches, normalised error "
                  f"{e:.2e} (prob), {ef:.2e} (logits, peak {np.abs(blobs['fc']).max():.3g})")
            assert e <= TOL and ef <= TOL, (name, batch, kw, e, ef)
    print(f"{name}: worst normalised error vs the fp64 restatement {worst:.2e}")


def test_a_net_without_these_layers_never_opens_the_library(cuda, tmp_path):
    """libfeather_hip.so alone in a directory: a net without ShuffleChannel / Slice runs (Concat included), one with either fails at its first
    Reshape with FHIP_E_UNSUPPORTED and a message that names the missing library; with the library in place, /proc/self/maps shows it only
    after a net that needs it."""
    from feathercnn_amd import _lib
    shutil.copy(_lib.lib_path(), tmp_path / "libfeather_hip.so")
    code = (
        "import numpy as np\n"
        "from feathercnn_amd import FeatherHipError\n"
        "from feathercnn_amd.net import Net\n"
        "head = '7767517\\n3 4\\nInput data 0 1 data 0=8 1=8 2=8\\n'\n"
        "mapped = lambda: 'libfeather_shuffle' in open('/proc/self/maps').read()\n"
        "for name, lines in (('plain', 'ReLU r 1 1 data r\\nConcat c 2 1 data r c 0=0\\n'), ('shuffle', 'ReLU r 1 1 data r\\nShuffleChannel c 1 1 r c 0=2\\n'),\n"
        "                    ('slice', 'ReLU r 1 1 data r\\nSlice c 1 2 r c d -23300=2,4,4\\n')):\n"
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
        lines = {ln.split()[0]: ln for ln in r.stdout.splitlines() if ln.split() and ln.split()[0] in ("plain", "shuffle", "slice")}
        assert "plain ran unmapped" in lines["plain"], r.stdout
        for name in ("shuffle", "slice"):
            if expect == "refused":
                assert "refused" in lines[name] and "libfeather_shuffle.so" in lines[name] and "code -1" in lines[name] and "unmapped" in lines[name], r.stdout
            else:
                assert lines[name] == f"{name} ran mapped", r.stdout
