"""libfeather_lrn.so (LRN, alone and with the Pooling layer behind it) on the MI355X.

* LRN: every row of tests/lrn_cases.py between guards (tests/guarded.py's canary and poison words): nothing outside the output is written,
  every output word is, the input does not change; element-wise within T = E_REF + 16 ulp of the float64 restatement (tests/lrn_cases.py
  derives T) and within the project's 1e-4 per plane; the rows of the 16-byte path again with both tensors one float off the boundary, and
  every across-channel row unsplit, in chunks of 16 channels and in chunks of 5: identical bits; two runs give the same bits;
* LRN -> Pooling in one launch: bit for bit fhip_pooling(fhip_lrn_forward(x)) on every row of POOL_ROWS, and within tolerance of the
  float64 restatement;
* fhip_lrn_route / fhip_lrn_pool_route name every instantiation the library's code object holds, and the tables reach every one;
* graph capture replays the eager result; out overlapping in is refused;
* feather::Net: tiny_lrn at fusion levels 0 .. 3, with sub-batches, the graph and concurrency, against lrn_ref.Net at the project's 1e-4
  normalised, levels >= 2 within 1e-5 of level 0, and the blobs on both sides of a fused LRN -> Pooling at level 2 bit-identical to level
  1's; a fused layer above the size up to which one launch pays runs the two kernels through the scratch arena, same bits; alexnet, caffenet
  and googlenet at batch 4 at their smallest inputs; one launch per fused LRN -> Pooling and one
  per plain LRN by kernel trace.
Each test prints its own figures."""
import os

import numpy as np
import pytest

import kernel_instances as KI
import ktrace
import lrn_cases as LC
import lrn_ref as R
from guarded import CANARY, POISON

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "feathercnn_amd", "libfeather_lrn.so")
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


def _kw(r):
    return dict(local_size=r.local_size, alpha=r.alpha, beta=r.beta, bias=r.bias, region=r.region)


def _want64(r, x):
    return R.lrn(x, r.local_size, r.alpha, r.beta, r.bias, r.region, np.float64)


def _run(r, x, offset=0, chunk=None):
    """One guarded launch -> (the output's bits, the route)."""
    from feathercnn_amd import lrn, lrn_route
    xi, out = Region(x.shape, x, offset), Region(x.shape, "poison", offset)
    lrn(xi.tensor, out=out.tensor, chunk=chunk, **_kw(r))
    route = lrn_route(xi.tensor, r.local_size, r.region, out=out.tensor)
    assert out.guards_intact() and out.unwritten() == 0, (r.id, offset, chunk, route)
    assert xi.unchanged(), (r.id, offset, chunk)
    return out.bits(), route


def _held(ls):
    return ls if ls in (3, 5) else 0


GROUPS = [(f"across ls={ls}", [r for r in LC.ACROSS_ROWS if r.local_size == ls]) for ls in LC.SIZES] + [("published", [LC.PUBLISHED]), ("within", LC.WITHIN_ROWS)]


# ---- LRN -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [g[1] for g in GROUPS], ids=[g[0] for g in GROUPS])
def test_lrn_against_float64_between_guards(cuda, rows):
    worst, worst_plane, launches, at = 0.0, 0.0, 0, None
    for r in rows:
        x = LC.make_input(r)
        want = _want64(r, x)
        bits, route = _run(r, x)
        vec = r.region == 0 and r.h * r.w % 4 == 0
        assert route == (f"fhip::lrn_across_kernel<{4 if vec else 1}, {_held(r.local_size)}>" if r.region == 0 else "fhip::lrn_within_kernel"), (r.id, route)
        y = bits.view(np.float32)
        err = np.abs(y.astype(np.float64) - want) / np.abs(want)
        e, ep = float(err.max()), float(R.plane_nerr(y, want))
        if e > worst:
            worst, at = e, r.id
        worst_plane = max(worst_plane, ep)
        print(f"{r.id}: {route}: worst element-wise relative error {e:.3e} = {e / LC.T:.3f} T, per plane {ep:.2e}")
        assert e <= LC.T, (r.id, route, e, LC.T)
        assert ep <= TOL, (r.id, ep)
        launches += 1
        variants = [(0, None)]  # (offset, chunk) whose bits must equal the first launch's
        if vec:
            variants.append((1, None))  # the 4-byte path on the same data
        if r.region == 0:
            variants += [(0, 0), (0, 5)] + [(0, k) for k in LC.CHUNKS] + ([(1, LC.CHUNK)] if vec else [])  # unsplit, an odd chunk, the library's
        for off, chunk in variants:
            again, route2 = _run(r, x, off, chunk)
            if off:
                assert route2 == f"fhip::lrn_across_kernel<1, {_held(r.local_size)}>", (r.id, route2)
            assert np.array_equal(again, bits), (r.id, off, chunk, route2)
            launches += 1
    print(f"{len(rows)} rows, {launches} launches: worst element-wise error {worst:.3e} = {worst / LC.T:.3f} T at {at!r}; worst per plane {worst_plane:.2e}")


def _pool_dict(p):
    return {"kernel": p.kernel, "stride": p.stride, "pad": (p.pad,) * 4, "pooling_type": int(p.avg)}


@pytest.mark.parametrize("p", LC.POOL_ROWS, ids=[p.id for p in LC.POOL_ROWS])
def test_lrn_pool_equals_the_two_launches_bit_for_bit(cuda, p):
    from feathercnn_amd import lrn, lrn_pool, lrn_pool_route
    from feathercnn_amd.net import pool_param, pooling
    r = p.lrn
    x = LC.make_input(r)
    oh, ow = R.pool_output_dim(r.h, r.w, p.kernel, p.stride, (p.pad,) * 4)
    y64 = _want64(r, x)
    want = R.pooling(y64, p.kernel, p.stride, (p.pad,) * 4, p.avg)
    # the average may cancel: its bound is relative to the window's mean magnitude, plus one rounding per tap of the float32 sum
    scale = R.pooling(np.abs(y64), p.kernel, p.stride, (p.pad,) * 4, True) if p.avg else np.abs(want)
    bound = (LC.T + (p.kernel * p.kernel + 1) * 2.0 ** -24 if p.avg else LC.T) * scale
    for off in (0, 1):
        xi, out = Region(x.shape, x, off), Region((r.n, r.c, oh, ow), "poison", off)
        lrn_pool(xi.tensor, _pool_dict(p), out=out.tensor, **_kw(r))
        route = lrn_pool_route(xi.tensor, _pool_dict(p), r.local_size, r.region, out=out.tensor)
        assert route == p.route, (p.id, route)
        assert out.guards_intact() and out.unwritten() == 0 and xi.unchanged(), (p.id, off, route)
        two = pooling(lrn(xi.tensor, **_kw(r)), pool_param(r.c, r.h, r.w, **_pool_dict(p)))
        assert tuple(two.shape) == (r.n, r.c, oh, ow)
        assert np.array_equal(out.bits(), two.cpu().numpy().view(np.int32)), (p.id, off, route)
        got = out.bits().view(np.float32).astype(np.float64)
        assert (np.abs(got - want) <= bound).all(), (p.id, off, float((np.abs(got - want) / scale).max()), LC.T)
    print(f"{p.id}: {route}: {r.n}x{r.c}x{r.h}x{r.w} -> {oh}x{ow}, fused == lrn + pooling bit for bit; worst error / bound = {float((np.abs(got - want) / bound).max()):.3f}")


def test_the_routes_of_the_tables_are_every_instantiation(cuda):
    """The names fhip_lrn_route and fhip_lrn_pool_route give for the tensors the two sweeps above launch (which assert them launch by launch)
    are every kernel descriptor of the library's gfx950 code object, and nothing else."""
    import torch
    from feathercnn_amd import lrn_pool_route, lrn_route
    raw = torch.empty(1 << 19, device="cuda")
    seen = set()
    for r in LC.LRN_ROWS:
        for off in (0, 1):
            x = raw[off:off + r.n * r.c * r.h * r.w].view(r.n, r.c, r.h, r.w)
            seen.add(lrn_route(x, r.local_size, r.region, out=x))  # only the alignment is looked at
    for p in LC.POOL_ROWS:
        r = p.lrn
        seen.add(lrn_pool_route(raw[:r.n * r.c * r.h * r.w].view(r.n, r.c, r.h, r.w), _pool_dict(p), r.local_size, r.region))
    assert seen == set(KI.instances(LIB)), (sorted(seen), KI.instances(LIB))
    print(f"{len(seen)} instantiations, all named by a row: {sorted(seen)}")


def test_graph_capture_and_overlap(cuda):
    import torch
    from feathercnn_amd import FeatherHipError, lrn, lrn_pool
    for r, pool in ((LC.ACROSS_ROWS[-2], {"kernel": 3, "stride": 2}), (LC.WITHIN_ROWS[3], {"kernel": 2, "stride": 2, "pooling_type": 1})):
        x = torch.from_numpy(LC.make_input(r)).cuda()
        eager, eager_p = lrn(x, **_kw(r)), lrn_pool(x, pool, **_kw(r))
        out, out_p = torch.full_like(eager, float("nan")), torch.full_like(eager_p, float("nan"))
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(graph, stream=side):
                lrn(x, out=out, **_kw(r))
                lrn_pool(x, pool, out=out_p, **_kw(r))
        assert torch.isnan(out).all() and torch.isnan(out_p).all()  # captured, not run
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager) and torch.equal(out_p, eager_p), r.id
        x.copy_(x.flip(0).flip(1))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, lrn(x, **_kw(r))) and torch.equal(out_p, lrn_pool(x, pool, **_kw(r))), r.id
    with pytest.raises(FeatherHipError, match="overlap"):
        lrn(x, out=x, **_kw(r))
    both = torch.zeros(2 * x.numel(), device="cuda")
    a, b = both[:x.numel()].view(x.shape), both[x.numel():].view(x.shape)
    a.copy_(x)
    lrn(a, out=b, **_kw(r))  # a tensor right behind the other is no overlap
    assert torch.equal(b, lrn(x, **_kw(r))) and torch.equal(a, x)


# ---- feather::Net ----------------------------------------------------------------------------------------------------------------------
_REF = {}


def _reference(name, size, batch, seed):
    from feathercnn_amd import model_zoo
    key = (name, size, batch, seed)
    if key not in _REF:
        model = model_zoo.MODELS[name](size=size)
        x = np.random.default_rng(seed).uniform(-1, 1, (batch, 3, size, size)).astype(np.float32)
        _REF[key] = (model, x, R.Net(model[0], model[1]).run(model[2], x, model[3], keep=True))
    return _REF[key]


def _net(model, x, level, **kw):
    from feathercnn_amd.net import Net
    net = Net(fusion=level, **kw)
    net.SetExtendedLayers(True)
    net.LoadParam(model[0])
    net.LoadWeights(model[1])
    net.FeedInput(model[2], x)
    net.Forward()
    return net


TINY_BLOBS = ("pool1", "pool2", "norm3", "pool3", "relu3", "norm4", "pool5", "heads", "fc", "prob")
_LEVEL0 = {}


def _level0():
    """tiny_lrn's blobs at fusion level 0, computed once."""
    if not _LEVEL0:
        model, x, _ = _reference("tiny_lrn", 16, 5, 21)
        net = _net(model, x, 0)
        _LEVEL0.update({name: net.Extract(name) for name in TINY_BLOBS})
    return _LEVEL0


@pytest.mark.parametrize("level,kw", [(0, {}), (1, {}), (2, {}), (3, {}), (2, {"sub_batches": 2}), (2, {"graph": True}), (3, {"graph": True, "tuned": True}),
                                      (2, {"concurrency": True}), (2, {"concurrency": True, "graph": True, "sub_batches": 2})])
def test_tiny_lrn_against_the_restatement(cuda, level, kw):
    from feathercnn_amd import model_zoo
    model, x, blobs = _reference("tiny_lrn", 16, 5, 21)
    net = _net(model, x, level, **kw)
    if kw.get("graph"):
        net.Forward()  # the replay
    worst = 0.0
    got = {}
    for name in TINY_BLOBS + (("norm1", "norm2", "norm5") if level < 2 else ()):
        got[name] = net.Extract(name)
        e = R.nerr(got[name], blobs[name])
        worst = max(worst, e)
        assert got[name].shape == blobs[name].shape and e <= TOL, (level, kw, name, e)
    if level >= 2:
        vs0 = {name: R.nerr(got[name], _level0()[name]) for name in TINY_BLOBS}
        assert all(e <= 1e-5 for e in vs0.values()), vs0
    if kw.get("sub_batches"):  # two replicas with a share of the batch each: what one computes
        one = _net(model, x, level, **{k: v for k, v in kw.items() if k != "sub_batches"})
        vs1 = {name: R.nerr(got[name], one.Extract(name)) for name in TINY_BLOBS}
        assert all(e <= 1e-5 for e in vs1.values()), vs1
    fuse, keep = model_zoo.LRN_POOLS["tiny_lrn"]
    routed = [nm for _, nm, a in net.layers() if a == "LRN"]
    assert sorted(routed) == sorted(fuse + keep)
    names = [nm for _, nm, _ in net.layers()]
    assert all(("pool" + nm[-1] in names) == (level < 2) for nm in fuse)
    print(f"tiny_lrn level {level} {kw}: worst normalised error {worst:.2e}, {len(routed)} LRN-route layers of {len(names)}")


def test_the_fused_layer_is_bit_identical_to_the_two_layers(cuda):
    """At fusion level 2 the blobs on both sides of norm1 -> pool1, norm2 -> pool2 and norm5 -> pool5 carry the bits they carry at level 1,
    where the two layers run one after the other; the normalised tensor itself refuses Extract; and at level 0 every LRN top is the
    library call on its bottom."""
    import torch
    from feathercnn_amd import FeatherHipError, lrn
    model, x, _ = _reference("tiny_lrn", 16, 5, 21)
    one, two = _net(model, x, 1), _net(model, x, 2)
    bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.int32)
    for bottom, inner, top in (("relu1", "norm1", "pool1"), ("relu2", "norm2", "pool2"), ("conv5", "norm5", "pool5")):
        assert np.array_equal(bits(one.Extract(bottom)), bits(two.Extract(bottom))), bottom
        assert np.array_equal(bits(one.Extract(top)), bits(two.Extract(top))), top
        with pytest.raises(FeatherHipError, match="fused"):
            two.Extract(inner)
    two.Extract("norm3")  # the LRN with two readers keeps its blob
    lv0 = _net(model, x, 0)
    t = lambda name: torch.from_numpy(lv0.Extract(name)).cuda()
    f = np.float32
    for top, bottom, kw in (("norm1", "relu1", dict(local_size=5, alpha=f(1.0), beta=f(0.75))), ("norm2", "relu2", dict(local_size=3, alpha=f(2.0), beta=f(0.5), region=1)),
                            ("norm3", "split1_0", dict(local_size=5, alpha=f(0.5), beta=f(0.6), bias=f(2.0))), ("norm4", "pool4", dict(local_size=3, alpha=f(1.0), beta=f(0.75))),
                            ("norm5", "conv5", dict(local_size=5, alpha=f(1.0), beta=f(0.75)))):
        assert np.array_equal(bits(lv0.Extract(top)), lrn(t(bottom), **kw).cpu().numpy().view(np.int32)), top


def test_a_fused_layer_above_the_one_launch_size_runs_the_pair_through_the_arena(cuda):
    """Above 4 * 192 * 56 * 56 elements the one-launch kernel measured slower than the two: the fused layer then runs
    fhip_lrn_forward into the net's scratch arena and fhip_pooling from there.  The layer list, the refusal to extract the normalised tensor
    and the bits are those of the one-launch form; the arena is what tells the two apart."""
    from feathercnn_amd import FeatherHipError, model_zoo
    for plane, two in ((97, True), (96, False)):  # 256 * 97^2 = 2408704 > 2408448 >= 256 * 96^2 = 2359296
        g = model_zoo.GraphBuilder(3)
        g.pool("pool", g.lrn("norm", g.input("data", 256, plane, plane), 5, 5.0, 0.75), 3, 2)
        model = g.finish() + ("data", "pool")
        x = np.random.default_rng(plane).standard_normal((1, 256, plane, plane)).astype(np.float32)
        one, fused = _net(model, x, 1), _net(model, x, 2)
        assert fused.layers() == [("Input", "data", None), ("LRN", "norm", "LRN")] and len(one.layers()) == 3
        assert (fused.memory()["arena_bytes"] >= x.size * 4) == two and one.memory()["arena_bytes"] == 0, (plane, fused.memory())
        got = fused.Extract("pool")
        assert np.array_equal(got.view(np.int32), one.Extract("pool").view(np.int32)), plane
        want = R.pooling(R.lrn(x, 5, 5.0, 0.75, 1.0, 0, np.float64), 3, 2)
        assert got.shape == want.shape and (np.abs(got - want) <= LC.T * np.abs(want)).all(), plane
        with pytest.raises(FeatherHipError, match="fused"):
            fused.Extract("norm")


@pytest.mark.parametrize("plane,kernel,avg", [(12, 12, True), (12, 13, True), (8, 8, True), (12, 12, False), (13, 13, True)])
def test_a_window_that_covers_the_plane_runs_the_pair(cuda, plane, kernel, avg):
    """fhip_pooling sums a window that covers the unpadded plane (Caffe's 'kernel = plane' in place of global_pooling) with its plane-reduce
    kernels, in another order than its generic kernel: fhip_lrn_pool_forward refuses that geometry, and the fused layer of fusion level 2
    runs fhip_lrn_forward and fhip_pooling through the arena, so that its bits are those of level 1.  144- and 169-pixel planes take the
    wave-per-plane kernel, the 64-pixel plane the LDS one."""
    import torch
    from feathercnn_amd import FeatherHipError, lrn_pool, model_zoo
    g = model_zoo.GraphBuilder(3)
    g.pool("pool", g.lrn("norm", g.input("data", 19, plane, plane), 5, 5.0, 0.75), kernel, 2, avg=avg)
    model = g.finish() + ("data", "pool")
    x = np.random.default_rng(plane + kernel).standard_normal((3, 19, plane, plane)).astype(np.float32)
    one, fused = _net(model, x, 1), _net(model, x, 2)
    assert fused.layers() == [("Input", "data", None), ("LRN", "norm", "LRN")] and len(one.layers()) == 3
    assert fused.memory()["arena_bytes"] >= x.size * 4 and one.memory()["arena_bytes"] == 0
    got = fused.Extract("pool")
    assert got.shape == (3, 19, 1, 1) and np.array_equal(got.view(np.int32), one.Extract("pool").view(np.int32))
    y64 = R.lrn(x, 5, 5.0, 0.75, 1.0, 0, np.float64)
    want = y64.mean(axis=(2, 3), keepdims=True) if avg else y64.max(axis=(2, 3), keepdims=True)
    scale = np.abs(y64).mean(axis=(2, 3), keepdims=True) if avg else np.abs(want)
    assert (np.abs(got - want) <= (LC.T + (plane * plane + 1) * 2.0 ** -24 if avg else LC.T) * scale).all()
    with pytest.raises(FeatherHipError, match="whole unpadded plane"):
        lrn_pool(torch.from_numpy(x).cuda(), {"kernel": kernel, "stride": 2, "pooling_type": int(avg)}, 5, 5.0, 0.75)


def test_sub_batch_replicas_give_the_bits_of_one_net(cuda):
    """The LRN and pooling kernels work image by image and in a fixed order: two replicas with a share of the batch each (3 + 2 images) give,
    bit for bit, what one net gives -- plain layers of both regions, a one-launch LRN -> Pooling and one that runs the pair."""
    from feathercnn_amd import model_zoo
    g = model_zoo.GraphBuilder(3)
    a, b, c, d = g.split("split", g.input("data", 19, 12, 12), 4)
    g.lrn("across", a, 5, 5.0, 0.75)
    g.lrn("within", b, 3, 9.0, 0.5, region=1)
    g.pool("pool", g.lrn("norm", c, 5, 5.0, 0.75), 3, 2)
    g.pool("whole", g.lrn("norm_w", d, 3, 3.0, 0.6), 12, 1, avg=True)
    model = g.finish() + ("data", "pool")
    x = np.random.default_rng(8).standard_normal((5, 19, 12, 12)).astype(np.float32)
    for level in (0, 2):
        one, two = _net(model, x, level), _net(model, x, level, sub_batches=2)
        for name in ("across", "within", "pool", "whole"):
            got = two.Extract(name)
            assert got.shape[0] == 5 and np.array_equal(got.view(np.int32), one.Extract(name).view(np.int32)), (level, name)


@pytest.mark.parametrize("name,size", [("alexnet", 67), ("caffenet", 67), ("googlenet", 31)])
def test_zoo_nets_batch4_against_the_restatement(cuda, name, size):
    from feathercnn_amd import model_zoo
    model, x, blobs = _reference(name, size, 4, 33)
    fuse, keep = model_zoo.LRN_POOLS[name]
    layers = R.resample_ref.shuffle_ref.parse_param(model[0])
    last_fc = [nm for t, nm, *_ in layers if t == "InnerProduct"][-1]
    outs = {}
    for level in (0, 1, 2, 3):
        net = _net(model, x, level, tuned=(level == 3))
        errs = {o: R.nerr(net.Extract(o), blobs[o]) for o in (last_fc, "prob")}
        outs[level] = net.Extract(last_fc)
        routed = [nm for _, nm, a in net.layers() if a == "LRN"]
        names = [nm for _, nm, _ in net.layers()]
        print(f"{name} {size} px batch 4, level {level}: " + ", ".join(f"{o} {e:.2e}" for o, e in errs.items()) + f"; {len(routed)} LRN-route layers of {len(names)}")
        assert all(e <= TOL for e in errs.values()), (name, level, errs)
        assert sorted(routed) == sorted(fuse + keep) and len(routed) == 2
        for nm in fuse + keep if level < 2 else keep:  # every LRN top that has storage
            assert R.nerr(net.Extract(nm), blobs[nm]) <= TOL, (name, level, nm)
        net.close()
    for level in (2, 3):
        assert R.nerr(outs[level], outs[0]) <= 1e-5, (level, R.nerr(outs[level], outs[0]))


def test_one_launch_per_layer_by_kernel_trace(cuda, tmp_path):
    """An LRN -> Pooling at fusion level 2, then a plain LRN, one Forward each in a fresh child process under rocprofv3 (kernel trace only),
    cut at the three marker launches around them: exactly one kernel each, under the names the route functions report."""
    text, rows, _ = ktrace.trace("lrn_trace_child.py", [], tmp_path, TRACE_TIMEOUT)
    routes = [ln.split(" ", 1)[1] for ln in text.splitlines() if ln.startswith("route ")]
    assert routes == ["fhip::lrn_pool_lds_kernel<5>", "fhip::lrn_across_kernel<1, 5>"], text[-3000:]
    windows = ktrace.between(rows, 3)  # the child separates its two Forwards with three fhip_relu launches
    for which, route in enumerate(routes):
        window = windows[which]
        print(f"kernels of {'the fused LRN -> Pooling' if which == 0 else 'the plain LRN'}:", window)
        assert len(window) == 1 and route.replace(" ", "") in window[0].replace(" ", "").replace("void", ""), window
