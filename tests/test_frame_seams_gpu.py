"""The seams of Padding, Crop and PixelShuffle and the zero-Padding fold on the MI355X (tests/frame_seam_cases.py and
tests/frame_fold_cases.py are the tables) against tests/frame_seam_ref.py's float64 Net, every blob rounded to float32, which always
evaluates the net as written: Padding, then the convolution -- never the folded form.

* One test id per producer row: its consumers, both planes, fusion levels 0, 2 and 3 tuned; batch 3, then batch 1 through the same handle.
  Every output, and P's top wherever the level keeps it, is compared per (n, c) plane (plane_nerr) against the project's seam tolerance, 1e-4
  (tests/test_seams_gpu.py, tests/test_resample_seams_gpu.py).  A window or PixelShuffle top whose bottoms the level lets Extract must ALSO
  equal the restatement of those bottoms bit for bit: these layers are copies.  The claim column (FS.expect) is checked on net.layers(),
  conv_params() and ExtractDevice.
* One test id per fold row: levels 0, 2, 3 tuned and 3 tuned with the graph replayed once; batch 4, then batch 1.  Each net asserts folded or
  kept, the four pads and the route layer "k" reports, and the plan state its row exists for.
* Two walks the pair form cannot hold: a Crop that is a no-op at one input size and a crop at another (and an alias of an alias under
  concurrency), and per-channel Padding values read from the middle of the .bin stream.

Each test prints its net count, its time and its worst error per level.  On a HIP error the session ends (pytest.exit): nothing more runs on
that GPU."""
import time

import numpy as np
import pytest

import frame_fold_cases as FF
import frame_ref
import frame_seam_cases as FS
import frame_seam_ref as R
import seam_cases as SC

pytestmark = pytest.mark.gpu
TOL = 1e-4
FAULTS = ("illegal memory access", "unspecified launch failure", "hipError")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _open(param, weights, level, kw, dilated=False):
    from feathercnn_amd.net import Net
    net = Net(fusion=level, **kw)
    net.SetFrame()
    if dilated:
        net.SetDilated(True)
    net.LoadParam(param)
    net.LoadWeights(weights)
    return net


def _guard(what, err):
    if any(w in str(err) for w in FAULTS):
        pytest.exit(f"GPU fault in {what}: {err}; nothing more runs on this GPU", returncode=3)


def _try_extract(net, name):
    """The blob, or None where the level has fused or chained it away."""
    from feathercnn_amd import FeatherHipError
    try:
        return net.Extract(name)
    except FeatherHipError as err:
        _guard(name, err)
        assert "fused into its consumer" in str(err) or "transformed input" in str(err) or "chained" in str(err), str(err)
        return None


def _same_address(net):
    from feathercnn_amd import FeatherHipError

    def fn(top, bottom):
        try:
            return net.ExtractDevice(top)[0] == net.ExtractDevice(bottom)[0]
        except FeatherHipError:
            return None
    return fn


def _check_copies(case, level, net, ref, verdict):
    """The framing layers of the case that still stand: top == restatement(bottoms as the net holds them), bit for bit."""
    checked = 0
    for side, name in (("p", "p"), ("c", case.c_first)):
        v = verdict[side]
        if v in (None, "folded"):
            continue
        layer = FS._layer(case, name)
        bottoms = [_try_extract(net, b) for b in layer[2]]
        if any(b is None for b in bottoms):
            continue
        if v == "absorbed":  # the shuffle and the ReLU behind it in one launch: the activation of the shuffle (a zero's sign is the device maximum's own)
            relu = FS._layer(case, "c")
            slope = relu[4].get(0)
            want = frame_ref.pixel_shuffle(bottoms[0], layer[4].get(0, 1), layer[4].get(1, 0), frame_ref.RELU_PLAIN if slope is None else frame_ref.RELU_SLOPE,
                                           0.0 if slope is None else np.float32(slope))
            got = _try_extract(net, "c")
            assert got is not None and got.shape == want.shape and np.array_equal(got, want) and not np.isnan(got).any(), (case.id, level, side)
        else:
            got = _try_extract(net, layer[3][0])
            assert got is not None and _same_bits(got, R.frame_layer(layer, bottoms, ref.pc.get(name))), (case.id, level, side, v)
        checked += 1
    return checked


def _run_net(case, level, kw, ref, blobs, x, over):
    net = None
    try:
        net = _open(case.param, case.weights, level, kw, case.dilated)
        worst, copies = 0.0, 0
        for batch in (SC.BATCH, 1):
            net.FeedInput("data", x[:batch])
            net.Forward()
            for o in case.outputs:
                got = net.Extract(o)
                assert got.shape == blobs[o][:batch].shape, (case.id, level, kw, o, got.shape)
                e = R.plane_nerr(got, blobs[o][:batch])
                worst = max(worst, e)
                if not e <= TOL:
                    over.append((case.id, level, kw, batch, o, e))
            verdict = FS.expect(case.pname, case.cname, level)
            p = _try_extract(net, case.p_top)
            if p is None:
                assert level >= 2 and verdict["p"] in ("folded", "absorbed"), (case.id, level, verdict)
            else:
                assert verdict["p"] not in ("folded", "absorbed"), (case.id, level, verdict)
                assert p.shape == blobs[case.p_top][:batch].shape, (case.id, level, kw, batch, case.p_top)
                e = R.plane_nerr(p, blobs[case.p_top][:batch])
                worst = max(worst, e)
                if not e <= TOL:
                    over.append((case.id, level, kw, batch, case.p_top, e))
            FS.check_claim(case, level, net, _same_address(net))
            copies += _check_copies(case, level, net, ref, verdict)
        return worst, copies
    except Exception as err:
        _guard(f"{case.id} at level {level} {kw}", err)
        raise
    finally:
        if net is not None:
            net.close()


@pytest.mark.parametrize("pname", FS.row_names())
def test_seams_of_one_producer(cuda, pname):
    t0, t_ref = time.perf_counter(), 0.0
    worst = [0.0] * len(FS.LEVELS)
    nets, copies, over, at = 0, 0, [], (0.0, "")
    for case in FS.cases_of(pname):
        x = case.input()
        t1 = time.perf_counter()
        ref = R.Net(case.param, case.weights)
        blobs = ref.run("data", x, keep=True)
        t_ref += time.perf_counter() - t1
        for i, (level, kw) in enumerate(FS.LEVELS):
            e, k = _run_net(case, level, kw, ref, blobs, x, over)
            worst[i] = max(worst[i], e)
            at = max(at, (e, case.id))
            nets += 1
            copies += k
    print(f"{pname}: {nets} nets in {time.perf_counter() - t0:.2f} s ({t_ref:.2f} s of it the float64 reference), {copies} bit-for-bit copies; worst plane_nerr per level " +
          ", ".join(f"{lv}: {e:.2e}" for (lv, _), e in zip(FS.LEVELS, worst)) + f"; worst case {at[1]}")
    assert nets and copies and not over, (len(over), over[:20])


# ---- the fold ----------------------------------------------------------------------------------------------------------------------------
def _check_fold_claim(n, level, kw, net, batch):
    c = n.claim(level, kw.get("tuned", False))
    info = net.layers()
    names = [nm for _, nm, _ in info]
    where = (n.id, level, kw, batch)
    assert ("pad" not in names) == c["folded"] and "k" in names, (where, names)
    for t, nm, a in info:
        assert (a == "FRAME") == (t in FS.FRAME_TYPES), (where, info)
    k = names.index("k")
    q = net.conv_params()[k][0]
    assert (q.pad_top, q.pad_bottom, q.pad_left, q.pad_right) == c["pads"], (where, (q.pad_top, q.pad_bottom, q.pad_left, q.pad_right), c["pads"])
    assert (q.output_h, q.output_w) == n.out_plane() and (q.input_h, q.input_w) == (n.plane if c["folded"] else n.padded()), where
    assert info[k][2] == c["algo"], (where, info[k], c["algo"])
    present = [l[1] for l in frame_ref.parse_param(n.model()[0])]
    for gone in ("pool", "sum", "relu", "bn", "scale", "pw"):
        if gone in present:
            assert (gone not in names) == (gone in c["gone"]), (where, gone, names)
    assert net.residuals().get(k, 0) == c["residual"], (where, net.residuals(), c["residual"])
    pair = net.fused_pointwise().get(k)
    assert (None if pair is None else pair[1]) == c["pair"], (where, pair, c["pair"])
    chains = {names[i]: v for i, v in net.chains(raw=True).items()}
    assert chains == c["chain"], (where, chains, c["chain"])
    return c


def _run_fold(n, level, kw, ref, blobs, over):
    param, weights, outputs = n.model()
    net = None
    try:
        net = _open(param, weights, level, kw)
        worst = 0.0
        for batch in FF.BATCHES:
            x = n.input(batch)
            net.FeedInput("data", x)
            net.Forward()
            first = [net.Extract(o) for o in outputs]
            if kw.get("graph"):  # replay the captured graph once
                net.Forward()
                for o, a in zip(outputs, first):
                    assert _same_bits(net.Extract(o), a), (n.id, level, kw, batch, o)
            for o, got in zip(outputs, first):
                assert got.shape == blobs[o][:batch].shape, (n.id, level, kw, batch, o, got.shape)
                e = R.plane_nerr(got, blobs[o][:batch])
                worst = max(worst, e)
                if not e <= TOL:
                    over.append((n.id, level, kw, batch, o, e))
            c = _check_fold_claim(n, level, kw, net, batch)
            pad = _try_extract(net, "pad")
            assert (pad is None) == c["folded"], (n.id, level, kw, batch)
            if pad is not None:  # a Padding that stays is a copy of its own bottom, -0.0 included
                layer = [l for l in ref.layers if l[1] == "pad"][0]
                bottom = _try_extract(net, layer[2][0])
                assert bottom is not None and _same_bits(pad, R.frame_layer(layer, [bottom])), (n.id, level, kw, batch)
        return worst
    except Exception as err:
        _guard(f"{n.id} at level {level} {kw}", err)
        raise
    finally:
        if net is not None:
            net.close()


@pytest.mark.parametrize("row", sorted(FF.ROWS))
def test_the_fold_against_one_plan_kind(cuda, row):
    t0 = time.perf_counter()
    worst = [0.0] * len(FF.SETTINGS)
    nets, over, at = 0, [], (0.0, "")
    for n in FF.ROWS[row]:
        param, weights, _ = n.model()
        ref = R.Net(param, weights)
        blobs = ref.run("data", n.input(max(FF.BATCHES)), keep=True)
        for i, (level, kw) in enumerate(FF.SETTINGS):
            e = _run_fold(n, level, kw, ref, blobs, over)
            worst[i] = max(worst[i], e)
            at = max(at, (e, n.id))
            nets += 1
    print(f"fold {row}: {nets} nets in {time.perf_counter() - t0:.2f} s; worst plane_nerr per setting " +
          ", ".join(f"{lv}{'g' if kw.get('graph') else ''}: {e:.2e}" for (lv, kw), e in zip(FF.SETTINGS, worst)) + f"; worst net {at[1]}")
    assert nets and not over, (len(over), over[:20])


# ---- the walks ---------------------------------------------------------------------------------------------------------------------------
WALK_SHAPES = ((12, 8), (13, 9), (12, 8))  # Crop 3=8 4=12: the whole blob at 12 x 8, a real crop at 13 x 9
WALK_SETTINGS = ((0, {}), (2, {}), (3, {"tuned": True}), (2, {"concurrency": True}), (3, {"tuned": True, "concurrency": True}))


def _crop_then_conv():
    """Input -> conv1x1 -> Crop(3=8 4=12) -> conv3x3: -> (param, weights, outputs, the Crop's bottom)."""
    from feathercnn_amd import model_zoo
    g = model_zoo.GraphBuilder(71)
    x = g.conv("c1", g.input("data", SC.C0, 12, 8), SC.C0, SC.C0, 1)
    x = g.crop("crop", x, outw=8, outh=12)
    g.conv("c3", x, SC.C0, SC.C0, 3, 1, 1)
    return g.finish() + (("c3",), "c1")


def _crop_split_two():
    """Input -> Crop(3=8 4=12) -> Split -> two 1x1 layers: at 12 x 8 the Split's tops are aliases of an alias of the input."""
    from feathercnn_amd import model_zoo
    g = model_zoo.GraphBuilder(72)
    x = g.crop("crop", g.input("data", SC.C0, 12, 8), outw=8, outh=12)
    a, b = g.split("fork", x)
    outs = (g.conv("ca", a, SC.C0, SC.C0, 1), g.conv("cb", b, SC.C0, 16, 1))
    return g.finish() + (outs, "data")


@pytest.mark.parametrize("which", ["crop_then_conv", "crop_split_two"])
def test_a_crop_that_is_a_no_op_at_one_shape_and_a_crop_at_another(cuda, which):
    param, weights, outputs, crop_bottom = _crop_then_conv() if which == "crop_then_conv" else _crop_split_two()
    ref = R.Net(param, weights)
    rng = np.random.default_rng(73)
    xs = {shape: rng.normal(0, 1, (SC.BATCH, SC.C0) + shape).astype(np.float32) for shape in set(WALK_SHAPES)}
    want = {shape: ref.run("data", x, keep=True) for shape, x in xs.items()}
    t0, worst = time.perf_counter(), 0.0
    for level, kw in WALK_SETTINGS:
        net = None
        try:
            net = _open(param, weights, level, kw)
            for step, shape in enumerate(WALK_SHAPES):
                where = (which, level, kw, step, shape)
                net.FeedInput("data", xs[shape])
                net.Forward()
                fresh = _open(param, weights, level, kw)
                fresh.FeedInput("data", xs[shape])
                fresh.Forward()
                for o in outputs + ("crop",):
                    got = net.Extract(o)
                    assert _same_bits(got, fresh.Extract(o)), (where, o)
                    e = R.plane_nerr(got, want[shape][o])
                    worst = max(worst, e)
                    assert got.shape == want[shape][o].shape and e <= TOL, (where, o, e)
                assert net.layers() == fresh.layers(), where
                fresh.close()
                noop = shape == (12, 8)
                crop, below = net.ExtractDevice("crop"), net.ExtractDevice(crop_bottom)
                assert crop[1] == (SC.BATCH, SC.C0, 12, 8) and below[1] == (SC.BATCH, SC.C0) + shape, (where, crop[1], below[1])
                assert (crop[0] == below[0]) == noop, (where, "the Crop's top must share its bottom's storage exactly where it changes nothing")
                assert _same_bits(net.Extract("crop"), R.frame_layer([l for l in ref.layers if l[1] == "crop"][0], [net.Extract(crop_bottom)])), where
                if which == "crop_split_two":  # Split tops behind the Crop: aliases of an alias at 12 x 8, of the Crop's own storage at 13 x 9
                    for top in ("fork_0", "fork_1"):
                        assert net.ExtractDevice(top)[0] == crop[0], (where, top)
                        assert _same_bits(net.Extract(top), net.Extract("crop")), (where, top)
        except Exception as err:
            _guard(f"{which} at level {level} {kw}", err)
            raise
        finally:
            if net is not None:
                net.close()
    print(f"{which}: {len(WALK_SETTINGS)} settings x {len(WALK_SHAPES)} shapes in {time.perf_counter() - t0:.2f} s; worst plane_nerr {worst:.2e}")


def test_per_channel_padding_values_between_two_layers_weights(cuda):
    """conv -> Padding(per-channel values) -> BatchNorm -> conv: the Padding reads 12 floats from the middle of the .bin.  A reader one float off
    shifts the BatchNorm's four arrays and the last convolution's weights."""
    from feathercnn_amd import model_zoo
    g = model_zoo.GraphBuilder(74)
    x = g.conv("a", g.input("data", SC.C0, 11, 9), SC.C0, SC.C0, 3, 1, 1)
    x = g.padding("pad", x, 1, 1, 1, 1, per_channel=SC.C0)
    out = g.conv("b", g.bn("bn", x, SC.C0), SC.C0, SC.C0, 3, 1, 1)
    param, weights = g.finish()
    ref = R.Net(param, weights)
    assert ref.read == len(weights) and ref.pc["pad"].shape == (SC.C0,)
    x = np.random.default_rng(75).normal(0, 1, (SC.BATCH, SC.C0, 11, 9)).astype(np.float32)
    want = ref.run("data", x, keep=True)
    layer = [l for l in ref.layers if l[1] == "pad"][0]
    worst = []
    for level, kw in FS.LEVELS:
        net = None
        try:
            net = _open(param, weights, level, kw)
            for batch in (SC.BATCH, 1):
                net.FeedInput("data", x[:batch])
                net.Forward()
                got = net.Extract(out)
                e = R.plane_nerr(got, want[out][:batch])
                assert got.shape == want[out][:batch].shape and e <= TOL, (level, kw, batch, e)
                worst.append(e)
                names = [nm for _, nm, _ in net.layers()]
                assert "pad" in names and "bn" in names, (level, names)  # nothing folds a Padding with per-channel values, nothing a BatchNorm behind it
                pad = net.Extract("pad")
                assert R.plane_nerr(pad, want["pad"][:batch]) <= TOL
                if level == 0:
                    assert _same_bits(pad, frame_ref.pad(net.Extract("a"), 1, 1, 1, 1, per_channel=ref.pc["pad"])), (level, batch)
                assert _same_bits(pad, R.frame_layer(layer, [net.Extract("a")], ref.pc["pad"])), (level, batch)
        except Exception as err:
            _guard(f"per-channel Padding at level {level} {kw}", err)
            raise
        finally:
            if net is not None:
                net.close()
    print(f"per-channel Padding: {len(FS.LEVELS)} nets; worst plane_nerr {max(worst):.2e}")
