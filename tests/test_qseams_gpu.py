"""Int8 layers next to every other layer type of feather::Net on the MI355X (tests/qseam_cases.py), compared in the three stages of
tests/qseam_ref.py: the fp32 layers against tests/seam_ref.py (float64) by plane_nerr at the project's 1e-4 (TOL of test_seams_gpu.py),
every int8 layer against its restatement from the device's own bottom blob by np.array_equal.

One test id per row of QC.rows(); it loops over the row's consumers, its planes and the five settings of LEVELS.  Each net runs batch 3,
then batch 1 through the same handle.  The claim (QC.check_claim, then qseam_ref.int8_layers' own: which layers each int8 layer absorbed)
is asserted on the planner's answers BEFORE any blob is compared.  Each test prints its worst plane_nerr per setting and its run time.

The refusals (tests/qseam_refusals.py) run each planner rule's int8 net and its fp32 twin; the twin must fire the rule."""
import time

import numpy as np
import pytest

import qseam_cases as QC
import qseam_ref as QR
import qseam_refusals as QF
import seam_ref as R

pytestmark = pytest.mark.gpu
TOL = 1e-4
FAULTS = ("illegal memory access", "unspecified launch failure", "hipError")


def _guard(what, fn, *a, **k):
    """As _run of test_seams_gpu.py: the first HIP error ends the session, so that nothing more runs on the card."""
    try:
        return fn(*a, **k)
    except Exception as err:
        if any(w in str(err) for w in FAULTS):
            pytest.exit(f"GPU fault in {what}: {err}; nothing more runs on this GPU", returncode=3)
        raise


def open_net(param, weights, level, kw, dilated=False):
    from feathercnn_amd.net import Net
    net = Net(fusion=level, **kw)
    try:
        net.SetQuantized(True)
        if dilated:
            net.SetDilated(True)
        net.LoadParam(param)
        net.LoadWeights(weights)
    except Exception:
        net.close()
        raise
    return net


def compare(ref, net, x, level, blobs_to_check, what, over=None, refused_ok=()):
    """Stages 2, then 1 and 3 (see qseam_ref) for a net that has run Forward on `x`: -> the worst plane_nerr over `blobs_to_check`."""
    from feathercnn_amd import FeatherHipError
    given = QR.int8_layers(ref, x, net, level)
    blobs = ref.run("data", x, keep=True, given=given)
    worst = 0.0
    for o in blobs_to_check:
        try:
            got = net.Extract(o)
        except FeatherHipError as err:
            assert o in refused_ok and level >= 1 and ("fused into its consumer" in str(err) or "transformed input" in str(err)), (what, o, str(err))
            continue
        assert blobs[o] is not None, (what, o, "extractable, but inside an int8 layer's fusion by the claim")
        assert got.shape == blobs[o].shape, (what, o, got.shape)
        e = R.plane_nerr(got, blobs[o])
        worst = max(worst, e)
        if over is None:
            assert e <= TOL, (what, o, e)
        elif not e <= TOL:
            over.append((what, o, e))
    return worst


def _run_net(case, ref, level, kw, x, over):
    net = open_net(case.param, case.weights, level, kw, case.dilated)
    try:
        worst = 0.0
        for batch in (QC.BATCH, 1):
            net.FeedInput("data", x[:batch])
            for _ in range(2 if kw.get("graph") else 1):  # the second Forward is the replay
                net.Forward()
            if batch == QC.BATCH:
                QC.check_claim(case, level, net)
            split = case.pname.startswith("split_")
            worst = max(worst, compare(ref, net, x[:batch], level, list(case.outputs) + [case.p_top], (case.id, level, kw, batch), over,
                                       refused_ok=() if split else (case.p_top,)))
        return worst
    finally:
        net.close()


def _row(row):
    t0 = time.perf_counter()
    worst = [0.0] * len(QC.LEVELS)
    nets, over, at = 0, [], (0.0, None)
    for case in QC.cases_of(row):
        x = case.input()
        ref = R.Net(case.param, case.weights)
        for i, (level, kw) in enumerate(QC.LEVELS):
            e = _guard(f"{case.id} at level {level} {kw}", _run_net, case, ref, level, kw, x, over)
            worst[i] = max(worst[i], e)
            at = (e, case.id) if e >= at[0] else at
            nets += 1
    print(f"{row}: {nets} nets in {time.perf_counter() - t0:.2f} s; worst plane_nerr per setting " +
          ", ".join(f"{QF.setting(lv, kw)}: {e:.2e}" for (lv, kw), e in zip(QC.LEVELS, worst)) + f"; worst case {at[1]}")
    assert nets and not over, (nets, len(over), over[:20])


@pytest.mark.parametrize("row", list(QC.rows()))
def test_int8_seams_of_one_row(cuda, row):
    _row(row)


# ---- refusals with a positive control -----------------------------------------------------------------------------------------------------
def _forward(net, x, graph):
    net.FeedInput("data", x)
    for _ in range(2 if graph else 1):
        net.Forward()


@pytest.mark.parametrize("name", list(QF.REFUSALS))
def test_refusal_with_its_control(cuda, name):
    """The fp32 twin fires the rule (asserted on the planner's answers); the int8 net does not, equals the restatement layer by layer and
    meets the float64 evaluation behind it."""
    from feathercnn_amd import FeatherHipError
    t0, worst = time.perf_counter(), 0.0
    for variant in QF.REFUSALS[name]:
        level, kw = variant.level, variant.kw
        x = variant.input()
        twin = open_net(*variant.twin, level, kw)
        try:
            _guard(f"{name}/{variant.tag} twin", _forward, twin, x, kw.get("graph"))
            variant.fired(twin)  # the control
        finally:
            twin.close()
        ref = R.Net(*variant.quant)
        net = open_net(*variant.quant, level, kw)
        try:
            for batch in variant.batches:
                failed = None
                try:
                    _guard(f"{name}/{variant.tag}", _forward, net, x[:batch], kw.get("graph"))
                except FeatherHipError as err:  # a plan the launches refuse (a first layer without its raw filters): the plan is the finding
                    failed = err
                variant.refused(net)  # the planner's answers, before any blob
                if failed:
                    raise failed
                worst = max(worst, compare(ref, net, x[:batch], level, variant.outputs, (name, variant.tag, batch)))
        finally:
            net.close()
    print(f"{name}: {len(QF.REFUSALS[name])} pairs in {time.perf_counter() - t0:.2f} s; worst plane_nerr {worst:.2e}")


def test_int8_layer_on_the_side_stream(cuda):
    """plan_concurrency: an int8 convolution has no scratch, so it leaves the net's stream where its only consumer is not the next layer and
    a convolution runs in between.  concurrency=True must equal concurrency=False bit for bit on every output, eager and as a replayed
    graph, at batch 3 and then batch 1; the int8 layers equal the restatement in every run."""
    param, weights, outputs, x = QF.concurrency_net()
    ref = R.Net(param, weights)
    for level in (2, 3):
        got = {}
        for conc in (False, True):
            for graph in (False, True):
                kw = {"concurrency": conc, "graph": graph, "tuned": level == 3}
                net = open_net(param, weights, level, kw)
                try:
                    for batch in (QC.BATCH, 1):
                        _guard(f"concurrency {kw}", _forward, net, x[:batch], graph)
                        e = compare(ref, net, x[:batch], level, outputs, ("concurrency", level, kw, batch))
                        got[(conc, graph, batch)] = [net.Extract(o) for o in outputs]
                        print(f"concurrency level {level} {kw} batch {batch}: worst plane_nerr {e:.2e}")
                finally:
                    net.close()
        for (conc, graph, batch), blobs in got.items():
            for a, b in zip(blobs, got[(False, False, batch)]):
                assert np.array_equal(a.view(np.int32), b.view(np.int32)), (level, conc, graph, batch)


@pytest.mark.parametrize("name", list(QF.FOLD_EDGES))
def test_fold_edges(cuda, name):
    """Level 2, exact: the fold into d[] and the bias on a layer without a bias term, on a depthwise layer, and on a filter that is all zero
    (s_w = 0, d = 0: the channel is the affine layer's `add`, or its ReLU)."""
    param, weights, outputs, x, zero_channel = QF.FOLD_EDGES[name]()
    ref = R.Net(param, weights)
    net = open_net(param, weights, 2, {})
    try:
        for batch in (QC.BATCH, 1):
            _guard(f"fold edge {name}", _forward, net, x[:batch], False)
            names = [n for _, n, _ in net.layers()]
            assert not [n for n in names if n.startswith("aff")], (name, names)  # the claim: every affine layer is folded
            compare(ref, net, x[:batch], 2, outputs, (name, batch))
            if zero_channel is not None:
                k, value = zero_channel
                got = net.Extract(outputs[0])[:, k]
                assert np.array_equal(got, np.full_like(got, value)), (name, k, value, np.unique(got))
    finally:
        net.close()
