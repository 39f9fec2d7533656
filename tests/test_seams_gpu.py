"""Every producer / consumer pair of Net layer types on the MI355X against tests/seam_ref.py (float64, every blob rounded to float32).

One test id per producer; it loops over the consumers of tests/seam_cases.py, both planes, and the five settings of SC.LEVELS.  Each net
runs batch 3, then batch 1 through the same handle (the Reshape path across the seam).  Every output is compared per (n, c) plane
(plane_nerr), so that one wrong plane cannot hide behind a large neighbour, against the project's 1e-4 (the TOL of the net fuzzer and of the
shuffle / gate net tests); P's top as well wherever the level keeps it.  The claim column (SC.expect) is checked on net.layers() and the
fhip_net_layer_* queries.  Each test prints its worst error per setting."""
import time

import numpy as np
import pytest

import seam_cases as SC
import seam_ref as R

pytestmark = pytest.mark.gpu
TOL = 1e-4


def _run(case, level, kw, blobs, x, over=None):
    """-> (worst plane_nerr, (rule, fired) or None).  With a list `over`, errors above TOL are noted there instead of asserted at once, so
    that a row reports all of its misses."""
    try:
        return _run_net(case, level, kw, blobs, x, over)
    except Exception as err:
        if any(w in str(err) for w in ("illegal memory access", "unspecified launch failure", "hipError")):
            pytest.exit(f"GPU fault in {case.id} at level {level} {kw}: {err}; nothing more runs on this GPU", returncode=3)
        raise


def _within(e, what, over):
    if over is None:
        assert e <= TOL, what
    elif not e <= TOL:
        over.append(what)


def _run_net(case, level, kw, blobs, x, over):
    from feathercnn_amd import FeatherHipError
    from feathercnn_amd.net import Net
    net = Net(fusion=level, **kw)
    try:
        if case.dilated:
            net.SetDilated(True)
        net.LoadParam(case.param)
        net.LoadWeights(case.weights)
        worst = 0.0
        for batch in (SC.BATCH, 1):
            net.FeedInput("data", x[:batch])
            for _ in range(2 if kw.get("graph") else 1):  # the second Forward is the replay
                net.Forward()
            for o in case.outputs:
                got = net.Extract(o)
                assert got.shape == blobs[o][:batch].shape, (case.id, level, kw, o, got.shape)
                e = R.plane_nerr(got, blobs[o][:batch])
                worst = max(worst, e)
                _within(e, (case.id, level, kw, batch, o, e), over)
            try:
                p = net.Extract(case.p_top)
            except FeatherHipError as err:  # absorbed into its consumer, or a chained Winograd layer's transformed output
                assert level >= 1 and not case.pname.startswith("split_") and ("fused into its consumer" in str(err) or "transformed input" in str(err)), (case.id, level, str(err))
            else:
                e = R.plane_nerr(p, blobs[case.p_top][:batch])
                worst = max(worst, e)
                assert p.shape == blobs[case.p_top][:batch].shape, (case.id, level, kw, batch, case.p_top)
                _within(e, (case.id, level, kw, batch, case.p_top, e), over)
            if batch == SC.BATCH:
                claim = SC.check_claim(case, level, net)
        return worst, claim
    finally:
        net.close()


def _row(pname):
    t0, t_ref = time.perf_counter(), 0.0
    worst = [0.0] * len(SC.LEVELS)
    nets, over, at = 0, [], (0.0, None)
    for case in SC.cases_of(pname):
        x = case.input()
        t1 = time.perf_counter()
        blobs = R.Net(case.param, case.weights).run("data", x, keep=True)
        t_ref += time.perf_counter() - t1
        for i, (level, kw) in enumerate(SC.LEVELS):
            e, _ = _run(case, level, kw, blobs, x, over)
            worst[i] = max(worst[i], e)
            at = max(at, (e, case.id))
            nets += 1
    print(f"{pname}: {nets} nets in {time.perf_counter() - t0:.2f} s ({t_ref:.2f} s of it the float64 reference); worst plane_nerr per setting " +
          ", ".join(f"{lv}{'+tuned' if kw.get('tuned') else ''}{'+graph' if kw.get('graph') else ''}: {e:.2e}" for (lv, kw), e in zip(SC.LEVELS, worst)) + f"; worst case {at[1]}")
    assert not over, (len(over), over[:20])
    return worst


@pytest.mark.parametrize("pname", list(SC.PRODUCERS))
def test_seams_of_one_producer(cuda, pname):
    _row(pname)


def test_every_rule_fired_and_was_refused(cuda):
    """For each rule of SC.RULES: the first case of the table that fires it and the first that is a near miss of it, at fusion level 2,
    run here and checked on the planner's own answers.  residual: both operand orders and the Split-blocked variant."""
    want = {}
    for pname in SC.PRODUCERS:
        for cname in SC.CONSUMERS:
            verdict, rule = SC.expect(pname, cname, 2)
            if rule is None:
                continue
            keys = [(rule, verdict != "kept")]
            if rule == "residual":
                keys = [(rule, cname if verdict != "kept" else pname.startswith("split_") and "split")]
            for key in keys:
                if key not in want:
                    try:
                        want[key] = SC.build_case(pname, cname, SC.PLANES[0])
                    except SC.Incompatible:
                        pass
    for rule in SC.RULES:
        need = [(rule, "elt_first"), (rule, "elt_second"), (rule, "split"), (rule, False)] if rule == "residual" else [(rule, True), (rule, False)]
        for key in need:
            assert key in want, key
    seen = []
    for key, case in want.items():
        x = case.input()
        blobs = R.Net(case.param, case.weights).run("data", x, keep=True)
        _, claim = _run(case, 2, {}, blobs, x)
        assert claim is not None and claim[0] == key[0], (key, case.id, claim)
        seen.append((key, case.id, claim[1]))
    for key, cid, fired in seen:
        print(f"{key[0]:12s} {'fired  ' if fired else 'refused'} {cid}")
    for rule in SC.RULES:
        assert {f for k, _, f in seen if k[0] == rule} == {True, False}, rule
