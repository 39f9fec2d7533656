"""The seams of the Interp and HardSwish layers on the MI355X (tests/resample_seam_cases.py is the table) against tests/resample_ref.py's
float64 Net, every blob rounded to float32.

One test id per producer; it loops over that row's consumers, both planes, and fusion levels 0 and 2.  Each net runs batch 3, then batch 1
through the same handle (the Reshape path across the seam).  Every output is compared per (n, c) plane (plane_nerr) against the project's
1e-4 normalised; P's top as well wherever the level keeps it.  The claim column (RS.expect) is checked on net.layers().  Each test prints
its worst error per level."""
import time

import pytest

import resample_ref as R
import resample_seam_cases as RS
import seam_cases as SC

pytestmark = pytest.mark.gpu
TOL = 1e-4


def _run_net(case, level, kw, blobs, x, over):
    from feathercnn_amd import FeatherHipError
    from feathercnn_amd.net import Net
    net = Net(fusion=level, **kw)
    try:
        net.SetExtendedLayers(True)
        if case.dilated:
            net.SetDilated(True)
        net.LoadParam(case.param)
        net.LoadWeights(case.weights)
        worst = 0.0
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
            try:
                p = net.Extract(case.p_top)
            except FeatherHipError as err:  # absorbed into its consumer
                assert level >= 1 and "fused into its consumer" in str(err), (case.id, level, str(err))
            else:
                assert p.shape == blobs[case.p_top][:batch].shape, (case.id, level, kw, batch, case.p_top)
                e = R.plane_nerr(p, blobs[case.p_top][:batch])
                worst = max(worst, e)
                if not e <= TOL:
                    over.append((case.id, level, kw, batch, case.p_top, e))
            if batch == SC.BATCH:
                RS.check_claim(case, level, net)
        return worst
    except Exception as err:
        if any(w in str(err) for w in ("illegal memory access", "unspecified launch failure", "hipError")):
            pytest.exit(f"GPU fault in {case.id} at level {level} {kw}: {err}; nothing more runs on this GPU", returncode=3)
        raise
    finally:
        net.close()


@pytest.mark.parametrize("pname", RS.row_names())
def test_seams_of_one_producer(cuda, pname):
    t0, t_ref = time.perf_counter(), 0.0
    worst = [0.0] * len(RS.LEVELS)
    nets, over, at = 0, [], (0.0, None)
    for case in RS.cases_of(pname):
        x = case.input()
        t1 = time.perf_counter()
        blobs = R.Net(case.param, case.weights).run("data", x, keep=True)
        t_ref += time.perf_counter() - t1
        for i, (level, kw) in enumerate(RS.LEVELS):
            e = _run_net(case, level, kw, blobs, x, over)
            worst[i] = max(worst[i], e)
            at = max(at, (e, case.id))
            nets += 1
    print(f"{pname}: {nets} nets in {time.perf_counter() - t0:.2f} s ({t_ref:.2f} s of it the float64 reference); worst plane_nerr per level " +
          ", ".join(f"{lv}: {e:.2e}" for (lv, _), e in zip(RS.LEVELS, worst)) + f"; worst case {at[1]}")
    assert nets and not over, (len(over), over[:20])
