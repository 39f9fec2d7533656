"""The seams of the Interp and HardSwish layers without a GPU (tests/resample_seam_cases.py is the table):

* the table holds both types on both sides, each next to every neighbour type the issue names and next to each other;
* every case builds, parses and evaluates with tests/resample_ref.py's float64 Net, reads its whole .bin, and every output plane reaches
  1e-3 of the tensor's maximum, so that the per-plane metric of tests/test_resample_seams_gpu.py is defined everywhere;
* the claim column holds on the fused layer list at levels 0 .. 3: an Interp and the Eltwise that alone reads its top are one layer from
  level 2 on, in either operand order, and nothing else absorbs or is absorbed by the two types.

tests/test_seams_cpu.py::test_the_table_is_complete reads create_layer, which does not hold the opt-in types: this file has that duty for
them."""
import numpy as np
import pytest

import resample_ref as R
import resample_seam_cases as RS
import seam_cases as SC

ALIVE = 1e-3
_RESULTS = {}


def _evaluate(pname):
    if pname not in _RESULTS:
        rows = []
        for case in RS.cases_of(pname):
            net = R.Net(case.param, case.weights)
            rows.append((case, net, net.run("data", case.input(), keep=True)))
        _RESULTS[pname] = rows
    return _RESULTS[pname]


def test_the_table_holds_both_types_on_both_sides():
    produced = {t: set() for t in RS.NEW_TYPES}  # new type as the consumer -> the producers' types it met
    consumed = {t: set() for t in RS.NEW_TYPES}  # new type as the producer -> the consumers' types it met
    for pname, cname in RS.pairs():
        for plane in SC.PLANES:
            try:
                case = RS.build_case(pname, cname, plane)
            except SC.Incompatible:
                continue
            for t in RS.NEW_TYPES & case.c_types:
                produced[t] |= case.p_types
            for t in RS.NEW_TYPES & case.p_types:
                consumed[t] |= case.c_types
    for t in RS.NEW_TYPES:
        assert RS.NEIGHBOURS | RS.NEW_TYPES <= produced[t], (t, (RS.NEIGHBOURS | RS.NEW_TYPES) - produced[t])
        assert RS.NEIGHBOURS | RS.NEW_TYPES <= consumed[t], (t, (RS.NEIGHBOURS | RS.NEW_TYPES) - consumed[t])
    # the table of tests/seam_cases.py is as it was: this module extends copies
    assert not set(RS.NEW_UNARY) & set(SC.UNARY) and not set(RS.NEW_PRODUCERS) & set(SC.PRODUCERS) and "like" not in SC.CONSUMERS
    # the one fusion has both operand orders, on a plane where the 16-byte kernel runs and on one where it cannot
    for cname in ("elt_first", "elt_second"):
        assert RS.build_case("half", cname, (12, 8)) and RS.build_case("up2", "like", (11, 9))
        assert RS.expect("half", cname, 2) == "collapsed" and RS.expect("half", cname, 1) == "kept"


@pytest.mark.parametrize("pname", RS.row_names())
def test_every_case_evaluates_and_every_output_plane_is_alive(pname):
    rows = _evaluate(pname)
    assert len(rows) >= 6, (pname, len(rows))
    for case, net, blobs in rows:
        assert net.read == len(case.weights), case.id
        assert case.c_first in [l[1] for l in net.layers] and case.p_top in blobs, case.id
        for o in case.outputs:
            y = blobs[o].astype(np.float64)
            assert y.ndim == 4 and y.shape[0] == SC.BATCH and np.isfinite(y).all(), (case.id, o)
            peak = np.abs(y).max(axis=(2, 3))
            assert peak.min() >= ALIVE * peak.max(), (case.id, o, float(peak.min() / peak.max()))
        alone = net.run("data", case.input()[:1], keep=True)
        assert np.array_equal(alone[case.c_top], blobs[case.c_top][:1]), case.id


@pytest.mark.parametrize("pname", RS.row_names())
def test_the_claim_column_on_the_fused_layer_list(pname):
    from feathercnn_amd import FeatherHipError
    from feathercnn_amd.net import Net
    collapsed = 0
    for case in RS.cases_of(pname):
        for level in (0, 1, 2, 3):
            net = Net(fusion=level)
            net.SetExtendedLayers(True)
            if case.dilated:
                net.SetDilated(True)
            net.LoadParam(case.param)
            net.LoadWeights(case.weights)
            with pytest.raises(FeatherHipError, match="has not been fed"):
                net.Forward()  # the fusion pass runs first; the list it leaves is the fused one
            collapsed += RS.check_claim(case, level, net) == "collapsed"
            net.close()
    assert (collapsed > 0) == (pname == "half"), (pname, collapsed)  # the only Interp whose plane an Eltwise operand of the table reaches


def test_a_default_net_refuses_every_case():
    from feathercnn_amd import FeatherHipError
    from feathercnn_amd.net import Net
    case = RS.build_case("conv3x3", "hswish", SC.PLANES[0])
    with pytest.raises(FeatherHipError, match="code -200"):
        Net().LoadParam(case.param)
