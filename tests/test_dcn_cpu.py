"""Deformable convolution without a device: the switch and the refusals of the Net runtime's param reader, the output size and the route
rule against the header's formulas over the case table, and the room float32 leaves every case of tests/dcn_cases.py."""
import numpy as np
import pytest

import dcn_cases as C

DCN = "0=4 1=3 4=1 5=1 6=180"  # 5 input channels, 4 outputs, 3x3 taps


def _one(params, bottoms="in0 off msk"):
    lines = ["Input in0 0 1 in0 0=8 1=8 2=5", "Input off 0 1 off 0=8 1=8 2=18", "Input msk 0 1 msk 0=8 1=8 2=9",
             f"DeformableConv2D l {len(bottoms.split())} 1 {bottoms} top {params}"]
    return ("7767517\n4 4\n" + "\n".join(lines) + "\n").encode()


def _net(param, deformable=True):
    from feathercnn_amd.net import Net
    net = Net()
    if deformable:
        net.SetDeformable()
    net.LoadParam(param)
    return net


def _refused(param, code, word, **kw):
    from feathercnn_amd import FeatherHipError
    with pytest.raises(FeatherHipError, match=f"code {code}") as e:
        _net(param, **kw)
    assert word in str(e.value), str(e.value)
    return str(e.value)


def test_the_switch():
    from feathercnn_amd import FeatherHipError
    from feathercnn_amd.net import Net
    assert "(fhip_net_set_deformable lifts this)" in _refused(_one(DCN), -200, "DeformableConv2D", deformable=False)
    for bottoms in ("in0 off msk", "in0 off"):
        assert ("DeformableConv2D", "l", "DCN") in _net(_one(DCN, bottoms)).layers()
    with pytest.raises(FeatherHipError, match="before LoadParam"):
        _net(_one(DCN)).SetDeformable(False)
    net = Net()
    net.SetDeformable()
    net.SetDeformable(False)  # on-then-off equals the default
    with pytest.raises(FeatherHipError, match="code -200"):
        net.LoadParam(_one(DCN))


@pytest.mark.parametrize("params,word", [
    (DCN + " 19=1", "19=1"), (DCN + " 8=1", "8=1"), (DCN + " 7=2", "7=2"), ("0=0 1=3 6=180", "0=0"), ("0=4 1=0 6=180", "1=0"), (DCN + " 11=0", "11=0"),
    (DCN + " 3=0", "3=0"), (DCN + " 13=0", "13=0"), (DCN + " 2=0", "2=0"), (DCN + " 12=0", "12=0"), (DCN + " 15=-1", "15=-1"), (DCN + " 14=-1", "14=-1"),
    (DCN + " 16=-1", "16=-1"), ("0=4 1=3 4=-1 6=180", "4=-1"), ("0=4 1=3 6=181", "6=181"), (DCN + " 9=7", "9=7"), ("0=65536 1=32768 6=180", "2^31"),
], ids=lambda v: str(v).replace(" ", "_"))
def test_loadparam_refusals_name_the_layer_and_the_param(params, word):
    msg = _refused(_one(params), -100, word)
    assert "layer l" in msg and "DeformableConv2D" in msg


def test_other_bottom_counts_are_refused():
    for bottoms in ("in0", "in0 off msk msk"):
        assert "2 or 3 bottoms" in _refused(_one(DCN, bottoms), -100, "layer l")


def test_the_zoo_nets_load_and_output_size_and_route_are_the_headers():
    from feathercnn_amd import dcn as M, model_zoo
    layers = _net(model_zoo.centernet_resdcn18(dry=True)[0]).layers()
    assert [a for t, _, a in layers if t == "DeformableConv2D"] == ["DCN"] * 3
    assert ("DeformableConv2D", "dcn", "DCN") in _net(model_zoo.tiny_dcn(dry=True)[0]).layers()
    seen = {C.PACK}
    for case in C.CASES:
        _, c, h, w, k, (kh, kw), (sh, sw), (dh, dw), (pt, pb, pl, pr), g, _, _, _, _, _, out, kernel = case
        want = ((h + pt + pb - (dh * (kh - 1) + 1)) // sh + 1, (w + pl + pr - (dw * (kw - 1) + 1)) // sw + 1)
        assert M.dcn_output_dim(h, w, (kh, kw), (dh, dw), (sh, sw), (pt, pb, pl, pr)) == want == out, case
        assert M.dcn_route(c, k, kh, kw, g) == M.route_rule(c, k, kh, kw, g) == kernel == (C.SMALL if k <= 64 else C.LARGE), case
        seen.add(kernel)
    assert seen == C.targets()


@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_every_case_leaves_float32_room(case):
    t = C.case(case)
    y32 = C.in_float(case, t, np.float32)
    assert y32.shape == t["y"].shape == (case[0], case[4]) + case[15] and np.abs(y32 - t["y"]).max() / np.abs(t["y"]).max() <= C.TOL / 10
