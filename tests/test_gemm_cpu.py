"""Gemm and MatMul without a device: the restatement tests/gemm_ref.py against numpy on the MatMul rank rules, the description struct and
the constants against feather_gemm.h, the route per case, every refusal that comes before a device call, and the switch.  (The refusals a
net makes at Reshape -- a blob of rank 4, batch extents 2 against 3, a K that differs -- need planned shapes, so a device:
tests/test_gemm_gpu.py.)"""
import ctypes
import os
import re

import numpy as np
import pytest

import gemm_cases as C
import gemm_ref as R
import side_contract as SC
from feathercnn_amd.gemm import GemmDesc, gemm_route

HEADER = open(os.path.join(SC.INCLUDE, "feather_hip", "feather_gemm.h")).read()
lib = SC.fixture("gemm")


@pytest.mark.parametrize("sa,sb,tb", [((5,), (5,), 0), ((4, 5), (5, 3), 0), ((5,), (5, 3), 0), ((4, 5), (5,), 0), ((4, 5), (5,), 1), ((4, 5), (3, 5), 1), ((2, 4, 5), (2, 5, 3), 0),
                                      ((2, 4, 5), (5, 3), 0), ((4, 5), (2, 3, 5), 1), ((1, 4, 5), (2, 5, 3), 0)])
def test_the_restatement_is_numpys_matmul(sa, sb, tb):
    rng = np.random.default_rng(len(sa) * 10 + len(sb))
    a, b = rng.uniform(-1, 1, sa), rng.uniform(-1, 1, sb)
    want = np.matmul(a, np.swapaxes(b, -1, -2) if tb and b.ndim > 1 else b)
    got = R.matmul(a, b, bool(tb))
    assert got.shape == (want.shape or (1,)) and np.allclose(got, want, rtol=0, atol=1e-14)


def test_the_constants_and_the_struct_are_the_headers():
    import sys
    from feathercnn_amd import gemm as G_function, net as N
    G = sys.modules["feathercnn_amd.gemm"]  # the module: the package's attribute of that name is the function it exports
    define = lambda name: int(re.search(r"#define FHIP_GEMM_%s (\d+)" % name, HEADER).group(1))  # noqa: E731
    assert (G.NET_ROUTE, G.TILE_SMALL, G.TILE_WIDE, G.K_STEP, G.WIDE_BLOCKS, G.THIN_MAX) == tuple(define(n) for n in ("NET_ROUTE", "TILE_SMALL", "TILE_WIDE", "K_STEP", "WIDE_BLOCKS", "THIN_MAX"))
    body = re.search(r"typedef struct\s*\{(.*?)\}\s*fhip_gemm_desc;", HEADER, re.S).group(1)
    fields = [(kind, name.strip()) for kind, names in re.findall(r"^\s*(int|float) ([\w, ]+);", body, re.M) for name in names.split(",")]
    assert fields == [({ctypes.c_int: "int", ctypes.c_float: "float"}[t], n) for n, t in GemmDesc._fields_]
    assert G.NET_ROUTE == N.GEMM_ROUTE and N.LATER_ROUTE_NAMES[N.GEMM_ROUTE] == "GEMM" and callable(G_function)


@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_the_route_of_every_case(case):
    assert gemm_route(GemmDesc(**C.build(case)[0])) == C.route_name(case[3])


def test_the_auto_rule():
    base = dict(m=197, n=197, k=64, batch=12, c_broadcast=-1, lda=64, ldb=197, ldd=197, a_batch_stride=197 * 64, b_batch_stride=197 * 64, d_batch_stride=197 * 197, alpha=1.0)
    assert gemm_route(GemmDesc(**base)) == "fhip::gemm_kernel<0, 0, 0>"  # 12 * 2 * 2 wide blocks: below 512
    assert gemm_route(GemmDesc(**dict(base, batch=128))) == "fhip::gemm_kernel<0, 0, 1>"  # 512
    assert gemm_route(GemmDesc(**dict(base, batch=127))) == "fhip::gemm_kernel<0, 0, 0>"
    assert gemm_route(GemmDesc(**dict(base, batch=384, n=64, k=197, lda=197, ldb=64, ldd=64))) == "fhip::gemm_kernel<0, 0, 0>"  # p v: N = 64 stays at the small tile


def _desc(**kw):
    return GemmDesc(**dict(dict(m=4, n=6, k=5, batch=2, c_broadcast=3, lda=5, ldb=6, ldc=6, ldd=6, a_batch_stride=20, b_batch_stride=30, c_batch_stride=24, d_batch_stride=24,
                                alpha=1.0, beta=1.0), **kw))


@pytest.mark.parametrize("kw,code,word", [
    (dict(m=0), -2, "< 1"), (dict(batch=0), -2, "< 1"), (dict(c_broadcast=5), -2, "c_broadcast"), (dict(c_broadcast=-2), -2, "c_broadcast"), (dict(trans_a=2), -2, "0 or 1"),
    (dict(lda=4), -2, "leading dimension"), (dict(trans_b=1, ldb=4), -2, "leading dimension"), (dict(ldc=5), -2, "leading dimension"), (dict(out_transpose=1, ldd=3), -2, "leading dimension"),
    (dict(b_batch_stride=-1), -2, "negative"), (dict(d_batch_stride=0), -2, "D must not be 0"), (dict(a_batch_stride=2 ** 31 - 1), -2, "2^31"), (dict(alpha=float("nan")), -2, "finite"),
    (dict(beta=float("inf")), -2, "finite"), (dict(tile=32), -1, "tile"),
], ids=lambda v: str(v).replace(" ", ""))
def test_the_library_refuses_before_any_device_call(lib, kw, code, word):
    desc, name = _desc(**kw), ctypes.create_string_buffer(96)
    assert lib.fhip_gemm_route(ctypes.byref(desc), name, 96) == code and word in lib.fhip_gemm_last_error().decode(), lib.fhip_gemm_last_error()
    assert lib.fhip_gemm_forward(ctypes.byref(desc), 64, 64, 64, 64, None) == code  # asked only once the route has refused: the same checks come first


def test_null_and_unaligned_pointers(lib):
    fwd = lambda desc, a=64, c=64, d=64: lib.fhip_gemm_forward(ctypes.byref(desc), a, 64, c, d, None)  # noqa: E731
    assert fwd(_desc(), a=None) == -2 and b"null" in lib.fhip_gemm_last_error()
    assert fwd(_desc(), c=None) == -2 and b"null" in lib.fhip_gemm_last_error()  # C is read: c_broadcast 3
    assert fwd(_desc(), d=66) == -2 and b"aligned" in lib.fhip_gemm_last_error()
    assert lib.fhip_gemm_forward(None, 64, 64, 64, 64, None) == -2 and lib.fhip_gemm_route(ctypes.byref(_desc()), None, 96) == -2 and lib.fhip_gemm_last_error() != b""


def _net(gemm=True, detection=True):
    from feathercnn_amd.net import Net
    net = Net()
    net.SetGemm(gemm)
    net.SetTransformer()
    net.SetDetection(detection)
    return net


def _param(*lines):
    return ("7767517\n%d %d\n" % (len(lines), sum(int(ln.split()[3]) for ln in lines)) + "\n".join(lines) + "\n").encode()


INPUTS = ["Input %s 0 1 %s" % (b, b) for b in "abc"]
GOOD = ["MatMul l 2 1 a b top", "MatMul l 2 1 a b top 0=1", "Gemm l 2 1 a b top", "Gemm l 3 1 a b c top 0=5.0e-1 1=-2.0 2=1 3=1 14=1", "Gemm l 1 1 a top 5=1 6=1 8=4 9=3 10=-1",
        "Gemm l 1 1 b top 4=1 6=1 7=4 8=2 9=3 10=3", "Gemm l 2 1 a c top 5=1 8=4 9=3"]
BAD = {"Gemm l 2 1 a b top 11=1": (-100, "output_N1M"), "Gemm l 2 1 a b top 12=4": (-100, "12=4"), "Gemm l 2 1 a b top 18=1": (-1, "int8"), "Gemm l 2 1 a b top 2=2": (-100, "0 or 1"),
       "Gemm l 1 1 a top": (-100, "2 bottom(s)"), "Gemm l 3 1 a b c top 6=1 10=0": (-100, "2 bottom(s)"), "Gemm l 1 1 a top 5=1 8=4": (-100, "9=0"),
       "Gemm l 1 1 a top 5=1 6=1 8=4 9=3 10=5": (-100, "10=5"), "MatMul l 1 1 a top": (-100, "two bottoms"), "MatMul l 2 1 a b top 0=2": (-100, "0=2")}


@pytest.mark.parametrize("line", GOOD, ids=lambda v: v.replace(" ", "_"))
def test_loadparam_takes_the_good_forms(line):
    net = _net()
    net.LoadParam(_param(*INPUTS, line))
    assert [a for t, _, a in net.layers() if t != "Input"] == ["GEMM"]


@pytest.mark.parametrize("line", sorted(BAD), ids=lambda v: v.replace(" ", "_"))
def test_loadparam_refusals_name_the_layer(line):
    from feathercnn_amd import FeatherHipError
    code, word = BAD[line]
    with pytest.raises(FeatherHipError, match="code %d" % code) as e:
        _net().LoadParam(_param(*INPUTS, line))
    assert "layer l" in str(e.value) and word in str(e.value), str(e.value)


@pytest.mark.parametrize("line", GOOD[:3])
def test_the_switch_and_the_hint(line):
    from feathercnn_amd import FeatherHipError
    for kw, word in ((dict(gemm=False), "(fhip_net_set_gemm lifts this)"), (dict(detection=False), "set both")):
        with pytest.raises(FeatherHipError, match="code -200") as e:
            _net(**kw).LoadParam(_param(*INPUTS, line))
        assert line.split()[0] in str(e.value) and word in str(e.value), str(e.value)


def test_weights_and_the_zoo():
    from feathercnn_amd import FeatherHipError, model_zoo
    net = _net()
    net.LoadParam(_param(*INPUTS, "Gemm l 1 1 a top 5=1 8=4 9=3"))
    with pytest.raises(FeatherHipError) as e:
        net.LoadWeights(b"\x47\x6b\x30\x01" + b"\0" * 24)  # the fp16 tag
    assert "fp16" in str(e.value), str(e.value)
    with pytest.raises(FeatherHipError) as e:
        net.LoadWeights(b"\0" * 12)
    assert "Layer l loading weights failed" in str(e.value), str(e.value)
    param, nbytes, data, out = model_zoo.tiny_matmul(dry=True)
    assert nbytes == len(model_zoo.tiny_matmul()[1]) and (data, out) == ("data", "out")
    net = _net()
    net.LoadParam(param)
    assert [t for t, _, a in net.layers() if a == "GEMM"] == ["MatMul", "MatMul", "Gemm", "Gemm", "MatMul"]
