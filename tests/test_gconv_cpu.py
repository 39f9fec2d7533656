"""The grouped-convolution route (1 < group < C) without a GPU: every case of the GPU sweep's table
(tests/gconv_cases.py) is one libfeather_gconv.so (include/feather_hip/feather_gconv.h) takes and routes as the table says, and its
sources include only what the side libraries share; bad arguments are refused on the host with a message; fhip_conv_select_algo still answers -1 for a partial
group; the buffer sizes are pure; feather::Net loads the two zoo nets that hold grouped layers and reports the route for them; the
fp64 restatement the GPU tests compare against (tests/gconv_ref.py) equals the reference's recorded results on slices
(tests/golden/gconv_golden.npz).  What the library shares with the other run-time libraries -- its exports, the instantiations it holds, its route code, the build
of its application, its last-error state -- is in tests/test_side_contract_cpu.py."""
import ctypes
import glob
import os
import re

import numpy as np
import pytest

import gconv_cases as GC
import gconv_ref as R
import side_contract

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "feather_hip", "feather_gconv.h")
SOURCES = os.path.join(ROOT, "feathercnn_amd", "csrc_gconv")
BADARG, UNSUPPORTED = -2, -1


lib = side_contract.fixture("gconv")


def _param(c=16, k=16, group=4, h=8, w=8, kh=3, kw=3, s=1, pads=(1, 1, 1, 1), bias=1, act=1, **over):
    from feathercnn_amd import _lib
    sh, sw = GC.strides(s)
    pl, pr, pt, pb = pads
    p = _lib.fhip_conv_param(output_channels=k, input_channels=c, input_h=h, input_w=w, kernel_h=kh, kernel_w=kw,
                             output_h=(h + pt + pb - kh) // sh + 1, output_w=(w + pl + pr - kw) // sw + 1, stride_h=sh, stride_w=sw,
                             pad_left=pl, pad_bottom=pb, pad_right=pr, pad_top=pt, group=group, bias_term=bias, activation=act)
    for name, v in over.items():
        setattr(p, name, v)
    return p


def _forward(lib, p, batch=1, out=0x1000, x=0x2000, packed=0x3000, bias=0x4000):
    """fhip_gconv_forward with made-up device addresses: a call the host checks refuse never reaches the device, so they are never read."""
    v = ctypes.c_void_p
    return lib.fhip_gconv_forward(ctypes.byref(p), batch, v(out), v(x), v(packed), None, v(bias), None)


def test_every_instantiation_has_a_case():
    src = "".join(open(p).read() for p in glob.glob(os.path.join(SOURCES, "*.hip")) + glob.glob(os.path.join(SOURCES, "*.h")))
    # no helper header of feathercnn_amd/csrc: every kernel is in csrc_gconv.  Beyond the public headers it includes only what the side
    # libraries share (csrc_side), and those headers declare no kernel and take nothing of csrc but common.h (which holds none either)
    kernel_decl = r"__global__\s+(?:__launch_bounds__\((?:[^()]|\([^()]*\))*\)\s+)?void\s+(\w+)"
    quoted = r'#include\s+"(?!feather_hip/)([^"]*)'
    side = os.path.join(ROOT, "feathercnn_amd", "csrc_side")
    assert set(re.findall(quoted, src)) <= set(os.listdir(side))
    shared = "".join(open(p).read() for p in glob.glob(os.path.join(side, "*.h")))
    assert set(re.findall(quoted, shared)) <= set(os.listdir(side)) | {"common.h"}
    assert not re.findall(kernel_decl, shared + open(os.path.join(ROOT, "feathercnn_amd", "csrc", "common.h")).read())
    assert len({c[0] for c in GC.CASES}) == len(GC.CASES)
    # every case is one the library takes, and the restated dispatch is the library's own
    from feathercnn_amd import _lib
    lib = _lib.load_gconv_library()
    for case in GC.CASES:
        _, c, k, group, h, w, kh, kw, s, pads, offset = case
        p = _param(c, k, group, h, w, kh, kw, s, pads)
        assert lib.fhip_gconv_supported(ctypes.byref(p)) == 1, case[0]
        name = ctypes.create_string_buffer(96)
        at = 0x10000 + 4 * offset
        assert lib.fhip_gconv_route(ctypes.byref(p), ctypes.c_void_p(at), ctypes.c_void_p(at), name, 96) == 0
        assert name.value.decode() == GC.instance(case), case[0]
        sb, pk = ctypes.c_size_t(1), ctypes.c_size_t()
        assert lib.fhip_gconv_get_buffer_size(ctypes.byref(p), 3, ctypes.byref(sb), ctypes.byref(pk)) == 0
        assert sb.value == 0 and pk.value == 4 * GC.packed_floats(c, k, group, kh, kw, s, pads), case[0]


def test_refusals_come_before_any_device_call(lib):
    err = lambda: lib.fhip_gconv_last_error().decode()
    # the groups this library leaves to the tuned routes of the main library
    for group, word in ((1, "dense"), (0, "dense"), (-2, "dense"), (16, "depthwise")):
        p = _param(group=group)
        assert lib.fhip_gconv_supported(ctypes.byref(p)) == 0 and word in err(), group
        assert _forward(lib, p) == BADARG and word in err()
    # channel counts that the groups do not divide
    for kw_, word in (({"c": 18}, "input_channels"), ({"k": 18}, "output_channels"), ({"c": 8, "group": 16}, "input_channels")):
        p = _param(**kw_)
        assert lib.fhip_gconv_supported(ctypes.byref(p)) == 0 and word in err(), kw_
        assert _forward(lib, p) == BADARG
    # geometry
    for over, word in (({"kernel_h": 0}, "kernel"), ({"stride_w": 0}, "stride"), ({"pad_left": -1}, "padding"), ({"input_h": 0}, "input size"),
                       ({"output_h": 7}, "output_h"), ({"output_w": 9}, "output_h"), ({"activation": 2}, "activation"),
                       ({"kernel_h": 11, "output_h": 0}, "larger")):
        p = _param(**over)
        assert lib.fhip_gconv_supported(ctypes.byref(p)) == 0 and word in err(), over
        assert _forward(lib, p) == BADARG, over
    # arguments of the calls
    good = _param()
    assert lib.fhip_gconv_supported(ctypes.byref(good)) == 1
    assert lib.fhip_gconv_supported(None) == 0
    assert _forward(lib, good, batch=0) == BADARG and "batch" in err()
    for kw_ in ({"out": None}, {"x": None}, {"packed": None}):
        assert _forward(lib, good, **kw_) == BADARG and "null" in err(), kw_
    assert _forward(lib, good, bias=None) == BADARG and "bias" in err()
    for kw_ in ({"out": 0x1002}, {"x": 0x2001}, {"packed": 0x3003}, {"bias": 0x4002}):
        assert _forward(lib, good, **kw_) == BADARG and "aligned" in err(), kw_
    sb, pk = ctypes.c_size_t(), ctypes.c_size_t()
    assert lib.fhip_gconv_get_buffer_size(ctypes.byref(good), 0, ctypes.byref(sb), ctypes.byref(pk)) == BADARG
    assert lib.fhip_gconv_get_buffer_size(ctypes.byref(good), 1, None, ctypes.byref(pk)) == BADARG
    assert lib.fhip_gconv_get_buffer_size(ctypes.byref(_param(group=1)), 1, ctypes.byref(sb), ctypes.byref(pk)) == BADARG
    v = ctypes.c_void_p
    assert lib.fhip_gconv_init(ctypes.byref(good), None, v(0x1000), None) == BADARG
    assert lib.fhip_gconv_init(ctypes.byref(good), v(0x1000), None, None) == BADARG
    assert lib.fhip_gconv_init(ctypes.byref(good), v(0x1002), v(0x2000), None) == BADARG and "aligned" in err()
    assert lib.fhip_gconv_init(ctypes.byref(_param(group=16)), v(0x1000), v(0x2000), None) == BADARG
    name = ctypes.create_string_buffer(96)
    assert lib.fhip_gconv_route(ctypes.byref(good), v(0x1000), v(0x2000), None, 96) == BADARG
    assert lib.fhip_gconv_route(ctypes.byref(_param(group=1)), v(0x1000), v(0x2000), name, 96) == BADARG
    # every refusal above is listed in the header
    text = open(HEADER).read()
    for word in ("group == 1", "input_channels % group", "output_channels % group", "4-byte aligned", "batch < 1", "NULL bias"):
        assert word in text, word


def test_select_algo_still_refuses_a_partial_group(lib):
    from feathercnn_amd import ConvBooster, ConvParam, GroupedConv
    p = ConvParam.make(16, 16, 12, 3, 1, 1, group=4)
    assert ConvBooster().SelectAlgo(p) == -1 and ConvBooster().SelectAlgo(p, tuned=True) == -1
    assert GroupedConv.Supported(p)
    assert not GroupedConv.Supported(ConvParam.make(16, 16, 12, 3, 1, 1, group=1))
    assert not GroupedConv.Supported(ConvParam.make(16, 16, 12, 3, 1, 1, group=16))


def test_buffer_sizes_are_pure_and_monotonic_in_batch():
    from feathercnn_amd import ConvParam, GroupedConv
    g = GroupedConv()
    last = None
    for batch in (1, 2, 7, 64):
        p = ConvParam.make(128, 128, 56, 3, 1, 1, group=32, batch=batch)
        sizes = g.GetBufferSize(p)
        assert sizes == g.GetBufferSize(p)
        assert sizes[1] == 128 * 4 * 9 * 4  # K * C/group * taps floats: no padding at 4 channels per group
        if last is not None:
            assert sizes[0] >= last[0] and sizes[1] == last[1]
        last = sizes
    # K/group = 6 is padded to two chunks of 4
    assert g.GetBufferSize(ConvParam.make(32, 24, 9, 1, 1, 0, group=4))[1] == 4 * 2 * 8 * 1 * 4 * 4


@pytest.mark.parametrize("name", ["tiny_grouped", "resnext50_32x4d"])
def test_net_loads_the_grouped_nets(name):
    from feathercnn_amd import model_zoo
    from feathercnn_amd.net import Net
    p, b, _, _ = model_zoo.MODELS[name]()
    layers = R.parse_param(p)
    grouped = [nm for t, nm, _, _, pd in layers if t.startswith("Convolution") and 1 < pd.get(7, 1) and
               pd.get(6, 0) // (pd.get(0, 0) // pd.get(7, 1)) // pd.get(1, 0) ** 2 != pd.get(7, 1)]
    assert len(grouped) == {"tiny_grouped": 4, "resnext50_32x4d": 16}[name]
    if name == "tiny_grouped":
        assert tuple(grouped) == model_zoo.GROUPED_LAYERS[name]
    assert R.Net(p, b).read == len(b)  # the restatement reads every weight byte ...
    for level in (0, 1, 2, 3):
        net = Net(fusion=level)
        net.LoadParam(p)
        net.LoadWeights(b)  # ... and so does the runtime (a short or long read is an error)
        routes = {nm: a for _, nm, a in net.layers()}
        assert all(routes[nm] == "GCONV" for nm in grouped), routes
        assert sum(a == "GCONV" for a in routes.values()) == len(grouped)
    net = Net()
    net.LoadParam(p)
    with pytest.raises(Exception):
        net.LoadWeights(b[:-4])


def test_restatement_equals_the_recorded_reference():
    """The reference on slices (tests/golden/make_gconv_golden.py) against the fp64 definition, <= 1e-4 normalised."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "gconv_golden.npz"))
    names = [str(n) for n in g["names"]]
    assert len(names) >= 6
    seen = set()
    worst = 0.0
    for n in names:
        c, k, group, h, w, kh, kw, sh, sw, pl, pr, pt, pb, bias, relu, batch = (int(v) for v in g[n + "/geom"])
        assert 1 < group < c
        y = R.conv(g[n + "/x"], g[n + "/w"], g[n + "/b"] if bias else None, group, (sh, sw), (pl, pr, pt, pb), bool(relu))
        assert y.shape == g[n + "/y"].shape
        e = R.nerr(g[n + "/y"], y)
        worst = max(worst, e)
        assert e <= 1e-4, (n, e)
        seen |= {(kh, sh), ("cg", c // group)}
        if (pl, pt) != (pr, pb):
            seen.add("asym")
    print(f"recorded reference vs fp64 restatement: worst normalised error {worst:.2e}")
    assert {(3, 1), (3, 2), (1, 1), (5, 1), "asym", ("cg", 4), ("cg", 3)} <= seen


def test_restatement_against_an_independent_convolution():
    """tests/gconv_ref.py against torch's CPU convolution in float64 on the sweep's geometries (two implementations of the definition)."""
    import torch
    for case in GC.CASES:
        _, c, k, group, h, w, kh, kw, s, (pl, pr, pt, pb), _ = case
        x, wt, b = R.synth(c, k, h, w, kh, kw, group, 2, seed=5)
        y = R.conv(x, wt, b, group, GC.strides(s), (pl, pr, pt, pb), True)
        xt = torch.nn.functional.pad(torch.from_numpy(x).double(), (pl, pr, pt, pb))
        t = torch.nn.functional.conv2d(xt, torch.from_numpy(wt).double(), torch.from_numpy(b).double(), stride=GC.strides(s), groups=group)
        assert y.shape[2:] == GC.out_dims(case)
        assert np.abs(y - t.relu().numpy()).max() < 1e-12, case[0]
