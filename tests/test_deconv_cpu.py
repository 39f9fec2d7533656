"""The transposed-convolution route without a GPU: the fp64 definition the GPU tests compare against (tests/deconv_ref.py) equals torch's
CPU conv_transpose2d in float64 on every sweep geometry, satisfies the adjoint identity against the project's convolution checker, and
equals the reference's recorded results on the zero-stuffed input with the flipped kernel (tests/golden/deconv_golden.npz);
every case of the sweep table (tests/deconv_cases.py) is one libfeather_deconv.so takes and routes as the table says; bad arguments are
refused on the host with a message; feather::Net loads the three zoo nets that hold deconvolution layers, reports the route for them and
refuses what the definition leaves out.  What the library shares with the other run-time libraries -- its exports, the instantiations it holds, its route code, the build
of its application, its last-error state -- is in tests/test_side_contract_cpu.py."""
import ctypes
import os

import numpy as np
import pytest

import deconv_cases as DC
import deconv_ref as R
import side_contract

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BADARG = -2


lib = side_contract.fixture("deconv")


def _param(c=32, k=64, group=1, h=8, w=8, kh=4, kw=4, s=2, pads=(1, 1, 1, 1), out_pads=(0, 0), bias=1, act=1, **over):
    from feathercnn_amd import _lib
    sh, sw = DC.strides(s)
    pl, pr, pt, pb = pads
    p = _lib.fhip_deconv_param(output_channels=k, input_channels=c, input_h=h, input_w=w, kernel_h=kh, kernel_w=kw,
                               output_h=(h - 1) * sh + kh - pt - pb + out_pads[1], output_w=(w - 1) * sw + kw - pl - pr + out_pads[0],
                               stride_h=sh, stride_w=sw, pad_left=pl, pad_bottom=pb, pad_right=pr, pad_top=pt, group=group, bias_term=bias,
                               activation=act, output_pad_right=out_pads[0], output_pad_bottom=out_pads[1])
    for name, v in over.items():
        setattr(p, name, v)
    return p


def _forward(lib, p, batch=1, out=0x1000, x=0x2000, packed=0x3000, bias=0x4000):
    """fhip_deconv_forward with made-up device addresses: a call the host checks refuse never reaches the device, so they are never read."""
    v = ctypes.c_void_p
    return lib.fhip_deconv_forward(ctypes.byref(p), batch, v(out), v(x), v(packed), None, v(bias), None)


# ---- the definition ------------------------------------------------------------------------------------------------------------------
def _torch_weight(wt, group):
    import torch
    k, cg, kh, kw = wt.shape
    return torch.from_numpy(wt).double().reshape(group, k // group, cg, kh, kw).transpose(1, 2).reshape(group * cg, k // group, kh, kw)


def test_restatement_against_torch_conv_transpose2d():
    """tests/deconv_ref.py against torch's CPU conv_transpose2d in float64 on every sweep geometry: directly (stride, padding,
    output_padding, groups) where the pads are symmetric, and on all of them by cropping torch's unpadded result."""
    import torch
    F = torch.nn.functional
    worst, direct = 0.0, 0
    for case in DC.CASES:
        name, c, k, group, h, w, kh, kw, s, (pl, pr, pt, pb), (opr, opb), _ = case
        sh, sw = DC.strides(s)
        x, wt, b = R.synth(c, k, h, w, kh, kw, group, 2, seed=5, sh=sh, sw=sw)
        y = R.deconv(x, wt, b, group, (sh, sw), (pl, pr, pt, pb), (opr, opb), True)
        ho, wo = DC.out_dims(case)
        assert y.shape == (2, k, ho, wo), name
        xt, wtt, bt = torch.from_numpy(x).double(), _torch_weight(wt, group), torch.from_numpy(b).double()
        full = F.conv_transpose2d(xt, wtt, bt, stride=(sh, sw), groups=group).relu().numpy()
        e = float(np.abs(full[:, :, pt:pt + ho, pl:pl + wo] - y).max())
        if pl == pr and pt == pb:
            t = F.conv_transpose2d(xt, wtt, bt, stride=(sh, sw), padding=(pt, pl), output_padding=(opb, opr), groups=group).relu().numpy()
            e = max(e, float(np.abs(t - y).max()))
            direct += 1
        worst = max(worst, e)
        assert e <= 1e-12, (name, e)
    print(f"deconv_ref vs torch conv_transpose2d (fp64): worst absolute difference {worst:.2e} on {len(DC.CASES)} geometries, {direct} direct")
    assert direct >= 15


def test_adjoint_of_the_projects_convolution():
    """<conv(x, w), y> = <x, deconv(y, w)>: the transposed convolution is the adjoint of the convolution the project's own checker
    (oracle.best()) computes, with the same [K][C] weights read as [C_deconv_out = conv_in][...]: conv maps C -> K with w [K][C][kh][kw],
    its adjoint maps K -> C with the deconvolution weights [C][K][kh][kw] = w transposed in the first two axes."""
    import oracle
    from oracle import Geom
    chk = oracle.best()
    rng = np.random.default_rng(11)
    worst, ran = 0.0, 0
    for c, k, h, w, ks, s, p in ((5, 7, 9, 11, 3, 2, 1), (4, 6, 8, 8, 4, 2, 1), (3, 8, 10, 7, 3, 1, 1), (6, 4, 12, 12, 2, 2, 0), (16, 8, 13, 13, 5, 3, 2)):
        geom = Geom(c, k, h, w, ks, ks, s, s, p, p, p, p, 1, 0, 0)
        x = rng.uniform(-1, 1, (2, c, h, w)).astype(np.float32)
        wt = rng.uniform(-1, 1, (k, c, ks, ks)).astype(np.float32)
        cx = np.asarray(chk.forward(geom, x, wt, None), np.float64)  # [2][K][oh][ow]
        y = rng.uniform(-1, 1, cx.shape).astype(np.float32)
        # the adjoint's output must have the convolution's input size: output padding makes up what the stride's floor division dropped
        oph, opw = (h + 2 * p - ks) % s, (w + 2 * p - ks) % s
        if oph > p or opw > p:
            continue
        d = R.deconv(y, np.ascontiguousarray(wt.transpose(1, 0, 2, 3)), None, 1, (s, s), (p, p, p, p), (opw, oph))
        assert d.shape == x.shape
        lhs, rhs = float((cx * y).sum()), float((x.astype(np.float64) * d).sum())
        e = abs(lhs - rhs) / max(abs(lhs), 1e-30)
        worst, ran = max(worst, e), ran + 1
        assert e <= 1e-4, ((c, k, h, w, ks, s, p), lhs, rhs)
    print(f"adjoint identity against {type(chk).__name__}: worst relative difference {worst:.2e}")
    assert ran >= 4


def test_restatement_equals_the_recorded_reference():
    """The reference on the stuffed input with the flipped kernel (tests/golden/make_deconv_golden.py) against the fp64 definition,
    <= 1e-4 normalised."""
    path = os.path.join(ROOT, "tests", "golden", "deconv_golden.npz")
    assert os.path.getsize(path) <= os.path.getsize(os.path.join(ROOT, "tests", "golden", "gconv_golden.npz"))
    g = np.load(path)
    names = [str(n) for n in g["names"]]
    assert len(names) >= 8
    worst, seen = 0.0, set()
    for n in names:
        c, k, h, w, ks, s, p, op, bias, relu, batch = (int(v) for v in g[n + "/geom"])
        y = R.deconv(g[n + "/x"], g[n + "/w"], g[n + "/b"] if bias else None, 1, (s, s), (p, p, p, p), (op, op), bool(relu))
        assert y.shape == g[n + "/y"].shape
        e = R.nerr(g[n + "/y"], y)
        worst = max(worst, e)
        assert e <= 1e-4, (n, e)
        seen.add((ks, s, p, op))
    print(f"recorded reference vs fp64 definition: worst normalised error {worst:.2e}")
    assert {(4, 2, 1, 0), (2, 2, 0, 0), (3, 2, 1, 1), (3, 1, 1, 0)} <= seen


# ---- the library ---------------------------------------------------------------------------------------------------------------------
def test_every_instantiation_has_a_case(lib):
    assert len({c[0] for c in DC.CASES}) == len(DC.CASES)
    for case in DC.CASES:
        _, c, k, group, h, w, kh, kw, s, pads, out_pads, offset = case
        p = _param(c, k, group, h, w, kh, kw, s, pads, out_pads)
        assert lib.fhip_deconv_supported(ctypes.byref(p)) == 1, (case[0], lib.fhip_deconv_last_error())
        name = ctypes.create_string_buffer(160)
        assert lib.fhip_deconv_route(ctypes.byref(p), name, 160) == 0
        assert name.value.decode() == DC.instance(case), case[0]
        sb, pk = ctypes.c_size_t(1), ctypes.c_size_t()
        assert lib.fhip_deconv_get_buffer_size(ctypes.byref(p), 3, ctypes.byref(sb), ctypes.byref(pk)) == 0
        assert sb.value == 0 and pk.value >= 4 * k * (c // group) * kh * kw, case[0]
        q = _param(c, k, group, h, w, kh, kw, s, pads, out_pads, output_h=0, output_w=0)
        assert lib.fhip_deconv_assign_output_dim(ctypes.byref(q)) == 0 and (q.output_h, q.output_w) == DC.out_dims(case)


def test_refusals_come_before_any_device_call(lib):
    err = lambda: lib.fhip_deconv_last_error().decode()
    for over, word in (({"kernel_h": 0}, "kernel"), ({"stride_w": 0}, "stride"), ({"pad_left": -1}, "padding"), ({"input_h": 0}, "input size"),
                       ({"output_h": 7}, "output_h"), ({"output_w": 9}, "output_h"), ({"activation": 2}, "activation"), ({"group": 0}, "group"),
                       ({"group": 3}, "input_channels"), ({"input_channels": 48, "group": 3}, "output_channels"),
                       ({"output_pad_right": 2, "output_w": 18}, "smaller than the stride"), ({"output_pad_bottom": 2, "output_h": 18}, "smaller than the stride"),
                       ({"output_pad_right": -1}, "negative output padding"),
                       ({"pad_right": 0, "output_pad_right": 1, "output_w": 18}, "larger than the padding"),
                       ({"pad_bottom": 0, "output_pad_bottom": 1, "output_h": 18}, "larger than the padding"),
                       ({"pad_top": 20, "pad_bottom": 20, "output_h": -22}, "empty")):
        p = _param(**over)
        assert lib.fhip_deconv_supported(ctypes.byref(p)) == 0 and word in err(), (over, err())
        assert _forward(lib, p) == BADARG, over
    good = _param()
    assert lib.fhip_deconv_supported(ctypes.byref(good)) == 1
    assert lib.fhip_deconv_supported(None) == 0
    assert _forward(lib, good, batch=0) == BADARG and "batch" in err()
    for kw_ in ({"out": None}, {"x": None}, {"packed": None}):
        assert _forward(lib, good, **kw_) == BADARG and "null" in err(), kw_
    assert _forward(lib, good, bias=None) == BADARG and "bias" in err()
    for kw_ in ({"out": 0x1002}, {"x": 0x2001}, {"packed": 0x3004}, {"bias": 0x4002}):
        assert _forward(lib, good, **kw_) == BADARG and "aligned" in err(), kw_
    sb, pk = ctypes.c_size_t(), ctypes.c_size_t()
    assert lib.fhip_deconv_get_buffer_size(ctypes.byref(good), 0, ctypes.byref(sb), ctypes.byref(pk)) == BADARG
    assert lib.fhip_deconv_get_buffer_size(ctypes.byref(good), 1, None, ctypes.byref(pk)) == BADARG
    v = ctypes.c_void_p
    assert lib.fhip_deconv_init(ctypes.byref(good), None, v(0x1000), None) == BADARG
    assert lib.fhip_deconv_init(ctypes.byref(good), v(0x1000), None, None) == BADARG
    assert lib.fhip_deconv_init(ctypes.byref(good), v(0x1004), v(0x2000), None) == BADARG and "aligned" in err()
    assert lib.fhip_deconv_route(ctypes.byref(good), None, 96) == BADARG
    assert lib.fhip_deconv_assign_output_dim(None) == BADARG


def test_buffer_sizes_are_pure_and_independent_of_batch_and_plane():
    from feathercnn_amd import Deconv, DeconvParam
    d = Deconv()
    sizes = {d.GetBufferSize(DeconvParam.make(128, 64, h, batch=b)) for h in (8, 32) for b in (1, 16)}
    assert sizes == {(0, 4 * 64 * 128 * 16)}  # k4 s2: four phases of four taps, 2 x 64 rows fill the 128-row tile: no padding at all
    assert d.GetBufferSize(DeconvParam.make(128, 64, 8, k=3, p=1, op=1))[1] == 4 * 128 * 128 * (4 + 2)  # k3 s2 paired: 4 + 2 taps for 9 useful


# ---- feather::Net --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny_deconv", "style_transfer", "unet_k4"])
def test_net_loads_the_deconvolution_nets(name):
    from feathercnn_amd import model_zoo
    from feathercnn_amd.net import Net
    p, b, _, _ = model_zoo.MODELS[name]()
    layers = R.gconv_ref.parse_param(p)
    deconvs = [nm for t, nm, _, _, _ in layers if t in R.DECONV_TYPES]
    assert sorted(deconvs) == sorted(model_zoo.DECONV_LAYERS[name])
    assert R.Net(p, b).read == len(b)  # the restatement reads every weight byte ...
    for level in (0, 1, 2, 3):
        net = Net(fusion=level)
        net.LoadParam(p)
        net.LoadWeights(b)  # ... and so does the runtime (a short or long read is an error)
        routes = {nm: a for _, nm, a in net.layers()}
        assert all(routes[nm] == "DECONV" for nm in deconvs), routes
        assert sum(a == "DECONV" for a in routes.values()) == len(deconvs)
        types = {nm: t for t, nm, _ in net.layers()}
        assert all(types[nm] in R.DECONV_TYPES for nm in deconvs)
    net = Net()
    net.LoadParam(p)
    with pytest.raises(Exception):
        net.LoadWeights(b[:-4])


def _one_layer(extra="", type_="Deconvolution", wsize=16 * 8 * 16, base="0=8 1=4 3=2 4=1 5=1"):
    return f"7767517\n2 2\nInput data 0 1 data 0=8 1=8 2=16\n{type_} up 1 1 data up {base} 6={wsize} {extra}\n".encode()


@pytest.mark.parametrize("extra,code", [("2=2", -200), ("12=2", -200), ("20=16", -200), ("21=16", -200), ("8=1", -200), ("9=1", -200),
                                        ("18=2", -100), ("19=2", -100), ("18=1 15=0", -100), ("19=1 16=0", -100), ("7=3", -100)])
def test_load_param_refuses_what_the_definition_leaves_out(extra, code):
    from feathercnn_amd import FeatherHipError
    from feathercnn_amd.net import Net
    net = Net()
    with pytest.raises(FeatherHipError) as e:
        net.LoadParam(_one_layer(extra))
    assert f"code {code}" in str(e.value), str(e.value)
    ok = Net()
    ok.LoadParam(_one_layer("18=1 19=1"))  # output padding below the stride and within the pad: accepted
    assert ok.layers()[1] == ("Deconvolution", "up", "DECONV")
    dw = Net()
    dw.LoadParam(_one_layer("7=16", "DeconvolutionDepthWise", wsize=16 * 16, base="0=16 1=4 3=2 4=1 5=0"))
    assert dw.layers()[1][2] == "DECONV"
