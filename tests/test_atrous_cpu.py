"""The dilated-convolution route without a GPU: the fp64 definition the GPU tests compare against (tests/atrous_ref.py) equals torch's CPU
conv2d(dilation=) in float64 on every sweep geometry, equals the plain convolution with the zero-stuffed kernel, and equals the reference's
recorded results with that kernel (tests/golden/atrous_golden.npz); every case of the sweep table (tests/atrous_cases.py) is one
libfeather_atrous.so (include/feather_hip/feather_atrous.h) takes and routes as the table says;
bad arguments are refused on the host with a message by every entry point; feather::Net refuses a dilated Convolution by default and loads
it after SetDilated, reports the route and keeps refusing a dilated Deconvolution; the zoo nets parse.
What the library shares with the other run-time libraries -- its exports, the instantiations it holds, its route code, the build
of its application, its last-error state -- is in tests/test_side_contract_cpu.py."""
import ctypes
import os

import numpy as np
import pytest

import atrous_cases as AC
import atrous_ref as R
import gconv_ref
import side_contract

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BADARG, UNSUPPORTED = -2, -1


lib = side_contract.fixture("atrous")


def _param(c=16, k=64, group=1, h=9, w=8, kh=3, kw=3, s=1, pads=(2, 2, 2, 2), dil=(2, 2), bias=1, act=1, **over):
    from feathercnn_amd import _lib
    sh, sw = AC.strides(s)
    pl, pr, pt, pb = pads
    ho, wo = AC.out_dims(("", c, k, group, h, w, kh, kw, s, pads, dil, 0))
    p = _lib.fhip_atrous_param(output_channels=k, input_channels=c, input_h=h, input_w=w, kernel_h=kh, kernel_w=kw, output_h=ho, output_w=wo,
                               stride_h=sh, stride_w=sw, pad_left=pl, pad_bottom=pb, pad_right=pr, pad_top=pt, group=group, bias_term=bias,
                               activation=act, dilation_h=dil[0], dilation_w=dil[1])
    for name, v in over.items():
        setattr(p, name, v)
    return p


def _forward(lib, p, batch=1, out=0x1000, x=0x2000, packed=0x3000, bias=0x4000):
    """fhip_atrous_forward with made-up device addresses: a call the host checks refuse never reaches the device, so they are never read."""
    v = ctypes.c_void_p
    return lib.fhip_atrous_forward(ctypes.byref(p), batch, v(out), v(x), v(packed), None, v(bias), None)


# ---- the definition ------------------------------------------------------------------------------------------------------------------
def test_restatement_against_torch_conv2d_dilation():
    """tests/atrous_ref.py against torch's CPU conv2d(dilation=) in float64 on every sweep geometry (asymmetric pads by padding the input
    first), to 1e-12."""
    import torch
    F = torch.nn.functional
    worst = 0.0
    for case in AC.CASES:
        name, c, k, group, h, w, kh, kw, s, (pl, pr, pt, pb), dil, _ = case
        x, wt, b = R.synth(c, k, h, w, kh, kw, group, 2, seed=5)
        y = R.atrous(x, wt, b, group, AC.strides(s), (pl, pr, pt, pb), dil, True)
        assert y.shape == (2, k) + AC.out_dims(case), name
        xt = F.pad(torch.from_numpy(x).double(), (pl, pr, pt, pb))
        t = F.conv2d(xt, torch.from_numpy(wt).double(), torch.from_numpy(b).double(), stride=AC.strides(s), dilation=dil, groups=group).relu().numpy()
        e = float(np.abs(t - y).max())
        worst = max(worst, e)
        assert e <= 1e-12, (name, e)
    print(f"atrous_ref vs torch conv2d(dilation=) (fp64): worst absolute difference {worst:.2e} on {len(AC.CASES)} geometries")


def test_restatement_equals_the_plain_convolution_with_the_stuffed_kernel():
    """A dilated convolution is the plain convolution (tests/gconv_ref.py, checked elsewhere against the project's oracle) with d - 1 zeros
    between the taps -- the identity the recorded reference fixtures rest on -- and, where only the centre tap is ever inside the plane, the
    1x1 convolution with the centre weights."""
    worst = 0.0
    for case in AC.CASES:
        name, c, k, group, h, w, kh, kw, s, pads, dil, _ = case
        x, wt, b = R.synth(c, k, h, w, kh, kw, group, 2, seed=6)
        y = R.atrous(x, wt, b, group, AC.strides(s), pads, dil)
        z = gconv_ref.conv(x, R.stuffed_kernel(wt, dil), b, group, AC.strides(s), pads)
        e = float(np.abs(z - y).max())
        worst = max(worst, e)
        assert y.shape == z.shape and e <= 1e-12, (name, e)
    case = next(c for c in AC.CASES if c[0] == "row4_centre_only_d12")
    _, c, k, group, h, w, kh, kw, s, pads, dil, _ = case
    x, wt, b = R.synth(c, k, h, w, kh, kw, group, 2, seed=7)
    centre = gconv_ref.conv(x, wt[:, :, 1:2, 1:2], b)
    assert np.abs(centre - R.atrous(x, wt, b, group, (1, 1), pads, dil)).max() <= 1e-12
    print(f"atrous_ref vs the stuffed-kernel convolution (fp64): worst absolute difference {worst:.2e}")


def test_restatement_equals_the_recorded_reference():
    """The reference with the zero-stuffed kernel (tests/golden/make_atrous_golden.py) against the fp64 definition, <= 1e-4 normalised
    (SURVEY.md 8(d))."""
    path = os.path.join(ROOT, "tests", "golden", "atrous_golden.npz")
    assert os.path.getsize(path) <= os.path.getsize(os.path.join(ROOT, "tests", "golden", "deconv_golden.npz"))
    g = np.load(path)
    names = [str(n) for n in g["names"]]
    assert len(names) >= 6
    worst = 0.0
    for n in names:
        c, k, h, w, ks, s, p, d, bias, relu, batch = (int(v) for v in g[n + "/geom"])
        assert d > 1 and g[n + "/w"].shape == (k, c, ks, ks)  # the un-stuffed weights are what is stored
        y = R.atrous(g[n + "/x"], g[n + "/w"], g[n + "/b"] if bias else None, 1, (s, s), (p,) * 4, (d, d), bool(relu))
        assert y.shape == g[n + "/y"].shape
        e = R.nerr(g[n + "/y"], y)
        worst = max(worst, e)
        assert e <= 1e-4, (n, e)
    print(f"recorded reference vs fp64 definition: worst normalised error {worst:.2e}")


# ---- the library ---------------------------------------------------------------------------------------------------------------------
def test_every_instantiation_has_a_case(lib):
    assert len({c[0] for c in AC.CASES}) == len(AC.CASES)
    for case in AC.CASES:
        _, c, k, group, h, w, kh, kw, s, pads, dil, offset = case
        p = _param(c, k, group, h, w, kh, kw, s, pads, dil)
        assert lib.fhip_atrous_supported(ctypes.byref(p)) == 1, (case[0], lib.fhip_atrous_last_error())
        name = ctypes.create_string_buffer(160)
        assert lib.fhip_atrous_route(ctypes.byref(p), name, 160) == 0
        assert name.value.decode() == AC.instance(case), case[0]
        assert AC.instance(case) in AC.accepted_routes(case)
        sb, pk = ctypes.c_size_t(1), ctypes.c_size_t()
        assert lib.fhip_atrous_get_buffer_size(ctypes.byref(p), 3, ctypes.byref(sb), ctypes.byref(pk)) == 0
        assert sb.value == 0 and pk.value >= 4 * k * (c // group) * kh * kw, case[0]
        q = _param(c, k, group, h, w, kh, kw, s, pads, dil, output_h=0, output_w=0)
        assert lib.fhip_atrous_assign_output_dim(ctypes.byref(q)) == 0 and (q.output_h, q.output_w) == AC.out_dims(case)
        for route in AC.accepted_routes(case):  # the named-route calls accept what the table says, on the host
            assert lib.fhip_atrous_get_buffer_size_route(ctypes.byref(p), 1, route.encode(), ctypes.byref(sb), ctypes.byref(pk)) == 0, (case[0], route)


def test_refusals_come_before_any_device_call(lib):
    err = lambda: lib.fhip_atrous_last_error().decode()
    v = ctypes.c_void_p
    sb, pk = ctypes.c_size_t(), ctypes.c_size_t()
    name = ctypes.create_string_buffer(160)
    for over, word in (({"dilation_h": 1, "dilation_w": 1, "output_h": 13, "output_w": 12}, "dilation 1 x 1"), ({"dilation_h": 0}, "dilation must be"),
                       ({"dilation_w": -2}, "dilation must be"), ({"group": 3}, "input_channels"), ({"input_channels": 48, "group": 3, "output_channels": 64}, "output_channels"),
                       ({"group": 0}, "group"), ({"pad_left": -1}, "negative padding"), ({"pad_bottom": -1}, "negative padding"),
                       ({"dilation_h": 7, "output_h": 1}, "extent"), ({"dilation_w": 6, "output_w": 0}, "extent"),
                       ({"output_h": 7}, "output_h"), ({"output_w": 9}, "output_h"), ({"activation": 2}, "activation"), ({"kernel_h": 0}, "kernel"),
                       ({"stride_w": 0}, "stride"), ({"input_h": 0}, "input size"),
                       ({"input_channels": 1 << 16, "input_h": 1 << 8, "input_w": 1 << 8, "output_h": 256, "output_w": 256}, "2^31"),
                       ({"output_channels": 1 << 20, "input_h": 64, "input_w": 64, "output_h": 64, "output_w": 64}, "2^31")):
        p = _param(**over)
        assert lib.fhip_atrous_supported(ctypes.byref(p)) == 0 and word in err(), (over, err())
        # every other entry point refuses the same params
        assert _forward(lib, p) == BADARG, over
        assert lib.fhip_atrous_get_buffer_size(ctypes.byref(p), 1, ctypes.byref(sb), ctypes.byref(pk)) == BADARG, over
        assert lib.fhip_atrous_init(ctypes.byref(p), v(0x1000), v(0x2000), None) == BADARG, over
        assert lib.fhip_atrous_route(ctypes.byref(p), name, 160) == BADARG, over
        assert lib.fhip_atrous_forward_route(ctypes.byref(p), 1, v(0x1000), v(0x2000), v(0x3000), None, v(0x4000), None, AC.GENERIC.encode()) == BADARG, over
        assert lib.fhip_atrous_init_route(ctypes.byref(p), v(0x1000), v(0x2000), None, AC.GENERIC.encode()) == BADARG, over
        assert lib.fhip_atrous_get_buffer_size_route(ctypes.byref(p), 1, AC.GENERIC.encode(), ctypes.byref(sb), ctypes.byref(pk)) == BADARG, over
    good = _param()
    assert lib.fhip_atrous_supported(ctypes.byref(good)) == 1
    assert lib.fhip_atrous_supported(None) == 0
    assert _forward(lib, good, batch=0) == BADARG and "batch" in err()
    for kw_ in ({"out": None}, {"x": None}, {"packed": None}):
        assert _forward(lib, good, **kw_) == BADARG and "null" in err(), kw_
    assert _forward(lib, good, bias=None) == BADARG and "bias" in err()
    for kw_ in ({"out": 0x1002}, {"x": 0x2001}, {"packed": 0x3004}, {"bias": 0x4002}):
        assert _forward(lib, good, **kw_) == BADARG and "aligned" in err(), kw_
    assert _forward(lib, good, batch=1 << 20) == BADARG and "2^31" in err()  # the batch can make a tensor too large as well
    assert lib.fhip_atrous_get_buffer_size(ctypes.byref(good), 0, ctypes.byref(sb), ctypes.byref(pk)) == BADARG
    assert lib.fhip_atrous_get_buffer_size(ctypes.byref(good), 1, None, ctypes.byref(pk)) == BADARG
    assert lib.fhip_atrous_init(ctypes.byref(good), None, v(0x1000), None) == BADARG
    assert lib.fhip_atrous_init(ctypes.byref(good), v(0x1000), None, None) == BADARG
    assert lib.fhip_atrous_init(ctypes.byref(good), v(0x1004), v(0x2000), None) == BADARG and "aligned" in err()
    assert lib.fhip_atrous_route(ctypes.byref(good), None, 96) == BADARG
    assert lib.fhip_atrous_assign_output_dim(None) == BADARG
    # named routes: an unknown name, no name, and a route that cannot run the layer
    assert lib.fhip_atrous_forward_route(ctypes.byref(good), 1, v(0x1000), v(0x2000), v(0x3000), None, v(0x4000), None, b"fhip::nothing") == BADARG
    assert lib.fhip_atrous_forward_route(ctypes.byref(good), 1, v(0x1000), v(0x2000), v(0x3000), None, v(0x4000), None, None) == BADARG
    assert lib.fhip_atrous_forward_route(ctypes.byref(good), 1, v(0x1000), v(0x2000), v(0x3000), None, v(0x4000), None, AC.dw(1, True).encode()) == UNSUPPORTED


def test_buffer_sizes_and_routes_are_pure_host_calls():
    """No device is needed (this test runs without one), and the packed size depends on the layer alone: not on the batch or the plane."""
    from feathercnn_amd import AtrousConv, AtrousParam
    a = AtrousConv()
    sizes = {a.GetBufferSize(AtrousParam.make(512, 1024, h, d=12, batch=b)) for h in (28, 41) for b in (1, 16)}
    assert sizes == {(0, 4 * 1024 * 512 * 9)}  # DeepLab's fc6: 8 full 128-row panels, no padding
    assert a.GetBufferSize(AtrousParam.make(16, 72, 8, d=2))[1] == 4 * 128 * 16 * 9  # two 64-row panels for 72 channels
    assert a.GetBufferSize(AtrousParam.make(32, 32, 8, d=2, group=32))[1] == 4 * 32 * 9  # depthwise: the filters as they are
    assert a.Route(AtrousParam.make(512, 1024, 40, d=12)) == AC.mfma(AC.BIG, False, True)  # ROW4 applies, and is never selected
    assert a.Route(AtrousParam.make(512, 1024, 41, d=12)) == AC.mfma(AC.BIG, False, True)
    assert a.Route(AtrousParam.make(512, 512, 41, d=2)) == AC.mfma(AC.BIG, False, True)
    assert a.Route(AtrousParam.make(960, 960, 32, d=2, group=960)) == AC.dw(1, True)
    assert not AtrousConv.Supported(AtrousParam(output_channels=8, input_channels=8, input_h=8, input_w=8, kernel_h=3, kernel_w=3, output_h=6, output_w=6,
                                                dilation_h=1, dilation_w=1))


# ---- feather::Net --------------------------------------------------------------------------------------------------------------------
def _one_layer(extra="", type_="Convolution", wsize=16 * 8 * 9, base="0=8 1=3 4=2 5=1"):
    return f"7767517\n2 2\nInput data 0 1 data 0=8 1=8 2=16\n{type_} c 1 1 data c {base} 6={wsize} {extra}\n".encode()


def test_net_refuses_dilation_by_default_and_loads_it_after_the_switch():
    from feathercnn_amd import FeatherHipError
    from feathercnn_amd.net import Net
    for extra in ("2=2", "12=2", "2=2 12=3"):
        with pytest.raises(FeatherHipError) as e:
            Net().LoadParam(_one_layer(extra))  # a default net answers a dilated Convolution line with -200, as it always did
        assert "code -200" in str(e.value) and "dilated" in str(e.value), str(e.value)
        net = Net()
        net.SetDilated(True)
        net.LoadParam(_one_layer(extra))
        assert net.layers()[1] == ("Convolution", "c", "ATROUS")  # reported from LoadParam on
    off = Net()
    off.SetDilated(True)
    off.SetDilated(False)  # off again before LoadParam: the default
    with pytest.raises(FeatherHipError) as e:
        off.LoadParam(_one_layer("2=2"))
    assert "code -200" in str(e.value)
    plain = Net()
    plain.SetDilated(True)
    plain.LoadParam(_one_layer(""))  # dilation 1 keeps its route with the switch on
    assert plain.layers()[1][2] != "ATROUS"
    with pytest.raises(FeatherHipError) as e:
        plain.SetDilated(False)  # after LoadParam the switch is refused
    assert "code -2" in str(e.value) and "before LoadParam" in str(e.value)
    # a dilated Deconvolution stays refused, with or without the switch
    for on in (False, True):
        net = Net()
        net.SetDilated(on)
        with pytest.raises(FeatherHipError) as e:
            net.LoadParam(_one_layer("2=2", "Deconvolution", wsize=16 * 8 * 16, base="0=8 1=4 3=2 4=1 5=1"))
        assert "code -200" in str(e.value), str(e.value)
    # a grouped dilated layer (1 < group < C) is this route's, not gconv's
    gr = Net()
    gr.SetDilated(True)
    gr.LoadParam(_one_layer("2=2 7=4", "ConvolutionDepthWise", wsize=4 * 8 * 9))
    assert gr.layers()[1][2] == "ATROUS"


@pytest.mark.parametrize("name", ["tiny_dilated", "deeplab_largefov", "deeplab_v2_aspp"])
def test_zoo_nets_parse(name):
    from feathercnn_amd import model_zoo
    from feathercnn_amd.net import Net
    if name == "tiny_dilated":
        p, b, _, _ = model_zoo.MODELS[name]()
        assert R.Net(p, b).read == len(b)  # the restatement reads every weight byte ...
    else:
        p, nbytes, _, _ = model_zoo.MODELS[name](dry=True)
        b = None
        assert (20.4e6 if name == "deeplab_largefov" else 37.8e6) < nbytes / 4 < (20.6e6 if name == "deeplab_largefov" else 38.0e6)
    layers = R.shuffle_ref.parse_param(p)
    dilated = [nm for t, nm, _, _, pd in layers if t in ("Convolution", "ConvolutionDepthWise") and R.dilation_of(pd) != (1, 1)]
    assert sorted(dilated) == sorted(model_zoo.DILATED_LAYERS[name])
    for level in (0, 1, 2, 3):
        net = Net(fusion=level)
        net.SetDilated(True)
        net.LoadParam(p)
        if b is not None:
            net.LoadWeights(b)  # ... and so does the runtime (a short or long read is an error)
        routes = {nm: a for _, nm, a in net.layers()}
        assert all(routes[nm] == "ATROUS" for nm in dilated), routes
        assert sum(a == "ATROUS" for a in routes.values()) == len(dilated)
    if b is not None:
        net = Net()
        net.SetDilated(True)
        net.LoadParam(p)
        with pytest.raises(Exception):
            net.LoadWeights(b[:-4])
    rates = {nm: R.dilation_of(pd) for t, nm, _, _, pd in layers if nm in dilated}
    if name == "deeplab_largefov":
        assert rates["fc6"] == (12, 12) and rates["conv5_2"] == (2, 2)
    if name == "deeplab_v2_aspp":
        assert [rates[f"fc6_{j}"][0] for j in (1, 2, 3, 4)] == [6, 12, 18, 24]


def test_restatement_runs_tiny_dilated():
    from feathercnn_amd import model_zoo
    p, b, i, o = model_zoo.tiny_dilated()
    x = np.random.default_rng(3).uniform(-1, 1, (2, 3, 16, 16)).astype(np.float32)
    blobs = R.Net(p, b).run(i, x, o, keep=True)
    shapes = {k: v.shape for k, v in blobs.items()}
    assert shapes["a1"] == (2, 64, 16, 16) and shapes["a3"] == (2, 96, 8, 8) and shapes["a_far"] == (2, 48, 8, 8) and shapes[o] == (2, 8, 4, 4)
    assert all(np.abs(blobs[nm]).max() > 1e-3 for nm in model_zoo.DILATED_LAYERS["tiny_dilated"])  # no layer of the net is dead
