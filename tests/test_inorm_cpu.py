"""libfeather_inorm.so (InstanceNorm and the activations of generative nets) without a GPU.

Checks of the yardstick, which need no library and pass on any tree (test_restatement_against_torch,
test_offset_planes_tell_the_two_variance_forms_apart, test_pixel_round_trip_under_the_parity_bound, the restatement half of
test_relu_with_a_slope_loads_and_is_restated_as_leaky): the fp64 definition the GPU tests compare against (tests/inorm_ref.py) equals
torch's CPU instance_norm / activations in float64; in float32 the two-pass form meets the project's bound on offset planes where
E[x^2] - E[x]^2 misses it.  That a slope is no longer dropped on the device is checked in tests/test_inorm_gpu.py, not here.

Checks of the feature: fhip_instance_norm_route names the instantiation tests/inorm_cases.py states for every case; bad arguments are refused on the host; feather::Net loads the three zoo nets that hold the new layers, consuming every weight byte,
and refuses what the definition leaves out; a ReLU with a slope loads as a ReLU and is restated as the leaky one.  What the library shares with the other run-time libraries -- its exports, the instantiations it holds, its route code, the build
of its application, its last-error state -- is in tests/test_side_contract_cpu.py."""
import ctypes

import numpy as np
import pytest

import inorm_cases as IC
import inorm_ref as R
import side_contract

BADARG = -2
NEW_MODELS = ["tiny_generative", "style_transfer_in", "pix2pix_unet"]


lib = side_contract.fixture("inorm")


# ---- the definition ------------------------------------------------------------------------------------------------------------------
def test_restatement_against_torch():
    import torch
    F = torch.nn.functional
    rng = np.random.default_rng(1)
    worst = 0.0
    for (n, c, h, w), affine, eps in (((2, 3, 8, 8), True, 1e-3), ((3, 5, 7, 7), True, 1e-5), ((1, 4, 1, 1), True, 1e-3), ((2, 6, 13, 9), False, 1e-3),
                                      ((3, 2, 64, 64), True, 0.0), ((1, 1, 1, 5), False, 0.5)):
        x = rng.normal(0.5, 2.0, (n, c, h, w))
        gamma, beta = (rng.uniform(0.5, 1.5, c), rng.uniform(-0.1, 0.1, c)) if affine else (None, None)
        if h * w > 1:
            want = F.instance_norm(torch.from_numpy(x), weight=None if gamma is None else torch.from_numpy(gamma),
                                   bias=None if beta is None else torch.from_numpy(beta), eps=eps).numpy()
        else:  # F.instance_norm refuses a plane of one pixel; the kernel under it (one group per channel) does not
            want = torch.native_group_norm(torch.from_numpy(x), None, None, n, c, 1, c, eps)[0].numpy()
            want = want * gamma.reshape(1, c, 1, 1) + beta.reshape(1, c, 1, 1)
        got = R.instance_norm(x, gamma, beta, eps)
        e = float(np.abs(got - want).max())
        worst = max(worst, e)
        assert e <= 1e-12, ((n, c, h, w), e)
        assert np.abs(R.instance_norm(x, gamma, beta, eps, "relu") - np.maximum(want, 0)).max() <= 1e-12
        assert np.abs(R.instance_norm(x, gamma, beta, eps, "leaky_relu", 0.2) - F.leaky_relu(torch.from_numpy(want), 0.2).numpy()).max() <= 1e-12
    one = R.instance_norm(np.full((1, 2, 1, 1), 3.0), np.array([2.0, 2.0]), np.array([0.25, -0.5]))
    assert np.array_equal(one.reshape(-1), [0.25, -0.5])  # a plane of one pixel: y = beta
    x = np.concatenate([rng.uniform(-20, 20, 1000), [0.0, -0.0, 88.0, -88.0]]).reshape(1, 4, 251)
    t = torch.from_numpy(x)
    s = rng.uniform(0.05, 0.35, 4)
    for got, want in ((R.activation(x, "leaky_relu", 0.2), F.leaky_relu(t, 0.2)), (R.activation(x, "prelu", slopes=s), F.prelu(t, torch.from_numpy(s))),
                      (R.activation(x, "prelu", slope=0.25), F.prelu(t, torch.tensor([0.25], dtype=torch.float64))),
                      (R.activation(x, "sigmoid"), torch.sigmoid(t)), (R.activation(x, "tanh"), torch.tanh(t)),
                      (R.activation(x, "clip", lo=-0.5, hi=0.75), torch.clamp(t, -0.5, 0.75))):
        e = float(np.abs(got - want.numpy()).max())
        worst = max(worst, e)
        assert e <= 1e-12, e
    print(f"inorm_ref vs torch (fp64): worst absolute difference {worst:.2e}")


def test_offset_planes_tell_the_two_variance_forms_apart():
    """Planes of N(+-100, 1) in float32 against float64: the two-pass form stays below the project's 1e-4 with a wide margin, the one-pass
    form E[x^2] - E[x]^2 misses it -- so tests/test_inorm_gpu.py's offset test, at 1e-4, refuses a kernel built on the latter."""
    rng = np.random.default_rng(2)
    for hw in (7, 64, 256):
        for mean in (100.0, -100.0):
            x = rng.normal(mean, 1.0, (2, 3, hw, hw)).astype(np.float32)
            want = R.instance_norm(x, eps=1e-3)
            two = R.plane_nerr(R.instance_norm(x, eps=1e-3, dtype=np.float32), want)
            one = R.plane_nerr(R.instance_norm_one_pass(x, eps=1e-3), want)
            print(f"offset planes {hw}x{hw} mean {mean:+.0f}: two-pass {two:.2e}, one-pass {one:.2e}")
            assert two <= 2e-5 and one >= 5e-4, (hw, mean, two, one)


# ---- the library ---------------------------------------------------------------------------------------------------------------------
def _route(lib, case):
    _, n, c, h, w, offset = case
    name = ctypes.create_string_buffer(96)
    v = ctypes.c_void_p
    assert lib.fhip_instance_norm_route(n, c, h, w, v(0x10000 + 4 * offset), v(0x20000 + 4 * offset), name, 96) == 0
    return name.value.decode()


def test_every_instantiation_has_a_case(lib):
    assert len({c[0] for c in IC.CASES}) == len(IC.CASES) and len({c[0] for c in IC.ACT_CASES}) == len(IC.ACT_CASES)
    for case in IC.CASES:
        _, n, c, h, w, _ = case
        assert _route(lib, case) == IC.instance(case), case[0]
        sb = ctypes.c_size_t(1)
        assert lib.fhip_instance_norm_get_buffer_size(n, c, h, w, ctypes.byref(sb)) == 0
        assert sb.value == IC.scratch_bytes(case), case[0]
    assert {IC.route(c) for c in IC.CASES} == {"wave", "block256", "block1024", "split"}
    assert any(n % 2 and n > 1 for _, n, *_ in IC.CASES)  # batch sizes that are not powers of two


def test_refusals_come_before_any_device_call(lib):
    err = lambda: lib.fhip_inorm_last_error().decode()
    v = ctypes.c_void_p

    def fwd(n=2, c=3, h=8, w=8, out=0x1000, x=0x2000, gamma=0x3000, beta=0x4000, eps=1e-3, act=0, scratch=None):
        return lib.fhip_instance_norm_forward(n, c, h, w, v(out) if out else None, v(x) if x else None, v(gamma), v(beta), eps, act, 0.2,
                                              v(scratch) if scratch else None, None)
    for kw, word in (({"n": 0}, "dimension"), ({"c": 0}, "dimension"), ({"h": -1}, "dimension"), ({"n": 1 << 15, "c": 1 << 10, "h": 8, "w": 8}, "2^31"),
                     ({"out": None}, "null"), ({"x": None}, "null"), ({"out": 0x1002}, "aligned"), ({"gamma": 0x3001}, "aligned"),
                     ({"eps": -1e-3}, "eps"), ({"eps": float("nan")}, "eps"), ({"act": 3}, "activation"),
                     ({"h": 256, "w": 256}, "scratch"), ({"h": 256, "w": 256, "scratch": 0x5004}, "8-byte")):
        assert fwd(**kw) == BADARG and word in err(), (kw, err())

    def forced(route, h, w, scratch=0x5000):
        return lib.fhip_instance_norm_forward_route(route, 2, 3, h, w, v(0x1000), v(0x2000), None, None, 1e-3, 0, 0.0, v(scratch) if scratch else None, None)
    for args, word in (((4, 8, 8), "route"), ((-1, 8, 8), "route"), ((0, 33, 32), "fit"), ((1, 65, 64), "fit"), ((2, 129, 128), "fit"),
                       ((3, 8, 8, None), "scratch")):
        assert forced(*args) == BADARG and word in err(), (args, err())
    sb = ctypes.c_size_t()
    assert lib.fhip_instance_norm_get_buffer_size(1, 1, 0, 1, ctypes.byref(sb)) == BADARG
    assert lib.fhip_instance_norm_get_buffer_size(1, 1, 1, 1, None) == BADARG
    assert lib.fhip_instance_norm_route(1, 1, 1, 1, None, None, None, 96) == BADARG

    def act(kind=0, out=0x1000, x=0x2000, n=2, c=3, hw=64, p0=0.1, p1=0.0, slopes=None):
        return lib.fhip_activation_forward(kind, v(out) if out else None, v(x) if x else None, n, c, hw, p0, p1, v(slopes) if slopes else None, None)
    for kw, word in (({"kind": 5}, "kind"), ({"kind": -1}, "kind"), ({"out": None}, "null"), ({"x": 0x2002}, "aligned"), ({"hw": 0}, "dimension"),
                     ({"kind": 4, "p0": 1.0, "p1": -1.0}, "min <= max"), ({"kind": 1, "slopes": 0x3002}, "aligned")):
        assert act(**kw) == BADARG and word in err(), (kw, err())


# ---- feather::Net --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NEW_MODELS)
def test_net_loads_the_generative_nets(name):
    from feathercnn_amd import model_zoo
    from feathercnn_amd.net import Net
    p, b, _, _ = model_zoo.MODELS[name]()
    layers = R.gconv_ref.parse_param(p)
    assert R.Net(p, b).read == len(b)  # the restatement reads every weight byte ...
    norms = [nm for t, nm, _, _, _ in layers if t == "InstanceNorm"]
    assert norms and any(t == "TanH" for t, *_ in layers)
    if name != "style_transfer_in":  # Johnson's net has plain ReLUs only
        assert any(t == "ReLU" and pd.get(0, 0.0) for t, _, _, _, pd in layers)
    if name == "tiny_generative":
        assert {"InstanceNorm", "PReLU", "Sigmoid", "TanH", "Clip", "ReLU"} <= {t for t, *_ in layers}
    for level in (0, 1, 2, 3):
        net = Net(fusion=level)
        net.LoadParam(p)
        net.LoadWeights(b)  # ... and so does the runtime, in the same order (a short read is an error)
        got = net.layers()
        assert [(t, nm) for t, nm, _ in got] == [(t, nm) for t, nm, _, _, _ in layers]
        assert [nm for _, nm, a in got if a == "INORM"] == norms
    net = Net()
    net.LoadParam(p)
    with pytest.raises(Exception):
        net.LoadWeights(b[:-4])


def test_existing_zoo_models_are_byte_identical_builders():
    """GraphBuilder.relu without a slope writes what it always wrote: no params."""
    from feathercnn_amd import model_zoo
    g = model_zoo.GraphBuilder(1)
    g.input("data", 3, 8, 8)
    g.relu("r", "data")
    g.relu("l", "r", slope=0.2)
    assert g.lines[1] == "ReLU r 1 1 data r" and g.lines[2] == "ReLU l 1 1 r l 0=0.200000"


def _one(line, c=8):
    return f"7767517\n2 2\nInput data 0 1 data 0=8 1=8 2={c}\n{line}\n".encode()


@pytest.mark.parametrize("line,code", [("InstanceNorm n 1 1 data n 0=0", -100), ("InstanceNorm n 1 1 data n 0=-8", -100), ("InstanceNorm n 1 1 data n", -100),
                                       ("InstanceNorm n 1 1 data n 0=8 1=-1.0e-3", -100), ("PReLU n 1 1 data n 0=0", -100),
                                       ("Clip n 1 1 data n 0=1.0 1=-1.0", -100), ("HardSwish n 1 1 data n", -200), ("Interp n 1 1 data n", -200)])
def test_load_param_refuses_what_the_definition_leaves_out(line, code):
    from feathercnn_amd import FeatherHipError
    from feathercnn_amd.net import Net
    net = Net()
    with pytest.raises(FeatherHipError) as e:
        net.LoadParam(_one(line))
    assert f"code {code}" in str(e.value), str(e.value)


def test_load_param_accepts_the_new_layers():
    from feathercnn_amd.net import Net
    for line, want in (("InstanceNorm n 1 1 data n 0=8", ("InstanceNorm", "n", "INORM")), ("InstanceNorm n 1 1 data n 0=8 1=0.0 2=0", ("InstanceNorm", "n", "INORM")),
                       ("PReLU n 1 1 data n 0=1", ("PReLU", "n", None)), ("PReLU n 1 1 data n 0=8", ("PReLU", "n", None)),
                       ("Sigmoid n 1 1 data n", ("Sigmoid", "n", None)), ("TanH n 1 1 data n", ("TanH", "n", None)),
                       ("Clip n 1 1 data n 0=0.0 1=6.0", ("Clip", "n", None)), ("Clip n 1 1 data n", ("Clip", "n", None))):
        net = Net()
        net.LoadParam(_one(line))
        assert net.layers()[1] == want, line
    # affine = 0 reads no weights, affine reads 2 * channels floats
    net = Net()
    net.LoadParam(_one("InstanceNorm n 1 1 data n 0=8 2=0"))
    net.LoadWeights(b"")
    net = Net()
    net.LoadParam(_one("InstanceNorm n 1 1 data n 0=8"))
    net.LoadWeights(np.ones(16, np.float32).tobytes())
    with pytest.raises(Exception):
        net2 = Net()
        net2.LoadParam(_one("InstanceNorm n 1 1 data n 0=8"))
        net2.LoadWeights(np.ones(15, np.float32).tobytes())


def test_relu_with_a_slope_loads_and_is_restated_as_leaky():
    from feathercnn_amd.net import Net
    param = _one("ReLU r 1 1 data r 0=0.2")
    net = Net()
    net.LoadParam(param)
    assert net.layers()[1] == ("ReLU", "r", None)
    x = np.linspace(-2, 2, 2 * 8 * 8 * 8, dtype=np.float32).reshape(2, 8, 8, 8)
    y = R.Net(param, b"").run("data", x, "r")
    assert np.array_equal(y, np.where(x > 0, x, (x.astype(np.float64) * np.float64(np.float32(0.2)))).astype(np.float32))
    assert (y[x < 0] < 0).all()
    plain = R.Net(_one("ReLU r 1 1 data r"), b"").run("data", x, "r")
    assert np.array_equal(plain, np.maximum(x, 0))


def test_pixel_round_trip_under_the_parity_bound():
    """The seeded input of tests/test_inorm_gpu.py's FeedPixels -> style_transfer_in -> ExtractPixels test, on the host, with the restatement's
    output shifted by the whole parity bound (1e-4 of its peak) in either direction: no byte changes by more than 1.  The share of bytes
    that change is 1e-4 * 127.5 = 1.3 % of a quantisation step by arithmetic (measured here: 1.33 %), which is MORE than the 0.5 % the GPU
    test allows: that cap is met only by a blob error below 0.005 / 127.5 = 3.9e-5 of the peak, so it is the tighter of the two checks, not
    a consequence of the 1e-4 bound.  It is kept as it stands; at 3e-5 the share must be inside it."""
    from feathercnn_amd import model_zoo
    param, weights, i, o = model_zoo.style_transfer_in()
    _, x = R.pixel_input()
    want = R.Net(param, weights).run(i, x, o)
    peak = float(np.abs(want).max())
    assert peak <= 1.0  # TanH
    base = R.pixel_output(want)
    assert base.shape == (2, R.PIXEL_SIZE, R.PIXEL_SIZE, 3) and base.dtype == np.uint8
    for bound, cap in ((1e-4, 2 * 1e-4 * 127.5), (3e-5, R.PIXEL_CAP)):
        worst_frac, worst_diff = 0.0, 0
        for sign in (1.0, -1.0):
            moved = R.pixel_output((want.astype(np.float64) + sign * bound * peak).astype(np.float32))
            d = np.abs(moved.astype(np.int32) - base.astype(np.int32))
            worst_frac, worst_diff = max(worst_frac, float((d != 0).mean())), max(worst_diff, int(d.max()))
        print(f"pixel round trip under a uniform {bound:.0e} shift: {100 * worst_frac:.3f} % of bytes change, by at most {worst_diff}; "
              f"output range {base.min()} .. {base.max()}")
        assert worst_diff <= 1 and worst_frac <= cap, (bound, worst_frac, worst_diff)
