"""libfeather_resample.so (Interp: nearest / bilinear resize; HardSwish) without a GPU.

Checks of the yardstick, which need no library: the float64 restatement the GPU tests compare against (tests/resample_ref.py) equals
torch.nn.functional.interpolate on every bilinear row of tests/resample_cases.py and torch's `nearest` on the integer scales, the float32
restatement (the bit-for-bit yardstick) stays within float32 rounding of it, and it runs tiny_resample.

Checks of the feature (every one fails on the parent commit, where there is no library, no switch and no builder): fhip_interp_route selects the
instantiation the header states for every row, offset and mode; bad arguments are refused on the host with their word; feather::Net
refuses both types by default and names the switch, loads them with route RESAMPLE after SetExtendedLayers, and answers every hostile
param line with its code and a message; fusion level 2 collapses the one upsample-add-ReLU of tiny_resample and leaves the Interp with
two readers alone; the zoo nets load at every level.  What the library shares with the other run-time libraries -- its exports, the instantiations it holds, its route code, the build
of its application, its last-error state -- is in tests/test_side_contract_cpu.py.

Hostile param lines are this file's duty for the two types: create_layer does not hold them, so tests/loader_cases.py and
tests/seam_cases.py are silent about them (the seams: tests/test_resample_seams_cpu.py)."""
import ctypes

import numpy as np
import pytest

import resample_cases as RC
import resample_ref as R
import side_contract

BADARG = -2
NEW_MODELS = ["tiny_resample", "mobilenet_v3_large", "mobilenet_v3_small", "deeplab_largefov_full", "unet_bilinear", "fpn_resnet50"]


lib = side_contract.fixture("resample")


# ---- the definition ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("align", [False, True])
def test_float64_restatement_against_torch_bilinear(align):
    """Bound: 4 * 2^-24 * max(in_h, in_w) * max|x| -- the definition rounds each source position once to float32 (an error of up to half
    an ulp of a value below max(in_h, in_w)), torch keeps it in float64; a coefficient error e moves an output by at most 2 e max|x| per
    axis."""
    import torch
    import torch.nn.functional as F
    rng = np.random.default_rng(5)
    worst = 0.0
    for i, o in RC.PLANES:
        x = rng.standard_normal((2, 3) + i)
        got = R.interp(x, R.BILINEAR, o[0], o[1], align, dtype=np.float64)
        want = F.interpolate(torch.from_numpy(x), size=o, mode="bilinear", align_corners=align).numpy()
        bound = 4 * 2.0 ** -24 * max(i) * np.abs(x).max()
        e = float(np.abs(got - want).max())
        worst = max(worst, e / bound)
        assert got.shape == want.shape and e <= bound, (i, o, align, e, bound)
    print(f"resample_ref bilinear (align_corner={align}) vs torch float64: worst error / bound = {worst:.3f}")


def test_nearest_restatement_against_torch_on_integer_scales():
    import torch
    import torch.nn.functional as F
    assert len(RC.INTEGER_SCALES) >= 8
    rng = np.random.default_rng(6)
    for i, o in RC.INTEGER_SCALES:
        x = rng.standard_normal((2, 3) + i).astype(np.float32)
        want = F.interpolate(torch.from_numpy(x), size=o, mode="nearest").numpy()
        assert np.array_equal(R.interp(x, R.NEAREST, o[0], o[1]), want), (i, o)  # the size given: hs = in / (float)out
        hs, ws = RC.by_scale(i, o)
        assert R.output_dim(i[0], i[1], hs, ws) == o
        assert np.array_equal(R.interp(x, R.NEAREST, o[0], o[1], height_scale=hs, width_scale=ws), want), (i, o)  # hs = 1 / scale


def test_float32_restatement_is_the_float64_one_rounded():
    rng = np.random.default_rng(7)
    for mode, align, i, o, by in RC.cases():
        x = rng.standard_normal((2, 3) + i).astype(np.float32)
        res = rng.standard_normal((2, 3) + o).astype(np.float32)
        hs, ws = RC.by_scale(i, o) if by == "scale" else (0.0, 0.0)
        for kw in ({}, {"residual": res}, {"residual": res, "relu": True}):
            a = R.interp(x, mode, o[0], o[1], bool(align), hs, ws, dtype=np.float32, **kw)
            b = R.interp(x, mode, o[0], o[1], bool(align), hs, ws, dtype=np.float64, **kw)
            assert a.dtype == np.float32 and a.shape == (2, 3) + o
            assert np.abs(a - b).max() <= 1e-6 * max(np.abs(b).max(), np.abs(x).max()), (mode, align, i, o, by)
            if mode == R.NEAREST and not kw:
                assert np.array_equal(a, b.astype(np.float32))
    x = np.linspace(-8, 8, 4001, dtype=np.float32)
    for alpha, beta in RC.HARDSWISH_PARAMS:
        a, b = R.hard_swish(x, alpha, beta, np.float32), R.hard_swish(x, alpha, beta, np.float64)
        assert np.abs(a - b).max() <= 1e-6 * np.abs(b).max()


def test_hard_swish_restatement_against_torch():
    import torch
    import torch.nn.functional as F
    x = np.linspace(-6, 6, 2401)
    got = R.hard_swish(x, 1.0 / 6, 0.5, np.float64)
    want = F.hardswish(torch.from_numpy(x)).numpy()
    # alpha is handed to the library as the float32 nearest 1 / 6 (relative error below 2^-24): the restatement follows it
    assert np.abs(got - want).max() <= 36 * 2.0 ** -24
    assert np.array_equal(R.hard_swish(np.float32([-3, -2.5, 0, 2.5, 3]), 0.2, 0.5), np.float32([0, -0.0, 0, 2.5, 3]))
    assert np.array_equal(R.hard_swish(np.float32([-4, -3, 3, 4]), 1.0 / 6, 0.5)[[0, 3]], np.float32([0, 4]))


def test_restatement_runs_tiny_resample():
    from feathercnn_amd import model_zoo
    p, b, i, o = model_zoo.tiny_resample()
    ref = R.Net(p, b)
    assert ref.read == len(b)
    for size, want in ((24, {"up1": (12, 12), "up2": (24, 24), "shrink": (5, 7), "aligned": (9, 13), "to_ref": (9, 13), "down": (5, 5)}),
                       (20, {"up1": (10, 10), "up2": (20, 20), "shrink": (4, 6), "aligned": (7, 11), "to_ref": (7, 11), "down": (5, 5)})):
        x = np.random.default_rng(3).uniform(-1, 1, (2, 3, size, size)).astype(np.float32)
        blobs = ref.run(i, x, o, keep=True)
        assert {k: blobs[k].shape[2:] for k in want} == want
        assert np.allclose(blobs["prob"].reshape(2, -1).sum(axis=1), 1.0, atol=1e-5)
        assert all(np.abs(blobs[k]).max() > 1e-3 for k in want)  # no layer of the net is dead
        # the layers under test from their inputs: nearest is a copy, the fused chain is the three layers
        assert np.array_equal(blobs["up1"], R.interp(blobs["relu3"], R.NEAREST, *want["up1"], height_scale=2.0, width_scale=2.0))
        assert np.array_equal(blobs["sum1_relu"], R.interp(blobs["relu3"], R.NEAREST, *want["up1"], height_scale=2.0, width_scale=2.0,
                                                           residual=blobs["lat"], relu=True))
        assert (blobs["hs1"] < 0).any() and (blobs["hs2"] < 0).any()  # HardSwish is not a ReLU


# ---- the library ---------------------------------------------------------------------------------------------------------------------
def test_instantiations_and_route_names(lib):
    name = ctypes.create_string_buffer(96)
    v = ctypes.c_void_p
    seen = set()
    for mode, _, i, o, by in RC.cases():
        hs, ws = RC.by_scale(i, o) if by == "scale" else (0.0, 0.0)
        for off in RC.OFFSETS:
            for which in range(3):  # the pointer that is moved: out, in, residual
                offs = [off if which == k else 0 for k in range(3)]
                ptrs = [v(0x10000 * (k + 1) + 4 * offs[k]) for k in range(3)]
                assert lib.fhip_interp_route(mode, 2, 3, i[0], i[1], o[0], o[1], hs, ws, *ptrs, name, 96) == 0
                want = RC.expected_route(mode, i, o, hs, ws, *offs)
                assert name.value.decode() == want, (mode, i, o, by, off, which, name.value.decode())
                seen.add(want)
        assert lib.fhip_interp_route(mode, 2, 3, i[0], i[1], o[0], o[1], hs, ws, v(0x10000), v(0x20000), None, name, 96) == 0
        assert name.value.decode() == RC.expected_route(mode, i, o, hs, ws)  # no residual: NULL counts as aligned
    # the 16-byte paths only where width and pointers allow
    assert lib.fhip_interp_route(1, 1, 1, 4, 4, 8, 8, 0.0, 0.0, v(0x10000), v(0x20000), None, name, 96) == 0 and name.value.decode() == "fhip::interp_nearest2x_kernel"
    assert lib.fhip_interp_route(1, 1, 1, 4, 4, 8, 8, 0.0, 0.0, v(0x10000), v(0x20004), None, name, 96) == 0 and name.value.decode() == "fhip::interp_vec4_kernel<1>"
    assert lib.fhip_interp_route(1, 1, 1, 4, 4, 8, 8, 0.0, 0.0, v(0x10008), v(0x20000), None, name, 96) == 0 and name.value.decode() == "fhip::interp_gather_kernel<1>"
    assert lib.fhip_interp_route(1, 1, 1, 3, 3, 6, 6, 2.0, 2.0, v(0x10000), v(0x20000), None, name, 96) == 0 and name.value.decode() == "fhip::interp_gather_kernel<1>"
    for count, off in ((8, 0), (8, 1), (7, 0)):
        assert lib.fhip_hardswish_route(v(0x10000 + 4 * off), v(0x20000), 1, 1, count, name, 96) == 0
        assert name.value.decode() == f"fhip::hardswish_kernel<{'true' if count % 4 == 0 and off == 0 else 'false'}>"
        seen.add(name.value.decode())
    assert seen == RC.targets()  # the table's rows reach every instantiation the library holds
    assert lib.fhip_interp_route(3, 2, 3, 4, 4, 8, 8, 0.0, 0.0, None, None, None, name, 96) == BADARG and "resize_type 3" in lib.fhip_resample_last_error().decode()


def test_output_dim(lib):
    h, w = ctypes.c_int(), ctypes.c_int()
    dim = lambda *a: (lib.fhip_interp_output_dim(*a, ctypes.byref(h), ctypes.byref(w)), h.value, w.value)
    assert dim(12, 12, 0.45, 0.6, 0, 0) == (0, 5, 7) and dim(12, 12, 0.75, 1.1, 0, 0) == (0, 9, 13)
    assert dim(12, 12, 2.0, 2.0, 5, 0) == (0, 5, 24) and dim(12, 12, float("nan"), -1.0, 5, 7) == (0, 5, 7)  # a scale that is not used is not looked at
    for i, o in RC.PLANES:
        hs, ws = RC.by_scale(i, o)
        assert dim(i[0], i[1], hs, ws, 0, 0) == (0,) + o
    err = lambda: lib.fhip_resample_last_error().decode()
    for args, word in (((0, 4, 1.0, 1.0, 0, 0), "dimension"), ((4, 4, float("nan"), 1.0, 0, 0), "finite"), ((4, 4, 1.0, float("inf"), 0, 0), "finite"),
                       ((4, 4, 0.0, 1.0, 0, 0), "positive"), ((4, 4, -2.0, 1.0, 0, 0), "positive"), ((4, 4, 0.1, 1.0, 0, 0), "below 1"),
                       ((4, 4, 1.0, 1e9, 0, 0), "2^31"), ((4, 4, 1.0, 1.0, -3, 0), "at least 1"), ((4, 4, 1.0, 1.0, 0, -1), "at least 1")):
        assert dim(*args)[0] == BADARG and word in err(), (args, err())
    assert lib.fhip_interp_output_dim(4, 4, 1.0, 1.0, 0, 0, None, ctypes.byref(w)) == BADARG and "null" in err()


def test_refusals_come_before_any_device_call(lib):
    err = lambda: lib.fhip_resample_last_error().decode()
    v = lambda p: ctypes.c_void_p(p) if p else None
    nan, inf = float("nan"), float("inf")

    def interp(mode=2, align=0, n=2, c=3, ih=4, iw=4, oh=8, ow=8, hs=0.0, ws=0.0, out=0x100000, x=0x200000, res=0x300000, relu=0):
        return lib.fhip_interp_forward(mode, align, n, c, ih, iw, oh, ow, hs, ws, v(out), v(x), v(res), relu, None)
    for kw, word in (({"mode": 0}, "resize_type 0"), ({"mode": 3}, "resize_type 3"), ({"mode": -1}, "resize_type"), ({"n": 0}, "dimension"), ({"c": 0}, "dimension"),
                     ({"ih": 0}, "dimension"), ({"iw": -1}, "dimension"), ({"oh": 0}, "dimension"), ({"ow": 0}, "dimension"),
                     ({"n": 1 << 15, "c": 1 << 10, "ih": 8, "iw": 8, "oh": 1, "ow": 1}, "2^31"), ({"n": 1 << 15, "c": 1 << 10, "oh": 8, "ow": 8}, "2^31"),
                     ({"out": None}, "null"), ({"x": None}, "null"), ({"out": 0x100002}, "aligned"), ({"x": 0x200001}, "aligned"), ({"res": 0x300003}, "aligned"),
                     ({"hs": nan}, "scale"), ({"ws": inf}, "scale"), ({"hs": -2.0}, "scale"), ({"relu": 2}, "relu"),
                     ({"out": 0x200000}, "overlap"), ({"out": 0x200000 + 4 * (2 * 3 * 4 * 4 - 1)}, "overlap"), ({"x": 0x100000 + 4 * (2 * 3 * 8 * 8 - 1)}, "overlap")):
        assert interp(**kw) == BADARG and word in err(), (kw, err())

    def hs(out=0x1000, x=0x2000, n=2, c=3, hw=8, alpha=0.2, beta=0.5):
        return lib.fhip_hardswish_forward(v(out), v(x), n, c, hw, alpha, beta, None)
    for kw, word in (({"out": None}, "null"), ({"x": None}, "null"), ({"x": 0x2002}, "aligned"), ({"out": 0x1001}, "aligned"), ({"n": 0}, "dimension"),
                     ({"hw": 0}, "dimension"), ({"n": 1 << 15, "c": 1 << 10, "hw": 64}, "2^31"), ({"alpha": inf}, "finite"), ({"alpha": nan}, "finite"),
                     ({"beta": nan}, "finite"), ({"beta": -inf}, "finite"), ({"alpha": 0.0}, "zero")):
        assert hs(**kw) == BADARG and word in err(), (kw, err())
    name = ctypes.create_string_buffer(8)
    assert lib.fhip_hardswish_route(None, None, 1, 1, 4, None, 8) == BADARG and "null" in err()
    assert lib.fhip_interp_route(1, 1, 1, 4, 4, 8, 8, 0.0, 0.0, None, None, None, name, 0) == BADARG and "null" in err()


# ---- feather::Net --------------------------------------------------------------------------------------------------------------------
def _two(line, blobs=6):
    """An input [8][8][8], its global average and one more layer."""
    return f"7767517\n3 {blobs}\nInput data 0 1 data 0=8 1=8 2=8\nPooling gap 1 1 data gap 0=1 4=1\n{line}\n".encode()


def _load(line, extended=True):
    from feathercnn_amd.net import Net
    net = Net()
    if extended:
        net.SetExtendedLayers(True)
    net.LoadParam(_two(line))
    return net


def _refused(line, extended=True):
    from feathercnn_amd import FeatherHipError
    with pytest.raises(FeatherHipError) as e:
        _load(line, extended)
    return str(e.value)


def test_a_default_net_refuses_both_types_and_names_the_switch():
    from feathercnn_amd import FeatherHipError
    from feathercnn_amd.net import Net
    for line, type_ in (("Interp m 1 1 data m 0=2", "Interp"), ("HardSwish m 1 1 data m", "HardSwish"), ("Interp m 2 1 data gap m 0=1", "Interp")):
        msg = _refused(line, extended=False)
        assert "code -200" in msg and type_ in msg and "fhip_net_set_extended_layers" in msg, msg
    net = Net()
    net.SetExtendedLayers(True)
    net.SetExtendedLayers(False)  # on then off equals the default
    with pytest.raises(FeatherHipError) as e:
        net.LoadParam(_two("HardSwish m 1 1 data m"))
    assert "code -200" in str(e.value) and "fhip_net_set_extended_layers" in str(e.value)
    msg = _refused("PixelShuffle m 1 1 data m 0=2", extended=False)
    assert "code -200" in msg and "fhip_net_set_extended_layers" not in msg  # the switch does not lift this one, so the message does not offer it


def test_load_param_accepts_the_new_layers():
    for line, want in (("Interp m 1 1 data m 0=2", ("Interp", "m", "RESAMPLE")), ("Interp m 1 1 data m 0=1 1=2.0 2=2.0", ("Interp", "m", "RESAMPLE")),
                       ("Interp m 1 1 data m 0=2 3=5 4=7 6=1", ("Interp", "m", "RESAMPLE")), ("Interp m 2 1 data gap m 0=2", ("Interp", "m", "RESAMPLE")),
                       ("Interp m 2 1 gap data m 0=1", ("Interp", "m", "RESAMPLE")), ("Interp m 1 1 data m 0=2 5=0", ("Interp", "m", "RESAMPLE")),
                       ("HardSwish m 1 1 data m", ("HardSwish", "m", "RESAMPLE")), ("HardSwish m 1 1 data m 0=0.166667 1=0.5", ("HardSwish", "m", "RESAMPLE"))):
        net = _load(line)
        assert net.layers()[2] == want, line
        net.LoadWeights(b"")  # neither has weights
    # the older types load as before with the switch on
    assert _load("HardSigmoid m 1 1 data m").layers()[2] == ("HardSigmoid", "m", "GATE")
    assert _load("ReLU m 1 1 data m").layers()[2] == ("ReLU", "m", None)


def test_the_switch_is_refused_after_load_param():
    from feathercnn_amd import FeatherHipError
    from feathercnn_amd.net import Net
    for first in (False, True):
        net = Net()
        if first:
            net.SetExtendedLayers(True)
        net.LoadParam(_two("HardSwish m 1 1 data m" if first else "ReLU m 1 1 data m"))
        for on in (True, False):
            with pytest.raises(FeatherHipError) as e:
                net.SetExtendedLayers(on)
            assert "code -2" in str(e.value) and "before LoadParam" in str(e.value)


# A param value is stored as ncnn stores it: a token with '.', 'e' or 'E' is a float, any other token goes through atoi ("nan" and "inf" are
# 0), and the reader takes the 32 bits as the type it wants: the int -1 and 2147483647 are NaNs to a float reader, the float 1e30 is the int
# 1900671690 to an int reader and nan.0 the int 2143289344.
OK = None
HOSTILE_VALUES = ("-1", "0", "2147483647", "nan", "inf", "-1.5", "0.0", "1e30", "nan.0", "inf.0")
HOSTILE = {
    # Interp 0 = resize_type: nothing but 1 and 2
    ("Interp", 0): dict.fromkeys(HOSTILE_VALUES, "resize_type"),
    # 1 / 2 = scales (the size is not given): finite, positive, below 2^31
    ("Interp", 1): {**dict.fromkeys(HOSTILE_VALUES, "scale"), "1e30": "2^31"},
    ("Interp", 2): {**dict.fromkeys(HOSTILE_VALUES, "scale"), "1e30": "2^31"},
    # 3 / 4 = output size: 0 is "not given"; one huge extent alone is below 2^31 elements and is left to Reshape, which knows n and c
    ("Interp", 3): {"-1": "at least 1", "0": OK, "2147483647": OK, "nan": OK, "inf": OK, "-1.5": "at least 1", "0.0": OK, "1e30": OK, "nan.0": OK, "inf.0": OK},
    ("Interp", 4): {"-1": "at least 1", "0": OK, "2147483647": OK, "nan": OK, "inf": OK, "-1.5": "at least 1", "0.0": OK, "1e30": OK, "nan.0": OK, "inf.0": OK},
    # 5 = dynamic_target_size: refused unless 0
    ("Interp", 5): {"-1": "dynamic", "0": OK, "2147483647": "dynamic", "nan": OK, "inf": OK, "-1.5": "dynamic", "0.0": OK, "1e30": "dynamic", "nan.0": "dynamic",
                    "inf.0": "dynamic"},
    # 6 = align_corner: a flag, any value
    ("Interp", 6): dict.fromkeys(HOSTILE_VALUES, OK),
    # HardSwish 0 = alpha: finite and not zero; 1 = beta: finite
    ("HardSwish", 0): {"-1": "finite", "0": "finite", "2147483647": "finite", "nan": "finite", "inf": "finite", "-1.5": OK, "0.0": "finite", "1e30": OK,
                       "nan.0": "finite", "inf.0": "finite"},
    ("HardSwish", 1): {"-1": "finite", "0": OK, "2147483647": "finite", "nan": OK, "inf": OK, "-1.5": OK, "0.0": OK, "1e30": OK, "nan.0": "finite", "inf.0": "finite"},
}


@pytest.mark.parametrize("type_,pid", sorted(HOSTILE))
def test_hostile_param_values(type_, pid):
    """Every id of both types with negative, zero, huge, NaN and inf values: accepted where the definition gives the value a meaning, else
    -100 with a message that names the layer; nothing crashes."""
    for value, word in HOSTILE[(type_, pid)].items():
        base = "0=2 " if type_ == "Interp" and pid != 0 else ""
        line = f"{type_} m 1 1 data m {base}{pid}={value}"
        if word is OK:
            assert _load(line).layers()[2] == (type_, "m", "RESAMPLE"), line
        else:
            msg = _refused(line)
            assert "code -100" in msg and "layer m" in msg and word in msg, (line, msg)


@pytest.mark.parametrize("line,code,word", [("Interp m 3 1 data gap gap m 0=2", -100, "one or two bottoms"), ("Interp m 1 2 data m m2 0=2", -100, "one top"),
                                            ("Interp m 0 1 m 0=2", -300, "0 bottoms"), ("HardSwish m 2 1 data gap m", -100, "one bottom"),
                                            ("HardSwish m 1 2 data m m2", -100, "one top"), ("HardSwish m 0 1 m", -300, "0 bottoms"),
                                            ("Interp m 1 1 data m 0=2 3=65536 4=32768", -100, "2^31"), ("Interp m 1 1 data m 0=1 3=46341 4=46341", -100, "2^31"),
                                            ("Interp m 1 1 data m 0=2 3=2147483647 4=2147483647", -100, "2^31"),
                                            ("Interp m 1 1 data m 0=2 1=3e9 2=1.0", -100, "2^31"), ("Interp m 1 1 data m 0=2 1=1e39", -100, "scale"),
                                            ("Interp m 1 1 data m 0=3", -100, "bicubic"), ("Interp m 2 1 data gap m 0=3", -100, "bicubic"),
                                            ("Interp m 1 1 data m", -100, "resize_type 0"), ("Interp m 1 1 data m 0=2 5=1", -100, "dynamic_target_size 1"),
                                            ("PixelShuffle m 1 1 data m 0=2", -200, "PixelShuffle"), ("Padding m 1 1 data m 0=1", -200, "Padding"),
                                            ("Interp m 1 1 nowhere m 0=2", -300, "nowhere"), ("HardSwish m 1 1 data m 40=1.0", -2, "out of range")])
def test_load_param_refuses_with_the_switch_on(line, code, word):
    msg = _refused(line)
    assert f"code {code}" in msg and word in msg, msg


def _fused_layers(param, weights, level, dilated=False, keep_net=False):
    """The layer list after the fusion pass: Forward runs it first and then stops at the input that has not been fed."""
    from feathercnn_amd import FeatherHipError
    from feathercnn_amd.net import Net
    net = Net(fusion=level)
    net.SetExtendedLayers(True)
    if dilated:
        net.SetDilated(True)
    net.LoadParam(param)
    net.LoadWeights(weights)
    with pytest.raises(FeatherHipError, match="has not been fed"):
        net.Forward()
    return net if keep_net else net.layers()


def test_fusion_2_collapses_the_upsample_add_of_tiny_resample():
    from feathercnn_amd import model_zoo
    p, b, _, _ = model_zoo.tiny_resample()
    every = [nm for _, nm, *_ in R.shuffle_ref.parse_param(p)]
    collapse, keep = model_zoo.UPSAMPLE_ADDS["tiny_resample"]
    for level in (0, 1):
        got = _fused_layers(p, b, level)
        routes = {nm: (t, a) for t, nm, a in got}
        assert all(routes[nm] == ("Interp", "RESAMPLE") for nm in collapse + keep) and routes["hs1"] == routes["hs2"] == ("HardSwish", "RESAMPLE")
        assert routes["sum1"] == ("Eltwise", None) and ("sum1_relu" in routes) == (level == 0)  # level 1: the pairwise pass gave the ReLU to the Eltwise
        assert [nm for _, nm, _ in got] == [nm for nm in every if nm in routes]
    for level in (2, 3):
        net = _fused_layers(p, b, level, keep_net=True)
        got = net.layers()
        names = [nm for _, nm, _ in got]
        routes = {nm: (t, a) for t, nm, a in got}
        assert routes["up1"] == ("Interp", "RESAMPLE") and "sum1" not in names and "sum1_relu" not in names  # the chain is one layer ...
        assert names.index("up1") > names.index("lat")  # ... that stands where its last layer stood: behind the operand it adds
        assert names.index("up1") < names.index("split2")
        # the Interp with two readers stays as written, and so do those with no Eltwise behind them.  (sum2 is gone all the same: big_pw, the
        # convolution that produces its other operand, takes it into its epilogue by the older rule, with the blob up2 as the residual.)
        assert all(routes[nm] == ("Interp", "RESAMPLE") for nm in keep)
        assert "sum2" not in names and list(net.residuals()) == [names.index("big_pw")]
        from feathercnn_amd import FeatherHipError
        for blob, inside in (("up1", True), ("sum1", True), ("sum1_relu", False), ("up2", False), ("to_ref", False)):
            if inside:  # a blob inside the collapsed chain refuses Extract as the SE block's do
                with pytest.raises(FeatherHipError, match="fused into its consumer"):
                    net.ExtractDevice(blob)
            else:
                net.ExtractDevice(blob)
        assert sum(a == "RESAMPLE" for _, _, a in got) == 8
        rest = [nm for nm in names if nm != "up1"]
        assert rest == [nm for nm in every if nm in rest]  # nothing else moved


def test_fusion_2_collapses_the_top_down_path_of_fpn():
    from feathercnn_amd import model_zoo
    p, b, _, _ = model_zoo.fpn_resnet50(size=64)
    collapse, _ = model_zoo.UPSAMPLE_ADDS["fpn_resnet50"]
    got0 = {nm: (t, a) for t, nm, a in _fused_layers(p, b, 0)}
    assert all(got0[nm] == ("Interp", "RESAMPLE") for nm in collapse) and all(f"fpn_sum{k}" in got0 for k in (4, 3, 2))
    got = _fused_layers(p, b, 2)
    names = [nm for _, nm, _ in got]
    assert all(nm in names for nm in collapse) and not any(f"fpn_sum{k}" in names for k in (4, 3, 2))
    for k in (4, 3, 2):
        assert names.index(f"fpn_lat{k}") < names.index(f"fpn_up{k}") < names.index(f"fpn_p{k}")


@pytest.mark.parametrize("change,why", [(("Eltwise sum1 2 1 lat up1 sum1 0=1", "Concat sum1 2 1 lat up1 sum1 0=0"), "no Eltwise behind the Interp"),
                                        (("Eltwise sum1 2 1 lat up1 sum1 0=1", "Eltwise sum1 2 1 up1 up1 sum1 0=1"), "an Eltwise that reads the top twice")])
def test_chains_that_do_not_match_stay_layer_by_layer(change, why):
    from feathercnn_amd import model_zoo
    p, b, _, _ = model_zoo.tiny_resample()
    old, new = change
    assert old.encode() in p
    q = p.replace(old.encode(), new.encode())  # only the layer list is looked at: the shapes behind the changed layer do not matter
    names = {nm: (t, a) for t, nm, a in _fused_layers(q, b, 2)}
    assert "sum1" in names and names["up1"] == ("Interp", "RESAMPLE"), why


@pytest.mark.parametrize("name", NEW_MODELS)
def test_net_loads_the_new_nets(name):
    from feathercnn_amd import model_zoo
    from feathercnn_amd.net import Net
    assert name in model_zoo.EXTENDED_NETS
    kw = {} if name == "tiny_resample" else {"size": 64}
    p, b, i, o = model_zoo.MODELS[name](**kw)
    layers = R.shuffle_ref.parse_param(p)
    assert R.Net(p, b).read == len(b)  # the restatement reads every weight byte ...
    new = [nm for t, nm, *_ in layers if t in R.RESAMPLE_TYPES]
    assert new
    assert model_zoo.MODELS[name](dry=True, **kw) == (p, len(b), i, o)  # the dry builder writes the same .param and counts the same bytes
    for level in (0, 1, 2, 3):
        net = Net(fusion=level)
        net.SetExtendedLayers(True)
        if name in model_zoo.DILATED_LAYERS:
            net.SetDilated(True)
        net.LoadParam(p)
        net.LoadWeights(b)  # ... and so does the runtime (a short read is an error)
        got = net.layers()
        assert [(t, nm) for t, nm, _ in got] == [(t, nm) for t, nm, *_ in layers]
        assert [nm for _, nm, a in got if a == "RESAMPLE"] == new
    from feathercnn_amd import FeatherHipError
    with pytest.raises(FeatherHipError) as e:  # without the switch the file is refused at its first new layer
        net = Net()
        if name in model_zoo.DILATED_LAYERS:
            net.SetDilated(True)
        net.LoadParam(p)
    assert "code -200" in str(e.value)


def test_zoo_nets_are_the_published_ones():
    from feathercnn_amd import model_zoo
    count = lambda p, t: sum(tt == t for tt, *_ in R.shuffle_ref.parse_param(p))
    p, nbytes, _, _ = model_zoo.mobilenet_v3_large(dry=True)
    assert 5.2e6 < nbytes / 4 < 5.8e6 and count(p, "HardSwish") == 21 and count(p, "HardSigmoid") == 8 and count(p, "Eltwise") == 10  # 5.4 M parameters
    p, nbytes, _, _ = model_zoo.mobilenet_v3_small(dry=True)
    assert 2.3e6 < nbytes / 4 < 2.8e6 and count(p, "HardSwish") == 19 and count(p, "HardSigmoid") == 9 and count(p, "Eltwise") == 6  # 2.5 M parameters
    assert [model_zoo._divisible(v / 4) for v in (16, 72, 96, 120, 240, 288, 480, 576, 672, 960)] == [8, 24, 24, 32, 64, 72, 120, 144, 168, 240]
    p, _, _, o = model_zoo.deeplab_largefov_full(dry=True)
    # the trunk and head of deeplab_largefov line for line (the count line differs: one more layer and blob)
    assert p.split(b"\n", 2)[2].startswith(model_zoo.deeplab_largefov(dry=True)[0].split(b"\n", 2)[2]) and o == "fc8_interp"
    assert p.rstrip().endswith(b"Interp fc8_interp 1 1 fc8 fc8_interp 0=2 3=321 4=321")
    p, _, _, _ = model_zoo.unet_bilinear(dry=True)
    assert count(p, "Interp") == 5 and count(p, "Deconvolution") == 0 and count(model_zoo.unet_k4(dry=True)[0], "Deconvolution") == 5
    p, _, _, o = model_zoo.fpn_resnet50(dry=True)
    assert count(p, "Interp") == 3 and o == model_zoo.FPN_OUTPUTS[0] and all(f"Convolution {nm} ".encode() in p for nm in model_zoo.FPN_OUTPUTS)


def test_existing_builders_write_what_they_wrote():
    """GraphBuilder gained methods only: the .param text of nets that use none of them keeps its digest."""
    import hashlib
    from feathercnn_amd import model_zoo
    want = {"tiny_allsorts": "b910eddbebf3", "resnet50": "9346900569a1", "tiny_shuffle": "c8606d220268", "tiny_dilated": "a04e50b121f6", "tiny_generative": "89d183a43348"}
    got = {k: hashlib.sha256(model_zoo.MODELS[k](dry=True)[0]).hexdigest()[:12] for k in want}
    assert got == want, got
