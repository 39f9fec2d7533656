"""The int8 convolution route without a GPU: the header of libfeather_qconv.so (include/feather_hip/feather_qconv.h) names every
entry point with the binding's argument counts; fhip_qconv_supported refuses every case the definition lists,
with its reason, and draws the line of the reduction length at 133144; fhip_qconv_dequant_scales equals numpy to the bit; tiny_quant loads
and reports route 108 with Net.SetQuantized and is refused exactly as before without it; the restatement (tests/qconv_ref.py) stays
within the bound that round-to-nearest gives against the fp64 convolution of the fp32 values; and the readers refuse hostile int8 files
with a code, clean under AddressSanitizer and UndefinedBehaviorSanitizer, in a stand-alone program (tests/cpp/qconv_loader_main.cpp)."""
import ctypes
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import qconv_cases as QC
import qconv_ref as R
import side_contract

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "feather_hip", "feather_qconv.h")
CSRC = os.path.join(ROOT, "feathercnn_amd", "csrc")
DRIVER = os.path.join(ROOT, "tests", "cpp", "qconv_loader_main.cpp")
BADARG, UNSUPPORTED = -2, -1
F = np.float32


lib = side_contract.fixture("qconv")


# ---- the library ---------------------------------------------------------------------------------------------------------------------
def test_header_names_every_entry_point_with_the_bindings_argument_counts():
    from feathercnn_amd import _lib
    text = open(HEADER).read()
    declared = set(re.findall(r"FHIP_QCONV_API\s+[\w\s\*]+?\b(fhip_\w+)\s*\(", text))
    for name in ("assign_output_dim", "supported", "get_buffer_size", "init", "forward", "dequant_scales", "route", "get_buffer_size_route",
                 "init_route", "forward_route", "last_error"):
        assert f"fhip_qconv_{name}" in declared
    assert "fhip_quantize_forward" in declared
    # the argument counts of the binding are the header's
    for name, (_, args) in _lib.QCONV_SIGNATURES.items():
        decl = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, text, re.S).group(1)
        n = 0 if decl.strip() in ("", "void") else decl.count(",") + 1
        assert n == len(args), (name, n, len(args))
    assert re.search(r"#define FHIP_QCONV_MAX_REDUCTION %d\b" % R.MAX_R, text) and 127 * 127 * R.MAX_R < 2 ** 31 <= 127 * 127 * (R.MAX_R + 1)


def test_every_instantiation_has_a_case(lib):
    assert len({c[0] for c in QC.CASES}) == len(QC.CASES)
    for case in QC.CASES:
        p = QC.param(case)
        assert lib.fhip_qconv_supported(ctypes.byref(p)) == 1, (case[0], lib.fhip_qconv_last_error())
        name = ctypes.create_string_buffer(160)
        assert lib.fhip_qconv_route(ctypes.byref(p), name, 160) == 0 and name.value.decode() == case[-1][0], case[0]
        sizes = set()
        for route in case[-1]:
            sb, pk = ctypes.c_size_t(), ctypes.c_size_t()
            assert lib.fhip_qconv_get_buffer_size_route(ctypes.byref(p), 3, route.encode(), ctypes.byref(sb), ctypes.byref(pk)) == 0
            assert sb.value == 0 and pk.value >= case[1] * case[2] // case[3] * case[6] * case[7] and pk.value % 4 == 0
            sizes.add(pk.value)
        for route in QC.targets() - QC.HELPERS - set(case[-1]):
            sb, pk = ctypes.c_size_t(), ctypes.c_size_t()
            assert lib.fhip_qconv_get_buffer_size_route(ctypes.byref(p), 3, route.encode(), ctypes.byref(sb), ctypes.byref(pk)) == UNSUPPORTED, (case[0], route)
    p = QC.param(QC.CASES[0])
    assert lib.fhip_qconv_get_buffer_size_route(ctypes.byref(p), 1, b"fhip::no_such_kernel", ctypes.byref(sb), ctypes.byref(pk)) == BADARG


def test_supported_refuses_what_the_definition_lists(lib):
    base = QC.CASES[0]
    for over, reason in ((dict(dilation_h=2), "dilation"), (dict(dilation_w=0), "dilation"), (dict(pad_left=-233), "negative padding"),
                         (dict(pad_top=-1), "negative padding"), (dict(group=2), "partial group"), (dict(group=16), "partial group"),
                         (dict(int8_scale_term=101), "requantised"), (dict(int8_scale_term=-1), "int8_scale_term"), (dict(activation=2), "activation"),
                         (dict(output_h=4), "assign_output_dim"), (dict(kernel_h=9), "larger than the padded input"), (dict(stride_w=0), "stride"),
                         (dict(input_channels=0), "channels")):
        p = QC.param(base, **over)
        assert lib.fhip_qconv_supported(ctypes.byref(p)) == 0, over
        assert reason.encode() in lib.fhip_qconv_last_error(), (over, lib.fhip_qconv_last_error())
        sb, pk = ctypes.c_size_t(), ctypes.c_size_t()
        assert lib.fhip_qconv_get_buffer_size(ctypes.byref(p), 1, ctypes.byref(sb), ctypes.byref(pk)) == BADARG
        v = ctypes.c_void_p
        assert lib.fhip_qconv_forward(ctypes.byref(p), 1, v(0x1000), v(0x2000), v(0x3000), None, v(0x4000), v(0x5000), 1.0, None) == BADARG
    assert lib.fhip_qconv_supported(ctypes.byref(QC.param(base, int8_scale_term=100))) == 1
    assert lib.fhip_qconv_supported(ctypes.byref(QC.param(base, int8_scale_term=2))) == 1
    assert lib.fhip_qconv_supported(None) == 0
    # the reduction length: 1x1, C = R
    for c, ok in ((R.MAX_R, 1), (R.MAX_R + 1, 0)):
        case = ("r", c, 4, 1, 2, 2, 1, 1, 1, QC.P0, (1,), ())
        assert lib.fhip_qconv_supported(ctypes.byref(QC.param(case))) == ok, c
    assert b"133144" in lib.fhip_qconv_last_error()
    # the input scale belongs to the forward call and to dequant_scales
    p, v = QC.param(base), ctypes.c_void_p
    for s_in in (0.0, -1.0, float("nan"), float("inf")):
        assert lib.fhip_qconv_forward(ctypes.byref(p), 1, v(0x1000), v(0x2000), v(0x3000), None, v(0x4000), v(0x5000), s_in, None) == BADARG
        assert b"s_in" in lib.fhip_qconv_last_error()
        assert lib.fhip_quantize_forward(v(0x1000), v(0x2000), 4, s_in, None) == BADARG


def test_dequant_scales_equal_numpy_to_the_bit(lib):
    from feathercnn_amd import FeatherHipError, dequant_scales
    rng = np.random.default_rng(3)
    for s_in in (1.0, 0.0078125, 3.1415927, 1e-20, 1e20, float(rng.uniform(0.1, 300))):
        s_w = np.concatenate([rng.uniform(1e-3, 1e4, 500), [0.0, 1e-30, 1e30, 1.0, 127.0]]).astype(F)
        got, want = dequant_scales(s_w, s_in), R.dequant_scales(s_w, s_in)
        assert got.dtype == F and np.array_equal(got.view(np.int32), want.view(np.int32)), s_in
        assert got[500] == 0.0  # ncnn's convention for s_w == 0
    for bad_w, bad_in in (([1.0, -1.0], 1.0), ([np.nan], 1.0), ([np.inf], 1.0), ([1.0], 0.0), ([1.0], -2.0), ([1.0], np.nan), ([1.0], np.inf)):
        with pytest.raises(FeatherHipError, match="code -2"):
            dequant_scales(np.array(bad_w, F), bad_in)


# ---- feather::Net --------------------------------------------------------------------------------------------------------------------
def test_tiny_quant_loads_with_the_switch_and_is_refused_without_it():
    from feathercnn_amd import FeatherHipError, model_zoo
    from feathercnn_amd.net import Net
    p, b, i, o = model_zoo.tiny_quant()
    assert model_zoo.tiny_quant() == (p, b, i, o) and model_zoo.tiny_quant(dry=True) == (p, len(b), i, o)  # deterministic; dry counts the same bytes
    assert "tiny_quant" in model_zoo.QUANTIZED_NETS and all(n in model_zoo.MODELS for n in model_zoo.QUANTIZED_NETS)
    net = Net()
    net.SetQuantized(True)
    net.LoadParam(p)
    net.LoadWeights(b)
    routed = [nm for _, nm, a in net.layers() if a == "QCONV"]
    assert routed == list(model_zoo.QUANT_LAYERS["tiny_quant"]) and len(routed) == 6
    with pytest.raises(FeatherHipError, match="before LoadParam"):
        net.SetQuantized(False)
    for flip in (False, True):
        net = Net()
        if flip:
            net.SetQuantized(True)
            net.SetQuantized(False)  # on then off equals the default
        with pytest.raises(FeatherHipError) as e:
            net.LoadParam(p)
        assert "code -200" in str(e.value) and "layer conv1: int8 convolution is not supported" in str(e.value) and "quantized" not in str(e.value)
    # an InnerProduct alone: the default net gets as far as the weights and refuses the int8 tag there, as it always has
    head = b"7767517\n2 2\nInput data 0 1 data 0=1 1=1 2=16\nInnerProduct fc 1 1 data fc 0=4 1=0 2=64 8=1\n"
    g = model_zoo.GraphBuilder(1, quant={})
    g.fc("fc", g.input("data", 16, 1, 1), 16, 4, bias=False)
    text, blob = g.finish()
    assert text == head
    net = Net()
    net.LoadParam(text)
    with pytest.raises(FeatherHipError, match="int8 weights are not supported"):
        net.LoadWeights(blob)
    net = Net()
    net.SetQuantized(True)
    net.LoadParam(text)
    net.LoadWeights(blob)
    assert net.layers()[1] == ("InnerProduct", "fc", "QCONV")
    # with the switch on, what stays refused does not offer the switch
    for line, word in (("Convolution c 1 1 data c 0=4 1=1 6=64 8=101", "requantised"), ("Convolution c 1 1 data c 0=4 1=3 2=2 6=576 8=1", "dilated"),
                       ("Convolution c 1 1 data c 0=4 1=3 4=-233 6=576 8=1", "automatic padding"), ("Convolution c 1 1 data c 0=4 1=1 6=32 7=2 8=1", "partial group"),
                       ("InnerProduct c 1 1 data c 0=4 2=64 8=101", "requantised")):
        net = Net()
        net.SetQuantized(True)
        net.SetDilated(True)
        with pytest.raises(FeatherHipError) as e:
            net.LoadParam(b"7767517\n2 2\nInput data 0 1 data 0=1 1=1 2=16\n" + line.encode() + b"\n")
        assert "code -200" in str(e.value) and word in str(e.value) and "fhip_net_set_" not in str(e.value), (line, str(e.value))


# ---- a derived bound -----------------------------------------------------------------------------------------------------------------
def test_the_quantised_convolution_stays_within_the_rounding_bound():
    """y_q = sum(q_x q_w) / (s_in s_w) against the fp64 convolution y of the fp32 values x, w.  With q_x = x s_in + e_x, q_w = w s_w + e_w and
    |e| <= 0.5 (round to nearest; nothing clamps: the scales are 127 / absmax), a tap's error is (w e_x / s_in + x e_w / s_w + e_x e_w / (s_in
    s_w)), at most 0.5 |w| / s_in + 0.5 |x| / s_w + 0.25 / (s_in s_w).  Summed over the taps of each output, plus the fp32 roundings of x * s_in
    and w * s_w before the integer rounding (2^-24 relative, i.e. up to 127 * 2^-24 more on each e) and of the result (float(acc), the scale
    and its reciprocal, the product: four roundings, 2^-24 relative each), that is the per-output bound -- derived, not measured."""
    rng = np.random.default_rng(11)
    c, k, h, w = 16, 12, 9, 10
    x = rng.standard_normal((2, c, h, w)).astype(F)
    wt = (rng.standard_normal((k, c, 3, 3)) * 0.2).astype(F)
    wq, s_w = R.quantise_weights(wt)
    s_in = F(127) / np.abs(x).max()
    d = R.dequant_scales(s_w, s_in)
    got = R.qconv(x, wq, d, s_in, None, 1, (1, 1), QC.P1).astype(np.float64)
    xp = np.pad(x.astype(np.float64), ((0, 0), (0, 0), (1, 1), (1, 1)))
    want = np.zeros((2, k, h, w))
    sum_abs_x = np.zeros((2, 1, h, w))   # sum over the taps inside the plane of |x|
    taps_in = np.zeros((1, 1, h, w))
    inside = np.pad(np.ones((1, 1, h, w)), ((0, 0), (0, 0), (1, 1), (1, 1)))
    sum_abs_w = np.zeros((k, h, w))      # sum over the taps inside the plane of |w[k]|
    for i in range(3):
        for j in range(3):
            win = xp[:, :, i:i + h, j:j + w]
            want += np.einsum("nchw,kc->nkhw", win, wt[:, :, i, j].astype(np.float64))
            sum_abs_x += np.abs(win).sum(axis=1, keepdims=True)
            m = inside[0, 0, i:i + h, j:j + w]
            taps_in[0, 0] += m * c
            sum_abs_w += np.abs(wt[:, :, i, j].astype(np.float64)).sum(axis=1)[:, None, None] * m
    e = 0.5 + 127 * 2.0 ** -24
    sw = s_w.astype(np.float64).reshape(1, k, 1, 1)
    bound = e * sum_abs_w[None] / float(s_in) + e * sum_abs_x / sw + e * e * taps_in / (float(s_in) * sw)
    bound += 4 * 2.0 ** -24 * (np.abs(want) + bound)
    err = np.abs(got - want)
    print(f"quantised vs fp64 convolution: worst error / bound {float((err / bound).max()):.3f}, worst error {float(err.max()):.3e}")
    assert (err <= bound).all(), float((err / bound).max())
    assert float((err / bound).max()) > 0.01  # the bound is not vacuous


# ---- hostile files, in a stand-alone program ------------------------------------------------------------------------------------------
def _int8_block(wq, pad=True, tag=0x000D4B38):
    raw = np.asarray(wq, np.int8).tobytes()
    return struct.pack("<I", tag) + raw + (bytes(-len(raw) % 4) if pad else b"")


def _hostile_cases():
    """(name, param, bin, switch, expectation): expectation = (stage, code or None) of the refusal, or None for a control that loads."""
    f4 = lambda *v: np.asarray(v, "<f4").tobytes()
    head = "7767517\n2 2\nInput data 0 1 data 0=4 1=4 2=3\n"
    conv = lambda over=None: (head + "Convolution c 1 1 data c " + " ".join(f"{k}={v}" for k, v in sorted({0: 2, 1: 3, 5: 1, 6: 54, 8: 1, **(over or {})}.items())) + "\n").encode()
    wq = np.arange(54, dtype=np.int8) - 27          # 54 bytes: padded to 56
    good = _int8_block(wq) + f4(0.5, -0.5) + f4(20.0, 30.0) + f4(8.0)
    scales = lambda s_w, s_in: _int8_block(wq) + f4(0.5, -0.5) + f4(*s_w) + f4(s_in)
    ip = (head.replace("0=4 1=4 2=3", "0=1 1=1 2=16") + "InnerProduct c 1 1 data c 0=4 1=0 2=64 8=1\n").encode()
    ipw = np.arange(64, dtype=np.int8)
    cases = [
        ("control", conv(), good, True, None),
        ("control_scale_term_2", conv({8: 2}), good, True, None),
        ("control_inner_product", ip, _int8_block(ipw) + f4(1, 2, 3, 4) + f4(5.0), True, None),
        ("control_zero_weight_scale", conv(), scales((0.0, 30.0), 8.0), True, None),
        ("switch_off", conv(), good, False, ("param", -200)),
        ("switch_off_inner_product", ip, _int8_block(ipw) + f4(1, 2, 3, 4) + f4(5.0), False, ("weights", None)),
        ("payload_cut_short", conv(), good[:4 + 30], True, ("weights", None)),
        ("payload_cut_at_the_tag", conv(), good[:2], True, ("weights", None)),
        ("padding_missing", conv(), _int8_block(wq, pad=False), True, ("weights", None)),
        ("padding_missing_rest_follows", conv(), _int8_block(wq, pad=False) + f4(0.5, -0.5) + f4(20.0, 30.0) + f4(8.0), True, ("weights", None)),
        ("fp32_tagged_weights", conv(), struct.pack("<I", 0) + f4(*range(54)) + f4(0.5, -0.5) + f4(20.0, 30.0) + f4(8.0), True, ("weights", None)),
        ("fp16_tagged_weights", conv(), struct.pack("<I", 0x01306B47) + bytes(108) + f4(0.5, -0.5) + f4(20.0, 30.0) + f4(8.0), True, ("weights", None)),
        ("scale_block_missing", conv(), _int8_block(wq) + f4(0.5, -0.5), True, ("weights", None)),
        ("input_scale_missing", conv(), _int8_block(wq) + f4(0.5, -0.5) + f4(20.0, 30.0), True, ("weights", None)),
        ("input_scale_nan", conv(), scales((20.0, 30.0), np.nan), True, ("weights", None)),
        ("input_scale_zero", conv(), scales((20.0, 30.0), 0.0), True, ("weights", None)),
        ("input_scale_negative", conv(), scales((20.0, 30.0), -8.0), True, ("weights", None)),
        ("input_scale_inf", conv(), scales((20.0, 30.0), np.inf), True, ("weights", None)),
        ("weight_scale_negative", conv(), scales((20.0, -30.0), 8.0), True, ("weights", None)),
        ("weight_scale_nan", conv(), scales((np.nan, 30.0), 8.0), True, ("weights", None)),
        ("scale_term_101", conv({8: 101}), good, True, ("param", -200)),
        ("scale_term_negative", conv({8: -1}), good, True, ("param", -200)),
        ("inner_product_scale_term_101", ip.replace(b"8=1", b"8=101"), _int8_block(ipw) + f4(1, 2, 3, 4) + f4(5.0), True, ("param", -200)),
        ("weight_data_size_not_a_multiple", conv({6: 55}), good, True, ("param", -100)),
        ("weight_data_size_huge", conv({6: 2147483646}), good, True, ("weights", None)),
        ("inner_product_cut_short", ip, _int8_block(ipw)[:40], True, ("weights", None)),
        ("partial_group", (head.replace("2=3", "2=4") + "Convolution c 1 1 data c 0=4 1=1 6=8 7=2 8=1\n").encode(), good, True, ("param", -200)),
        ("dilated", conv({2: 2}), good, True, ("param", -200)),
        ("automatic_pads", conv({4: -233}), good, True, ("param", -200)),
    ]
    return cases


def _judge(cases, stdout):
    lines = [l for l in stdout.splitlines() if l.startswith("case ")]
    assert len(lines) == len(cases), stdout[-2000:]
    bad = []
    for i, ((name, _, _, _, want), line) in enumerate(zip(cases, lines)):
        m = re.match(r"case (\d{4}) param (-?\d+) weights (-?\d+|skip) \| (.*)$", line)
        assert m and int(m.group(1)) == i, line
        rp, rw, msg = int(m.group(2)), m.group(3), m.group(4)
        stage, code = ("param", rp) if rp else ("weights", int(rw)) if rw not in ("skip", "0") else (None, 0)
        if want is None:
            if stage:
                bad.append(f"{name}: the control did not load: {line}")
        elif stage != want[0] or (want[1] is not None and code != want[1]) or not msg.strip():
            bad.append(f"{name}: wanted a refusal at the {want[0]} ({want[1]}), got: {line}")
    return bad


@pytest.fixture(scope="module")
def hostile(tmp_path_factory):
    cases = _hostile_cases()
    d = tmp_path_factory.mktemp("qconv_loader_cases")
    for i, (_, param, blob, switch, _) in enumerate(cases):
        open(d / f"{i:04d}.param", "wb").write(param)
        open(d / f"{i:04d}.bin", "wb").write(blob)
        if not switch:
            open(d / f"{i:04d}.off", "wb").close()
    return cases, str(d)


def test_hostile_int8_files_are_refused_with_a_code(hostile, tmp_path):
    """Plain build: g++ against the built library, every case in one child process."""
    from feathercnn_amd import _lib
    cases, d = hostile
    libdir = os.path.dirname(_lib.lib_path())
    exe = str(tmp_path / "qconv_loader")
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), DRIVER, "-o", exe, "-L" + libdir, "-lfeather_hip",
                    "-Wl,-rpath," + libdir], check=True, capture_output=True, text=True)
    out = subprocess.run([exe, d, str(len(cases))], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    bad = _judge(cases, out.stdout)
    assert not bad, "\n".join(bad)
    assert "int8 loader: %d cases" % len(cases) in out.stdout


def test_hostile_int8_files_are_clean_under_sanitizers(hostile, tmp_path):
    """Sanitised build, the way tests/test_loader_hostile_cpu.py builds its runner: every translation unit of libfeather_hip.so with its host
    side under ASan + UBSan, linked with the driver into one ordinary executable.  Nothing is loaded into python and nothing is preloaded."""
    cases, d = hostile
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    objdir = str(tmp_path / "obj")
    san = "-fsanitize=address,undefined"
    host = f"-Xarch_host {san} -Xarch_host -fno-sanitize-recover=undefined -g"
    subprocess.run(["make", "-s", "-j", str(min(8, os.cpu_count() or 1)), "-C", CSRC, "OBJDIR=" + objdir, "EXTRA=" + host, "objects"],
                   check=True, capture_output=True, text=True)
    objs = sorted(os.path.join(objdir, f) for f in os.listdir(objdir) if f.endswith(".o"))
    assert len(objs) >= 7
    exe = str(tmp_path / "qconv_loader_san")
    subprocess.run([hipcc, "-std=c++17", "-O1", "-g", "-Xarch_host", san, "-Xarch_host", "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"),
                    "-x", "c++", DRIVER, "-x", "none"] + objs + [san, "-o", exe, "-ldl"], check=True, capture_output=True, text=True)
    out = subprocess.run([exe, d, str(len(cases))], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    assert "ERROR: AddressSanitizer" not in out.stderr and "runtime error:" not in out.stderr and "LeakSanitizer" not in out.stderr, out.stderr[-3000:]
    bad = _judge(cases, out.stdout)
    assert not bad, "\n".join(bad)
