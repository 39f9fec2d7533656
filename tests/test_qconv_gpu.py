"""The int8 convolution route (libfeather_qconv.so, include/feather_hip/feather_qconv.h) on the MI355X.  Every comparison is
np.array_equal against the numpy restatement (tests/qconv_ref.py): the definition is exact, so the tolerance is zero.

* fhip_quantize_forward on the values where a rounding rule can go wrong, with s_in = 1 and with an s_in whose product rounds in fp32;
* every route of every case of tests/qconv_cases.py, forced by name through the _route calls (the first one also through the selecting
  calls), with bias + ReLU, bias alone and neither, random data over the whole q range;
* the accumulator: |acc| = 18 580 608 > 2^24 must reach the dequantisation as an exact integer;
* padding is a select: a NaN and an inf pixel reach the outputs whose window holds them and no other;
* the guarded-buffer contract (tests/guarded.py) for out, in, packed and the bias on one MFMA and one generic shape; misaligned pointers;
* feather::Net: tiny_quant at batch 3, fusion levels 0, 1, 2 (the fold as the header defines it), re-planned to another batch, graph mode on;
The directory without libfeather_qconv.so is in tests/test_side_contract_gpu.py.
"""
import ctypes

import numpy as np
import pytest

import qconv_cases as QC
import qconv_ref as R
import side_contract
from guarded import Guarded, describe

pytestmark = pytest.mark.gpu
F = np.float32


lib = side_contract.fixture("qconv", gpu=True)


_stream = side_contract.stream


def _run(lib, case, batch, x, wq, d, b, s_in, relu, route, selecting=False):
    """Pack and run one layer under `route` (selecting: through fhip_qconv_init / fhip_qconv_forward); returns the output."""
    import torch
    v = ctypes.c_void_p
    p = QC.param(case, bias=0 if b is None else 1, relu=int(relu))
    sb, pk = ctypes.c_size_t(), ctypes.c_size_t()
    rn = route.encode()
    if selecting:
        assert lib.fhip_qconv_get_buffer_size(ctypes.byref(p), batch, ctypes.byref(sb), ctypes.byref(pk)) == 0, lib.fhip_qconv_last_error()
    else:
        assert lib.fhip_qconv_get_buffer_size_route(ctypes.byref(p), batch, rn, ctypes.byref(sb), ctypes.byref(pk)) == 0, lib.fhip_qconv_last_error()
    assert sb.value == 0 and pk.value % 4 == 0
    tw = torch.from_numpy(wq).cuda()
    packed = torch.full((pk.value,), 0x5A, dtype=torch.uint8, device="cuda")
    tx, td = torch.from_numpy(x).cuda(), torch.from_numpy(d).cuda()
    tb = None if b is None else torch.from_numpy(b).cuda()
    out = torch.full((batch, p.output_channels, p.output_h, p.output_w), float("nan"), dtype=torch.float32, device="cuda")
    bp = v(tb.data_ptr()) if tb is not None else None
    if selecting:
        rc = lib.fhip_qconv_init(ctypes.byref(p), v(packed.data_ptr()), v(tw.data_ptr()), _stream())
        rc = rc or lib.fhip_qconv_forward(ctypes.byref(p), batch, v(out.data_ptr()), v(tx.data_ptr()), v(packed.data_ptr()), None, v(td.data_ptr()), bp,
                                          float(s_in), _stream())
    else:
        rc = lib.fhip_qconv_init_route(ctypes.byref(p), v(packed.data_ptr()), v(tw.data_ptr()), _stream(), rn)
        rc = rc or lib.fhip_qconv_forward_route(ctypes.byref(p), batch, v(out.data_ptr()), v(tx.data_ptr()), v(packed.data_ptr()), None, v(td.data_ptr()),
                                                bp, float(s_in), _stream(), rn)
    assert rc == 0, lib.fhip_qconv_last_error()
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _want(case, x, wq, d, b, s_in, relu):
    _, c, k, group, h, w, kh, kw, s, pads, _, _ = case
    return R.qconv(x, wq, d, s_in, b, group, (s, s), pads, relu)


# ---- quantise alone ------------------------------------------------------------------------------------------------------------------
QUANT_VALUES = [0.5, 1.5, -0.5, -2.5, 0.49999997, -0.49999997, 126.5, 127.5, -127.5, 1e9, np.inf, -np.inf, np.nan, 0.0, -0.0]


@pytest.mark.parametrize("s_in", [1.0, 1.0000001, 0.3333333, 3.1415927])
def test_quantise_rounds_half_away_from_zero(cuda, s_in):
    """0.49999997 + 0.5 rounds to 1.0 in fp32: a trunc(t + 0.5) kernel gives 1 where roundf gives 0.  The scales other than 1 make x * s_in
    round in fp32 before roundf sees it; dividing the values by the scale puts the products next to the halves again."""
    import torch
    from feathercnn_amd import quantize
    base = np.array(QUANT_VALUES, F)
    with np.errstate(invalid="ignore", over="ignore"):
        x = np.concatenate([base, (base / F(s_in)).astype(F), np.nextafter((base / F(s_in)).astype(F), F(0)), np.linspace(-130, 130, 2081, dtype=F)])
    got = quantize(torch.from_numpy(x).cuda(), s_in).cpu().numpy()
    want = R.quantise(x, s_in)
    assert got.dtype == np.int8 and np.array_equal(got.astype(np.int32), want), [(float(a), int(b), int(c)) for a, b, c in zip(x, got, want) if b != c][:8]
    if s_in == 1.0:
        assert want[:15].tolist() == [1, 2, -1, -3, 0, 0, 127, 127, -127, 127, 127, -127, 0, 0, 0]


# ---- every route ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", QC.CASES, ids=[c[0] for c in QC.CASES])
def test_every_route_equals_the_restatement(lib, case):
    from feathercnn_amd import dequant_scales
    name, c, k, group, h, w, kh, kw, s, pads, batches, routes = case
    told = ctypes.create_string_buffer(160)
    p = QC.param(case)
    assert lib.fhip_qconv_route(ctypes.byref(p), told, 160) == 0 and told.value.decode() == routes[0], (name, told.value)
    for batch in batches:
        x, wq, s_w, s_in, bias = R.synth(c, k, h, w, kh, kw, group, batch, seed=len(name) + batch)
        s_w[0] = 0.0  # ncnn's convention: d = 0
        d = dequant_scales(s_w, s_in)
        assert np.array_equal(d.view(np.int32), R.dequant_scales(s_w, s_in).view(np.int32))
        for has_bias, relu in QC.EPILOGUES:
            b = bias if has_bias else None
            want = _want(case, x, wq, d, b, s_in, relu)
            assert np.abs(want).max() > 0
            for i, route in enumerate(routes):
                for selecting in ((True, False) if i == 0 else (False,)):
                    got = _run(lib, case, batch, x, wq, d, b, s_in, relu, route, selecting)
                    bad = np.argwhere(got != want)
                    assert got.shape == want.shape and np.array_equal(got, want), (name, route, batch, has_bias, relu, len(bad), bad[:4].tolist())


# ---- the accumulator -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", [QC.MFMA64, QC.MFMA128, QC.GENERIC, QC.GENERIC16])
def test_the_accumulator_is_int32_past_2_to_24(lib, route):
    """C = 128, 3x3, every q = 127 and every w = 127 (channel 1: -127): the interior sums are +-18 580 608 = 127 * 127 * 1152 > 2^24 and, being
    no multiple of a power of two large enough, not the sum a float accumulator reaches.  float32(acc) * d + b must come out exactly."""
    case = ("acc", 128, 2, 1, 5, 5, 3, 3, 1, QC.P1, (1,), (route,))
    x = np.full((1, 128, 5, 5), 127.0, F)
    wq = np.full((2, 128, 3, 3), 127, np.int8)
    wq[1] = -127
    d = np.array([3.0000002, 1.0], F)  # d[0] makes the product round; d[1] shows the rounded conversion itself
    b = np.array([0.25, -7.0], F)
    want = _want(case, x, wq, d, b, 1.0, False)
    acc = R.accumulate(R.quantise(x, 1.0), wq, 1, (1, 1), QC.P1)
    assert acc[0, 0, 2, 2] == 18580608 and acc[0, 1, 2, 2] == -18580608 and acc[0, 0, 2, 2] > 2 ** 24
    assert want[0, 1, 2, 2] == F(F(-18580608) * F(1.0)) + F(-7.0)
    got = _run(lib, case, 1, x, wq, d, b, 1.0, False, route)
    assert np.array_equal(got, want), (got[0, :, 2, 2], want[0, :, 2, 2])
    # an odd sum past 2^24: the conversion itself must round (to nearest even), not truncate
    wq[0, 0, 1, 1] = 126
    want = _want(case, x, wq, d, b, 1.0, False)
    assert R.accumulate(R.quantise(x, 1.0), wq, 1, (1, 1), QC.P1)[0, 0, 2, 2] == 18580608 - 127
    assert np.array_equal(_run(lib, case, 1, x, wq, d, b, 1.0, False, route), want)


# ---- padding is a select -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mfma_3x3_s1", "generic_5x5_c3", "dw3x3_s1", "dw3x3_s2"])
def test_a_nan_and_an_inf_pixel_reach_their_windows_only(lib, name):
    case = next(c for c in QC.CASES if c[0] == name)
    _, c, k, group, h, w, kh, kw, s, pads, _, routes = case
    x, wq, s_w, s_in, bias = R.synth(c, k, h, w, kh, kw, group, 2, seed=77)
    d = R.dequant_scales(s_w, s_in)
    clean = _want(case, x, wq, d, bias, s_in, False)
    x2 = x.copy()
    x2[0, 1, 0, 0] = np.nan   # a corner: most of its neighbours' windows lie in the padding
    x2[1, 2, h - 1, w - 1] = np.inf
    want = _want(case, x2, wq, d, bias, s_in, False)
    assert np.isfinite(want).all() and (want != clean).any()  # NaN quantises to 0, inf to 127: finite, and visible
    for route in routes:
        got = _run(lib, case, 2, x2, wq, d, bias, s_in, False, route)
        assert np.array_equal(got, want), (name, route)
        assert np.array_equal(got == clean, want == clean)  # nothing outside the two windows moved


# ---- the guarded-buffer contract -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,offset", [("mfma_3x3_s1", 0), ("mfma_3x3_s1", 1), ("mfma_k130", 1), ("generic_5x5_c3", 1), ("generic16_7x7_c3", 1), ("dw3x3_s2", 1)])
def test_nothing_outside_the_tensors_is_written_or_read(lib, name, offset):
    """out and packed between poisoned guards, in, d and the bias between NaN guards (tests/guarded.py): every word of out and packed is
    written, no guard word changes, no input changes, and the result is still the restatement's, so no guard NaN reached it."""
    import torch
    v = ctypes.c_void_p
    case = next(c for c in QC.CASES if c[0] == name)
    _, c, k, group, h, w, kh, kw, s, pads, _, routes = case
    batch = 3
    x, wq, s_w, s_in, bias = R.synth(c, k, h, w, kh, kw, group, batch, seed=5)
    d = R.dequant_scales(s_w, s_in)
    for has_bias in (1, 0):
        p = QC.param(case, bias=has_bias, relu=1)
        sb, pk = ctypes.c_size_t(), ctypes.c_size_t()
        assert lib.fhip_qconv_get_buffer_size(ctypes.byref(p), batch, ctypes.byref(sb), ctypes.byref(pk)) == 0
        gx, gd = Guarded(x.size, x, offset), Guarded(k, d, offset)
        gb = Guarded(k, bias if has_bias else "nan", offset)  # without bias_term the bias must not be read
        gy, gp = Guarded(batch * k * p.output_h * p.output_w, "poison", offset), Guarded(pk.value // 4, "poison", 0)
        tw = torch.from_numpy(wq).cuda()
        snaps = [g.snapshot() for g in (gx, gd, gb)]
        rc = lib.fhip_qconv_init(ctypes.byref(p), v(gp.ptr), v(tw.data_ptr()), _stream())
        rc = rc or lib.fhip_qconv_forward(ctypes.byref(p), batch, v(gy.ptr), v(gx.ptr), v(gp.ptr), None, v(gd.ptr), v(gb.ptr), float(s_in), _stream())
        assert rc == 0, lib.fhip_qconv_last_error()
        torch.cuda.synchronize()
        for what, g in (("output", gy), ("packed weights", gp), ("input", gx), ("d", gd), ("bias", gb)):
            assert g.guards_intact() is None, f"{name}: {what} guard: {describe(g.guards_intact())}"
        assert gy.unwritten() == 0, (name, gy.unwritten())
        for g, snap in zip((gx, gd, gb), snaps):
            assert g.unchanged(snap), (name, g.first_change(snap))
        # Init is idempotent and writes every packed byte: a second Init over zeros gives the same bytes
        first = gp.bits().clone()
        gp.bits().zero_()
        assert lib.fhip_qconv_init(ctypes.byref(p), v(gp.ptr), v(tw.data_ptr()), _stream()) == 0
        torch.cuda.synchronize()
        assert torch.equal(gp.bits(), first) and gp.guards_intact() is None
        want = _want(case, x, wq, d, bias if has_bias else None, s_in, True)
        assert np.array_equal(gy.values().reshape(want.shape), want), name


def test_misaligned_pointers_are_refused(lib):
    case = QC.CASES[0]
    p = QC.param(case)
    v = ctypes.c_void_p
    good = dict(out=0x10000, x=0x20000, packed=0x30000, d=0x40000, bias=0x50000)
    for which, delta in (("out", 2), ("x", 1), ("packed", 4), ("packed", 8), ("d", 2), ("bias", 3)):
        a = dict(good)
        a[which] += delta
        rc = lib.fhip_qconv_forward(ctypes.byref(p), 1, v(a["out"]), v(a["x"]), v(a["packed"]), None, v(a["d"]), v(a["bias"]), 1.0, None)
        assert rc == -2 and b"aligned" in lib.fhip_qconv_last_error(), (which, rc)
    assert lib.fhip_qconv_init(ctypes.byref(p), v(0x30004), v(0x1000), None) == -2 and b"aligned" in lib.fhip_qconv_last_error()


# ---- feather::Net --------------------------------------------------------------------------------------------------------------------
_MODEL = {}


def _tiny():
    """tiny_quant, a seeded batch-3 input and the restatement's blobs per fusion level, computed once."""
    if not _MODEL:
        from feathercnn_amd import model_zoo
        model = model_zoo.tiny_quant()
        x = np.random.default_rng(41).uniform(-1, 1, (3, 3, 16, 16)).astype(F)
        _MODEL.update(model=model, x=x, want={level: R.net_forward(model, x, level) for level in (0, 1, 2)})
    return _MODEL["model"], _MODEL["x"], _MODEL["want"]


def _net(model, level, graph=True):
    from feathercnn_amd.net import Net
    net = Net(fusion=level, graph=graph)
    net.SetQuantized(True)
    net.LoadParam(model[0])
    net.LoadWeights(model[1])
    return net


@pytest.mark.parametrize("level", [0, 1, 2])
def test_tiny_quant_equals_the_restatement_bit_for_bit(cuda, level):
    """Batch 3, graph mode on, every blob the level keeps.  At level 2 the BatchNorm + Scale behind conv3 are folded into its dequantisation
    as feather_qconv.h defines it -- which is NOT what levels 0 and 1 compute, and the restatement shows the difference."""
    from feathercnn_amd import model_zoo
    model, x, want = _tiny()
    net = _net(model, level)
    net.FeedInput("data", x)
    net.Forward()
    net.Forward()  # the second Forward replays the captured graph
    routed = [nm for _, nm, a in net.layers() if a == "QCONV"]
    assert routed == list(model_zoo.QUANT_LAYERS["tiny_quant"])
    for name, ref in want[level].items():
        if name == "data" or (level >= 1 and name in ("conv1", "conv2", "dw", "pw", "conv3_scale")):
            continue  # absorbed by the ReLU fusions: no storage at this level
        got = net.Extract(name)
        assert got.shape == ref.shape and np.array_equal(got, ref), (level, name, int((got != ref).sum()))
    assert np.array_equal(net.Extract("fc"), want[level]["fc"])
    if level == 2:
        assert not {"BatchNorm", "Scale", "ReLU"} & {t for t, _, _ in net.layers()} and not np.array_equal(want[2]["conv3_relu"], want[0]["conv3_relu"])  # the fold is visible in the bits
    net.close()


def test_a_new_batch_size_replans_and_still_matches(cuda):
    model, x, want = _tiny()
    for level in (1, 2):
        net = _net(model, level)
        for n in (3, 5, 1, 3):
            xn = np.concatenate([x, x[::-1]], axis=0)[:n]
            net.FeedInput("data", xn)
            net.Forward()
            ref = R.net_forward(model, xn, level) if n != 3 else want[level]
            for name in ("conv3_relu", "relu_pw", "fc"):
                assert np.array_equal(net.Extract(name), ref[name]), (level, n, name)
        net.close()
