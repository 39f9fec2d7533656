"""The int8 route on q8 tensors (libfeather_q8.so, include/feather_hip/feather_q8.h) on the MI355X.  Every comparison is np.array_equal against
the numpy restatement (tests/q8_ref.py on tests/qconv_ref.py): the definition is exact, so the tolerance is zero.

* every route of every form of every case of tests/q8_cases.py (tests/q8_sweep.py): forced by name, the selected one also through the selecting
  calls; bias + ReLU, bias alone, neither; int8 inputs also with garbage in their pad bytes; every output between guards -- every word
  written, the pad bytes 0, nothing outside touched;
* the requantise rounding: s_out = 0.5 and d = 1 on odd sums (exact halves, both signs), sums that clamp, with and without bias, ReLU, a fold;
* asymmetric weights (the operand maps: a swapped row / column or a permuted k passes symmetric data);
* max pooling, ReLU, quantize and dequantize of a q8 tensor;
* the chain property on the device: conv -> ReLU -> max pool -> conv with q8 tensors between equals the fp32-between form of libfeather_qconv.so;
* one kernel trace (tests/q8_trace_child.py): the sweep launches every instantiation of the library.
"""
import ctypes

import numpy as np
import pytest

import kernel_instances as KI
import ktrace
import q8_cases as QC
import q8_ref as Q
import q8_sweep as SW
import qconv_ref as R
import side_contract
from guarded import Guarded

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module")
def lib(cuda):
    return side_contract.library("q8")


def _same(name, form, route, got, want):
    if form[1]:
        got, pads = got
        assert not pads.any(), (name, route, "pad bytes of the q8 output are not 0")
    bad = np.argwhere(got != want)
    assert got.shape == want.shape and np.array_equal(got, want), (name, form, route, len(bad), bad[:4].tolist())


# ---- every route ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", QC.CASES, ids=[c[0] for c in QC.CASES])
def test_every_route_equals_the_restatement(lib, case):
    told = ctypes.create_string_buffer(160)
    x, q, wq, s_w, s_in, bias = SW.data(case, seed=len(case[0]))
    d = R.dequant_scales(s_w, s_in)
    for form in case[-1]:
        routes = QC.routes(case, form)
        p = QC.param(case, form)
        assert lib.fhip_q8_route(ctypes.byref(p), told, 160) == 0 and told.value.decode() == routes[0], (case[0], form, told.value)
        for has_bias, relu in QC.EPILOGUES:
            b = bias if has_bias else None
            want = SW.want(case, form, x, q, wq, d, b, s_in, relu)
            if form[1]:
                assert 0 < (np.abs(want) == 127).mean() < 0.9 and (want == 0).mean() < 0.9  # the output clamps here and there, and not everywhere
            for i, route in enumerate(routes):
                for selecting, garbage in (((True, False), (False, True)) if i == 0 else ((False, False),)):
                    got = SW.run(lib, case, form, route, x, q, wq, d, b, s_in, relu, selecting, garbage=garbage and form[0])
                    _same(case[0], form, route, got, want)


# ---- the requantise rounding ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", [QC.II, QC.FI], ids=["int8_in", "fp32_in"])
def test_requantise_rounds_half_away_from_zero_and_clamps(lib, form):
    """A 1x1 layer with C = K = 16 whose weights are w * identity: acc[k] = w * q[k].  With d = 1 and s_out = 0.5 every odd sum is an exact
    half -- 63.5 must give 64, -63.5 must give -64 -- and w = 127 makes every |q| > 2 clamp.  A bias of 0.5 moves the halves, a fold
    (d' = 0.75, b' = 0.25) makes the product round, ReLU cuts the negative half."""
    q = np.arange(-127, 128, dtype=np.int32)
    q = np.concatenate([q, q[:1]])  # 256 values = 16 channels x 16 pixels
    q = q.reshape(1, 16, 4, 4)
    x = q.astype(F)  # s_in = 1: quantise(x) = q
    case = ("round", 16, 16, 1, 4, 4, 1, 1, 1, QC.P0, 1, (form,))
    for w in (1, 127):
        wq = (np.eye(16, dtype=np.int8) * w).reshape(16, 16, 1, 1)
        for d, b, relu in ((1.0, None, False), (1.0, None, True), (1.0, 0.5, False), (0.75, 0.25, True), (0.75, 0.25, False)):
            dv = np.full(16, d, F)
            bv = None if b is None else np.full(16, b, F)
            want = Q.conv(q if form[0] else x, wq, dv, bv, 1, (1, 1), QC.P0, relu, None if form[0] else 1.0, 0.5)
            if (w, d, b, relu) == (1, 1.0, None, False):
                assert want[0, 0, 0, 0] == -64 and want.reshape(-1)[127 + 127] == 64 and want.reshape(-1)[127 + 1] == 1 and want.reshape(-1)[127 - 1] == -1
            if w == 127:
                assert (np.abs(want) == 127).sum() >= 120
            for route in QC.routes(case, form):
                got, pads = SW.run(lib, case, form, route, x, q, wq, dv, bv, 1.0, relu, s_out=0.5)
                assert np.array_equal(got, want), (w, d, b, relu, route, got.reshape(-1)[:8], want.reshape(-1)[:8])


@pytest.mark.parametrize("bad", [0.0, -1.0, float("nan"), float("inf")])
def test_a_bad_output_scale_is_refused(lib, bad):
    case = QC.CASES[1]
    p = QC.param(case, QC.II)
    v = ctypes.c_void_p
    rc = lib.fhip_q8_forward(ctypes.byref(p), 1, v(0x10000), v(0x20000), v(0x30000), None, v(0x40000), v(0x50000), 1.0, bad, None)
    assert rc == -2 and b"s_out" in lib.fhip_q8_last_error()


def test_misaligned_tensors_are_refused(lib):
    case = QC.CASES[1]
    v = ctypes.c_void_p
    for form, which, delta in ((QC.II, "out", 4), (QC.II, "x", 8), (QC.IF, "out", 2), (QC.FI, "x", 2), (QC.II, "packed", 4), (QC.II, "d", 2)):
        a = dict(out=0x10000, x=0x20000, packed=0x30000, d=0x40000)
        a[which] += delta
        p = QC.param(case, form)
        rc = lib.fhip_q8_forward(ctypes.byref(p), 1, v(a["out"]), v(a["x"]), v(a["packed"]), None, v(a["d"]), v(0x50000), 1.0, 1.0, None)
        assert rc == -2 and b"aligned" in lib.fhip_q8_last_error(), (form, which, rc)


# ---- asymmetric weights --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("big", [True, False], ids=["128_rows", "64_rows"])
def test_asymmetric_weights_show_the_operand_maps(lib, big):
    """w[k][c][tap] = a value that is different for every (k, c, tap) and an input with ONE non-zero (pixel, channel) at a time would be the
    full check; this is its cheap form: weights k + 3 * c + 7 * tap - 60 (asymmetric in every pair of indices), an input that is 1 in one
    channel per pixel (channel = pixel index mod C).  A permuted k, a swapped row / column or a shifted tap each change the sums."""
    case = ("asym", 24, 20, 1, 5, 4, 3, 3, 1, QC.P1, 2, (QC.II,))
    c, k = 24, 20
    kk, cc, tt = np.meshgrid(np.arange(k), np.arange(c), np.arange(9), indexing="ij")
    wq = (kk + 3 * cc + 7 * tt - 60).astype(np.int8).reshape(k, c, 3, 3)
    q = np.zeros((2, c, 5, 4), np.int32)
    for n in range(2):
        for i in range(20):
            q[n, (i + 5 * n) % c, i // 4, i % 4] = 1 + n
    d = np.ones(k, F)
    for form in (QC.II, QC.IF):
        want = Q.conv(q, wq, d, None, 1, (1, 1), QC.P1, False, None, 1.0 if form[1] else None)
        assert len(np.unique(want)) > 60
        got = SW.run(lib, case, form, QC.MFMA(big, True, form[1]), q.astype(F), q, wq, d, None, 1.0, False, s_out=1.0)
        got = got[0] if form[1] else got
        assert np.array_equal(got, want), (form, np.argwhere(got != want)[:4].tolist())


# ---- the tensor calls ----------------------------------------------------------------------------------------------------------------
def _q8_guarded(t):
    """A q8 tensor (numpy int8) between guards; -> the Guarded."""
    import torch
    g = Guarded(t.size // 4, "poison", 0)
    g.bits().view(torch.int8).copy_(torch.from_numpy(np.ascontiguousarray(t).reshape(-1)))
    return g


def _bytes_of(g, shape):
    import torch
    return g.bits().view(torch.int8).cpu().numpy().reshape(shape)


def test_quantize_and_dequantize(lib):
    """C = 20, 3x5, batch 2: halves, +-inf and NaN at s = 1 and at a scale whose products round; the pad bytes are 0; dequantize divides."""
    import torch
    v = ctypes.c_void_p
    n, c, h, w = 2, 20, 3, 5
    rng = np.random.default_rng(3)
    for s in (1.0, 0.3333333):
        x = (rng.uniform(-140, 140, (n, c, h, w)) / s).astype(F)
        special = np.array([0.5, 1.5, -0.5, -2.5, 0.49999997, -0.49999997, 126.5, 127.5, -127.5, np.inf, -np.inf, np.nan, 0.0, -0.0], F)
        with np.errstate(invalid="ignore", over="ignore"):
            x.reshape(-1)[:28] = np.concatenate([special, (special / F(s)).astype(F)])
        want = Q.quantize(x, s)
        out = Guarded(want.size // 4, "poison", 0)
        tx = torch.from_numpy(x).cuda()
        assert lib.fhip_q8_quantize_forward(v(out.ptr), v(tx.data_ptr()), n, c, h, w, s, side_contract.stream()) == 0, lib.fhip_q8_last_error()
        torch.cuda.synchronize()
        assert out.guards_intact() is None and out.unwritten() == 0
        got = _bytes_of(out, want.shape)
        assert np.array_equal(got, want) and not Q.pad_bytes(got, c).any()
        back = Guarded(n * c * h * w, "poison", 1)
        assert lib.fhip_q8_dequantize_forward(v(back.ptr), v(out.ptr), n, c, h, w, s, side_contract.stream()) == 0, lib.fhip_q8_last_error()
        torch.cuda.synchronize()
        assert back.guards_intact() is None and back.unwritten() == 0
        assert np.array_equal(back.values().reshape(n, c, h, w), Q.dequantize(want, c, s))
    assert lib.fhip_q8_quantize_forward(v(0x1000), v(0x2000), 1, 1, 1, 1, 0.0, None) == -2


def test_relu(lib):
    import torch
    v = ctypes.c_void_p
    q = np.random.default_rng(4).integers(-128, 128, (2, 20, 3, 5)).astype(np.int32)
    t = Q.pack(q)
    src, out = _q8_guarded(t), Guarded(t.size // 4, "poison", 0)
    snap = src.snapshot()
    assert lib.fhip_q8_relu_forward(v(out.ptr), v(src.ptr), t.size, side_contract.stream()) == 0, lib.fhip_q8_last_error()
    torch.cuda.synchronize()
    assert out.guards_intact() is None and out.unwritten() == 0 and src.unchanged(snap)
    assert np.array_equal(_bytes_of(out, t.shape), Q.pack(Q.relu(q)))
    assert lib.fhip_q8_relu_forward(v(src.ptr), v(src.ptr), t.size, side_contract.stream()) == 0  # in place
    torch.cuda.synchronize()
    assert src.guards_intact() is None and np.array_equal(_bytes_of(src, t.shape), Q.pack(Q.relu(q)))
    assert lib.fhip_q8_relu_forward(v(src.ptr), v(src.ptr), 24, None) == -2


@pytest.mark.parametrize("h,w,kernel,stride,pad,glob", [(7, 7, 2, 2, 0, False), (8, 8, 3, 2, 1, False), (5, 6, 2, 2, 0, True), (4, 4, 2, 3, 1, False)],
                         ids=["2x2_s2_clipped", "3x3_s2_p1", "global", "empty_windows"])
def test_max_pool(lib, h, w, kernel, stride, pad, glob):
    """C = 20, batch 2.  7x7 under 2x2 s2 has a clipped last window; with a pad the window origin subtracts both pads, as fhip_pooling;
    4x4 under 2x2 s3 p1 has windows that lie outside the plane: -127, and 0 in the pad bytes."""
    import torch
    from feathercnn_amd import _lib
    v = ctypes.c_void_p
    n, c = 2, 20
    q = np.random.default_rng(h * w).integers(-127, 128, (n, c, h, w)).astype(np.int32)
    want = Q.max_pool(q, kernel, stride, pad, glob)
    if (stride, pad) == (3, 1):
        assert (want == -127).all(axis=(0, 1)).any()  # an empty window
    p = _lib.fhip_pool_param(channels=c, input_h=h, input_w=w, kernel_h=kernel, kernel_w=kernel, stride_h=stride, stride_w=stride, pad_left=pad,
                             pad_right=pad, pad_top=pad, pad_bottom=pad, pooling_type=0, global_pooling=int(glob))
    src = _q8_guarded(Q.pack(q))
    t = Q.pack(want)
    out = Guarded(t.size // 4, "poison", 0)
    snap = src.snapshot()
    assert lib.fhip_q8_max_pool_forward(ctypes.byref(p), n, v(out.ptr), v(src.ptr), side_contract.stream()) == 0, lib.fhip_q8_last_error()
    torch.cuda.synchronize()
    assert out.guards_intact() is None and out.unwritten() == 0 and src.unchanged(snap)
    got = _bytes_of(out, t.shape)
    assert np.array_equal(got, t), np.argwhere(got != t)[:4].tolist()
    p.pooling_type = 1
    assert lib.fhip_q8_max_pool_forward(ctypes.byref(p), n, v(out.ptr), v(src.ptr), None) == -2 and b"max" in lib.fhip_q8_last_error()


# ---- the chain property, through the package ---------------------------------------------------------------------------------------
def test_a_q8_chain_equals_the_fp32_chain_of_the_qconv_library(cuda):
    """conv1 (fp32 in, C = 3) -> ReLU -> 2x2 max pool -> conv2 (C = 20 -> 24, int8 in, fp32 out) with q8 tensors between, against the same two
    layers run by libfeather_qconv.so with fp32 tensors between (conv2's s_in = conv1's s_out): bit for bit, because quantise commutes with
    ReLU and max."""
    import torch
    from feathercnn_amd import Q8Conv, Q8Param, QuantConv, QuantParam, ReLU, None_, q8_max_pool, q8_relu
    rng = np.random.default_rng(8)
    x = rng.uniform(-1, 1, (2, 3, 10, 10)).astype(F)
    w1, w2 = rng.integers(-127, 128, (20, 3, 3, 3)).astype(np.int8), rng.integers(-127, 128, (24, 20, 3, 3)).astype(np.int8)
    s1, s2 = F(127.0), F(11.3)  # conv1's input scale; conv1's output scale = conv2's input scale
    d1 = R.dequant_scales(np.full(20, 40.0, F), s1)
    d2 = R.dequant_scales(np.full(24, 30.0, F), s2)
    b1 = rng.standard_normal(20).astype(F)
    dev = lambda a: torch.from_numpy(a).cuda()

    def layer(conv, p, wq):
        _, pk = conv.GetBufferSize(p)
        packed = torch.empty(pk, dtype=torch.uint8, device="cuda")
        conv.Init(p, packed, dev(wq))
        return packed

    # the q8 chain
    pa = Q8Param.make(3, 20, 10, 3, 1, 1, bias=True, act=None_, batch=2, input_int8=False, output_int8=True)
    pb = Q8Param.make(20, 24, 5, 3, 1, 1, bias=False, act=ReLU, batch=2, input_int8=True, output_int8=False)
    ka, kb = layer(Q8Conv(), pa, w1), layer(Q8Conv(), pb, w2)
    t1 = torch.empty((2, 2, 10, 10, 16), dtype=torch.int8, device="cuda")
    Q8Conv().Forward(pa, t1, dev(x), ka, dev(d1), dev(b1), s_in=s1, s_out=s2)
    t2 = q8_max_pool(q8_relu(t1, out=t1), 20)
    y = torch.empty((2, 24, 5, 5), dtype=torch.float32, device="cuda")
    Q8Conv().Forward(pb, y, t2, kb, dev(d2), None)
    # the fp32 chain
    qa = QuantParam.make(3, 20, 10, 3, 1, 1, bias=True, act=None_, batch=2)
    qb = QuantParam.make(20, 24, 5, 3, 1, 1, bias=False, act=ReLU, batch=2)
    la, lb = layer(QuantConv(), qa, w1), layer(QuantConv(), qb, w2)
    f1 = torch.empty((2, 20, 10, 10), dtype=torch.float32, device="cuda")
    QuantConv().Forward(qa, f1, dev(x), la, dev(d1), dev(b1), s1)
    f2 = torch.nn.functional.max_pool2d(torch.relu(f1), 2)  # plumbing of the comparison only
    z = torch.empty((2, 24, 5, 5), dtype=torch.float32, device="cuda")
    QuantConv().Forward(qb, z, f2.contiguous(), lb, dev(d2), None, s2)
    torch.cuda.synchronize()
    y, z = y.cpu().numpy(), z.cpu().numpy()
    want = R.qconv(np.maximum(R.qconv(x, w1, d1, s1, b1, 1, (1, 1), QC.P1), 0).reshape(2, 20, 5, 2, 5, 2).max(axis=(3, 5)), w2, d2, s2, None, 1, (1, 1), QC.P1, True)
    assert np.abs(want).max() > 0 and np.array_equal(z, want) and np.array_equal(y, want), (int((y != want).sum()), int((z != want).sum()))


# ---- the kernel trace ----------------------------------------------------------------------------------------------------------------
def test_the_sweep_launches_every_instantiation(cuda, tmp_path):
    """One child under rocprofv3 --kernel-trace (tests/q8_trace_child.py, a run of its own): the sweep of tests/q8_sweep.py and the four tensor
    calls launch every instantiation tests/q8_cases.targets() names -- which is every instantiation the library holds
    (tests/test_q8_contract_cpu.py)."""
    _, rows, _ = ktrace.trace("q8_trace_child.py", [], tmp_path, 240)
    launched = {KI.normalise(name) for _, name, *_ in rows}
    assert launched, "the trace holds no kernel"
    missing = sorted(QC.targets() - launched)
    assert not missing, (missing, sorted(n for n in launched if "q8_" in n))
