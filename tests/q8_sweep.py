"""One way to run a layer of tests/q8_cases.py on the device and to restate it: run() packs and launches one (case, form, route) through the
C-ABI of libfeather_q8.so with the output in a guarded buffer (tests/guarded.py), want() is tests/q8_ref.py's answer, and sweep() walks every
route of every case once -- tests/test_q8_gpu.py compares, tests/q8_trace_child.py runs it under the kernel trace."""
import ctypes

import numpy as np

import q8_cases as QC
import q8_ref as Q
import qconv_ref as R
import side_contract
from guarded import Guarded, describe

F = np.float32
V = ctypes.c_void_p
S_OUT = F(0.37)  # a requantisation scale whose products round in fp32


def data(case, seed):
    """(x fp32, q = quantise(x; s_in), wq, s_w, s_in, bias) of a case."""
    _, c, k, group, h, w, kh, kw, _, _, batch, _ = case
    x, wq, s_w, s_in, bias = R.synth(c, k, h, w, kh, kw, group, batch, seed=seed)
    # dequantised values over the whole q range of the next layer and past it: the sums have a deviation of about sqrt(R) * 73 * 73, and
    # these weight scales bring y to a deviation of 150 .. 600, which S_OUT turns into 55 .. 220
    r = c // group * kh * kw
    s_w = (np.random.default_rng(seed + 1).uniform(0.5, 2.0, k) * np.sqrt(r) * 5400.0 / (300.0 * s_in)).astype(F)
    s_w[0] = 0.0  # ncnn's convention: d = 0
    return x, R.quantise(x, s_in), wq, s_w, s_in, bias


def want(case, form, x, q, wq, d, b, s_in, relu, s_out=S_OUT):
    """The restatement: fp32 NCHW, or the int32 NCHW content of the q8 output."""
    _, c, k, group, h, w, kh, kw, s, pads, _, _ = case
    return Q.conv(q if form[0] else x, wq, d, b, group, (s, s), pads, relu, None if form[0] else s_in, s_out if form[1] else None)


def run(lib, case, form, route, x, q, wq, d, b, s_in, relu, selecting=False, garbage=False, s_out=S_OUT):
    """Pack and run one layer under `route` (selecting: through fhip_q8_init / fhip_q8_forward).  The output lies between guards and starts
    as poison: -> fp32 NCHW, or (the int32 NCHW content of the q8 output, its pad bytes); asserts that every word was written and no guard
    word changed.  garbage: the pad bytes of a q8 input hold 0x55 instead of 0."""
    import torch
    _, c, k, group, h, w, kh, kw, s, pads, batch, _ = case
    p = QC.param(case, form, bias=0 if b is None else 1, relu=int(relu))
    sb, pk = ctypes.c_size_t(), ctypes.c_size_t()
    rn = route.encode()
    err = lib.fhip_q8_last_error
    if selecting:
        assert lib.fhip_q8_get_buffer_size(ctypes.byref(p), batch, ctypes.byref(sb), ctypes.byref(pk)) == 0, err()
    else:
        assert lib.fhip_q8_get_buffer_size_route(ctypes.byref(p), batch, rn, ctypes.byref(sb), ctypes.byref(pk)) == 0, err()
    assert sb.value == 0 and pk.value % 16 == 0
    tw = torch.from_numpy(wq).cuda()
    packed = torch.full((pk.value,), 0x5A, dtype=torch.uint8, device="cuda")
    tin = torch.from_numpy(Q.pack(q, 0x55 if garbage else 0) if form[0] else x).cuda()
    td = torch.from_numpy(d).cuda()
    tb = None if b is None else torch.from_numpy(b).cuda()
    oh, ow = p.output_h, p.output_w
    words = batch * Q.blocks(k) * oh * ow * 4 if form[1] else batch * k * oh * ow
    out = Guarded(words, "poison", 0)
    bp = V(tb.data_ptr()) if tb is not None else None
    stream = side_contract.stream()
    if selecting:
        rc = lib.fhip_q8_init(ctypes.byref(p), V(packed.data_ptr()), V(tw.data_ptr()), stream)
        rc = rc or lib.fhip_q8_forward(ctypes.byref(p), batch, V(out.ptr), V(tin.data_ptr()), V(packed.data_ptr()), None, V(td.data_ptr()), bp, float(s_in),
                                       float(s_out), stream)
    else:
        rc = lib.fhip_q8_init_route(ctypes.byref(p), V(packed.data_ptr()), V(tw.data_ptr()), stream, rn)
        rc = rc or lib.fhip_q8_forward_route(ctypes.byref(p), batch, V(out.ptr), V(tin.data_ptr()), V(packed.data_ptr()), None, V(td.data_ptr()), bp,
                                             float(s_in), float(s_out), stream, rn)
    assert rc == 0, err()
    torch.cuda.synchronize()
    assert out.guards_intact() is None, (case[0], route, describe(out.guards_intact()))
    assert out.unwritten() == 0, (case[0], route, out.unwritten())
    if not form[1]:
        return out.values().reshape(batch, k, oh, ow)
    t = out.bits().view(torch.int8).cpu().numpy().reshape(batch, Q.blocks(k), oh, ow, 16)
    return Q.unpack(t, k), Q.pad_bytes(t, k)


def sweep(lib, check):
    """Every route of every form of every case, each epilogue; the selected route also through the selecting calls, int8 inputs also with
    garbage in their pad bytes.  check(case name, form, route, got, want) sees every result."""
    for ci, case in enumerate(QC.CASES):
        x, q, wq, s_w, s_in, bias = data(case, seed=100 + ci)
        d = R.dequant_scales(s_w, s_in)
        for form in case[-1]:
            routes = QC.routes(case, form)
            for has_bias, relu in QC.EPILOGUES:
                b = bias if has_bias else None
                ref = want(case, form, x, q, wq, d, b, s_in, relu)
                for i, route in enumerate(routes):
                    for selecting in ((True, False) if i == 0 else (False,)):
                        got = run(lib, case, form, route, x, q, wq, d, b, s_in, relu, selecting, garbage=form[0] and not selecting)
                        check(case[0], form, route, got, ref)
