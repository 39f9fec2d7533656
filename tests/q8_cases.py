"""The shape table of the q8 tests (tests/test_q8_cpu.py, tests/test_q8_gpu.py, tests/test_q8_contract_cpu.py): every kernel instantiation of
libfeather_q8.so has a case that selects it, and routes() lists all routes that can run a case in one form.

A case: (name, C, K, group, H, W, kh, kw, stride, pads (left, right, top, bottom), batch, forms); a form is (input is int8, output is int8).
The shapes are the smallest at which a route can go wrong: C = 24 and 20 leave 8 and 12 pad bytes in the last channel block, K = 20 / 70 / 130
are ragged against the 16-row tiles and both block heights, 3 * 35 = 105 pixel columns are ragged against the 64-column block and need two of
them, R = 144 (and 9 * 32 = 288) is no multiple of the instruction's 64."""
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "feathercnn_amd", "libfeather_q8.so")

_B = {True: "true", False: "false"}


def MFMA(big, in8, out8):
    return f"fhip::q8_mfma_kernel<{'4, 1' if big else '2, 2'}, {_B[in8]}, {_B[out8]}>"


def DW(out8):
    return f"fhip::q8_dw_kernel<{_B[out8]}>"


def GENERIC(dw):
    return f"fhip::q8_generic_kernel<{_B[dw]}>"


HELPERS = {"fhip::q8_quantize_kernel", "fhip::q8_dequantize_kernel", "fhip::q8_relu_kernel", "fhip::q8_max_pool_kernel", "fhip::q8_pack_mfma_kernel",
           "fhip::q8_pack_generic_kernel", "fhip::q8_pack_dw_kernel"}

II, IF, FI = (True, True), (True, False), (False, True)
P1 = (1, 1, 1, 1)
P0 = (0, 0, 0, 0)
P2 = (2, 2, 2, 2)
CASES = [
    ("mfma_c24_k20_3x3", 24, 20, 1, 7, 5, 3, 3, 1, P1, 3, (II, IF)),           # 105 columns, a ragged last chunk (R' = 288), 12 pad bytes out
    ("mfma_c16_k70_1x1", 16, 70, 1, 6, 6, 1, 1, 1, P0, 2, (II, IF, FI)),
    ("mfma_k130", 16, 130, 1, 5, 7, 1, 1, 1, P0, 3, (II, IF, FI)),             # two row tiles of the 128-row block, three of the 64-row one
    ("mfma_c32_k32_3x3_s2", 32, 32, 1, 9, 10, 3, 3, 2, (0, 1, 1, 0), 2, (II, IF, FI)),
    ("mfma_r144", 16, 20, 1, 5, 7, 3, 3, 1, P1, 3, (II, IF, FI)),
    ("mfma_c3_k20", 3, 20, 1, 6, 6, 3, 3, 1, P1, 2, (II, IF)),                 # int8 in takes any C: 13 pad channels per tap
    ("dw_c20_3x3_s1", 20, 20, 20, 7, 7, 3, 3, 1, P1, 2, (II, IF)),
    ("dw_c20_3x3_s2", 20, 20, 20, 8, 9, 3, 3, 2, P1, 2, (II, IF)),
    ("dw_c20_5x5", 20, 20, 20, 7, 6, 5, 5, 1, P2, 2, (II, IF)),
    ("generic_c3_k16", 3, 16, 1, 6, 7, 3, 3, 1, P1, 2, (FI,)),
    ("generic_c3_k6", 3, 6, 1, 9, 8, 5, 5, 2, P2, 2, (FI,)),
    ("generic_c24_k20", 24, 20, 1, 5, 5, 3, 3, 1, P1, 2, (FI,)),               # fp32 in with C % 16 != 0
    ("generic_dw_c8", 8, 8, 8, 6, 5, 3, 3, 1, P1, 2, (FI,)),
]
EPILOGUES = ((1, 1), (1, 0), (0, 0))  # (bias, relu)


def routes(case, form):
    """Every route that runs the case in this form; routes[0] is the one fhip_q8_route reports."""
    _, c, k, group, *_ = case
    in8, out8 = form
    if group > 1:
        return (DW(out8),) if in8 else (GENERIC(True),)
    if in8 or c % 16 == 0:
        big = k > 64
        return (MFMA(big, in8, out8), MFMA(not big, in8, out8)) + (() if in8 else (GENERIC(False),))
    return (GENERIC(False),)


def all_routes():
    return {MFMA(b, i, o) for b in (True, False) for i, o in (II, IF, FI)} | {DW(True), DW(False), GENERIC(True), GENERIC(False)}


def targets():
    return {r for c in CASES for f in c[-1] for r in routes(c, f)} | HELPERS


def param(case, form, bias=1, relu=0, **over):
    """fhip_q8_param of a case in one form (the ctypes struct)."""
    from feathercnn_amd import _lib
    _, c, k, group, h, w, kh, kw, s, (pl, pr, pt, pb), _, _ = case
    p = _lib.fhip_q8_param(output_channels=k, input_channels=c, input_h=h, input_w=w, kernel_h=kh, kernel_w=kw,
                           output_h=(h + pt + pb - kh) // s + 1, output_w=(w + pl + pr - kw) // s + 1, stride_h=s, stride_w=s, pad_left=pl,
                           pad_bottom=pb, pad_right=pr, pad_top=pt, group=group, bias_term=bias, activation=relu, dilation_h=1, dilation_w=1,
                           int8_scale_term=101 if form[1] else 1, input_int8=int(form[0]), output_int8=int(form[1]))
    for name, v in over.items():
        setattr(p, name, v)
    return p
