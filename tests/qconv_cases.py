"""The shape table of the int8 convolution tests (tests/test_qconv_cpu.py, tests/test_qconv_gpu.py): every kernel instantiation of
libfeather_qconv.so has a case that selects it, and every case lists all routes that can run it (fhip_qconv_*_route).

A case: (name, C, K, group, H, W, kh, kw, stride, pads (left, right, top, bottom), batches, routes); routes[0] is the one
fhip_qconv_route reports.  The shapes are the smallest at which a route can go wrong: R = 144 is no multiple of the instruction's 64, K = 20
/ 70 / 130 are ragged against the 16-row tiles, both block heights and the 16-channel chunks of the wider generic kernel, 3 * 35 = 105 pixel columns are ragged against the 64-column block and
need two of them, 19 depthwise channels and a 6-wide row are ragged against the four-output strips."""
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "feathercnn_amd", "libfeather_qconv.so")

MFMA128 = "fhip::qconv_mfma_kernel<4, 1>"
MFMA64 = "fhip::qconv_mfma_kernel<2, 2>"
GENERIC = "fhip::qconv_generic_kernel<4>"
GENERIC16 = "fhip::qconv_generic_kernel<16>"
DW1 = "fhip::qconv_dw3x3_kernel<1>"
DW2 = "fhip::qconv_dw3x3_kernel<2>"
HELPERS = {"fhip::quantize_kernel", "fhip::qconv_pack_generic_kernel", "fhip::qconv_pack_dw_kernel", "fhip::qconv_pack_mfma_kernel"}

P1 = (1, 1, 1, 1)
P0 = (0, 0, 0, 0)
CASES = [
    ("mfma_3x3_s1", 16, 20, 1, 5, 7, 3, 3, 1, P1, (3,), (MFMA64, MFMA128, GENERIC, GENERIC16)),
    ("mfma_3x3_s2", 16, 20, 1, 6, 9, 3, 3, 2, P1, (3,), (MFMA64, MFMA128, GENERIC, GENERIC16)),
    ("mfma_1x1", 64, 16, 1, 4, 4, 1, 1, 1, P0, (3,), (MFMA64, MFMA128, GENERIC, GENERIC16)),
    ("mfma_k130", 16, 130, 1, 5, 7, 1, 1, 1, P0, (3,), (MFMA128, MFMA64, GENERIC, GENERIC16)),
    ("mfma_asymmetric_pads", 32, 70, 1, 6, 5, 3, 3, 1, (0, 2, 1, 0), (3,), (MFMA128, MFMA64, GENERIC, GENERIC16)),
    ("generic_5x5_c3", 3, 5, 1, 6, 6, 5, 5, 1, (2, 2, 2, 2), (3,), (GENERIC, GENERIC16)),
    ("generic16_7x7_c3", 3, 20, 1, 9, 8, 7, 7, 2, (3, 3, 3, 3), (3,), (GENERIC16, GENERIC)),
    ("dw3x3_s1", 19, 19, 19, 5, 6, 3, 3, 1, P1, (3,), (DW1, GENERIC, GENERIC16)),
    ("dw3x3_s2", 19, 19, 19, 5, 6, 3, 3, 2, P1, (3,), (DW2, GENERIC, GENERIC16)),
    ("dw5x5_generic", 6, 6, 6, 7, 5, 5, 5, 1, (2, 2, 2, 2), (3,), (GENERIC, GENERIC16)),
    ("inner_product", 80, 10, 1, 1, 1, 1, 1, 1, P0, (1, 5), (MFMA64, MFMA128, GENERIC, GENERIC16)),
]
EPILOGUES = ((1, 1), (1, 0), (0, 0))  # (bias, relu)


def targets():
    return {r for c in CASES for r in c[-1]} | HELPERS


def param(case, bias=1, relu=0, **over):
    """fhip_qconv_param of a case (the ctypes struct)."""
    from feathercnn_amd import _lib
    _, c, k, group, h, w, kh, kw, s, (pl, pr, pt, pb), _, _ = case
    p = _lib.fhip_qconv_param(output_channels=k, input_channels=c, input_h=h, input_w=w, kernel_h=kh, kernel_w=kw,
                              output_h=(h + pt + pb - kh) // s + 1, output_w=(w + pl + pr - kw) // s + 1, stride_h=s, stride_w=s, pad_left=pl,
                              pad_bottom=pb, pad_right=pr, pad_top=pt, group=group, bias_term=bias, activation=relu, dilation_h=1, dilation_w=1,
                              int8_scale_term=1)
    for name, v in over.items():
        setattr(p, name, v)
    return p
