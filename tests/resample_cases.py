"""The shape table of libfeather_resample.so (Interp and HardSwish), shared by tests/test_resample_cpu.py and tests/test_resample_gpu.py:
the smallest shapes at which each path of the library can go wrong, and the kernel instantiation each of them must select
(include/feather_hip/feather_resample.h, fhip_interp_route).
"""
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "feathercnn_amd", "libfeather_resample.so")

NEAREST, BILINEAR = 1, 2

# (in_h, in_w) -> (out_h, out_w)
PLANES = [((1, 1), (1, 1)), ((1, 1), (3, 3)),  # a single pixel: every tap is that pixel
          ((1, 6), (2, 12)), ((6, 1), (12, 3)),  # one row / one column: the second tap of that axis is the first
          ((2, 2), (3, 5)), ((3, 3), (6, 6)),  # 3x3 -> 6x6: x2, output width no multiple of 4
          ((4, 4), (8, 8)), ((7, 7), (14, 14)), ((13, 13), (26, 26)),  # x2: aligned; odd input width (14 % 4 != 0); more than a few rows
          ((5, 3), (8, 8)), ((9, 7), (4, 3)), ((12, 12), (5, 5)),  # non-integer up-scale onto an aligned width; down-scales
          ((8, 8), (8, 8)), ((4, 4), (16, 16)), ((6, 10), (18, 30)),  # identity, x4, x3
          ((16, 16), (8, 8)),  # a down-scale onto an aligned width: still the general path
          ((40, 36), (80, 72))]  # x2 with more than one block of 256 lanes per image: 2 * 3 * 40 * 18 units

# integer scales, where torch's `nearest` is the same rule
INTEGER_SCALES = [(i, o) for i, o in PLANES if o[0] % i[0] == 0 and o[1] % i[1] == 0 and o[0] // i[0] == o[1] // i[1]]

CHANNELS = (1, 3, 17)
BATCHES = (1, 3)
OFFSETS = (0, 1, 2, 3)  # floats past a 16-byte boundary: 0 / 4 / 8 / 12 bytes

KERNELS = {"interp_nearest2x_kernel", "interp_vec4_kernel", "interp_gather_kernel", "hardswish_kernel"}

HARDSWISH_SIZES = (1, 3, 4, 1023, 4096 + 1)
HARDSWISH_PARAMS = ((0.2, 0.5), (1.0 / 6, 0.5))


def targets():
    """Every instantiation the library holds, as rocprofv3 and fhip_interp_route name it."""
    return ({"fhip::interp_nearest2x_kernel"} | {f"fhip::interp_{k}_kernel<{m}>" for k in ("vec4", "gather") for m in (1, 2)}
            | {f"fhip::hardswish_kernel<{v}>" for v in ("true", "false")})


def by_scale(i, o):
    """(height_scale, width_scale) that give plane `o` from plane `i` through int(in * scale), or None where no float32 scale is needed to
    be found: the smallest scale whose float32 product truncates to the wanted size."""
    import numpy as np
    out = []
    for n_in, n_out in zip(i, o):
        s = np.float32(n_out) / np.float32(n_in)
        for _ in range(4):  # step up until the float32 product reaches n_out
            if int(np.float32(n_in) * s) >= n_out:
                break
            s = np.nextafter(s, np.float32(np.inf), dtype=np.float32)
        assert int(np.float32(n_in) * s) == n_out, (n_in, n_out)
        out.append(float(s))
    return tuple(out)


def expected_route(mode, i, o, hs, ws, out_off=0, in_off=0, res_off=0):
    """The header's selection.  hs / ws: the layer's scales (0 where the size was given); offsets in floats past a 16-byte boundary."""
    import numpy as np
    step = lambda s, n_in, n_out: np.float32(1) / np.float32(s) if s else np.float32(n_in) / np.float32(n_out)
    if o[1] % 4 or out_off % 4 or res_off % 4:
        return f"fhip::interp_gather_kernel<{mode}>"
    if (mode == NEAREST and o[0] == 2 * i[0] and o[1] == 2 * i[1] and step(hs, i[0], o[0]) == 0.5 and step(ws, i[1], o[1]) == 0.5
            and in_off % 2 == 0):
        return "fhip::interp_nearest2x_kernel"
    return f"fhip::interp_{'vec4' if o[0] >= i[0] and o[1] >= i[1] else 'gather'}_kernel<{mode}>"


def cases():
    """(mode, align_corner, in plane, out plane, by): every row of PLANES in both modes, both align_corner values (bilinear) and with the
    size given ("size") and decided by a scale ("scale")."""
    out = []
    for i, o in PLANES:
        for by in ("size", "scale"):
            out.append((NEAREST, 0, i, o, by))
            for align in (0, 1):
                out.append((BILINEAR, align, i, o, by))
    return out
