"""The image output path without a GPU: libfeather_pixout.so (include/feather_hip/feather_pixout.h) refuses bad arguments on the host
before any device call; the GPU sweep's table (tests/pixout_cases.py) has the size it states; the Python wrappers refuse what the
library refuses; and the numpy restatement the GPU tests compare against equals the reference's recorded to_pixels results.
What the library shares with the other run-time libraries -- its exports, the instantiations it holds, its route code, the build
of its application, its last-error state -- is in tests/test_side_contract_cpu.py."""
import ctypes
import os

import numpy as np
import pytest

import pixels_ref as R
import pixout_cases as PC
import side_contract
import yuv_ref as Y

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BADARG = -2  # FHIP_E_BADARG


lib = side_contract.fixture("pixout")


def _call(lib, pixels=0x1000, pitch=0, x=0x2000, batch=1, ptype=R.PIXEL_RGB, w=8, h=8, tw=8, th=8, mean=None, norm=None):
    """fhip_float_to_pixels with made-up device addresses: a call the host checks refuse never reaches the device, so they are never read."""
    return lib.fhip_float_to_pixels(ctypes.c_void_p(pixels), pitch, ctypes.c_void_p(x), batch, ptype, w, h, tw, th, mean, norm, None)


def test_refusals_come_before_any_device_call(lib):
    for t in PC.REFUSED + [0, 3, 16, R.PIXEL_RGB | (R.PIXEL_RGB << 16), R.PIXEL_RGBA | (R.PIXEL_RGBA << 16), -1]:
        assert _call(lib, ptype=t) == BADARG, hex(t)
        assert b"output pixel type" in lib.fhip_pixout_last_error()
        assert lib.fhip_pixout_channels(t) == BADARG
    for name, t in PC.TYPES.items():
        assert lib.fhip_pixout_channels(t) == PC.CHANNELS[t], name
    assert _call(lib, pixels=None) == BADARG and _call(lib, x=None) == BADARG
    assert _call(lib, x=0x2002) == BADARG and b"aligned" in lib.fhip_pixout_last_error()
    for kw in ({"batch": 0}, {"w": 0}, {"h": 0}, {"tw": 0}, {"th": -1}):
        assert _call(lib, **kw) == BADARG, kw
    # a pitch smaller than a row of the type
    assert _call(lib, pitch=8 * 3 - 1) == BADARG and b"pitch" in lib.fhip_pixout_last_error()
    assert _call(lib, ptype=R.PIXEL_RGBA, pitch=8 * 4 - 1) == BADARG
    assert _call(lib, ptype=R.PIXEL_GRAY, pitch=7) == BADARG
    # a 1-pixel source axis cannot be resized (the reference reads index -1), as on the input side
    assert _call(lib, w=1, h=8, tw=4, th=8) == BADARG and b"1 pixel" in lib.fhip_pixout_last_error()
    assert _call(lib, w=8, h=1, tw=8, th=2) == BADARG
    # the host-destination form checks the same way
    assert lib.fhip_float_to_pixels_host(None, 0, ctypes.c_void_p(0x2000), 1, R.PIXEL_RGB, 8, 8, 8, 8, None, None, None) == BADARG
    assert lib.fhip_float_to_pixels_host(ctypes.c_void_p(0x1000), 0, ctypes.c_void_p(0x2000), 1, R.PIXEL_RGB2GRAY, 8, 8, 8, 8, None, None,
                                         None) == BADARG


def test_python_wrappers_refuse_before_the_library():
    import torch

    from feathercnn_amd import FeatherHipError, float_to_pixels
    for t in PC.REFUSED:
        with pytest.raises(FeatherHipError, match="not an output type"):
            float_to_pixels(torch.zeros(1, 3, 4, 4), t)
    for t, c in ((R.PIXEL_RGB, 1), (R.PIXEL_GRAY, 3), (R.PIXEL_RGBA, 3), (R.PIXEL_BGR2RGB, 4)):
        with pytest.raises(FeatherHipError, match=r"x: \[N\]"):  # C is not the type's channel count
            float_to_pixels(torch.zeros(2, c, 4, 4), t)
    with pytest.raises(FeatherHipError, match="CUDA"):
        float_to_pixels(torch.zeros(1, 3, 4, 4), R.PIXEL_RGB)  # no quiet host path


def test_every_instantiation_has_a_case():
    assert len(PC.cases()) == len(PC.TYPES) * len(PC.GEOMETRIES) * len(PC.MEAN_NORM) * len(PC.BATCHES) * 2


def test_main_library_keeps_its_instantiations():
    shared = os.path.join(ROOT, "feathercnn_amd", "csrc", "pixel_resample.h")
    assert "__global__" not in open(shared).read()  # helpers only: the census of feathercnn_amd/csrc scans this header too


def test_sweep_inputs_reach_both_clamps_and_truncate():
    """What the GPU sweep asserts of each pool, on the small geometries here: mapped values below 0, above 255 and with fractions."""
    for _, t, gn, (w, h, tw, th), form in PC.combos():
        if w * h > 4096:
            continue
        cn = PC.CHANNELS[t]
        mean, norm = PC.mean_norm(form, cn)
        v = R.mean_norm(PC.make_input(1, 4, cn, h, w, mean, norm), mean, norm)
        assert (v < 0).any() and (v > 255).any() and (v != np.trunc(v)).any(), (gn, form)
        assert np.abs(v).max() < 2.0 ** 31


def test_restatement_equals_the_recorded_reference():
    """Mat::to_pixels / to_pixels_resize as the reference computed them (tests/golden/yuv_golden.npz), per image and stacked the way the
    GPU tests build their batches."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "yuv_golden.npz"))
    assert len(g["topixels"]) >= 10
    for t, w, h, c, tw, th in g["topixels"]:
        m = g[f"mat_{w}x{h}x{c}"]
        assert PC.CHANNELS[int(t)] == c
        assert np.array_equal(Y.to_pixels_resize(m, int(t), int(tw), int(th)), g[f"topix_{t}_{w}x{h}x{c}_{tw}x{th}"])
    # substract_mean_normalize is per plane of the Mat: reversed types read plane 2 - k AFTER the mapping
    x = PC.make_input(3, 1, 3, 5, 7, *PC.mean_norm("both", 3))
    v = R.mean_norm(x, *PC.mean_norm("both", 3))[0]
    assert np.array_equal(Y.to_pixels(v, R.PIXEL_RGB2BGR), Y.to_pixels(v, R.PIXEL_RGB)[..., ::-1])
