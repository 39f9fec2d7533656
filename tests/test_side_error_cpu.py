"""The error state of the ten side libraries (feathercnn_amd/csrc_side/side_error.h): a refusal returns non-zero and leaves its text in
fhip_<x>_last_error of the calling thread, and of that thread only."""
import threading

import pytest

# library -> (symbol, arguments) of a call the host checks refuse before anything reaches the device
REFUSED = {
    "pixout": ("fhip_float_to_pixels", (None, 0, None, 0, 0, 0, 0, 0, 0, None, None, None)),
    "gconv": ("fhip_gconv_get_buffer_size", (None, 1, None, None)),
    "deconv": ("fhip_deconv_assign_output_dim", (None,)),
    "inorm": ("fhip_instance_norm_get_buffer_size", (0, 0, 0, 0, None)),
    "shuffle": ("fhip_channel_shuffle_forward", (None, None, 0, 0, 0, 0, 0, 0, None)),
    "canvas": ("fhip_canvas_output_transform", (None, 0, None, None, None, None, 0, None)),
    "atrous": ("fhip_atrous_assign_output_dim", (None,)),
    "gate": ("fhip_squeeze_get_buffer_size", (0, 0, 0, 0, None)),
    "resample": ("fhip_interp_output_dim", (0, 0, 0.0, 0.0, 0, 0, None, None)),
    "lrn": ("fhip_lrn_forward", (0, 0, 0.0, 0.0, 0.0, 0, 0, 0, 0, None, None, None)),
}


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_last_error_is_set_and_thread_local(name):
    from feathercnn_amd import _lib
    lib = getattr(_lib, f"load_{name}_library")()
    last_error = getattr(lib, f"fhip_{name}_last_error")
    symbol, args = REFUSED[name]
    assert getattr(lib, symbol)(*args) != 0
    assert last_error() != b""
    seen = []
    t = threading.Thread(target=lambda: seen.append(last_error()))
    t.start()
    t.join()
    assert seen == [b""]  # a thread that made no call has no error
    assert last_error() != b""
