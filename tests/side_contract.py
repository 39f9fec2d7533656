"""What the tests of the contract every run-time library shares need and feathercnn_amd/_lib.LIBRARIES does not hold, once: a row per side
library (SIDE), the call each library's host checks refuse (REFUSED), the main library's instantiation count, and the three helpers the
per-library test files use -- library(), stream() and build_app().  tests/test_side_contract_cpu.py and tests/test_side_contract_gpu.py
state the contract over these tables; a new library adds one row to _lib.LIBRARIES and one here and gets all of it."""
import collections
import ctypes
import importlib
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")

# cases: the module whose targets() names every instantiation of the library's code object (None: CANVAS_TARGETS below)
# shared: kernels of the main tree the library instantiates next to those its csrc_<x>/ declares
# kernels: the base names of its kernels, where its tests state them
# forbidden: words its sources do not hold ("atomic": after the first #include, below the comment that may speak of it)
# app: the reference-style application under tests/cpp/ and what its compile line adds
# switch: the Net switch a net needs before it loads the library's layers, as (C-ABI symbol, feather::Net method)
# wrappers: the public names of the package that call the library
Side = collections.namedtuple("Side", "cases shared kernels forbidden app switch wrappers", defaults=(set(), None, (), None, None, ()))
SIDE = {
    "pixout": Side("pixout_cases", app=("pixout_app_main.cpp", ["-ffp-contract=off"])),
    "gconv": Side("gconv_cases", app=("gconv_app_main.cpp", [])),
    "deconv": Side("deconv_cases", shared={"gemm_mfma_kernel"}, app=("deconv_app_main.cpp", [])),  # the shared main loop of csrc/gemm_core.h
    "inorm": Side("inorm_cases", wrappers=("instance_norm", "activation")),
    "shuffle": Side("shuffle_cases", kernels={"channel_map_kernel"}, wrappers=("channel_shuffle", "channel_slice", "channel_map")),
    "canvas": Side(None),
    "atrous": Side("atrous_cases", shared={"gemm_mfma_kernel"}, app=("atrous_app_main.cpp", []), switch=("fhip_net_set_dilated", "SetDilated")),
    "gate": Side("gate_cases", kernels="KERNELS", forbidden=("atomic",), app=("gate_app_main.cpp", []),  # fixed-order sums only
                 wrappers=("channel_gate", "squeeze", "excite", "gate_activation")),
    "resample": Side("resample_cases", kernels="KERNELS", forbidden=("atomic", "hipMalloc", "hipMemcpy"), app=("resample_app_main.cpp", []),
                     switch=("fhip_net_set_extended_layers", "SetExtendedLayers"), wrappers=("interp", "interp_output_dim", "interp_route", "hard_swish")),
    "lrn": Side("lrn_cases", kernels="KERNELS", forbidden=("atomic", "hipMalloc", "hipMemcpy", "getenv"),  # a forward only launches
                switch=("fhip_net_set_extended_layers", "SetExtendedLayers"), wrappers=("lrn", "lrn_pool", "lrn_route", "lrn_pool_route")),
    "qconv": Side("qconv_cases", switch=("fhip_net_set_quantized", "SetQuantized"),
                  wrappers=("QuantConv", "QuantParam", "quantize", "qconv_route", "dequant_scales")),
}
# the canvas library has no sweep table of its own (tests/test_canvas_gpu.py runs it through the chain): bias x ReLU on both kernels, the
# chain in its three forms (the first also for several images per canvas), the output transform with and without the 2x2 pooling
_B = ("false", "true")
CANVAS_TARGETS = ({f"fhip::canvas_chain_kernel<{b}, {r}, {fm}>" for b in _B for r in _B for fm in ("1, false", "1, true", "2, false", "3, false")} |
                  {f"fhip::canvas_output_kernel<{b}, {r}, {p}>" for b in _B for r in _B for p in _B})
# struct -> (the struct whose fields it starts with, the fields it adds)
STRUCT_TAILS = {"fhip_atrous_param": ("fhip_conv_param", ["dilation_h", "dilation_w"]), "fhip_qconv_param": ("fhip_atrous_param", ["int8_scale_term"])}
# library -> (symbol, arguments, word of the message or None) of a call the host checks refuse with FHIP_E_BADARG before anything reaches the device
REFUSED = {
    "pixout": ("fhip_float_to_pixels", (None, 0, None, 0, 0, 0, 0, 0, 0, None, None, None), None),
    "gconv": ("fhip_gconv_get_buffer_size", (None, 1, None, None), None),
    "deconv": ("fhip_deconv_assign_output_dim", (None,), None),
    "inorm": ("fhip_instance_norm_get_buffer_size", (0, 0, 0, 0, None), None),
    "shuffle": ("fhip_channel_shuffle_forward", (None, None, 0, 0, 0, 0, 0, 0, None), None),
    "canvas": ("fhip_canvas_output_transform", (None, 4, None, None, None, None, 0, None), "bad argument"),
    "atrous": ("fhip_atrous_assign_output_dim", (None,), None),
    "gate": ("fhip_squeeze_get_buffer_size", (0, 0, 0, 0, None), None),
    "resample": ("fhip_interp_output_dim", (0, 0, 0.0, 0.0, 0, 0, None, None), None),
    "lrn": ("fhip_lrn_forward", (0, 0, 0.0, 0.0, 0.0, 0, 0, 0, 0, None, None, None), None),
    "qconv": ("fhip_qconv_assign_output_dim", (None,), None),
}
BADARG = -2  # FHIP_E_BADARG


def main_library_holds(names):
    """The number of instantiations of this tree's main library; a change to it must come with the sweep cases (or removals) that account
    for it (tests/instance_cases.py)."""
    assert len(names) == 176, f"{len(names)} instantiations of the main library, expected 176"


def targets(name) -> set:
    """Every kernel instantiation the side library `name` holds, as its sweep table names them."""
    row = SIDE[name]
    return set(importlib.import_module(row.cases).targets()) if row.cases else set(CANVAS_TARGETS)


def kernels(name):
    """The base names of the library's kernels where its tests state them, else None."""
    row = SIDE[name]
    return getattr(importlib.import_module(row.cases), row.kernels) if isinstance(row.kernels, str) else row.kernels


def library(name):
    """The loaded library `name` of _lib.LIBRARIES; a tree that was not built fails the test."""
    from feathercnn_amd import _lib
    if not os.path.exists(_lib.path(name)):
        pytest.fail(f"{_lib.path(name)} is missing: run build() first")
    return _lib.load(name)


def fixture(name, gpu=False):
    """The module-scoped `lib` fixture of a test file: library(name), behind the `cuda` fixture in a GPU file."""
    if gpu:
        @pytest.fixture(scope="module")
        def lib(cuda):
            return library(name)
    else:
        @pytest.fixture(scope="module")
        def lib():
            return library(name)
    return lib


def stream():
    """torch's current stream as the C-ABI takes it."""
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def build_app(name, tmp_path) -> str:
    """Compile the reference-style application of the library `name` with plain g++ against include/ and link it against the product
    libraries; -> the executable."""
    from feathercnn_amd import _lib
    source, extra = SIDE[name].app
    libdir = os.path.dirname(_lib.path(name))
    exe = str(tmp_path / os.path.splitext(source)[0])
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", *extra, "-D__HIP_PLATFORM_AMD__", "-I" + INCLUDE, "-I" + os.path.join(INCLUDE, "feather"),
                    "-I/opt/rocm/include", os.path.join(ROOT, "tests", "cpp", source), "-o", exe, "-L" + libdir, "-lfeather_hip",
                    "-lfeather_" + name, "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True,
                   capture_output=True, text=True)
    return exe
