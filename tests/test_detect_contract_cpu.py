"""The contract of tests/test_q8_contract_cpu.py restated for the second row of feathercnn_amd/_lib.MORE_LIBRARIES, libfeather_detect.so: built
by the second list of csrc/Makefile and loaded from the second table because the tables the contract tests hold over LIBRARIES are closed;
everything they ask of a row is asked here.  The library has a route code of its own, FHIP_DETECT_NET_ROUTE in its own header and
DETECT_ROUTE in net.py, outside the closed set of FHIP_NET_ROUTE_* / ROUTE_* constants."""
import glob
import os
import re
import subprocess
import threading

import detect_cases as DC
import kernel_instances as KI
import side_contract as SC
from feathercnn_amd import _lib

NAME = "detect"
ROW = _lib.MORE_LIBRARIES[NAME]
KERNEL_DECL = r"__global__\s+(?:__launch_bounds__\((?:[^()]|\([^()]*\))*\)\s+)?void\s+(\w+)"
WRAPPERS = ("permute", "permute_concat", "normalize", "priorbox", "axis_softmax", "detection_output", "detect_route")


def _header():
    return "".join(open(os.path.join(SC.INCLUDE, "feather_hip", h)).read() for h in ROW.headers)


def test_the_second_tables_name_the_same_libraries():
    mk = open(os.path.join(SC.ROOT, "feathercnn_amd", "csrc", "Makefile")).read()
    assert list(_lib.MORE_LIBRARIES) == re.search(r"^SIDE_MORE\s*:=(.*)$", mk, re.M).group(1).split() == ["q8", NAME]
    assert not set(_lib.MORE_LIBRARIES) & set(_lib.LIBRARIES)
    assert _lib.path(NAME) == os.path.join(SC.ROOT, "feathercnn_amd", f"libfeather_{NAME}.so") == DC.LIB
    assert _lib.detect_path() == _lib.path(NAME) and (_lib.load_detect_library.func, _lib.load_detect_library.args) == (_lib.load, (NAME,))
    assert ROW.last_error == f"fhip_{NAME}_last_error" and ROW.macro == "FHIP_DETECT_API" and ROW.headers == ("feather_detect.h",)


def test_exports():
    lib = SC.library(NAME)
    declared = sorted(set(re.findall(ROW.macro + r"\s+[\w\s\*]+?\b(fhip_\w+)\s*\(", _header())))
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.path(NAME)], capture_output=True, text=True, check=True).stdout
    exported = sorted(s for s in re.findall(r"\s[TDB]\s+(\w+)$", out, re.M) if s.startswith("fhip_"))
    assert declared and declared == exported == sorted(ROW.signatures)
    assert ROW.last_error in declared
    for symbol in declared:
        assert getattr(lib, symbol).argtypes is not None  # load() resolved and typed every one
    dynamic = subprocess.run(["readelf", "-d", _lib.path(NAME)], capture_output=True, text=True, check=True).stdout
    assert "libfeather_" not in dynamic  # it stands alone
    import feathercnn_amd
    assert all(callable(getattr(feathercnn_amd, f)) for f in WRAPPERS)
    assert not re.findall(r"typedef struct \w+\s*\{", _header()) and ROW.structs == ()  # no struct crosses this boundary


def test_disjointness():
    for name, other in {**_lib.LIBRARIES, **_lib.MORE_LIBRARIES}.items():
        if name != NAME:
            assert not set(ROW.signatures) & set(other.signatures), other.file


def test_instantiations():
    names = KI.instances(_lib.path(NAME))
    assert names and set(names) == DC.targets(), f"library {names} / sweep table {sorted(DC.targets())}"
    sources = os.path.join(SC.ROOT, "feathercnn_amd", "csrc_" + NAME)
    src = "".join(open(p).read() for p in sorted(glob.glob(os.path.join(sources, "*.hip")) + glob.glob(os.path.join(sources, "*.h"))))
    declared = set(re.findall(KERNEL_DECL, src))
    assert declared == {KI.base(n) for n in names} == DC.KERNELS  # its kernels are declared under csrc_detect/
    for word in ("hipMalloc", "hipMemcpy", "getenv", "Synchronize", "atomicCAS", "atomicExch"):  # a forward only launches; its atomics only count
        assert word not in src.split("#include", 1)[1], word
    assert "-ffp-contract" not in open(os.path.join(SC.ROOT, "feathercnn_amd", "csrc", "Makefile")).read() and "#pragma clang fp contract(off)" in src


def test_the_closed_libraries_are_what_they_were():
    """The new kernels went into the new library: the main library holds the count tests/side_contract.py pins, libfeather_q8.so what
    tests/q8_cases.py names, and net.hip declares no kernel."""
    import helpers
    import q8_cases
    SC.main_library_holds(KI.instances(_lib.path(_lib.MAIN)))
    assert set(KI.instances(_lib.path("q8"))) == q8_cases.targets()
    assert "__global__" not in helpers.net_runtime_source()


def test_route_code():
    from feathercnn_amd import detect, net
    code = int(re.search(r"#define\s+FHIP_DETECT_NET_ROUTE\s+(\d+)", _header()).group(1))
    assert code == net.DETECT_ROUTE == detect.NET_ROUTE == 109 and net.ROUTE_NAMES[code] == "DETECT"
    assert list(net.ROUTE_NAMES.values()).count("DETECT") == 1 and code not in (getattr(net, k) for k in vars(net) if re.fullmatch(r"ROUTE_[A-Z]+", k))
    text = open(os.path.join(SC.INCLUDE, "feather_hip", "feather_net.h")).read()
    cxx = open(os.path.join(SC.INCLUDE, "feather", "net.h")).read()
    assert "fhip_net_set_detection" in text and "fhip_net_set_detection" in _lib.SIGNATURES and "SetDetection" in cxx and "ExtractDetections" in cxx
    for macro, value in (("FHIP_DETECT_MAX_PRIORS", detect.MAX_PRIORS), ("FHIP_DETECT_MAX_CLASSES", detect.MAX_CLASSES), ("FHIP_DETECT_MAX_TOP_K", detect.MAX_TOP_K),
                         ("FHIP_DETECT_CHUNK", detect.CHUNK), ("FHIP_PERMUTE_CONCAT_MAX", detect.PERMUTE_CONCAT_MAX)):
        assert eval(re.search(r"#define\s+%s\s+(.+)" % macro, _header()).group(1)) == value, macro
    assert detect.CHUNK == DC.CHUNK and detect.MAX_PRIORS >= 24564  # SSD512


def test_last_error():
    """A refusal returns FHIP_E_BADARG and leaves its text in fhip_detect_last_error of the calling thread, and of that thread only."""
    lib = SC.library(NAME)
    last_error = getattr(lib, ROW.last_error)
    assert lib.fhip_permute_output_dim(9, 3, 1, 1, 1, None, None, None) == SC.BADARG
    assert last_error() != b""
    seen = []
    t = threading.Thread(target=lambda: seen.append(last_error()))
    t.start()
    t.join()
    assert seen == [b""]  # a thread that made no call has no error
    assert last_error() != b""


def test_host_checks_refuse_before_the_device():
    """Every device entry refuses bad arguments with FHIP_E_BADARG on the host: none of these calls needs (or reaches) a GPU."""
    lib = SC.library(NAME)
    bad = SC.BADARG
    assert lib.fhip_permute_forward(6, 3, 1, 1, 1, 1, None, None, None) == bad and lib.fhip_permute_forward(2, 2, 1, 1, 1, 1, None, None, None) == bad
    assert lib.fhip_permute_forward(3, 3, 1, 1, 1, 1, None, None, None) == bad  # NULL pointers
    assert lib.fhip_permute_forward(3, 3, 1, 1 << 16, 1 << 8, 1 << 8, 16, 32, None) == bad  # 2^32 elements
    assert lib.fhip_permute_forward(3, 3, 1, 2, 2, 2, 16, 18, None) == bad  # misaligned
    assert lib.fhip_permute_forward(3, 3, 1, 2, 2, 2, 16, 32, None) == bad  # overlapping
    assert lib.fhip_permute_concat_forward(9, None, None, 1, None, None, None) == bad and lib.fhip_permute_concat_forward(1, None, None, 1, None, None, None) == bad
    assert lib.fhip_normalize_forward(1, 1, 1, 1, 0, 0.0, 16, 64, 128, None) == bad  # eps 0
    assert lib.fhip_normalize_forward(1, 1, 1, 1, 0, float("nan"), 16, 64, 128, None) == bad
    assert lib.fhip_normalize_forward(1, 1, 1, 1, 0, 1e-10, 16, 64, None, None) == bad
    assert lib.fhip_axis_softmax_forward(0, 1, 1, 16, 64, None) == bad and lib.fhip_axis_softmax_forward(1, 1, 1, None, 64, None) == bad
    assert lib.fhip_detection_output_forward(1, 1, 2, float("inf"), 1, 1, 0.5, 1, 16, 64, 128, 256, 512, None) == bad
    assert lib.fhip_detection_output_forward(2, 1, 2, 0.45, 1, 1, 0.5, 3, 16, 64, 128, 256, 512, None) == bad  # priors for 3 images of 2
    assert lib.fhip_detection_output_forward(1, 1, 2, 0.45, 1, 1, 0.5, 1, 16, 64, 128, 256, 516, None) == bad  # scratch not 8-byte aligned
    assert lib.fhip_detection_output_forward(1, 1, 2, 0.45, 2000, 1, 0.5, 1, 16, 64, 128, 256, 512, None) == bad
    assert lib.fhip_detect_route(99, 0, 0, 1, 1, 1, None, None, None, 0) == bad
