"""The contract of tests/test_q8_contract_cpu.py restated for the one row of feathercnn_amd/_lib.THIRD_LIBRARIES, libfeather_colpass.so: built by
the third list of csrc/Makefile and loaded from the third table because the tables the contract tests hold over LIBRARIES and
MORE_LIBRARIES are closed; everything they ask of a row is asked here.  The library is no layer type: the Net runtime routes two layers
of a chained Winograd run to it (fhip_net_set_colpass)."""
import ctypes
import glob
import os
import re
import subprocess
import threading

import colpass_cases as CC
import kernel_instances as KI
import side_contract as SC
from feathercnn_amd import _lib

NAME = "colpass"
ROW = _lib.THIRD_LIBRARIES[NAME]
KERNEL_DECL = r"__global__\s+(?:__launch_bounds__\((?:[^()]|\([^()]*\))*\)\s+)?void\s+(\w+)"


def _header():
    return "".join(open(os.path.join(SC.INCLUDE, "feather_hip", h)).read() for h in ROW.headers)


def _lists():
    mk = open(os.path.join(SC.ROOT, "feathercnn_amd", "csrc", "Makefile")).read()
    return [re.search(r"^%s\s*:=(.*)$" % v, mk, re.M).group(1).split() for v in ("SIDE", "SIDE_MORE", "SIDE_THIRD")]


def test_the_third_tables_name_the_same_library():
    side, more, third = _lists()
    assert list(_lib.THIRD_LIBRARIES) == third == [NAME]  # built by the one mechanism
    assert list(_lib.MORE_LIBRARIES) == more and [n for n in _lib.LIBRARIES if n != _lib.MAIN] == side
    assert not set(third) & (set(side) | set(more)) and not set(_lib.THIRD_LIBRARIES) & (set(_lib.LIBRARIES) | set(_lib.MORE_LIBRARIES))
    assert _lib.path(NAME) == os.path.join(SC.ROOT, "feathercnn_amd", f"libfeather_{NAME}.so") == CC.LIB
    assert _lib.colpass_path() == _lib.path(NAME) and (_lib.load_colpass_library.func, _lib.load_colpass_library.args) == (_lib.load, (NAME,))
    assert ROW.last_error == f"fhip_{NAME}_last_error" and ROW.macro == "FHIP_COLPASS_API" and ROW.headers == ("feather_colpass.h",)
    assert ROW.route is None and ROW.structs == () and not re.findall(r"typedef struct \w+\s*\{", _header())  # no struct of its own
    entry = open(os.path.join(SC.ROOT, "__graft_entry__.py")).read()
    assert "_lib.THIRD_LIBRARIES" in entry  # build() loads it with the others


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


def test_disjointness():
    for name, other in {**_lib.LIBRARIES, **_lib.MORE_LIBRARIES}.items():
        assert not set(ROW.signatures) & set(other.signatures), other.file


def test_instantiations():
    names = KI.instances(_lib.path(NAME))
    assert names and set(names) == CC.targets(), f"library {names} / table {sorted(CC.targets())}"
    sources = os.path.join(SC.ROOT, "feathercnn_amd", "csrc_" + NAME)
    src = "".join(open(p).read() for p in sorted(glob.glob(os.path.join(sources, "*.hip")) + glob.glob(os.path.join(sources, "*.h"))))
    declared = set(re.findall(KERNEL_DECL, src))
    assert declared == {KI.base(n) for n in names} == CC.KERNELS  # its kernels are declared under csrc_colpass/
    for word in ("atomic", "hipMalloc", "hipMemcpy", "getenv", "Synchronize"):  # a forward only launches
        assert word not in src.split("#include", 1)[1], word
    for shared in ("wino_butterfly.h", "wino_layout.h", "side_error.h"):  # one text of the butterflies and of the layout
        assert f'#include "{shared}"' in src


def test_the_closed_libraries_are_what_they_were():
    """The new kernels went into the new library: the main library holds the count tests/side_contract.py pins, the canvas library its
    pinned set, and net.hip declares no kernel."""
    import helpers
    SC.main_library_holds(KI.instances(_lib.path(_lib.MAIN)))
    assert set(KI.instances(_lib.path("canvas"))) == SC.targets("canvas")
    assert "__global__" not in helpers.net_runtime_source()


def test_net_switch_is_declared_everywhere():
    text = open(os.path.join(SC.INCLUDE, "feather_hip", "feather_net.h")).read()
    cxx = open(os.path.join(SC.INCLUDE, "feather", "net.h")).read()
    from feathercnn_amd.net import Net
    for symbol in ("fhip_net_set_colpass", "fhip_net_layer_colpass"):
        assert symbol in text and symbol in _lib.SIGNATURES
    assert "SetColpass" in cxx and callable(Net.SetColpass) and callable(Net.colpasses)


def _param(c, k, stride=1, h=24):
    return _lib.fhip_conv_param(k, c, h, h, 3, 3, (h + 2 - 3) // stride + 1, (h + 2 - 3) // stride + 1, stride, stride, 1, 1, 1, 1, 1, 1, 1)


def test_refusals_leave_a_message():
    """Layers the library does not take are refused on the host, with FHIP_E_UNSUPPORTED and a message; NULL is FHIP_E_BADARG."""
    lib = SC.library(NAME)
    last_error = getattr(lib, ROW.last_error)
    for what, c, k, stride in CC.REFUSALS:
        p = _param(c, k, stride)
        assert lib.fhip_colpass_supported(ctypes.byref(p), 2) == -1, what
        assert last_error() != b"", what
    for k in (64, 128, 192):
        ok = _param(64, k)
        assert lib.fhip_colpass_supported(ctypes.byref(ok), 2) == 0, k
    small = _param(64, 64, h=8)  # an 8-pixel plane runs on F(4x4,3x3)
    assert lib.fhip_colpass_supported(ctypes.byref(small), 2) == -1 and b"F(4x4,3x3)" in last_error()
    assert lib.fhip_colpass_supported(None, 2) == SC.BADARG and lib.fhip_colpass_supported(ctypes.byref(ok), 0) == SC.BADARG
    assert lib.fhip_colpass_tile_gemm(ctypes.byref(ok), 2, None, None, None, None, None) == SC.BADARG
    assert lib.fhip_colpass_output_to_next_input(ctypes.byref(ok), None, 2, None, None, None, None, None, 0, None) == SC.BADARG
    # a plan of another batch is refused before anything reaches the device
    pl = _lib.fhip_winograd_plan()
    assert _lib.load_library().fhip_winograd_f63_plan(ctypes.byref(ok), 3, ctypes.byref(pl)) == 0
    assert lib.fhip_colpass_tile_gemm(ctypes.byref(ok), 2, ctypes.byref(pl), 16, 32, 48, None) == SC.BADARG and b"plan" in last_error()


def test_last_error_is_per_thread():
    lib = SC.library(NAME)
    last_error = getattr(lib, ROW.last_error)
    assert lib.fhip_colpass_supported(None, 1) == SC.BADARG and last_error() != b""
    seen = []
    t = threading.Thread(target=lambda: seen.append(last_error()))
    t.start()
    t.join()
    assert seen == [b""]  # a thread that made no call has no error
    assert last_error() != b""
