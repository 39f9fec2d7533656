"""The contract every run-time library shares, held over EVERY row of feathercnn_amd/_lib.OPEN_LIBRARIES -- the last table, built by the last
list of csrc/Makefile (SIDE_OPEN).  The tables before it are closed by the tests that restate this contract for them; this one is open: a row's
sweep table comes from a naming rule -- tests/<name>_cases.py with targets(), KERNELS and LIB -- so the next library adds a row, a name in
SIDE_OPEN and a cases file, and this file tests it as it stands.  What only libfeather_yolo.so has (its route code) is asked at the end."""
import glob
import importlib
import os
import re
import subprocess
import threading

import pytest

import kernel_instances as KI
import side_contract as SC
from feathercnn_amd import _lib

NAMES = list(_lib.OPEN_LIBRARIES)
KERNEL_DECL = r"__global__\s+(?:__launch_bounds__\((?:[^()]|\([^()]*\))*\)\s+)?void\s+(\w+)"
FORBIDDEN = ("hipMalloc", "hipMemcpy", "getenv", "Synchronize", "atomicCAS", "atomicExch")  # a forward only launches; its atomics only count


def _cases(name):
    return importlib.import_module(name + "_cases")


def _header(name):
    return "".join(open(os.path.join(SC.INCLUDE, "feather_hip", h)).read() for h in _lib.OPEN_LIBRARIES[name].headers)


def _lists():
    mk = open(os.path.join(SC.ROOT, "feathercnn_amd", "csrc", "Makefile")).read()
    return mk, [re.search(r"^%s\s*:=(.*)$" % v, mk, re.M).group(1).split() for v in ("SIDE", "SIDE_MORE", "SIDE_THIRD", "SIDE_OPEN")]


def test_the_open_tables_name_the_same_libraries_and_come_last():
    mk, (side, more, third, open_) = _lists()
    assert NAMES == open_ and NAMES  # built by the one mechanism
    assert list(_lib.THIRD_LIBRARIES) == third and list(_lib.MORE_LIBRARIES) == more and [n for n in _lib.LIBRARIES if n != _lib.MAIN] == side
    assert not set(open_) & (set(side) | set(more) | set(third))
    assert not set(_lib.OPEN_LIBRARIES) & (set(_lib.LIBRARIES) | set(_lib.MORE_LIBRARIES) | set(_lib.THIRD_LIBRARIES))
    assert _lib.TABLES[-1] is _lib.OPEN_LIBRARIES and len(_lib.TABLES) == 4
    assert re.findall(r"^(SIDE(?:_\w+)?)\s*:=", mk, re.M) == ["SIDE", "SIDE_MORE", "SIDE_THIRD", "SIDE_OPEN"]  # the last list: no fifth behind it
    entry = open(os.path.join(SC.ROOT, "__graft_entry__.py")).read()
    assert "_lib.OPEN_LIBRARIES" in entry and "_lib.THIRD_LIBRARIES" in entry  # build() loads them with the others


@pytest.mark.parametrize("name", NAMES)
def test_the_row(name):
    row = _lib.OPEN_LIBRARIES[name]
    assert _lib.row(name) is row
    assert _lib.path(name) == os.path.join(SC.ROOT, "feathercnn_amd", f"libfeather_{name}.so") == _cases(name).LIB and row.file == f"libfeather_{name}.so"
    assert getattr(_lib, f"{name}_path")() == _lib.path(name)
    loader = getattr(_lib, f"load_{name}_library")
    assert (loader.func, loader.args) == (_lib.load, (name,))
    assert row.last_error == f"fhip_{name}_last_error" and row.macro == f"FHIP_{name.upper()}_API" and row.headers == (f"feather_{name}.h",)
    assert not re.findall(r"typedef struct \w+\s*\{", _header(name)) and row.structs == ()  # no struct crosses this boundary
    assert os.path.exists(os.path.join(SC.ROOT, "feathercnn_amd", f"csrc_{name}", f"{name}.hip"))


@pytest.mark.parametrize("name", NAMES)
def test_exports(name):
    row = _lib.OPEN_LIBRARIES[name]
    lib = SC.library(name)
    declared = sorted(set(re.findall(row.macro + r"\s+[\w\s\*]+?\b(fhip_\w+)\s*\(", _header(name))))
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.path(name)], capture_output=True, text=True, check=True).stdout
    exported = sorted(s for s in re.findall(r"\s[TDB]\s+(\w+)$", out, re.M) if s.startswith("fhip_"))
    assert declared and declared == exported == sorted(row.signatures)
    assert row.last_error in declared
    for symbol in declared:
        assert getattr(lib, symbol).argtypes is not None  # load() resolved and typed every one
    dynamic = subprocess.run(["readelf", "-d", _lib.path(name)], capture_output=True, text=True, check=True).stdout
    assert "libfeather_" not in dynamic  # it stands alone


@pytest.mark.parametrize("name", NAMES)
def test_disjointness(name):
    row = _lib.OPEN_LIBRARIES[name]
    for table in _lib.TABLES:
        for other_name, other in table.items():
            if other_name != name:
                assert not set(row.signatures) & set(other.signatures), other.file


@pytest.mark.parametrize("name", NAMES)
def test_instantiations(name):
    cases = _cases(name)
    names = KI.instances(_lib.path(name))
    assert names and set(names) == cases.targets(), f"library {names} / sweep table {sorted(cases.targets())}"
    sources = os.path.join(SC.ROOT, "feathercnn_amd", "csrc_" + name)
    src = "".join(open(p).read() for p in sorted(glob.glob(os.path.join(sources, "*.hip")) + glob.glob(os.path.join(sources, "*.h"))))
    declared = set(re.findall(KERNEL_DECL, src))
    assert declared == {KI.base(n) for n in names} == cases.KERNELS  # its kernels are declared under csrc_<name>/
    for word in FORBIDDEN:
        assert word not in src.split("#include", 1)[1], word
    assert '#include "side_error.h"' in src
    assert "-ffp-contract" not in open(os.path.join(SC.ROOT, "feathercnn_amd", "csrc", "Makefile")).read() and "#pragma clang fp contract(off)" in src


@pytest.mark.parametrize("name", NAMES)
def test_last_error_is_per_thread(name):
    """A refusal returns FHIP_E_BADARG and leaves its text in the last-error slot of the calling thread, and of that thread only: the route entry
    of every open library refuses a NULL name."""
    lib = SC.library(name)
    last_error = getattr(lib, _lib.OPEN_LIBRARIES[name].last_error)
    route = getattr(lib, f"fhip_{name}_route")
    assert route(*[None if a is not _lib._I else 0 for a in route.argtypes]) == SC.BADARG
    assert last_error() != b""
    seen = []
    t = threading.Thread(target=lambda: seen.append(last_error()))
    t.start()
    t.join()
    assert seen == [b""]  # a thread that made no call has no error
    assert last_error() != b""


def test_the_closed_libraries_are_what_they_were():
    """The new kernels went into the new library: the main library holds the count tests/side_contract.py pins, libfeather_detect.so and
    libfeather_q8.so what their cases files name, and the Net runtime declares no kernel."""
    import detect_cases
    import helpers
    import q8_cases
    SC.main_library_holds(KI.instances(_lib.path(_lib.MAIN)))
    assert set(KI.instances(_lib.path("detect"))) == detect_cases.targets()
    assert set(KI.instances(_lib.path("q8"))) == q8_cases.targets()
    source = helpers.net_runtime_source()
    assert "__global__" not in source and "create_yolo_layer" in source  # net_yolo.h is part of the runtime, and holds no kernel


def test_the_yolo_route_code_and_switch():
    from feathercnn_amd import net, yolo
    import feathercnn_amd
    code = int(re.search(r"#define\s+FHIP_YOLO_NET_ROUTE\s+(\d+)", _header("yolo")).group(1))
    assert code == net.YOLO_ROUTE == yolo.NET_ROUTE == feathercnn_amd.YOLO_NET_ROUTE == 110 and net.ROUTE_NAMES[code] == "YOLO"
    assert list(net.ROUTE_NAMES.values()).count("YOLO") == 1 and code not in (getattr(net, k) for k in vars(net) if re.fullmatch(r"ROUTE_[A-Z]+", k))
    text = open(os.path.join(SC.INCLUDE, "feather_hip", "feather_net.h")).read()
    cxx = open(os.path.join(SC.INCLUDE, "feather", "net.h")).read()
    assert "fhip_net_set_yolo" in text and "fhip_net_set_yolo" in _lib.SIGNATURES and "SetYolo(int rows = 256)" in cxx and callable(net.Net.SetYolo)
    assert all(callable(getattr(feathercnn_amd, f)) for f in ("reorg", "reorg_output_dim", "yolo_detection", "yolo_route"))
    for required in ("fhip_reorg_output_dim", "fhip_reorg_forward", "fhip_yolo_get_buffer_size", "fhip_yolo_detection_forward", "fhip_yolo_route",
                     "fhip_yolo_last_error"):
        assert required in _lib.OPEN_LIBRARIES["yolo"].signatures
