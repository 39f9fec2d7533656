"""The contract every run-time library shares, restated for the rows of feathercnn_amd/_lib.STANDALONE_LIBRARIES (libfeather_frame.so), built
by STANDALONE of csrc/Makefile.  The open table (tests/test_open_contract_cpu.py) was meant to take the next library, but
tests/test_roi_cpu.py holds _lib.OPEN_LIBRARIES to its two rows, so the library stands outside the tables and this file asks of it what that
one asks of an open row, by the same naming rule: tests/<name>_cases.py with targets(), KERNELS and LIB."""
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

NAMES = list(_lib.STANDALONE_LIBRARIES)
KERNEL_DECL = r"__global__\s+(?:__launch_bounds__\((?:[^()]|\([^()]*\))*\)\s+)?void\s+(\w+)"
FORBIDDEN = ("hipMalloc", "hipMemcpy", "getenv", "Synchronize", "atomicCAS", "atomicExch")  # a forward only launches


def _cases(name):
    return importlib.import_module(name + "_cases")


def _header(name):
    return "".join(open(os.path.join(SC.INCLUDE, "feather_hip", h)).read() for h in _lib.STANDALONE_LIBRARIES[name].headers)


def test_the_rows_stand_outside_the_tables_and_are_built_and_loaded_with_them():
    mk = open(os.path.join(SC.ROOT, "feathercnn_amd", "csrc", "Makefile")).read()
    assert NAMES == re.search(r"^STANDALONE\s*:=(.*)$", mk, re.M).group(1).split() == ["frame"]
    listed = {n for v in ("SIDE", "SIDE_MORE", "SIDE_THIRD", "SIDE_OPEN") for n in re.search(r"^%s\s*:=(.*)$" % v, mk, re.M).group(1).split()}
    assert not set(NAMES) & listed and not any(set(NAMES) & set(t) for t in _lib.TABLES)
    assert "$(STANDALONE:%=$(ROOT)/feathercnn_amd/libfeather_%.so)" in mk and "$(STANDALONE:%=$(OBJDIR)/%.o)" in mk  # the same two rules
    entry = open(os.path.join(SC.ROOT, "__graft_entry__.py")).read()
    assert "_lib.STANDALONE_LIBRARIES" in entry  # build() loads them with the others


@pytest.mark.parametrize("name", NAMES)
def test_the_row(name):
    row = _lib.STANDALONE_LIBRARIES[name]
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
    row = _lib.STANDALONE_LIBRARIES[name]
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
    row = _lib.STANDALONE_LIBRARIES[name]
    for table in _lib.TABLES + (_lib.STANDALONE_LIBRARIES,):
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
    """A refusal returns FHIP_E_BADARG and leaves its text in the last-error slot of the calling thread, and of that thread only: the route
    entry refuses a call whose pointers are NULL and whose ints are 0."""
    lib = SC.library(name)
    last_error = getattr(lib, _lib.STANDALONE_LIBRARIES[name].last_error)
    route = getattr(lib, f"fhip_{name}_route")
    assert route(*[None if a is not _lib._I else 0 for a in route.argtypes]) == SC.BADARG
    assert last_error() != b""
    seen = []
    t = threading.Thread(target=lambda: seen.append(last_error()))
    t.start()
    t.join()
    assert seen == [b""]  # a thread that made no call has no error
    assert last_error() != b""


def test_the_other_libraries_are_what_they_were():
    """The new kernels went into the new library: the main library holds the count tests/side_contract.py pins, and the Net runtime declares no
    kernel -- net_frame.h is part of it."""
    import helpers
    SC.main_library_holds(KI.instances(_lib.path(_lib.MAIN)))
    source = helpers.net_runtime_source()
    assert "__global__" not in source and "create_frame_layer" in source
