"""The contract every run-time library shares, held over EVERY row of feathercnn_amd/_lib.LATER_LIBRARIES, built by LATER of csrc/Makefile:
the libraries added after libfeather_frame.so, whose own list tests/test_frame_contract_cpu.py pins to its one row.  A row's sweep table
comes from the naming rule tests/<name>_cases.py (targets(), KERNELS, LIB).  Nothing here asserts how many rows the list has or what they
are called: the next library adds a row, a name to LATER and a cases file, and this file holds it to the contract as it stands."""
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

NAMES = list(_lib.LATER_LIBRARIES)
KERNEL_DECL = r"__global__\s+(?:__launch_bounds__\((?:[^()]|\([^()]*\))*\)\s+)?void\s+(\w+)"
FORBIDDEN = ("hipMalloc", "hipMemcpy", "getenv", "Synchronize", "atomicCAS", "atomicExch", "atomicAdd")  # a forward only launches


def _cases(name):
    return importlib.import_module(name + "_cases")


def _header(name):
    return "".join(open(os.path.join(SC.INCLUDE, "feather_hip", h)).read() for h in _lib.LATER_LIBRARIES[name].headers)


def _outside():
    return [t for t in (_lib.STANDALONE_LIBRARIES, _lib.LATER_LIBRARIES)]


def test_the_list_is_the_makefiles_and_is_built_and_loaded_with_the_others():
    mk = open(os.path.join(SC.ROOT, "feathercnn_amd", "csrc", "Makefile")).read()
    assert NAMES == re.search(r"^LATER\s*:=(.*)$", mk, re.M).group(1).split()
    listed = [n for v in ("SIDE", "SIDE_MORE", "SIDE_THIRD", "SIDE_OPEN", "STANDALONE") for n in re.search(r"^%s\s*:=(.*)$" % v, mk, re.M).group(1).split()]
    assert not set(NAMES) & set(listed) and len(set(NAMES)) == len(NAMES)
    assert not any(set(NAMES) & set(t) for t in _lib.TABLES + (_lib.STANDALONE_LIBRARIES,))
    assert "$(LATER:%=$(ROOT)/feathercnn_amd/libfeather_%.so)" in mk and "$(LATER:%=$(OBJDIR)/%.o)" in mk  # the same two rules
    entry = open(os.path.join(SC.ROOT, "__graft_entry__.py")).read()
    assert "_lib.LATER_LIBRARIES" in entry  # build() loads them with the others


@pytest.mark.parametrize("name", NAMES)
def test_the_row(name):
    row = _lib.LATER_LIBRARIES[name]
    assert _lib.row(name) is row
    assert _lib.path(name) == os.path.join(SC.ROOT, "feathercnn_amd", f"libfeather_{name}.so") == _cases(name).LIB and row.file == f"libfeather_{name}.so"
    assert getattr(_lib, f"{name}_path")() == _lib.path(name)
    loader = getattr(_lib, f"load_{name}_library")
    assert (loader.func, loader.args) == (_lib.load, (name,))
    assert row.last_error == f"fhip_{name}_last_error" and row.macro == f"FHIP_{name.upper()}_API" and row.headers == (f"feather_{name}.h",)
    assert not re.findall(r"typedef struct \w+\s*\{", _header(name)) and not re.findall(r"^\s*struct \w+\s*\{", _header(name), re.M) and row.structs == ()
    assert os.path.exists(os.path.join(SC.ROOT, "feathercnn_amd", f"csrc_{name}", f"{name}.hip"))


@pytest.mark.parametrize("name", NAMES)
def test_exports(name):
    row = _lib.LATER_LIBRARIES[name]
    lib = SC.library(name)
    declared = sorted(set(re.findall(row.macro + r"\s+[\w\s\*]+?\b(fhip_\w+)\s*\(", _header(name))))
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.path(name)], capture_output=True, text=True, check=True).stdout
    exported = sorted(s for s in re.findall(r"\s[TDB]\s+(\w+)$", out, re.M) if s.startswith("fhip_"))
    assert declared and declared == exported == sorted(row.signatures)
    assert row.last_error in declared and f"fhip_{name}_route" in declared
    for symbol in declared:
        assert getattr(lib, symbol).argtypes is not None  # load() resolved and typed every one
    dynamic = subprocess.run(["readelf", "-d", _lib.path(name)], capture_output=True, text=True, check=True).stdout
    assert "libfeather_" not in dynamic  # it stands alone


@pytest.mark.parametrize("name", NAMES)
def test_disjointness(name):
    row = _lib.LATER_LIBRARIES[name]
    for table in _lib.TABLES + tuple(_outside()):
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
    last_error = getattr(lib, _lib.LATER_LIBRARIES[name].last_error)
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
    """New kernels go into new libraries: the main library holds the count tests/side_contract.py pins, and the Net runtime declares no
    kernel."""
    import helpers
    SC.main_library_holds(KI.instances(_lib.path(_lib.MAIN)))
    assert "__global__" not in helpers.net_runtime_source()
