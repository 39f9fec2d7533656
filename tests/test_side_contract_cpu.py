"""The contract every run-time library shares, stated once over feathercnn_amd/_lib.LIBRARIES and tests/side_contract.py, without a GPU:
each library exports what its header and the Python binding declare; no two libraries share a symbol; the ctypes struct mirrors have the
headers' fields; each code object holds the instantiations its sweep table names and the kernels its sources declare; the route codes of
feather_net.h are those of feathercnn_amd/net.py and differ; the reference-style applications compile and link; and a refused call
leaves its text in the last-error state of the calling thread only (feathercnn_amd/csrc_side/side_error.h)."""
import glob
import itertools
import os
import re
import subprocess
import threading

import pytest

import helpers
import kernel_instances as KI
import side_contract as SC
from feathercnn_amd import _lib

ROOT = SC.ROOT
NAMES = list(_lib.LIBRARIES)
SIDES = [n for n in NAMES if n != _lib.MAIN]
KERNEL_DECL = r"__global__\s+(?:__launch_bounds__\((?:[^()]|\([^()]*\))*\)\s+)?void\s+(\w+)"


def _headers(name):
    return "".join(open(os.path.join(SC.INCLUDE, "feather_hip", h)).read() for h in _lib.LIBRARIES[name].headers)


def _dynamic(name):
    return subprocess.run(["readelf", "-d", _lib.path(name)], capture_output=True, text=True, check=True).stdout


def test_the_tables_name_the_same_libraries():
    """LIBRARIES is the main library and then SIDE of csrc/Makefile in its order; side_contract has a row and a refused call for each."""
    mk = open(os.path.join(ROOT, "feathercnn_amd", "csrc", "Makefile")).read()
    assert NAMES[0] == _lib.MAIN and SIDES == re.search(r"^SIDE\s*:=(.*)$", mk, re.M).group(1).split()  # built by the one mechanism
    assert list(SC.SIDE) == SIDES
    assert sorted(SC.REFUSED) == sorted(SIDES)
    for name in SIDES:
        assert _lib.path(name) == os.path.join(ROOT, "feathercnn_amd", f"libfeather_{name}.so")
        loader = getattr(_lib, f"load_{name}_library")  # the names the wrappers and tools/ call, defined from the table
        assert getattr(_lib, f"{name}_path")() == _lib.path(name) and (loader.func, loader.args) == (_lib.load, (name,))
        assert _lib.LIBRARIES[name].last_error == f"fhip_{name}_last_error"
    assert _lib.lib_path() == _lib.path(_lib.MAIN)


@pytest.mark.parametrize("name", NAMES)
def test_exports(name):
    row = _lib.LIBRARIES[name]
    lib = SC.library(name)
    declared = sorted(set(re.findall(row.macro + r"\s+[\w\s\*]+?\b(fhip_\w+)\s*\(", _headers(name))))
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.path(name)], capture_output=True, text=True, check=True).stdout
    exported = sorted(s for s in re.findall(r"\s[TDB]\s+(\w+)$", out, re.M) if s.startswith("fhip_"))
    assert declared and declared == exported == sorted(row.signatures)
    assert row.last_error in declared
    for symbol in declared:
        assert getattr(lib, symbol).argtypes is not None  # load() resolved and typed every one
    if name == _lib.MAIN:
        assert "libfeather_" not in _dynamic(name)  # the main library reaches the side libraries at run time only
    else:
        assert "libfeather_hip" not in _dynamic(name)  # and each of them stands alone
        import feathercnn_amd
        assert all(callable(getattr(feathercnn_amd, f)) for f in SC.SIDE[name].wrappers)


def test_disjointness():
    """No two of the twelve libraries export the same name: an application may load them all."""
    for a, b in itertools.combinations(NAMES, 2):
        assert not set(_lib.LIBRARIES[a].signatures) & set(_lib.LIBRARIES[b].signatures), (a, b)


def _fields(header_text, struct):
    """The field names of `typedef struct <struct> { ... }` in declaration order."""
    body = re.search(r"typedef struct %s\s*\{(.*?)\}" % struct, header_text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [re.search(r"(\w+)\s*$", part).group(1) for decl in body.split(";") if decl.strip() for part in decl.split(",")]


@pytest.mark.parametrize("name", [n for n in NAMES if _lib.LIBRARIES[n].structs])
def test_struct_mirrors(name):
    text = _headers(name)
    assert len(_lib.LIBRARIES[name].structs) == len(re.findall(r"typedef struct \w+\s*\{", text))  # every struct the headers define has a mirror
    for mirror in _lib.LIBRARIES[name].structs:
        fields = _fields(text, mirror.__name__)
        assert fields == [f[0] for f in mirror._fields_], mirror.__name__
        if mirror.__name__ in SC.STRUCT_TAILS:
            head, tail = SC.STRUCT_TAILS[mirror.__name__]
            assert fields == [f[0] for f in getattr(_lib, head)._fields_] + tail, mirror.__name__


@pytest.mark.parametrize("name", NAMES)
def test_instantiations(name):
    names = KI.instances(_lib.path(name))
    if name == _lib.MAIN:  # tests/test_kernel_instances_cpu.py holds the main library's list against its sweep table and its sources
        SC.main_library_holds(names)
        assert "__global__" not in helpers.net_runtime_source()  # net.hip only routes
        return
    assert names and set(names) == SC.targets(name), f"library {names} / sweep table {sorted(SC.targets(name))}"
    sources = os.path.join(ROOT, "feathercnn_amd", "csrc_" + name)
    src = "".join(open(p).read() for p in sorted(glob.glob(os.path.join(sources, "*.hip")) + glob.glob(os.path.join(sources, "*.h"))))
    declared = set(re.findall(KERNEL_DECL, src))
    assert declared and declared | SC.SIDE[name].shared == {KI.base(n) for n in names} and not declared & SC.SIDE[name].shared
    if SC.kernels(name) is not None:
        assert declared == SC.kernels(name)
    for word in SC.SIDE[name].forbidden:
        assert word not in (src.split("#include", 1)[1] if word == "atomic" else src), word


def test_routes():
    """Every FHIP_NET_ROUTE_* of feather_net.h is the ROUTE_* of net.py that one row of LIBRARIES names, no two are equal and none is one of
    the reference's ConvAlgo values; the switch a library's layers need is declared in both Net headers."""
    from feathercnn_amd import net
    text = open(os.path.join(SC.INCLUDE, "feather_hip", "feather_net.h")).read()
    header = {k: int(v) for k, v in re.findall(r"#define\s+FHIP_NET_(ROUTE_\w+)\s+(\d+)", text)}
    routed = {_lib.LIBRARIES[n].route: n for n in SIDES if _lib.LIBRARIES[n].route}
    assert header == {k: getattr(net, k) for k in routed} and len(routed) == 9
    assert {k for k in vars(net) if re.fullmatch(r"ROUTE_[A-Z]+", k) and k != "ROUTE_NAMES"} == set(routed)
    assert len(set(header.values())) == len(header) and not set(header.values()) & set(range(7))
    for constant, name in routed.items():
        assert constant == "ROUTE_" + name.upper() and net.ROUTE_NAMES[header[constant]] == name.upper()
        assert list(net.ROUTE_NAMES.values()).count(name.upper()) == 1
    cxx = open(os.path.join(SC.INCLUDE, "feather", "net.h")).read()
    for name in SIDES:
        if SC.SIDE[name].switch:
            assert SC.SIDE[name].switch[0] in text and SC.SIDE[name].switch[0] in _lib.SIGNATURES and SC.SIDE[name].switch[1] in cxx, name


@pytest.mark.parametrize("name", [n for n in SIDES if SC.SIDE[n].app])
def test_application(name, tmp_path):
    """The reference-style application (tests/cpp/<x>_app_main.cpp: the library's booster class or C-ABI next to feather::Net) compiles with
    plain g++ -std=c++11 -Wall against include/ and links against the product libraries; the library's GPU tests run it."""
    SC.library(name)
    assert os.path.exists(SC.build_app(name, tmp_path))


@pytest.mark.parametrize("name", sorted(SC.REFUSED))
def test_last_error(name):
    """A refusal returns FHIP_E_BADARG and leaves its text in fhip_<x>_last_error of the calling thread, and of that thread only."""
    lib = SC.library(name)
    last_error = getattr(lib, _lib.LIBRARIES[name].last_error)
    symbol, args, word = SC.REFUSED[name]
    assert getattr(lib, symbol)(*args) == SC.BADARG
    assert last_error() != b"" and (word or "").encode() in last_error()
    seen = []
    t = threading.Thread(target=lambda: seen.append(last_error()))
    t.start()
    t.join()
    assert seen == [b""]  # a thread that made no call has no error
    assert last_error() != b""
