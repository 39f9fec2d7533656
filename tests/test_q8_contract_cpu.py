"""The contract of tests/test_side_contract_cpu.py restated for the one row of feathercnn_amd/_lib.MORE_LIBRARIES (libfeather_q8.so), with the
helpers of tests/side_contract.py and tests/kernel_instances.py: the library is built by the second list of csrc/Makefile and loaded from the
second table only because the tables those tests hold (SIDE, LIBRARIES, side_contract.SIDE) are closed; everything they ask of a row is
asked here."""
import glob
import os
import re
import subprocess
import threading

import kernel_instances as KI
import q8_cases as QC
import side_contract as SC
from feathercnn_amd import _lib

NAME = "q8"
ROW = _lib.MORE_LIBRARIES[NAME]
KERNEL_DECL = r"__global__\s+(?:__launch_bounds__\((?:[^()]|\([^()]*\))*\)\s+)?void\s+(\w+)"
WRAPPERS = ("Q8Conv", "Q8Param", "q8_pack", "q8_unpack", "q8_relu", "q8_max_pool", "q8_route")


def _header():
    return "".join(open(os.path.join(SC.INCLUDE, "feather_hip", h)).read() for h in ROW.headers)


def _fields(header_text, struct):
    """The field names of `typedef struct <struct> { ... }` in declaration order."""
    body = re.search(r"typedef struct %s\s*\{(.*?)\}" % struct, header_text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [re.search(r"(\w+)\s*$", part).group(1) for decl in body.split(";") if decl.strip() for part in decl.split(",")]


def test_the_second_tables_name_the_same_library():
    mk = open(os.path.join(SC.ROOT, "feathercnn_amd", "csrc", "Makefile")).read()
    assert list(_lib.MORE_LIBRARIES) == re.search(r"^SIDE_MORE\s*:=(.*)$", mk, re.M).group(1).split()  # built by the one mechanism
    assert not set(_lib.MORE_LIBRARIES) & set(_lib.LIBRARIES)
    assert _lib.path(NAME) == os.path.join(SC.ROOT, "feathercnn_amd", f"libfeather_{NAME}.so") == QC.LIB
    assert _lib.q8_path() == _lib.path(NAME) and (_lib.load_q8_library.func, _lib.load_q8_library.args) == (_lib.load, (NAME,))
    assert ROW.last_error == f"fhip_{NAME}_last_error" and ROW.macro == "FHIP_Q8_API" and ROW.headers == ("feather_q8.h",)
    assert ROW.route is None  # no route code of its own: its layers report QCONV


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
    assert "libfeather_" not in dynamic  # it stands alone: neither libfeather_hip nor libfeather_qconv
    import feathercnn_amd
    assert all(callable(getattr(feathercnn_amd, f)) for f in WRAPPERS)


def test_disjointness():
    for other in _lib.LIBRARIES.values():
        assert not set(ROW.signatures) & set(other.signatures), other.file


def test_struct_mirrors():
    text = _header()
    assert len(ROW.structs) == len(re.findall(r"typedef struct \w+\s*\{", text)) == 1  # every struct the header defines has a mirror
    fields = _fields(text, "fhip_q8_param")
    assert fields == [f[0] for f in _lib.fhip_q8_param._fields_]
    assert fields == [f[0] for f in _lib.fhip_qconv_param._fields_] + ["input_int8", "output_int8"]


def test_instantiations():
    names = KI.instances(_lib.path(NAME))
    assert names and set(names) == QC.targets() == QC.all_routes() | QC.HELPERS, f"library {names} / sweep table {sorted(QC.targets())}"
    sources = os.path.join(SC.ROOT, "feathercnn_amd", "csrc_" + NAME)
    src = "".join(open(p).read() for p in sorted(glob.glob(os.path.join(sources, "*.hip")) + glob.glob(os.path.join(sources, "*.h"))))
    declared = set(re.findall(KERNEL_DECL, src))
    assert declared and declared == {KI.base(n) for n in names}  # its kernels are declared under csrc_q8/
    for word in ("atomic", "hipMalloc", "hipMemcpy", "getenv", "Synchronize"):  # a forward only launches
        assert word not in src.split("#include", 1)[1], word


def test_the_closed_libraries_are_what_they_were():
    """The new kernels went into the new library: libfeather_qconv.so holds what tests/qconv_cases.py names, by the same names."""
    import qconv_cases
    assert set(KI.instances(_lib.path("qconv"))) == qconv_cases.targets()


def test_last_error():
    """A refusal returns FHIP_E_BADARG and leaves its text in fhip_q8_last_error of the calling thread, and of that thread only."""
    lib = SC.library(NAME)
    last_error = getattr(lib, ROW.last_error)
    assert lib.fhip_q8_assign_output_dim(None) == SC.BADARG
    assert last_error() != b""
    seen = []
    t = threading.Thread(target=lambda: seen.append(last_error()))
    t.start()
    t.join()
    assert seen == [b""]  # a thread that made no call has no error
    assert last_error() != b""


def test_application(tmp_path):
    """tests/cpp/q8_app_main.cpp (booster::Q8Conv of include/booster/q8.h) compiles with plain g++ -std=c++11 -Wall against include/, links
    against the product libraries and its host-side checks hold."""
    SC.library(NAME)
    libdir = os.path.dirname(_lib.path(NAME))
    exe = str(tmp_path / "q8_app_main")
    r = subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I" + SC.INCLUDE, "-I" + os.path.join(SC.INCLUDE, "feather"),
                        "-I/opt/rocm/include", os.path.join(SC.ROOT, "tests", "cpp", "q8_app_main.cpp"), "-o", exe, "-L" + libdir, "-lfeather_hip",
                        "-lfeather_" + NAME, "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "q8 app ok" in r.stdout, (r.returncode, r.stdout, r.stderr)
