"""The model readers (LoadParam / LoadWeights of every layer type: feathercnn_amd/csrc/net_model.h, net_layers.h and the loaders of net.hip) on hostile files: the table of
tests/loader_cases.py through the stand-alone driver tests/cpp/net_loader_hostile_main.cpp, once against the built library and once
with the library's host side compiled under AddressSanitizer and UndefinedBehaviorSanitizer into the same executable.  Host side only:
no feed, forward or extract call, no GPU, nothing loaded into python.

What the table found when it was first run, the case that showed it, and the refusal the readers give now:

* abort (std::length_error out of ModelBin::load, a negative count cast to size_t) -- Convolution/conv1/6=-2147483648, the same on the
  depthwise and the grouped route, BatchNorm/conv2_bn/0=-1, InnerProduct/fc1/0=-1 and 2=-1 (and their INT_MIN forms): now -100 at the
  param ("weight_data_size does not fit ...", "negative channel count", "num_output must be positive").  A positive count no file of that
  length can hold (6=2147483647, InstanceNorm / PReLU / BatchNorm / Scale 0=2147483647) zero-filled gigabytes before it failed: ModelBin
  now refuses it before it allocates (-1 from LoadWeights, "file too short for N weights").
* UndefinedBehaviorSanitizer report -- Deconvolution/d1/1=2147483647 (output_channels * kernel_h * kernel_w past long long) and
  array*_len_int_max (len + 1 in int): the products are taken in steps, the length is compared as size_t.
* accepted -- a last layer with bottom_count_0 / bottom_count_-1 / top_count_0 / *_count_text (Softmax/prob, TanH/out; the layer faults at its
  first Reshape): now -300.  Convolution weight_data_size_plus_1 / _minus_1 and 6=-1 (truncated to whole channels, the stream out of
  step): -100.  Deconvolution 2=0 / 12=-1 / dilation_0: -100.  Slice/u2_slice/size_infinite (inf cast to int): -100.  Eltwise/sum/one_bottom:
  -300 at the param, where Reshape gave it.  Concat axis_1 / axis_-1: -100 at the param, where Reshape gave it.
* another code than the reference's -- empty_value and array*_len_larger / _len_huge_no_values gave -2; paramdict.cpp returns -1: now -1.

test_every_layer_type_has_cases and test_param_id_table_matches_the_readers were tried on a copy of the tree with
`type == "Softmax" || type == "Dummy"` in create_layer: the first failed with "no base model holds ['Dummy']", the second on the id table.

Decided only at the shape stage, EITHER here and not run: PReLU slopes_not_channels, Slice sizes_past_channels, ShuffleChannel group not
dividing the channels, Pooling kernel_0 / stride_0, Convolution stride_0 (read as 1) and negative strides or pads."""
import os
import re
import subprocess
import time

import pytest

import helpers
import loader_cases as L
from oracle import netcheck

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "feathercnn_amd", "csrc")
DRIVER = os.path.join(ROOT, "tests", "cpp", "net_loader_hostile_main.cpp")
# The only time limit: the child process.  The plain run of the whole table (1819 cases) took 0.26 s of wall time where this was written, the
# sanitised one 0.96 s; each child gets five times its figure.  That is little on a loaded machine: a TimeoutExpired here says that the
# machine was busy, not that the driver hung (a hung driver leaves its last finished case in the captured output).
PLAIN_LIMIT_S = 5 * 0.26
SANITISED_LIMIT_S = 5 * 0.96


@pytest.fixture(scope="module")
def table():
    t = L.cases()
    print(f"{len(t)} loader cases: " + ", ".join(f"{sum(c.expectation == e for c in t)} {e}" for e in (L.ACCEPT, L.REFUSE, L.EITHER)))
    return t


@pytest.fixture(scope="module")
def case_dir(table, tmp_path_factory):
    d = tmp_path_factory.mktemp("loader_cases")
    L.write_cases(table, str(d))
    return str(d)


def _net_hip():
    return helpers.net_runtime_source()  # net.hip and the net_*.h it includes: the factories are in the first, the layer classes in the headers


def _body(text, start):
    """The brace-balanced block that opens at or after text[start]."""
    a = text.index("{", start)
    depth, i = 0, a
    while True:
        depth += {"{": 1, "}": -1}.get(text[i], 0)
        i += 1
        if depth == 0:
            return text[a:i]


def _factory():
    """type string -> class name, read out of create_layer."""
    src = _net_hip()
    body = _body(src, src.index("static Layer* create_layer("))
    out = {}
    for cond, cls in re.findall(r"if \(([^;]*?)\) return new (\w+);", body):
        for t in re.findall(r'type == "(\w+)"', cond):
            out[t] = cls
    return out


def test_every_layer_type_has_cases():
    """A type added to create_layer fails here until a base model of tests/loader_cases.py holds it and PARAM_IDS lists its ids."""
    accepted = set(_factory())
    assert len(accepted) >= 25
    assert accepted <= L.base_types(), f"no base model holds {sorted(accepted - L.base_types())}"
    assert accepted == set(L.PARAM_IDS), sorted(accepted ^ set(L.PARAM_IDS))


def test_param_id_table_matches_the_readers():
    """PARAM_IDS against the LoadParam bodies: per class, the ids its types' value cases change are the ids the body reads."""
    src = _net_hip()
    by_class = {}
    for t, cls in _factory().items():
        by_class.setdefault(cls, []).append(t)
    for cls, types in by_class.items():
        struct = _body(src, re.search(r"struct %s\b[^;{]*\{" % cls, src).start())
        m = re.search(r"int LoadParam\(const ParamDict& pd\)", struct)
        body = _body(struct, m.start()) if m else ""
        ints, floats = set(), set()
        for key, default in re.findall(r"pd\.get\((\d+), ([^)]*)\)", body):
            (floats if re.search(r"[\d.]f\b|FLT_MAX", default) else ints).add(int(key))
        arrays = {int(k) for k in re.findall(r"pd\.has_array\((\d+)\)", body)}
        want = [set().union(*(L.PARAM_IDS[t][k] for t in types)) for k in range(3)]
        assert [ints, floats, arrays] == want, (cls, ints, floats, arrays, want)


def test_table_is_deterministic_and_bounded(table):
    again = L.cases()
    assert again == table
    assert 1000 <= len(table) <= 2000
    assert len({c.name for c in table}) == len(table)
    assert sum(c.expectation == L.ACCEPT for c in table) == len(L.base_models())
    # the weight-stream cuts stand on block boundaries that reach the end of every .bin
    for m in L.base_models():
        port = netcheck.PortNet(m.param, m.bin)
        assert port.consumed == len(m.bin) and port.blocks[-1][2] == len(m.bin), m.tag


def _judge(table, stdout):
    """Every case's line of the driver's output against its expectation -> list of complaints."""
    lines = [l for l in stdout.splitlines() if l.startswith("case ")]
    assert len(lines) == len(table), f"{len(lines)} lines for {len(table)} cases"
    bad = []
    for i, (c, line) in enumerate(zip(table, lines)):
        m = re.match(r"case (\d{4}) param (-?\d+) weights (-?\d+|skip) \| (.*)$", line)
        assert m and int(m.group(1)) == i, line
        rp, rw, msg = int(m.group(2)), m.group(3), m.group(4)
        refused = rp if rp else (int(rw) if rw != "skip" else 0)
        if c.expectation == L.ACCEPT and refused:
            bad.append(f"{i:04d} {c.name}: the control did not load: {line}")
        if c.expectation == L.REFUSE:
            if not refused:
                bad.append(f"{i:04d} {c.name}: accepted")
            elif not msg.strip():
                bad.append(f"{i:04d} {c.name}: refused without a message")
            elif c.code is not None and refused != c.code:
                bad.append(f"{i:04d} {c.name}: refused with {refused}, the reference's code is {c.code}")
    return bad


def _run(exe, case_dir, table, limit):
    t0 = time.perf_counter()
    out = subprocess.run([exe, case_dir, str(len(table))], capture_output=True, text=True, timeout=limit)
    wall = time.perf_counter() - t0
    lines = [l for l in out.stdout.splitlines() if l.startswith("case ")]
    summary = out.stdout.strip().splitlines()[-1] if out.stdout.strip() else ""
    print(f"{os.path.basename(exe)}: {wall:.2f} s wall; {summary}")
    if out.returncode != 0 or len(lines) != len(table):
        # the driver flushes one line per finished case: the case after the last line is the one that ended the process
        at = len(lines)
        name = table[at].name if at < len(table) else "(after the last case)"
        pytest.fail(f"driver ended with status {out.returncode} in case {at:04d} {name} ({at} of {len(table)} cases finished)\n" + out.stderr[-3000:])
    return out


def test_readers_meet_every_expectation(table, case_dir, tmp_path):
    """Plain build: g++ against the built library, the whole table in one child process."""
    from feathercnn_amd import _lib
    libdir = os.path.dirname(_lib.lib_path())
    exe = str(tmp_path / "net_loader_hostile")
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), DRIVER, "-o", exe, "-L" + libdir, "-lfeather_hip",
                    "-Wl,-rpath," + libdir], check=True, capture_output=True, text=True)
    out = _run(exe, case_dir, table, PLAIN_LIMIT_S)
    bad = _judge(table, out.stdout)
    assert not bad, f"{len(bad)} cases:\n" + "\n".join(bad[:60])
    assert "hostile loader: %d cases" % len(table) in out.stdout


def test_readers_are_clean_under_sanitizers(table, case_dir, tmp_path):
    """Sanitised build: every translation unit of libfeather_hip.so with its host side under ASan + UBSan (the whole library: it compiles
    in about half a minute), linked with the driver into one ordinary executable under tmp_path.  No preload: the runtime is linked in."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    objdir = str(tmp_path / "obj")
    san = "-fsanitize=address,undefined"
    host = f"-Xarch_host {san} -Xarch_host -fno-sanitize-recover=undefined -g"
    subprocess.run(["make", "-s", "-j", str(min(8, os.cpu_count() or 1)), "-C", CSRC, "OBJDIR=" + objdir, "EXTRA=" + host, "objects"],
                   check=True, capture_output=True, text=True)
    objs = sorted(os.path.join(objdir, f) for f in os.listdir(objdir) if f.endswith(".o"))
    assert len(objs) >= 7
    exe = str(tmp_path / "net_loader_hostile_san")
    subprocess.run([hipcc, "-std=c++17", "-O1", "-g", "-Xarch_host", san, "-Xarch_host", "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"),
                    "-x", "c++", DRIVER, "-x", "none"] + objs + [san, "-o", exe, "-ldl"], check=True, capture_output=True, text=True)
    out = _run(exe, case_dir, table, SANITISED_LIMIT_S)
    assert "ERROR: AddressSanitizer" not in out.stderr and "runtime error:" not in out.stderr and "LeakSanitizer" not in out.stderr, out.stderr[-3000:]
    bad = _judge(table, out.stdout)
    assert not bad, f"{len(bad)} cases:\n" + "\n".join(bad[:60])
