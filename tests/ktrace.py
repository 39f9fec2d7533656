"""One way to take and cut a kernel trace: trace() runs a child script in a fresh process under `rocprofv3 --kernel-trace` (no counters) and
reads the CSV files it leaves, between() cuts the kernels at the marker launches, and marker() is the launch the children put around what
they want seen."""
import csv
import ctypes
import glob
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_MARK = []


def trace(child, args, tmp_path, timeout, copies=False, stats=False, ok="child ok"):
    """Run tests/<child> with `args` under rocprofv3 and `timeout` seconds; it must exit with 0 and print `ok` (None: it prints no such line).
    -> (what it printed, the kernel launches as (start timestamp, name, grid, workgroup) sorted by start, the start timestamps of the
    device-to-device copies -- traced only with copies=True).  The grid is as the tool reports it, in work-items or blocks."""
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    assert os.path.exists(prof), "rocprofv3 not found: the trace cannot be taken (a failure, not a skip)"
    tag = "trace" + "".join(str(a) for a in args)
    d, log = tmp_path / tag, tmp_path / (tag + ".log")
    cmd = (["timeout", "-k", "10", str(timeout), prof, "--kernel-trace"] + ["--memory-copy-trace"] * copies + ["--stats"] * stats +
           ["--output-format", "csv", "-d", str(d), "-o", "trace", "--", sys.executable, os.path.join(HERE, child)] + [str(a) for a in args])
    with open(log, "w") as fh:
        rc = subprocess.run(cmd, stdout=fh, stderr=subprocess.STDOUT, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT)).returncode
    text = open(log).read()
    assert rc == 0 and (ok is None or ok in text), f"{child} exited with {rc}:\n{text[-3000:]}"
    files = glob.glob(os.path.join(str(d), "**", "*kernel_trace.csv"), recursive=True)
    assert files, f"no *kernel_trace.csv under {d}: {os.listdir(d)}"
    rows, moved = [], []
    for f in files:
        with open(f, newline="") as fh:
            rows += [(int(r["Start_Timestamp"]), r["Kernel_Name"], int(r.get("Grid_Size_X") or r["Grid_Size"]),
                      int(r.get("Workgroup_Size_X") or r["Workgroup_Size"])) for r in csv.DictReader(fh)]
    for f in glob.glob(os.path.join(str(d), "**", "*memory_copy_trace.csv"), recursive=True):
        with open(f, newline="") as fh:
            moved += [int(r["Start_Timestamp"]) for r in csv.DictReader(fh) if "DEVICE_TO_DEVICE" in (r.get("Direction") or "").upper()]
    return text, sorted(rows), moved


def between(rows, marks, copies=None):
    """The kernel names between each two of the `marks` marker launches (relu_kernel) the trace must hold: marks - 1 lists.  With the copies'
    timestamps also how many of them fall into each window."""
    at = [t for t, name, *_ in rows if "relu_kernel" in name]
    assert len(at) == marks, rows  # the child puts its fhip_relu launches around what it wants seen
    spans = list(zip(at, at[1:]))
    names = [[name for t, name, *_ in rows if a < t < b] for a, b in spans]
    return names if copies is None else (names, [sum(a < t < b for t in copies) for a, b in spans])


def marker():
    """In a child: fhip_relu on 256 floats between two device synchronisations, on the current stream."""
    import torch
    from feathercnn_amd import _lib
    if not _MARK:
        _MARK.append(torch.zeros(256, device="cuda"))
    at = ctypes.c_void_p(_MARK[0].data_ptr())
    torch.cuda.synchronize()
    assert _lib.load_library().fhip_relu(at, at, 256, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    torch.cuda.synchronize()
