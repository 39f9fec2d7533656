"""Measure the image output path (fhip_float_to_pixels / Net.ExtractPixels).  A measurement tool, not a test.

  1. In one process, alternating call by call: (a) the new kernel for N x 3x224x224 -> 224x224 and -> 640x480 RGB2BGR with mean / norm,
     (b) the existing fhip_pixels_to_float on the same pixel counts the other way round (224x224 and 640x480 uint8 BGR -> 224x224 fp32,
     the mirror-image traffic), (c) a device-to-device copy of the bytes each case moves (the achievable streaming rate).  Every case is
     timed twice: "resident" re-runs one buffer pair (N = 256 at 224x224 is 154 MB of fp32 + 39 MB of bytes: it fits the 256 MiB
     Infinity Cache), "cold" rotates through enough buffer pairs to exceed 1 GiB, so every call streams from HBM.  Torch events around
     each call, medians with min / max over --reps after a warm-up.
  2. A batch out of a net (3 -> 8 -> 3 convolutions at 224x224): Net.ExtractPixels (kernel + uint8 download) against Net.Extract (fp32
     download) + ncnn's host Mat::substract_mean_normalize + Mat::to_pixels_resize on T threads (tools/pixout_host_bench.cpp, g++).

    python tools/pixout_bench.py [--batch 256] [--reps 30] [--threads 16]
Prints one JSON object.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def touched_rows(h, th):
    """Source rows a resize reads (rows sy and sy + 1 of every output row), all of them at equal size."""
    if h == th:
        return h
    import pixels_ref as R
    sy, _, _ = R._coef(h, th)
    return np.unique(np.concatenate([sy, sy + 1])).size


class Case:
    """One timed call with `sets` rotating buffer pairs; bytes = what one call must move (touched source rows + the output)."""

    def __init__(self, name, kind, n, w, h, tw, th, sets):
        import torch

        from feathercnn_amd import PIXEL_BGR2RGB, PIXEL_RGB2BGR, float_to_pixels, pixels_to_float
        self.name, self.times, self.turn = name, [], 0
        mean, norm = [-1.5, 2.25, 0.5], [0.5, 2.0, 1.25]
        if kind == "out":
            src = [torch.rand((n, 3, h, w), device="cuda") * 380 - 60 for _ in range(sets)]
            dst = [torch.empty((n, th, tw, 3), dtype=torch.uint8, device="cuda") for _ in range(sets)]
            self.bytes = n * 3 * touched_rows(h, th) * w * 4 + n * th * tw * 3
            self.fn = lambda k: float_to_pixels(src[k], PIXEL_RGB2BGR, (tw, th), mean, norm, out=dst[k])
        elif kind == "in":
            src = [torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, device="cuda") for _ in range(sets)]
            dst = [torch.empty((n, 3, th, tw), device="cuda") for _ in range(sets)]
            self.bytes = n * touched_rows(h, th) * w * 3 + n * 3 * th * tw * 4
            self.fn = lambda k: pixels_to_float(src[k], PIXEL_BGR2RGB, (tw, th), mean, norm, out=dst[k])
        else:  # copy of `w` bytes read + `w` bytes written
            src = [torch.empty(w, dtype=torch.uint8, device="cuda") for _ in range(sets)]
            dst = [torch.empty(w, dtype=torch.uint8, device="cuda") for _ in range(sets)]
            self.bytes = 2 * w
            self.fn = lambda k: dst[k].copy_(src[k])
        self.sets = sets

    def run(self, record=True):
        import torch
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        self.fn(self.turn % self.sets)
        b.record()
        b.synchronize()
        self.turn += 1
        if record:
            self.times.append(a.elapsed_time(b))

    def result(self):
        med = statistics.median(self.times)
        return {"case": self.name, "median_us": round(med * 1e3, 1), "min_us": round(min(self.times) * 1e3, 1),
                "max_us": round(max(self.times) * 1e3, 1), "bytes_moved": int(self.bytes), "GBps": round(self.bytes / med / 1e6, 1)}


def kernel_group(n, reps, geometry, cold):
    """(a), (b) and the two copies of one geometry, alternated call by call."""
    import torch
    (w, h, tw, th), (iw, ih) = geometry
    label = "cold" if cold else "resident"
    out_bytes = n * 3 * touched_rows(h, th) * w * 4 + n * th * tw * 3
    sets = max(2, -(-(1 << 30) // out_bytes)) if cold else 1
    a = Case(f"(a) float_to_pixels {n} x 3x{w}x{h} -> {tw}x{th}, {label}", "out", n, w, h, tw, th, sets)
    b = Case(f"(b) pixels_to_float {n} x {iw}x{ih}x3 -> 224x224, {label}", "in", n, iw, ih, 224, 224, sets)
    ca = Case(f"copy of (a)'s bytes, {label}", "copy", 0, a.bytes // 2, 0, 0, 0, sets)
    cb = Case(f"copy of (b)'s bytes, {label}", "copy", 0, b.bytes // 2, 0, 0, 0, sets)
    group = [a, b, ca, cb]
    for _ in range(3 * max(sets, 1)):
        for c in group:
            c.run(record=False)
    for _ in range(reps):
        for c in group:
            c.run()
    res = [c.result() for c in group]
    res[0]["fraction_of_copy"] = round(res[0]["GBps"] / res[2]["GBps"], 3)
    res[1]["fraction_of_copy"] = round(res[1]["GBps"] / res[3]["GBps"], 3)
    res[0]["time_ratio_a_over_b"] = round(res[0]["median_us"] / res[1]["median_us"], 3)
    res[1]["spread_of_b"] = round((res[1]["max_us"] - res[1]["min_us"]) / res[1]["median_us"], 3)
    del group
    torch.cuda.empty_cache()
    return res


def extract_case(n, reps, threads):
    import torch

    from feathercnn_amd import PIXEL_RGB2BGR, model_zoo
    from feathercnn_amd.net import Net
    g = model_zoo.GraphBuilder(seed=31)
    top = g.conv("conv2", g.conv("conv1", g.input("data", 3, 224, 224), 3, 8, 3, 1, 1), 8, 3, 3, 1, 1)
    p, b = g.finish()
    net = Net(fusion=3, tuned=True)
    net.LoadParam(p)
    net.LoadWeights(b)
    net.FeedInput("data", np.random.default_rng(0).uniform(-1, 1, (n, 3, 224, 224)).astype(np.float32))
    net.Forward()
    mean, norm = np.array([-1.5, 2.25, 0.5], np.float32), np.array([0.5, 2.0, 1.25], np.float32)

    def timed(fn):
        fn()
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        return ts

    res = {"batch": n, "blob": "3x224x224", "host_threads": threads, "cases": []}
    extract = timed(lambda: net.Extract(top))
    res["Extract_fp32_ms"] = {"median": round(statistics.median(extract) * 1e3, 2), "min": round(min(extract) * 1e3, 2),
                              "max": round(max(extract) * 1e3, 2)}
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "pixout_host_bench")
        subprocess.run(["g++", "-std=c++11", "-O3", "-march=native", "-pthread", "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tools", "pixout_host_bench.cpp"), "-o", exe], check=True)
        for tw, th in ((224, 224), (640, 480)):
            dev = timed(lambda: net.ExtractPixels(top, PIXEL_RGB2BGR, (tw, th), mean, norm))
            out = subprocess.run([exe, str(n), "224", "224", str(tw), str(th), str(threads), str(reps)], capture_output=True, text=True,
                                 check=True).stdout.split()
            host = float(out[1])
            d = statistics.median(dev)
            res["cases"].append({"target": f"{tw}x{th}", "ExtractPixels_ms": {"median": round(d * 1e3, 2), "min": round(min(dev) * 1e3, 2),
                                                                              "max": round(max(dev) * 1e3, 2)},
                                 "host_to_pixels_resize_ms": {"median": round(host * 1e3, 2), "min": round(float(out[2]) * 1e3, 2),
                                                              "max": round(float(out[3]) * 1e3, 2)},
                                 "Extract_plus_host_ms": round((statistics.median(extract) + host) * 1e3, 2),
                                 "speedup": round((statistics.median(extract) + host) / d, 2)})
    net.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--threads", type=int, default=16)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("pixout_bench.py needs a GPU: nothing is measured without one")
    equal, up = ((224, 224, 224, 224), (224, 224)), ((224, 224, 640, 480), (640, 480))
    out = {"device": torch.cuda.get_device_name(0), "kernel": []}
    for geometry in (equal, up):
        for cold in (False, True):
            out["kernel"] += kernel_group(a.batch, a.reps, geometry, cold)
    out["extract"] = extract_case(a.batch, max(5, a.reps // 5), a.threads)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
