"""Measure the uint8 image input path (fhip_pixels_to_float / Net.FeedPixels).  A measurement tool, not a test.

  1. kernel time (torch events, best of --reps after warm-up) for 256 x 640x480 BGR -> 224x224 RGB with mean / norm and for 256 x 256x256
     BGR -> 224x224 RGB, the bytes the kernel must move (touched source rows + fp32 output) and that rate as a fraction of a device-to-device
     copy of the same byte count (the achievable streaming rate on this device);
  2. a batch from host memory into MobileNet-V1's input blob: Net.FeedPixels (one uint8 upload + the kernel) against ncnn's host
     Mat::from_pixels_resize + substract_mean_normalize on T threads (tools/pixels_host_bench.cpp, built with g++) + Net.FeedInput of the
     fp32 batch, in images/s.

    python tools/pixels_bench.py [--batch 256] [--reps 20] [--threads 1,8,16]
Prints one JSON object.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def touched_source_bytes(n, w, h, tw, th, cin):
    """Bytes of the source rows the resize reads (rows sy and sy + 1 of every output row; whole rows, each read once from HBM)."""
    if (w, h) == (tw, th):
        return n * w * h * cin
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import pixels_ref as R
    sy, _, _ = R._coef(h, th)
    rows = np.unique(np.concatenate([sy, sy + 1]))
    return n * rows.size * w * cin


def time_ms(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        best = min(best, a.elapsed_time(b))
    return best


def kernel_case(n, w, h, tw, th, reps, mean_norm):
    import torch

    from feathercnn_amd import PIXEL_BGR2RGB, pixels_to_float
    px = torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, device="cuda")
    out = torch.empty((n, 3, th, tw), device="cuda")
    mean, norm = ([104, 117, 123], [0.017] * 3) if mean_norm else (None, None)
    ms = time_ms(lambda: pixels_to_float(px, PIXEL_BGR2RGB, (tw, th), mean, norm, out=out), reps)
    moved = touched_source_bytes(n, w, h, tw, th, 3) + out.numel() * 4
    # the achievable rate: a device-to-device copy moving the same bytes (read + write)
    a = torch.empty(moved // 2 // 4 * 4, dtype=torch.uint8, device="cuda")
    b = torch.empty_like(a)
    copy_ms = time_ms(lambda: b.copy_(a), reps)
    copy_rate = 2 * a.numel() / copy_ms / 1e6
    rate = moved / ms / 1e6
    return {"case": f"{n} x {w}x{h} BGR -> {tw}x{th} RGB" + (" + mean/norm" if mean_norm else ""), "kernel_us": round(ms * 1e3, 1),
            "bytes_moved": int(moved), "GBps": round(rate, 1), "copy_GBps": round(copy_rate, 1), "fraction_of_copy": round(rate / copy_rate, 3),
            "images_per_s": round(n / ms * 1e3)}


def feed_case(n, w, h, reps, threads):
    import torch

    from feathercnn_amd import PIXEL_BGR2RGB, model_zoo
    from feathercnn_amd.net import Net
    p, b, i, _ = model_zoo.mobilenet_v1()
    net = Net(fusion=3, tuned=True)
    net.LoadParam(p)
    net.LoadWeights(b)
    px = np.random.default_rng(0).integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    mean, norm = np.array([104, 117, 123], np.float32), np.array([0.017] * 3, np.float32)

    def best(fn):
        fn()
        t = float("inf")
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            t = min(t, time.perf_counter() - t0)
        return t

    feed_pixels = best(lambda: net.FeedPixels(i, px, PIXEL_BGR2RGB, (224, 224), mean, norm))
    x = np.empty((n, 3, 224, 224), np.float32)
    feed_input = best(lambda: net.FeedInput(i, x))
    res = {"batch": n, "source": f"{w}x{h} BGR host memory", "FeedPixels_ms": round(feed_pixels * 1e3, 2),
           "FeedPixels_images_per_s": round(n / feed_pixels), "FeedInput_fp32_ms": round(feed_input * 1e3, 2), "host": []}
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "pixels_host_bench")
        subprocess.run(["g++", "-std=c++11", "-O3", "-march=native", "-pthread", "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tools", "pixels_host_bench.cpp"), "-o", exe], check=True)
        for t in threads:
            out = subprocess.run([exe, str(n), str(w), str(h), "224", "224", str(t), str(max(2, reps // 4)), "-"], capture_output=True,
                                 text=True, check=True).stdout
            conv = float(out.split()[1])
            res["host"].append({"threads": t, "from_pixels_resize_ms": round(conv * 1e3, 1),
                                "plus_FeedInput_images_per_s": round(n / (conv + feed_input))})
    net.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--threads", default="1,8,16")
    a = ap.parse_args()
    import torch
    out = {"device": torch.cuda.get_device_name(0),
           "kernel": [kernel_case(a.batch, 640, 480, 224, 224, a.reps, True), kernel_case(a.batch, 256, 256, 224, 224, a.reps, False)],
           "feed": feed_case(a.batch, 640, 480, max(3, a.reps // 4), [int(t) for t in a.threads.split(",")])}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
