"""Measure the NV21 frame input path (fhip_yuv420sp_to_float / Net.FeedYUV420sp).  A measurement tool, not a test.

  1. kernel time (torch events, best of --reps after warm-up) for --batch x 1920x1080 NV21 -> 224x224 RGB2BGR with mean / norm, for both
     chains (resize_first 1: resize_bilinear_yuv420sp first; 0: yuv420sp2rgb first, resize in RGB); the bytes the kernel must touch
     (source rows the resize reads + fp32 output) and that rate as a fraction of a device-to-device copy of the same byte count;
  2. a batch from host memory into MobileNet-V1's input blob, in images/s: Net.FeedYUV420sp (one uint8 upload of 1.5 bytes per pixel +
     the kernel), against the host chain yuv420sp2rgb + from_pixels_resize + substract_mean_normalize on T threads
     (tools/yuv_host_bench.cpp, built with g++) + Net.FeedInput of the fp32 batch, and against Net.FeedPixels of the same frames as BGR
     (3 bytes per pixel).

    python tools/yuv_bench.py [--batch 256] [--reps 20] [--threads 1,8,16]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

from pixels_bench import time_ms  # noqa: E402


def touched_source_bytes(n, w, h, tw, th, resize_first):
    """Bytes of the frame rows the kernel reads: Y rows sy, sy + 1 of every output row and the VU rows they (or, resize_first, the
    half-size resize) need; whole rows, each read once from HBM."""
    import pixels_ref as R
    sy, _, _ = R._coef(h, th)
    yrows = np.unique(np.concatenate([sy, sy + 1]))
    if resize_first:
        uy, _, _ = R._coef(h // 2, th // 2)
        vurows = np.unique(np.concatenate([uy, uy + 1]))
    else:
        vurows = np.unique(yrows >> 1)
    return n * (yrows.size + vurows.size) * w


def kernel_case(n, w, h, tw, th, reps, resize_first):
    import torch

    from feathercnn_amd import PIXEL_RGB2BGR, yuv420sp_to_float
    f = torch.randint(0, 256, (n, h * 3 // 2, w), dtype=torch.uint8, device="cuda")
    out = torch.empty((n, 3, th, tw), device="cuda")
    mean, norm = [104, 117, 123], [0.017] * 3
    ms = time_ms(lambda: yuv420sp_to_float(f, PIXEL_RGB2BGR, (tw, th), resize_first, mean, norm, out=out), reps)
    moved = touched_source_bytes(n, w, h, tw, th, resize_first) + out.numel() * 4
    a = torch.empty(moved // 2 // 4 * 4, dtype=torch.uint8, device="cuda")
    b = torch.empty_like(a)
    copy_ms = time_ms(lambda: b.copy_(a), reps)
    copy_rate = 2 * a.numel() / copy_ms / 1e6
    rate = moved / ms / 1e6
    del f, a, b
    return {"case": f"{n} x {w}x{h} NV21 -> {tw}x{th} RGB2BGR + mean/norm, resize_first={int(resize_first)}", "kernel_us": round(ms * 1e3, 1),
            "bytes_touched": int(moved), "GBps": round(rate, 1), "copy_GBps": round(copy_rate, 1),
            "fraction_of_copy": round(rate / copy_rate, 3), "images_per_s": round(n / ms * 1e3)}


def feed_case(n, w, h, reps, threads):
    import torch

    from feathercnn_amd import PIXEL_BGR, PIXEL_RGB2BGR, model_zoo
    from feathercnn_amd.net import Net
    p, b, i, _ = model_zoo.mobilenet_v1()
    net = Net(fusion=3, tuned=True)
    net.LoadParam(p)
    net.LoadWeights(b)
    f = np.random.default_rng(0).integers(0, 256, (n, h * 3 // 2, w), dtype=np.uint8)
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

    res = {"batch": n, "source": f"{w}x{h} NV21 host memory", "FeedYUV420sp": []}
    for rf in (True, False):
        s = best(lambda: net.FeedYUV420sp(i, f, PIXEL_RGB2BGR, (224, 224), rf, mean, norm))
        res["FeedYUV420sp"].append({"resize_first": int(rf), "ms": round(s * 1e3, 2), "images_per_s": round(n / s)})
    del f
    bgr = np.random.default_rng(1).integers(0, 256, (n, h, w, 3), dtype=np.uint8)  # the same frame size as BGR, 3 bytes per pixel
    s = best(lambda: net.FeedPixels(i, bgr, PIXEL_BGR, (224, 224), mean, norm))
    res["FeedPixels_BGR"] = {"ms": round(s * 1e3, 2), "images_per_s": round(n / s)}
    del bgr
    x = np.empty((n, 3, 224, 224), np.float32)
    feed_input = best(lambda: net.FeedInput(i, x))
    res["FeedInput_fp32_ms"] = round(feed_input * 1e3, 2)
    res["host"] = []
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "yuv_host_bench")
        subprocess.run(["g++", "-std=c++11", "-O3", "-march=native", "-pthread", "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tools", "yuv_host_bench.cpp"), "-o", exe], check=True)
        for t in threads:
            out = subprocess.run([exe, str(n), str(w), str(h), "224", "224", str(t), str(max(2, reps // 4))], capture_output=True,
                                 text=True, check=True).stdout
            conv = float(out.split()[1])
            res["host"].append({"threads": t, "yuv420sp2rgb_from_pixels_resize_ms": round(conv * 1e3, 1),
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
           "kernel": [kernel_case(a.batch, 1920, 1080, 224, 224, a.reps, rf) for rf in (True, False)],
           "feed": feed_case(a.batch, 1920, 1080, max(3, a.reps // 4), [int(t) for t in a.threads.split(",")])}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
