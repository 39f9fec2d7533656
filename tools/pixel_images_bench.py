"""Measure the mixed-size / cropped image input path (fhip_pixels_to_float_images / Net.FeedPixelImages).  A measurement tool, not a test.

  1. kernel time (torch events, best of --reps after warm-up) for 256 images cycling through 500x375, 640x480, 800x600, 1024x768,
     1280x720 and 1920x1080 BGR, centre-square ROI, to 224x224 RGB with mean / norm; the bytes it must move (the ROI rows the resize
     touches + the fp32 output) and that rate as a fraction of a device-to-device copy of the same byte count; next to it
     fhip_pixels_to_float on 256 x 640x480 (tools/pixels_bench.py's case);
  2. the same batch from host memory into MobileNet-V1's input blob: Net.FeedPixelImages (one copy per ROI's rows + the kernel) against
     the crops converted on the host (tools/pixel_images_host_bench.cpp: dense crop + Mat::from_pixels_resize + substract_mean_normalize
     on T threads) + Net.FeedInput of the fp32 batch, in images/s; and the per-image cost of the ROI copies against one upload of the
     same bytes.

    python tools/pixel_images_bench.py [--batch 256] [--reps 20] [--threads 1,8,16]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

SIZES = [(500, 375), (640, 480), (800, 600), (1024, 768), (1280, 720), (1920, 1080)]
TW = TH = 224


def centre_square(w, h):
    s = min(w, h)
    return (w - s) // 2, (h - s) // 2, s, s


def touched_roi_bytes(n, cin=3):
    """Bytes of the ROI rows the resize reads (rows sy and sy + 1 of every output row, each ROI row's rw * cin bytes once)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import pixels_ref as R
    total = 0
    for i in range(n):
        _, _, rw, rh = centre_square(*SIZES[i % len(SIZES)])
        sy, _, _ = R._coef(rh, TH)
        total += np.unique(np.concatenate([sy, sy + 1])).size * rw * cin
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--threads", default="1,8,16")
    a = ap.parse_args()
    import torch

    from feathercnn_amd import PIXEL_BGR2RGB, model_zoo, pixels_images_to_float
    from feathercnn_amd.net import Net
    from pixels_bench import kernel_case, time_ms
    n = a.batch
    mean, norm = [104, 117, 123], [0.017] * 3
    rng = np.random.default_rng(0)
    host = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for w, h in SIZES]
    dev = [torch.from_numpy(x).cuda() for x in host]
    imgs = [dev[i % len(SIZES)] for i in range(n)]
    rois = [centre_square(*SIZES[i % len(SIZES)]) for i in range(n)]

    # 1. the kernel alone: the plan built and uploaded once, as an application that reuses its buffers would
    from feathercnn_amd import load_library
    from feathercnn_amd.booster import _stream
    from feathercnn_amd.pixels import _image_descs, _plan
    import ctypes
    descs, _, keep = _image_descs(imgs, PIXEL_BGR2RGB, rois)
    plan = _plan(descs, PIXEL_BGR2RGB, TW, TH)
    plan_dev = torch.from_numpy(plan).cuda()
    out = torch.empty((n, 3, TH, TW), device="cuda")
    m, s = np.array(mean, np.float32), np.array(norm, np.float32)
    lib = load_library()

    def launch():
        rc = lib.fhip_pixels_to_float_images(ctypes.c_void_p(out.data_ptr()), plan.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(plan_dev.data_ptr()),
                                             m.ctypes.data_as(ctypes.c_void_p), s.ctypes.data_as(ctypes.c_void_p), _stream())
        assert rc == 0
    ms = time_ms(launch, a.reps)
    ref = pixels_images_to_float(imgs[:len(SIZES)], PIXEL_BGR2RGB, (TW, TH), rois[:len(SIZES)], mean, norm)
    torch.cuda.synchronize()
    assert torch.equal(ref.view(torch.int32), out[:len(SIZES)].view(torch.int32)), "the timed launch differs from the Python path"
    moved = touched_roi_bytes(n) + out.numel() * 4
    buf_a = torch.empty(moved // 2 // 4 * 4, dtype=torch.uint8, device="cuda")
    buf_b = torch.empty_like(buf_a)
    copy_ms = time_ms(lambda: buf_b.copy_(buf_a), a.reps)
    rate, copy_rate = moved / ms / 1e6, 2 * buf_a.numel() / copy_ms / 1e6
    kernel = {"case": f"{n} images cycling {', '.join(f'{w}x{h}' for w, h in SIZES)} BGR, centre square -> {TW}x{TH} RGB + mean/norm",
              "kernel_us": round(ms * 1e3, 1), "bytes_moved": int(moved), "GBps": round(rate, 1), "copy_GBps": round(copy_rate, 1),
              "fraction_of_copy": round(rate / copy_rate, 3), "images_per_s": round(n / ms * 1e3)}
    equal_size = kernel_case(n, 640, 480, TW, TH, a.reps, True)
    del buf_a, buf_b

    # 2. from host memory into MobileNet-V1's blob
    p, b, i, _ = model_zoo.mobilenet_v1()
    net = Net(fusion=3, tuned=True)
    net.LoadParam(p)
    net.LoadWeights(b)
    host_imgs = [host[k % len(SIZES)] for k in range(n)]
    reps = max(3, a.reps // 4)

    def best(fn):
        fn()
        t = float("inf")
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            t = min(t, time.perf_counter() - t0)
        return t

    feed_host = best(lambda: net.FeedPixelImages(i, host_imgs, PIXEL_BGR2RGB, (TW, TH), rois, mean, norm))
    feed_dev = best(lambda: net.FeedPixelImages(i, imgs, PIXEL_BGR2RGB, (TW, TH), rois, mean, norm))
    roi_bytes = sum(r[2] * r[3] * 3 for r in rois)
    packed = np.empty(roi_bytes, np.uint8)
    staging = torch.empty(roi_bytes, dtype=torch.uint8, device="cuda")
    one_upload = best(lambda: staging.copy_(torch.from_numpy(packed)))

    def pack_and_upload():  # the alternative to per-ROI copies: pack the crops on the host (one thread), then one upload
        o = 0
        for img, (x0, y0, rw, rh) in zip(host_imgs, rois):
            packed[o:o + rw * rh * 3].reshape(rh, rw, 3)[:] = img[y0:y0 + rh, x0:x0 + rw]
            o += rw * rh * 3
        staging.copy_(torch.from_numpy(packed))
    pack_upload = best(pack_and_upload)
    x = np.empty((n, 3, TH, TW), np.float32)
    feed_input = best(lambda: net.FeedInput(i, x))
    feed = {"batch": n, "source": "host memory, centre-square ROIs", "roi_bytes": int(roi_bytes),
            "FeedPixelImages_host_ms": round(feed_host * 1e3, 2), "FeedPixelImages_host_images_per_s": round(n / feed_host),
            "FeedPixelImages_device_ms": round(feed_dev * 1e3, 2), "one_upload_of_the_roi_bytes_ms": round(one_upload * 1e3, 2),
            "host_pack_then_one_upload_ms": round(pack_upload * 1e3, 2),
            "per_image_copy_overhead_us": round((feed_host - feed_dev - one_upload) / n * 1e6, 1),
            "FeedInput_fp32_ms": round(feed_input * 1e3, 2), "host": []}
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "pixel_images_host_bench")
        subprocess.run(["g++", "-std=c++11", "-O3", "-march=native", "-pthread", "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tools", "pixel_images_host_bench.cpp"), "-o", exe], check=True)
        for t in [int(v) for v in a.threads.split(",")]:
            res = subprocess.run([exe, str(n), str(TW), str(TH), str(t), str(max(2, reps // 2))] + [f"{w}x{h}" for w, h in SIZES],
                                 capture_output=True, text=True, check=True).stdout
            conv = float(res.split()[1])
            feed["host"].append({"threads": t, "crop_from_pixels_resize_ms": round(conv * 1e3, 1),
                                 "plus_FeedInput_images_per_s": round(n / (conv + feed_input))})
    net.close()
    del keep
    print(json.dumps({"device": torch.cuda.get_device_name(0), "kernel": kernel, "kernel_equal_size_640x480": equal_size, "feed": feed}))


if __name__ == "__main__":
    main()
