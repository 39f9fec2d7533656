#!/usr/bin/env python3
"""tools/frame_bench.py [--iters N] [--rounds R] [--batch B] [--net-batch B] [--no-nets] -- the framing layers on the device.

libfeather_frame.so at the shapes of the zoo's image-to-image nets: the reflection Paddings of cyclegan_resnet9 at 256 px (3 in front of the
7x7 convolutions on 3 and on 64 channels, 1 inside the nine residual blocks on 256 x 64 x 64), the two PixelShuffle stages of srresnet_x4
at 96 px (256 x 96 x 96 and 256 x 192 x 192, with and without the ReLU), a zero "SAME" Padding (0, 1, 0, 1) of MobileNet's 64 x 112 x 112 map
and an FCN-style Crop.  Each row moves its input once and its output once; next to it stands a plain hipMemcpyAsync device-to-device copy
that moves the same bytes (half of them read, half written), timed in the same call -- that copy is the yardstick -- and the fraction of the
HBM peak the project uses (benchkit.PEAK_HBM_GBS).  Times are device events around an eager loop of calls on a ring of buffers larger than
the 256 MiB last-level cache where the batch allows; microseconds per call, median of the rounds.

Then the zero-Padding fold: mobilenet_v1_tf at fusion level 1 (the Paddings run) and 2 (folded into the convolutions) next to mobilenet_v1,
whose convolutions pad symmetrically -- rounds alternate between the three nets, milliseconds per Forward, median.

No figure here is a pass / fail bound of any test.  One JSON line per row."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from benchkit import PEAK_HBM_GBS  # noqa: E402
from feathercnn_amd import frame, model_zoo  # noqa: E402
from feathercnn_amd.net import Net  # noqa: E402

RING_BYTES = 640 << 20


def timed(fn, sets, iters):
    iters = -(-iters // len(sets)) * len(sets)
    for k in range(min(len(sets), 3)):
        fn(*sets[-1 - k])
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for k in range(iters):
        fn(*sets[k % len(sets)])
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def device_copy():
    """hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, the current stream) of the HIP runtime this process has mapped -- the file
    torch loaded, found in the process's own map and opened by that path, so that no second runtime enters the process."""
    torch.cuda.current_stream()  # the runtime is mapped at the latest now
    with open("/proc/self/maps") as fh:
        paths = sorted({ln.split()[-1] for ln in fh if "libamdhip64.so" in ln})
    if len(paths) != 1:
        raise SystemExit(f"frame_bench: expected one mapped libamdhip64, found {paths}")
    hip = ctypes.CDLL(paths[0])
    fn = hip.hipMemcpyAsync
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]

    def copy(dst, src):
        rc = fn(dst.data_ptr(), src.data_ptr(), src.numel() * 4, 3, torch.cuda.current_stream().cuda_stream)
        if rc:
            raise RuntimeError(f"hipMemcpyAsync failed with {rc}")
    return copy


def row(label, fn, shape, out_shape, copy, iters, rounds):
    """fn(out, x) against copy(dst, src) of the same bytes, rounds alternating."""
    n_in, n_out = int(np.prod(shape)), int(np.prod(out_shape))
    moved = 4 * (n_in + n_out)
    count = max(2, min(16, RING_BYTES // moved + 1))
    sets = [(torch.empty(out_shape, device="cuda"), torch.randn(shape, device="cuda")) for _ in range(count)]
    half = (n_in + n_out) // 2
    copies = [(torch.empty(half, device="cuda"), torch.randn(half, device="cuda")) for _ in range(count)]
    t, c = [], []
    for _ in range(rounds):
        t.append(timed(fn, sets, iters))
        c.append(timed(copy, copies, iters))
    us, cus = statistics.median(t), statistics.median(c)
    print(json.dumps({"what": label, "in": list(shape), "out": list(out_shape), "MB": round(moved / 1e6, 2), "ring": count, "us": round(us, 2), "us_min": round(min(t), 2),
                      "us_max": round(max(t), 2), "GBps": round(moved / us / 1e3, 1), "hbm_frac": round(moved / us / 1e3 / PEAK_HBM_GBS, 3), "copy_us": round(cus, 2),
                      "copy_GBps": round(8 * half / cus / 1e3, 1), "vs_copy": round(cus / us, 3)}), flush=True)


def kernels(batch, iters, rounds):
    copy = device_copy()

    def window(label, shape, route_type, **kw):
        n, c, h, w = shape
        out_shape = (n,) + frame.window_output_dim(c, h, w, kw.get("front", 0), kw.get("behind", 0), kw.get("top", 0), kw.get("bottom", 0), kw.get("left", 0), kw.get("right", 0))
        pads = any(v > 0 for k, v in kw.items() if k != "type")
        name = frame.frame_route(frame.WINDOW, route_type, 0, int(pads), out_shape[3], 1)
        row(f"{label} [{name}]", lambda o, x: frame.window(x, out=o, **kw), shape, out_shape, copy, iters, rounds)

    def shuffle(label, shape, r, relu=frame.RELU_NONE):
        n, c, h, w = shape
        out_shape = (n,) + frame.pixel_shuffle_output_dim(r, c, h, w)
        name = frame.frame_route(frame.SHUFFLE, r, w, h)
        row(f"{label} [{name}]", lambda o, x: frame.pixel_shuffle(x, r, 0, relu, 0.2, out=o), shape, out_shape, copy, iters, rounds)

    for n in sorted({1, batch}):
        window(f"cyclegan_resnet9 pad1: reflect 3, n{n}", (n, 3, 256, 256), 2, type=frame.REFLECT, top=3, bottom=3, left=3, right=3)
        window(f"cyclegan_resnet9 res*_pad: reflect 1, n{n}", (n, 256, 64, 64), 2, type=frame.REFLECT, top=1, bottom=1, left=1, right=1)
        window(f"cyclegan_resnet9 pad_out: reflect 3, n{n}", (n, 64, 256, 256), 2, type=frame.REFLECT, top=3, bottom=3, left=3, right=3)
        window(f"mobilenet_v1_tf conv3_pad: zero 0,1,0,1, n{n}", (n, 64, 112, 112), 0, top=0, bottom=1, left=0, right=1)
        window(f"replicate 2 of 64 x 128 x 128, n{n}", (n, 64, 128, 128), 1, type=frame.REPLICATE, top=2, bottom=2, left=2, right=2)
        window(f"FCN crop 21 x 568 x 568 -> 500 x 500 at 19, n{n}", (n, 21, 568, 568), 0, top=-19, bottom=-49, left=-19, right=-49)
        shuffle(f"srresnet_x4 up1_ps: r 2, n{n}", (n, 256, 96, 96), 2)
        shuffle(f"srresnet_x4 up2_ps: r 2, n{n}", (n, 256, 192, 192), 2)
        shuffle(f"srresnet_x4 up2_ps + ReLU 0.2: r 2, n{n}", (n, 256, 192, 192), 2, frame.RELU_SLOPE)
        shuffle(f"espcn_x3 out: r 3 of 9 x 180 x 240, n{n}", (n, 9, 180, 240), 3)


def nets(batch, iters, rounds):
    built = {}
    for label, name, level in (("mobilenet_v1_tf fusion 1 (Paddings run)", "mobilenet_v1_tf", 1), ("mobilenet_v1_tf fusion 2 (Paddings folded)", "mobilenet_v1_tf", 2),
                               ("mobilenet_v1 fusion 1", "mobilenet_v1", 1), ("mobilenet_v1 fusion 2", "mobilenet_v1", 2)):
        p, b, i, o = model_zoo.MODELS[name]()
        net = Net(fusion=level)
        net.SetFrame()
        net.LoadParam(p)
        net.LoadWeights(b)
        net.FeedInput(i, np.random.default_rng(0).uniform(-1, 1, (batch, 3, 224, 224)).astype(np.float32))
        for _ in range(3):
            net.Forward()
        torch.cuda.synchronize()
        built[label] = (net, sum(t == "Padding" for t, _, _ in net.layers()), net.Extract(o))
    times = {k: [] for k in built}
    for _ in range(rounds):
        for label, (net, _, _) in built.items():  # the nets alternate inside a round
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters):
                net.Forward()
            torch.cuda.synchronize()
            times[label].append((time.perf_counter() - t0) * 1e3 / iters)
    tf1, tf2 = built["mobilenet_v1_tf fusion 1 (Paddings run)"][2], built["mobilenet_v1_tf fusion 2 (Paddings folded)"][2]
    for label, (net, paddings, _) in built.items():
        t = times[label]
        print(json.dumps({"what": f"{label}, n{batch}", "padding_layers": paddings, "layers": len(net.layers()), "ms": round(statistics.median(t), 4),
                          "ms_min": round(min(t), 4), "ms_max": round(max(t), 4)}), flush=True)
    print(json.dumps({"what": "mobilenet_v1_tf fusion 2 against fusion 1: the largest difference of the class probabilities", "max_abs": float(np.abs(tf1 - tf2).max())}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--net-batch", type=int, default=8)
    ap.add_argument("--no-nets", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("frame_bench needs the GPU: nothing is measured without one")
    kernels(args.batch, args.iters, args.rounds)
    if not args.no_nets:
        nets(args.net_batch, max(args.iters // 4, 10), args.rounds)
    print(json.dumps({"done": True}))


if __name__ == "__main__":
    main()
