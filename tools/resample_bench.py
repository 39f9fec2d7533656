#!/usr/bin/env python3
"""tools/resample_bench.py [--iters N] [--nets] -- the kernels of libfeather_resample.so on the tensors of the nets they are for, each against
a device-to-device copy of the same number of OUTPUT bytes timed in the same process, the candidates alternating, best of three rounds:
  nearest x2     FPN's top-down path on ResNet-50 at 224 px (256 channels, 7 -> 14 -> 28 -> 56), batch 16; alone, and fused with the add
  bilinear       DeepLab's logits, 21 channels 41 x 41 -> 321 x 321, batch 8
  bilinear x2    the decoder of unet_bilinear at 256 px, batch 4
  HardSwish      MobileNet-V3-Large's tensors at 224 px, batch 64
Reported: microseconds, and GB/s of the bytes written plus the bytes read once (the input, and the residual where there is one) -- the
traffic a perfect kernel moves; the copy moves the output's bytes twice (a read and a write), which is what its GB/s counts.
Cold: a ring of tensors of more than 256 MiB (the Infinity Cache) in all, walked in order.  Times are device events around an eager loop
of launches (bounded below by the host's cost per enqueue: a row near 8 us measures the enqueue, not the kernel).
The fused upsample-add-ReLU is also timed as a net (Interp, Eltwise, ReLU between two inputs) at fusion level 0 -- three launches -- against
level 2 -- one --, both replayed from their graphs, alternating, on the host clock between device-wide synchronisations.
--nets adds mobilenet_v3_large (batch 64, fusion level 2) through tools/net_bench.py.  Prints table rows and one JSON line at the end."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from benchkit import PEAK_HBM_GBS  # noqa: E402
from feathercnn_amd import hard_swish, interp, model_zoo  # noqa: E402
from feathercnn_amd.net import Net  # noqa: E402
from feathercnn_amd.resample import hard_swish_route, interp_route  # noqa: E402

# (label, mode, batch, channels, in plane, out plane, with a residual)
INTERP = [("fpn 256x7^2 x2", "nearest", 16, 256, 7, 14, False), ("fpn 256x14^2 x2", "nearest", 16, 256, 14, 28, False),
          ("fpn 256x28^2 x2", "nearest", 16, 256, 28, 56, False), ("fpn 256x14^2 x2 +add", "nearest", 16, 256, 14, 28, True),
          ("fpn 256x28^2 x2 +add", "nearest", 16, 256, 28, 56, True), ("deeplab 21x41^2->321^2", "bilinear", 8, 21, 41, 321, False),
          ("unet 256x8^2 x2", "bilinear", 4, 256, 8, 16, False), ("unet 512x16^2 x2", "bilinear", 4, 512, 16, 32, False),
          ("unet 256x32^2 x2", "bilinear", 4, 256, 32, 64, False), ("unet 128x64^2 x2", "bilinear", 4, 128, 64, 128, False),
          ("unet 64x128^2 x2", "bilinear", 4, 64, 128, 256, False)]
# (label, batch, channels, plane)
HARDSWISH = [("mbv3 16x112^2", 64, 16, 112), ("mbv3 240x28^2", 64, 240, 28), ("mbv3 240x14^2", 64, 240, 14), ("mbv3 480x14^2", 64, 480, 14),
             ("mbv3 672x14^2", 64, 672, 14), ("mbv3 672x7^2", 64, 672, 7), ("mbv3 960x7^2", 64, 960, 7)]
L3 = 256 << 20


def ring_of(shapes):
    """A ring of tensor sets (one tensor per shape) of more than the Infinity Cache in all."""
    per = sum(int(np.prod(s)) * 4 for s in shapes)
    ring = max(2, -(-(L3 + (L3 >> 2)) // per))
    return [tuple(torch.randn(s, device="cuda") for s in shapes) for _ in range(ring)]


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


def timed_wall(fn, sets, iters):
    """Host clock between two device-wide synchronisations: for work on a stream of its own (a net), which torch's events do not see."""
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / iters


def best_of(cands, sets, iters, rounds=3, timed=timed):
    best = {}
    for _ in range(rounds):
        for nm, fn in cands:
            t = timed(fn, sets, iters)
            best[nm] = min(best.get(nm, t), t)
    return best


def upsample_add_net(c, plane, level, x, lat):
    g = model_zoo.GraphBuilder(3)
    a = g.input("x", c, plane, plane)
    s = g.input("lat", c, 2 * plane, 2 * plane)
    g.relu("out", g.eltwise("sum", s, g.interp("up", a, "nearest", scale=2.0)))
    p, w = g.finish()
    net = Net(fusion=level, graph=True)
    net.SetExtendedLayers(True)
    net.LoadParam(p)
    net.LoadWeights(w)
    net.FeedInput("x", x)
    net.FeedInput("lat", lat)
    for _ in range(3):
        net.Forward()
    return net


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--nets", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("resample_bench needs a GPU")
    rows = []
    for label, mode, n, c, pi, po, res in INTERP:
        shapes = [(n, c, pi, pi), (n, c, po, po), (n, c, po, po)]  # input, output, and the residual / the copy's source
        out_bytes = n * c * po * po * 4
        moved = out_bytes + n * c * pi * pi * 4 + (out_bytes if res else 0)
        sets = ring_of(shapes)

        def ours(x, y, r):
            interp(x, mode, size=(po, po), residual=r if res else None, relu=res, out=y)

        def copy(x, y, r):
            y.copy_(r)

        t = best_of((("ours", ours), ("copy", copy)), sets, args.iters)
        route = interp_route(sets[0][0], mode, size=(po, po), out=sets[0][1], residual=sets[0][2] if res else None).replace("fhip::", "")
        row = {"shape": label, "batch": n, "route": route, "out_MB": out_bytes / 1e6, "us": t["ours"], "gbs": moved / t["ours"] / 1e3,
               "copy_us": t["copy"], "copy_gbs": 2 * out_bytes / t["copy"] / 1e3, "time_over_copy": t["ours"] / t["copy"]}
        print(json.dumps(row), flush=True)
        rows.append(row)
        del sets
        torch.cuda.empty_cache()
    for label, n, c, plane in HARDSWISH:
        shape = (n, c, plane, plane)
        nbytes = int(np.prod(shape)) * 4
        sets = ring_of([shape, shape])
        t = best_of((("ours", lambda x, y: hard_swish(x, 1.0 / 6, 0.5, out=y)), ("copy", lambda x, y: y.copy_(x))), sets, args.iters)
        row = {"shape": label, "batch": n, "route": hard_swish_route(sets[0][0], sets[0][1]).replace("fhip::", ""), "out_MB": nbytes / 1e6, "us": t["ours"],
               "gbs": 2 * nbytes / t["ours"] / 1e3, "copy_us": t["copy"], "copy_gbs": 2 * nbytes / t["copy"] / 1e3, "time_over_copy": t["ours"] / t["copy"]}
        print(json.dumps(row), flush=True)
        rows.append(row)
        del sets
        torch.cuda.empty_cache()
    nets = []
    for c, plane, n in ((256, 14, 16), (256, 28, 16)):
        x, lat = torch.randn((n, c, plane, plane), device="cuda"), torch.randn((n, c, 2 * plane, 2 * plane), device="cuda")
        pair = {lv: upsample_add_net(c, plane, lv, x, lat) for lv in (0, 2)}
        t = best_of([(f"level{lv}", (lambda lv=lv: pair[lv].Forward())) for lv in (0, 2)], [()], args.iters, timed=timed_wall)
        row = {"upsample_add_relu": f"{c}x{plane}^2 -> {2 * plane}^2", "batch": n, "us": t, "layers": {lv: len(pair[lv].layers()) for lv in pair},
               "level2_over_level0": t["level2"] / t["level0"]}
        print(json.dumps(row), flush=True)
        nets.append(row)
        for net in pair.values():
            net.close()
    if args.nets:
        import net_bench
        net_bench.run("mobilenet_v3_large", 64, 2)
    print(json.dumps({"resample_bench": rows, "upsample_add_nets": nets, "peak_hbm_gbs": PEAK_HBM_GBS}))


if __name__ == "__main__":
    main()
