#!/usr/bin/env python3
"""tools/yolo_bench.py [--iters N] [--rounds R] [--batches 1,32] -- the YOLO detection head on the device.

The two launches of libfeather_yolo.so's detection at YOLOv3-416 shapes -- three bottoms of 13 x 13, 26 x 26 and 52 x 52 cells, 3 boxes per
cell, 80 classes: 10647 boxes per image -- on random N(0, 1) heads with the objectness drawn from N(-3.3, 1), so that about one box in a
hundred is a candidate at the confidence threshold 0.25 and about nine in ten are at 0.01; NMS threshold 0.45, 256 rows.  Both versions run
the same shapes (version 2 reads them as three YoloDetectionOutput bottoms, with one class score raised by 10 so that its softmax leaves the
confidence to the objectness).  Also Reorg 0=2 on YOLOv2's passthrough plane (64 x 26 x 26).  Times are device
events around an eager loop of calls on a ring of fresh inputs; microseconds per call (both launches), median of the rounds, with GB/s of
the head bytes for the detection (the scoring kernel reads every plane once) and of the bytes moved for Reorg.  No figure here is a pass /
fail bound of any test.  One JSON line per row."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from feathercnn_amd import reorg, yolo_detection  # noqa: E402

CELLS = (13, 26, 52)
BOXES, CLASSES, ROWS = 3, 80, 256
BIASES = [10, 13, 16, 30, 33, 23, 30, 61, 62, 45, 59, 119, 116, 90, 156, 198, 373, 326]
MASK = [6, 7, 8, 3, 4, 5, 0, 1, 2]
SCALES = [32.0, 16.0, 8.0]


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


def row(label, fn, sets, iters, rounds, moved=None, **more):
    t = [timed(fn, sets, iters) for _ in range(rounds)]
    out = {"what": label, "us": round(statistics.median(t), 2), "us_min": round(min(t), 2), "us_max": round(max(t), 2)}
    if moved:
        out["GBps"] = round(moved / statistics.median(t) / 1e3, 1)
    out.update(more)
    print(json.dumps(out), flush=True)


def heads(batch, version):
    xs = []
    for c in CELLS:
        x = torch.randn((batch, BOXES, 5 + CLASSES, c, c), device="cuda")
        x[:, :, 2:4] *= 0.3
        x[:, :, 4] -= 3.3
        if version == 2:
            x[:, :, 5] += 10.0
        xs.append(x.reshape(batch, BOXES * (5 + CLASSES), c, c).contiguous())
    return xs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batches", default="1,32")
    args = ap.parse_args()
    for batch in [int(v) for v in args.batches.split(",")]:
        nbytes = sum(batch * BOXES * (5 + CLASSES) * c * c * 4 for c in CELLS)
        out = torch.empty((batch, ROWS, 6), device="cuda")
        for version in (3, 2):
            extra = dict(mask=MASK, anchors_scale=SCALES) if version == 3 else {}
            biases = BIASES if version == 3 else [b / 32 for b in BIASES[:2 * BOXES]]
            sets = [(heads(batch, version),) for _ in range(max(2, min(16, (320 << 20) // nbytes)))]
            for threshold in (0.25, 0.01):
                fn = lambda xs: yolo_detection(xs, CLASSES, BOXES, biases, threshold, 0.45, ROWS, out=out, **extra)  # noqa: E731
                fn(sets[0][0])
                kept = [int((o[:, 0] > 0).sum()) for o in out.cpu()][:4]
                row(f"yolov{version} 416 n{batch} detection, 10647 boxes, 80 classes, threshold {threshold}", fn, sets, args.iters, args.rounds, nbytes, kept=kept)
        shape = (batch, 64, 26, 26)
        moved = 2 * batch * 64 * 26 * 26 * 4
        sets = [(torch.randn(shape, device="cuda"), torch.empty((batch, 256, 13, 13), device="cuda")) for _ in range(max(2, min(64, (320 << 20) // moved)))]
        row(f"reorg stride 2 n{batch} 64x26^2", lambda x, y: reorg(x, 2, out=y), sets, args.iters, args.rounds, moved)
    print(json.dumps({"done": True}))


if __name__ == "__main__":
    main()
