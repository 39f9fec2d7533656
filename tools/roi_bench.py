#!/usr/bin/env python3
"""tools/roi_bench.py [--iters N] [--rounds R] [--batches 1,8] -- the heads of the two-stage detectors on the device.

libfeather_roi.so at the published shapes: Proposal on VGG-16's conv5 map of a 600 x 800 image -- 38 x 50 cells, 9 anchors: 17100 anchors per
image, pre_nms_topN 6000, after_nms_topN 300, NMS threshold 0.7, min_size 16 -- on uniform scores and deltas drawn from N(0, 0.2), so that
neighbouring anchors overlap as an RPN's do; ROIPooling 7 x 7 at 1/16 over the 512 channels of that map and the 300 ROIs the Proposal gave;
R-FCN's PSROIPooling 7 x 7 x 21 over 1029 score maps; and ROIAlign (version 1, sampling_ratio 2) on the ROIPooling shapes.  Times are device
events around an eager loop of calls on a ring of fresh inputs; microseconds per call, median of the rounds, with GB/s of the bytes a call
must move at the least (the Proposal: both bottoms read once; a ROI layer: its output written once).  No figure here is a pass / fail bound
of any test.  One JSON line per row."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from feathercnn_amd import proposal, psroi_pool, roi_align, roi_pool  # noqa: E402

H, W, A, ROIS = 38, 50, 9, 300


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


def rpn(batch):
    score = torch.rand((batch, 2 * A, H, W), device="cuda")
    bbox = torch.randn((batch, 4 * A, H, W), device="cuda") * 0.2
    return score, bbox


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batches", default="1,8")
    args = ap.parse_args()
    for batch in [int(v) for v in args.batches.split(",")]:
        info = torch.tensor([[600.0, 800.0, 1.0]] * batch, device="cuda")
        sets = [rpn(batch) for _ in range(8)]
        for pre in (6000, 0):
            fn = lambda s, b: proposal(s, b, info, pre_nms_topN=pre, after_nms_topN=ROIS)  # noqa: E731
            rois = fn(*sets[0])
            kept = [int((r[:, 2] >= r[:, 0]).sum()) for r in rois.cpu()][:4]
            row(f"proposal n{batch} 38x50x9 = 17100 anchors, pre_nms_topN {pre}, 300 rows", fn, sets, args.iters, args.rounds, batch * 6 * A * H * W * 4, kept=kept)
        rois = proposal(*sets[0], info, after_nms_topN=ROIS)
        feats = [(torch.randn((batch, 512, H, W), device="cuda"),) for _ in range(4)]
        out_bytes = batch * ROIS * 512 * 49 * 4
        row(f"roi_pool n{batch} 512x38x50, 300 rois, 7x7 at 1/16", lambda x: roi_pool(x, rois, 7, 0.0625), feats, args.iters, args.rounds, out_bytes)
        row(f"roi_align v1 s2 n{batch} 512x38x50, 300 rois, 7x7 at 1/16", lambda x: roi_align(x, rois, 7, 0.0625, 2, True, 1), feats, args.iters, args.rounds, out_bytes)
        row(f"roi_align v0 s0 n{batch} 512x38x50, 300 rois, 7x7 at 1/16", lambda x: roi_align(x, rois, 7, 0.0625, 0, False, 0), feats, args.iters, args.rounds, out_bytes)
        del feats
        maps = [(torch.randn((batch, 21 * 49, H, W), device="cuda"),) for _ in range(4)]
        row(f"psroi_pool n{batch} 1029x38x50, 300 rois, 7x7x21 at 1/16", lambda x: psroi_pool(x, rois, 21, 7, 0.0625), maps, args.iters, args.rounds,
            batch * ROIS * 21 * 49 * 4)
        del maps
    print(json.dumps({"done": True}))


if __name__ == "__main__":
    main()
