#!/usr/bin/env python3
"""tools/detect_bench.py [--iters N] [--rounds R] [--batches 1,32] [--no-nets] [--no-kernels] -- the SSD detection head on the device.

Nets: mobilenet_ssd and vgg16_ssd300 (Net.SetDetection; the second with Net.SetDilated) at batches 1 and 32 and fusion levels 1 and 2:
per-layer times of one eager forward (Net.forward_timed: device events around every layer, each bounded below by the host's cost per
enqueue), summed into the backbone (Convolution, BatchNorm / Scale, ReLU, Pooling, Split), the head (every layer of route DETECT), its
largest parts by layer type, and the whole forward; the median of --rounds forwards.  A Concat of permuted heads is one launch at level 2
and twelve permutes, twelve views and six copies at level 1, so `Concat` + `Permute` of the two levels is the fused rule's comparison.

Kernels: every kernel of libfeather_detect.so alone at SSD300 (8732 priors, VGG-16's six source maps) and SSD512 (24564 priors, seven
maps) sizes, batch from --batches, 21 classes: Permute order 3 of every location head, the fused permute-concat of all of them next to
the unfused form (a permute per source into a preallocated blob and a strided copy per source into the concatenated row), Normalize
on conv4_3 (512 channels), the strided softmax over [P][21] transposed (axis not innermost), DetectionOutput (nms_top_k 400, keep_top_k
200, confidence threshold 0.01) on softmaxed N(0, 3) logits.  Times are device events around an eager loop of launches on fresh tensors
of a ring larger than the Infinity Cache where the tensor is small enough; microseconds per call, median of the rounds, with GB/s of the
bytes a perfect kernel moves where that means something.  No figure here is a pass / fail bound of any test.  One JSON line per row."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from feathercnn_amd import axis_softmax, detection_output, model_zoo, normalize, permute, permute_concat, priorbox  # noqa: E402
from feathercnn_amd.net import Net  # noqa: E402

# (cells, priors per cell, channels of the source map)
SSD300 = [(38, 4, 512), (19, 6, 1024), (10, 6, 512), (5, 6, 256), (3, 4, 256), (1, 4, 256)]
SSD512 = [(64, 4, 512), (32, 6, 1024), (16, 6, 512), (8, 6, 256), (4, 6, 256), (2, 4, 256), (1, 4, 256)]
L3 = 256 << 20
BACKBONE = ("Convolution", "ConvolutionDepthWise", "BatchNorm", "Scale", "ReLU", "Pooling", "Split", "Input")


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


def ring(make, nbytes):
    return [make() for _ in range(max(2, min(64, -(-(L3 + (L3 >> 2)) // max(nbytes, 1)))))]


def row(label, fn, sets, iters, rounds, moved=None):
    t = [timed(fn, sets, iters) for _ in range(rounds)]
    out = {"what": label, "us": round(statistics.median(t), 2), "us_min": round(min(t), 2), "us_max": round(max(t), 2)}
    if moved:
        out["GBps"] = round(moved / statistics.median(t) / 1e3, 1)
    print(json.dumps(out), flush=True)
    return out


def kernels(name, maps, batch, iters, rounds):
    dev = "cuda"
    priors = sum(c * c * p for c, p, _ in maps)
    for cells, per, _ in maps[:3]:
        shape = (batch, 4 * per, cells, cells)
        nbytes = int(np.prod(shape)) * 4
        sets = ring(lambda: (torch.randn(shape, device=dev), torch.empty(shape, device=dev)), 2 * nbytes)
        row(f"{name} n{batch} permute order 3 {4 * per}x{cells}^2", lambda x, y: permute(x, 3, out=y.view(batch, cells, cells, 4 * per)), sets, iters, rounds, 2 * nbytes)
    nbytes = batch * 4 * priors * 4
    sets = ring(lambda: ([torch.randn((batch, 4 * p, c, c), device=dev) for c, p, _ in maps], torch.empty((batch, 4 * priors), device=dev),
                         [torch.empty((batch, c, c, 4 * p), device=dev) for c, p, _ in maps]), 3 * nbytes)
    row(f"{name} n{batch} permute-concat of {len(maps)} location heads", lambda xs, y, tmp: permute_concat(xs, out=y), sets, iters, rounds, 2 * nbytes)

    def unfused(xs, y, tmp):  # what fusion levels 0 and 1 run: a permute per source into a blob of its own, then a strided copy per source
        at = 0
        for x, t in zip(xs, tmp):
            permute(x, 3, out=t)
            y[:, at:at + t[0].numel()].copy_(t.view(batch, -1))
            at += t[0].numel()

    row(f"{name} n{batch} the same as {len(maps)} permutes and {len(maps)} copies", unfused, sets, iters, rounds, 4 * nbytes)
    cells = maps[0][0]
    shape = (batch, 512, cells, cells)
    nbytes = int(np.prod(shape)) * 4
    scale = torch.full((512,), 20.0, device=dev)
    sets = ring(lambda: (torch.randn(shape, device=dev), torch.empty(shape, device=dev)), 2 * nbytes)
    row(f"{name} n{batch} normalize 512x{cells}^2", lambda x, y: normalize(x, scale, out=y), sets, iters, rounds, 2 * nbytes)
    shape = (batch, 21, priors)
    sets = ring(lambda: (torch.randn(shape, device=dev), torch.empty(shape, device=dev)), 2 * batch * 21 * priors * 4)
    row(f"{name} n{batch} strided softmax [21][{priors}] axis 0", lambda x, y: axis_softmax(x, 1, out=y), sets, iters, rounds, 2 * batch * 21 * priors * 4)
    prior = torch.from_numpy(np.concatenate([priorbox(c, c, 300, 300, [30.0 + 40 * i], [60.0 + 40 * i], [2.0, 3.0][:1 if p == 4 else 2])
                                             for i, (c, p, _) in enumerate(maps)], axis=1)[None]).to(dev)
    assert prior.shape[2] == 4 * priors, (prior.shape, priors)

    def make():
        conf = torch.softmax(torch.randn((batch, priors, 21), device=dev) * 3, dim=2).reshape(batch, -1).contiguous()
        return torch.randn((batch, 4 * priors), device=dev) * 0.3, conf

    sets = [make() for _ in range(4)]
    out = torch.empty((batch, 200, 6), device=dev)
    row(f"{name} n{batch} detection_output P {priors}, 21 classes, top_k 400 / 200, threshold 0.01",
        lambda loc, conf: detection_output(loc, conf, prior, 21, 0.45, 400, 200, 0.01, out=out), sets, max(iters // 10, 5), rounds)
    print(json.dumps({"what": f"{name} n{batch} detections per image", "counts": [int((o[:, 0] > 0).sum()) for o in out.cpu()][:4]}), flush=True)


def nets(batch, rounds):
    for name in ("mobilenet_ssd", "vgg16_ssd300"):
        p, b, i, o = model_zoo.MODELS[name]()
        x = np.random.default_rng(1).uniform(-1, 1, (batch, 3, 300, 300)).astype(np.float32)
        for level in (1, 2):
            net = Net(fusion=level, tuned=True)
            net.SetDetection(True)
            if name in model_zoo.DILATED_LAYERS:
                net.SetDilated(True)
            net.LoadParam(p)
            net.LoadWeights(b)
            net.FeedInput(i, x)
            net.Forward()
            net.synchronize()
            runs = [net.forward_timed() for _ in range(rounds)]
            per = {}
            for r in runs:
                tot = {"backbone": 0.0, "head": 0.0}
                for t, nm, a, ms in r:
                    key = "head" if a == "DETECT" or "_mbox_" in nm else "backbone"
                    tot[key] += ms
                    if key == "head":
                        tot["head " + t] = tot.get("head " + t, 0.0) + ms
                for k, v in tot.items():
                    per.setdefault(k, []).append(v)
            out = {"what": f"{name} n{batch} level {level}", "layers": len(runs[0]), "launching_head_layers": sum(1 for t, nm, a, _ in runs[0] if a == "DETECT" and t in ("Permute", "Concat", "Softmax", "Normalize", "DetectionOutput"))}
            out.update({k + "_ms": round(statistics.median(v), 4) for k, v in sorted(per.items())})
            print(json.dumps(out), flush=True)
            net.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batches", default="1,32")
    ap.add_argument("--no-nets", action="store_true")
    ap.add_argument("--no-kernels", action="store_true")
    args = ap.parse_args()
    for batch in [int(v) for v in args.batches.split(",")]:
        if not args.no_kernels:
            kernels("ssd300", SSD300, batch, args.iters, args.rounds)
            kernels("ssd512", SSD512, batch, args.iters, args.rounds)
        if not args.no_nets:
            nets(batch, args.rounds)
    print(json.dumps({"done": True}))


if __name__ == "__main__":
    main()
