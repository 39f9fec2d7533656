#!/usr/bin/env python3
"""tools/gate_bench.py [--iters N] [--blocks] -- the kernels of libfeather_gate.so on the squeeze-and-excitation shapes of SE-ResNet-50
(batch 64) and EfficientNet-B0 (batch 256), each against its yardstick in the same process on the same tensors, the candidates
alternating, best of three rounds:
  squeeze  against fhip_pooling (global, average) of libfeather_hip.so -- the kernel the Net runs at fusion levels 0 and 1; bytes = the
           tensor once, as a fraction of the HBM rate benchkit/roofs.py uses;
  apply    out = max(x * g + r, 0): three tensor-sized passes, the same fraction; against the multiply followed by fhip_add (five passes);
  excite   one block per image against 2 / 4 / 8 slices of the output channels, in microseconds.
Cold: a ring of tensors of more than 256 MiB (the Infinity Cache) in all, walked in order.  Times are device events around an eager loop
of launches (bounded below by the host's cost per enqueue: a row near 8 us measures the enqueue, not the kernel).
--blocks adds one residual SE block as a net (Split, Pooling, InnerProduct, ReLU, InnerProduct, Sigmoid, Scale, Eltwise, ReLU) at fusion
level 0 against level 2, both replayed from their graphs, alternating (host clock between device-wide synchronisations: a net runs on
a stream of its own).  Prints table rows and one JSON line at the end."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from benchkit import PEAK_HBM_GBS  # noqa: E402
from feathercnn_amd import _lib, channel_gate, excite, model_zoo, squeeze  # noqa: E402
from feathercnn_amd.gate import gate_route  # noqa: E402
from feathercnn_amd.net import Net, add, pool_param  # noqa: E402

# (label, batch, C, plane, R)
SHAPES = [("se-r50 256x56^2", 64, 256, 56, 16), ("se-r50 512x28^2", 64, 512, 28, 32), ("se-r50 1024x14^2", 64, 1024, 14, 64),
          ("se-r50 2048x7^2", 64, 2048, 7, 128), ("eff-b0 144x28^2", 256, 144, 28, 6), ("eff-b0 480x14^2", 256, 480, 14, 20),
          ("eff-b0 1152x7^2", 256, 1152, 7, 48)]
L3 = 256 << 20


def ring_of(shape, tensors=1):
    elems = int(np.prod(shape))
    ring = max(2, -(-(L3 + (L3 >> 2)) // (elems * 4 * tensors)))
    return [tuple(torch.randn(shape, device="cuda") for _ in range(tensors)) for _ in range(ring)]


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


def block_net(c, plane, r, level, x, short):
    g = model_zoo.GraphBuilder(3)
    a = g.input("x", c, plane, plane)
    s = g.input("short", c, plane, plane)
    g.relu("out", g.eltwise("sum", s, g.se_block("se", a, c, r, "caffe")))
    p, w = g.finish()
    net = Net(fusion=level, graph=True)
    net.LoadParam(p)
    net.LoadWeights(w)
    net.FeedInput("x", x)
    net.FeedInput("short", short)
    for _ in range(3):
        net.Forward()
    return net


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--blocks", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gate_bench needs a GPU")
    lib = _lib.load_library()
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rows = []
    for label, n, c, plane, r in SHAPES:
        shape = (n, c, plane, plane)
        nbytes = n * c * plane * plane * 4
        mean, gate = torch.empty((n, c, 1, 1), device="cuda"), torch.rand((n, c, 1, 1), device="cuda")
        q = pool_param(c, plane, plane, plane, 1, pooling_type=1, global_pooling=True)

        def sq_ours(x):
            squeeze(x, out=mean)

        def sq_pool(x):
            lib.fhip_pooling(ctypes.byref(q), n, ctypes.c_void_p(mean.data_ptr()), ctypes.c_void_p(x.data_ptr()), stream())

        sets = ring_of(shape)
        sq = best_of((("ours", sq_ours), ("pooling", sq_pool)), sets, args.iters)
        del sets
        torch.cuda.empty_cache()

        def ap_fused(x, res, y):
            channel_gate(x, gate, res, relu=True, out=y)

        def ap_two(x, res, y):
            channel_gate(x, gate, out=y)
            lib.fhip_add(ctypes.c_void_p(y.data_ptr()), ctypes.c_void_p(y.data_ptr()), ctypes.c_void_p(res.data_ptr()), y.numel(), 1, stream())

        sets = ring_of(shape, 3)
        apl = best_of((("fused", ap_fused), ("mul+add", ap_two)), sets, max(args.iters // 2, 10))
        route = gate_route("squeeze", sets[0][0]).replace("fhip::", "")
        del sets
        torch.cuda.empty_cache()

        w1, w2 = torch.randn((r, c), device="cuda") / c ** 0.5, torch.randn((c, r), device="cuda") / r ** 0.5
        b1, b2 = torch.randn(r, device="cuda"), torch.randn(c, device="cuda")
        mset = [(torch.randn((n, c, 1, 1), device="cuda"),)]
        ex = best_of([(f"slices{s}", (lambda m, s=s: excite(m, w1, b1, w2, b2, "relu", "sigmoid", out=gate, slices=s))) for s in (1, 2, 4, 8)], mset, args.iters)
        row = {"shape": label, "batch": n, "tensor_MB": nbytes / 1e6, "squeeze_route": route, "squeeze_us": sq,
               "squeeze_frac_hbm": nbytes / sq["ours"] / 1e3 / PEAK_HBM_GBS, "pooling_frac_hbm": nbytes / sq["pooling"] / 1e3 / PEAK_HBM_GBS,
               "apply_us": apl, "apply_frac_hbm": 3 * nbytes / apl["fused"] / 1e3 / PEAK_HBM_GBS, "excite_us": ex}
        if args.blocks:
            x, short = torch.randn(shape, device="cuda"), torch.randn(shape, device="cuda")
            nets = {lv: block_net(c, plane, r, lv, x, short) for lv in (0, 2)}
            blk = best_of([(f"level{lv}", (lambda lv=lv: nets[lv].Forward())) for lv in (0, 2)], [()], args.iters, timed=timed_wall)
            row["block_us"] = blk
            row["block_ratio_level2_over_level0"] = blk["level2"] / blk["level0"]
            row["block_layers"] = {lv: len(nets[lv].layers()) for lv in nets}
            for net in nets.values():
                net.close()
        print(json.dumps(row), flush=True)
        rows.append(row)
        torch.cuda.empty_cache()
    print(json.dumps({"gate_bench": rows, "peak_hbm_gbs": PEAK_HBM_GBS}))


if __name__ == "__main__":
    main()
