#!/usr/bin/env python3
"""tools/conv1d_bench.py [--batch N] [--frames L] [--iters N] [--rounds R] -- the three convolution kernels of libfeather_conv1d.so on the
layer shapes of model_zoo.quartznet_5x5 (DESIGN.md 3.30 records the figures).

* the dense layers: the pointwise layers of the blocks and, beside them, three dense layers that are NOT in that net (its blocks are
  separable) but have its extents: 33 taps at stride 2, 3 taps, and 87 taps at dilation 2 -- each through fhip_conv1d_forward and, where the main library's general route can express the layer (no
  dilation, symmetric pads), the same layer through fhip_conv_forward(FHIP_IM2COL) on a [C][1][L] image, outputs compared;
* the depthwise layers of 33 .. 87 taps, with the bytes they must move (input once, output once) over the time.

Times are device events around a loop of calls on buffers allocated once, after a warm-up; microseconds per call, median and maximum of the
rounds.  GFLOP/s and GB/s are the operations and bytes the layer needs, computed here from its shape, over that time.  Every call reuses
the same buffers of a few megabytes, so they stay in the caches: the GB/s are no HBM bandwidth, and a round of 50 calls is a window of 1 to
8 ms (--iters lengthens it).  No figure is a
pass / fail bound of any test.  One JSON line per row."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from feathercnn_amd import IM2COL, ConvLayer, ConvParam, None_, conv1d  # noqa: E402
from tools.frame_bench import timed  # noqa: E402

# (what, C, K, kw, stride, dilation) at L frames (the first layer) or L / 2 (the others)
DENSE = (("first layer dense 64->256 k33 s2", 64, 256, 33, 2, 1), ("pointwise 256->256", 256, 256, 1, 1, 1), ("pointwise 256->512", 256, 512, 1, 1, 1),
         ("pointwise 512->512", 512, 512, 1, 1, 1), ("pointwise 512->1024", 512, 1024, 1, 1, 1), ("dense 256->256 k3", 256, 256, 3, 1, 1),
         ("dense 512->512 k87 d2", 512, 512, 87, 1, 2))
DEPTHWISE = ((256, 33, 1), (256, 39, 1), (512, 51, 1), (512, 63, 1), (512, 75, 1), (512, 87, 2))


def rounds_of(fn, iters, rounds):
    times = [timed(fn, [()], iters) for _ in range(rounds)]
    return round(statistics.median(times), 1), round(max(times), 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("conv1d_bench needs the GPU: nothing is measured without one")
    n = args.batch
    torch.manual_seed(0)
    for what, c, k, kw, s, d in DENSE:
        l = args.frames if s == 2 else args.frames // 2
        x = torch.rand((n, c, l), device="cuda") * 2 - 1
        w = (torch.rand((k, c, kw), device="cuda") * 2 - 1) / (c * kw) ** 0.5
        b = torch.rand((k,), device="cuda")
        left, right, lo = conv1d.conv1d_output_dim(l, kw, d, s, (kw - 1) * d // 2)  # symmetric, so that the general route can express it
        y = torch.empty((n, k, lo), device="cuda")
        run = lambda: conv1d.conv1d(x, w, b, s, d, left, right, out=y)
        us, us_max = rounds_of(run, args.iters, args.rounds)
        flops = 2.0 * n * k * lo * c * kw
        row = {"what": what, "n": n, "L": l, "Lo": lo, "kernel": conv1d.conv1d_route(c, k, kw, d, s), "us": us, "us_max": us_max, "GFLOPs": round(flops / us / 1e3, 1)}
        if d == 1 and left == right:
            p = ConvParam(output_channels=k, input_channels=c, input_h=1, input_w=l, kernel_h=1, kernel_w=kw, stride_h=1, stride_w=s, pad_left=left, pad_right=right, pad_top=0,
                          pad_bottom=0, group=1, bias_term=True, activation=None_, batch=n)
            layer = ConvLayer(p, w.reshape(k, c, 1, kw), b, algo=IM2COL)
            xi, yi = x.reshape(n, c, 1, l), torch.empty((n, k, 1, lo), device="cuda")
            scratch = torch.empty(max(layer.buffer_bytes // 4, 1), device="cuda")
            ius, ius_max = rounds_of(lambda: layer.Forward(xi, yi, scratch), args.iters, args.rounds)
            run()
            row.update({"im2col_us": ius, "im2col_us_max": ius_max, "im2col_over_conv1d": round(ius / us, 2),
                        "outputs_differ_by": float((yi.reshape(n, k, lo) - y).abs().max() / y.abs().max())})
        print(json.dumps(row), flush=True)
    for c, kw, d in DEPTHWISE:
        l = args.frames // 2
        x = torch.rand((n, c, l), device="cuda") * 2 - 1
        w = (torch.rand((c, 1, kw), device="cuda") * 2 - 1) / kw ** 0.5
        left, right, lo = conv1d.conv1d_output_dim(l, kw, d, 1, conv1d.SAME_UPPER)
        y = torch.empty((n, c, lo), device="cuda")
        us, us_max = rounds_of(lambda: conv1d.conv1d(x, w, None, 1, d, left, right, group=c, out=y), args.iters, args.rounds)
        print(json.dumps({"what": f"depthwise {c} k{kw} d{d}", "n": n, "L": l, "kernel": conv1d.conv1d_route(c, c, kw, d, 1, c), "us": us, "us_max": us_max,
                          "GB_per_s": round(4.0 * n * c * (l + lo) / us / 1e3, 1), "GFLOPs": round(2.0 * n * c * lo * kw / us / 1e3, 1)}), flush=True)
    print(json.dumps({"done": True}))


if __name__ == "__main__":
    main()
