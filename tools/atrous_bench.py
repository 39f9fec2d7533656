#!/usr/bin/env python
"""tools/atrous_bench.py [--batch N] [--iters I] [--nets] -- the dilated-convolution route on the DeepLab layer shapes.

Per layer: the selected route and every alternative fhip_atrous_forward_route accepts on the same tile shape (ROW4 against scalar, tap
skipping on against off), the same layer at dilation 1 with the same output size through fhip_conv_forward (equal FLOPs: what dilation
costs on the project's own main loop), and torch.nn.functional.conv2d(dilation=) on the same card.  The depthwise kernel is priced as a
fraction of a device-to-device copy of its bytes.  Timing: hip events around `iters` back-to-back launches after a warm-up; the candidates of a layer are alternated inside each of 7
repetitions, the figure is the median per launch and `spread` its min / max over the repetitions.  --nets adds the whole zoo nets (images/s at the given batch)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from feathercnn_amd import AtrousConv, AtrousLayer, AtrousParam, ConvLayer, ConvParam, model_zoo  # noqa: E402
from feathercnn_amd.net import Net  # noqa: E402

# name, C, K, plane, dilation, group, stride
LAYERS = [("conv5_d2_41", 512, 512, 41, 2, 1, 1), ("conv5_d2_40", 512, 512, 40, 2, 1, 1),
          ("fc6_d12_41", 512, 1024, 41, 12, 1, 1), ("fc6_d12_40", 512, 1024, 40, 12, 1, 1),
          ("aspp_d6_41", 512, 1024, 41, 6, 1, 1), ("aspp_d18_41", 512, 1024, 41, 18, 1, 1), ("aspp_d24_41", 512, 1024, 41, 24, 1, 1),
          ("aspp_d24_40", 512, 1024, 40, 24, 1, 1), ("fc6_d12_28", 512, 1024, 28, 12, 1, 1),
          ("dw_d2_32_c960", 960, 960, 32, 2, 960, 1), ("dw_d2_33_c960", 960, 960, 33, 2, 960, 1), ("dw_d2_s2_64_c576", 576, 576, 64, 2, 576, 2)]


def timed_all(fns, iters, reps=7):
    """{name: fn} -> {name: (median, min, max)} in microseconds per launch.  The candidates are ALTERNATED inside every repetition (a, b, c,
    a, b, c, ...), so clock and thermal drift hits them alike; min / max over the repetitions is the spread a difference has to exceed."""
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    got = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                fn()
            b.record()
            torch.cuda.synchronize()
            got[k].append(a.elapsed_time(b) * 1e3 / iters)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in got.items()}


def timed(fn, iters):
    return timed_all({"x": fn}, iters, 5)["x"][0]


def variants(route):
    """The route and its ROW4 / tap-skipping alternatives on the same tile shape."""
    if "AtrousGemmPolicy" not in route:
        return [route]
    head = route.split("fhip::AtrousGemmPolicy<")[0]
    return [f"{head}fhip::AtrousGemmPolicy<{r}, {s}> >" for r in ("true", "false") for s in ("true", "false")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--nets", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(1)
    for name, c, k, hw, d, group, s in LAYERS:
        p = AtrousParam.make(c, k, hw, 3, s, d, group=group, batch=args.batch)
        x = torch.from_numpy(rng.uniform(-1, 1, (args.batch, c, hw, hw)).astype(np.float32)).to(dev)
        w = torch.from_numpy((rng.uniform(-1, 1, (k, c // group, 3, 3)) / np.sqrt(9 * c / group)).astype(np.float32)).to(dev)
        b = torch.from_numpy(rng.uniform(-.1, .1, (k,)).astype(np.float32)).to(dev)
        sel = AtrousConv().Route(p)
        flops = 2.0 * args.batch * k * p.output_h * p.output_w * (c // group) * 9
        row = {"layer": name, "batch": args.batch, "selected": sel, "gflop": flops / 1e9, "us": {}}
        out = torch.empty((args.batch, k, p.output_h, p.output_w), device=dev)
        fns = {}
        for route in variants(sel):
            try:
                layer = AtrousLayer(p, w, b, route=route)
            except Exception:
                continue  # a form this layer cannot take (ROW4 on a 41-pixel plane)
            fns[route] = (lambda layer=layer: layer.Forward(x, out=out))
        fns["torch conv2d(dilation)"] = lambda: torch.nn.functional.conv2d(x, w, b, stride=s, padding=d, dilation=d, groups=group).relu_()
        # the same layer at dilation 1 and the same output size through the main library, output and scratch allocated once
        q = ConvParam(output_channels=k, input_channels=c, input_h=hw, input_w=hw, kernel_h=3, kernel_w=3, stride_h=s, stride_w=s, pad_left=1, pad_right=1,
                      pad_top=1, pad_bottom=1, group=group, bias_term=True, activation=1, batch=args.batch)
        plain = ConvLayer(q, w, b)
        pout = torch.empty(plain.out_shape(), device=dev)
        pscr = torch.empty(max(plain.buffer_bytes // 4, 1), device=dev)
        fns[f"fhip_conv_forward d1 (algo {plain.booster.algo})"] = lambda: plain.Forward(x, out=pout, scratch=pscr)
        res = timed_all(fns, args.iters)
        row["us"] = {k_: round(v[0], 2) for k_, v in res.items()}
        row["spread"] = {k_: [round(v[1], 2), round(v[2], 2)] for k_, v in res.items()}
        row["tflops_selected"] = flops / row["us"][sel] / 1e6
        m = (k + 127) // 128
        row["tiles"] = m * ((args.batch * p.output_h * p.output_w + 63) // 64) if "AtrousGemmPolicy" in sel else None
        if group > 1:
            y = torch.empty_like(out)
            nbytes = x.numel() * 4 + out.numel() * 4
            cp = timed(lambda: y.copy_(out), args.iters) * (nbytes / (2.0 * out.numel() * 4))  # a d2d copy moving the layer's bytes
            row["copy_us_for_same_bytes"] = cp
            row["fraction_of_copy_rate"] = cp / row["us"][sel]
        print(json.dumps(row), flush=True)
    if args.nets:
        for name in ("deeplab_largefov", "deeplab_v2_aspp"):
            pm, bn, i, o = model_zoo.MODELS[name]()
            net = Net(fusion=3, tuned=True, graph=True)
            net.SetDilated(True)
            net.LoadParam(pm)
            net.LoadWeights(bn)
            x = rng.uniform(-1, 1, (args.batch, 3, 321, 321)).astype(np.float32)
            xd = torch.from_numpy(x).to(dev)

            def step():
                net.FeedInput(i, xd)
                net.Forward()
            us = timed(step, 5)
            print(json.dumps({"net": name, "batch": args.batch, "ms": us / 1e3, "images_per_s": args.batch / (us / 1e6)}), flush=True)
            net.close()


if __name__ == "__main__":
    main()
