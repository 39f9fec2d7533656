"""Measure the transposed-convolution route (fhip_deconv_forward, libfeather_deconv.so) on the up-sampling layers of pix2pix / U-Net
decoders, a style-transfer net and an FCN head.  A measurement tool, not a test.

For each shape three things are timed in one process, interleaved round by round:
  baseline  what the library offered before this route: a zero-stuffing copy (the input written into a zeroed tensor with stride - 1
            zeros between pixels and kernel - 1 - pad zeros around it; the zeros are written once, outside the timing) plus the existing
            ConvLayer (tuned selection) on the stuffed tensor with the spatially flipped kernel.  Group 1 only;
  new       fhip_deconv_forward;
  gemm 1x1  a 1x1 convolution with the same multiply-accumulate count on the same output plane (C * taps-per-phase input channels ->
            K), i.e. what the shared main loop of gemm_core.h reaches without a gather and with 16-byte stores (group 1 only).
Each timing is `--inner` launches between two events (so launch overhead is shared the way a net shares it), `--reps` timings per way after
a warm-up, median with min / max.  Reported: time per launch, the algorithmic rate 2 K C kh kw H W N / time as a fraction of the fp32
MFMA peak, and the outputs of baseline and new are compared once (<= 1e-4 normalised).

    python tools/deconv_bench.py [--batch 16] [--reps 15] [--inner 10]
Prints one JSON object.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_TF = 157.3  # fp32 MFMA peak of the MI355X
# C, K, H, kernel, stride, pad, output pad, group
SHAPES = [(512, 256, 16, 4, 2, 1, 0, 1), (256, 128, 32, 4, 2, 1, 0, 1), (128, 64, 64, 4, 2, 1, 0, 1), (64, 3, 128, 4, 2, 1, 0, 1),
          (256, 128, 32, 2, 2, 0, 0, 1), (128, 64, 64, 2, 2, 0, 0, 1),
          (128, 64, 64, 3, 2, 1, 1, 1), (64, 32, 128, 3, 2, 1, 1, 1),
          (21, 21, 64, 4, 2, 1, 0, 21)]


def timed(fn, inner):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def shape_rows(c, k, h, ks, s, p, op, group, batch, reps, inner):
    import torch

    from feathercnn_amd import ALGO_NAMES, ConvLayer, ConvParam, DeconvLayer, DeconvParam
    gen = torch.Generator(device="cuda").manual_seed(c + k + h)
    cg = c // group
    w = (torch.rand((k, cg, ks, ks), device="cuda", generator=gen) * 2 - 1) / (cg * (-(-ks // s)) ** 2) ** 0.5
    bias = torch.rand((k,), device="cuda", generator=gen) * 0.2 - 0.1
    x = torch.rand((batch, c, h, h), device="cuda", generator=gen) * 2 - 1
    pd = DeconvParam.make(c, k, h, ks, s, p, op, group=group, batch=batch)
    new = DeconvLayer(pd, w, bias)
    ho = pd.output_h
    y_new = torch.empty((batch, k, ho, ho), device="cuda")
    ways = {"new: fhip_deconv_forward [" + new.deconv.Route(pd).replace("fhip::", "") + "]": lambda: new.Forward(x, out=y_new)}
    err = None
    if group == 1:
        e = ks - 1 - p
        hs = (h - 1) * s + 1 + 2 * e + op
        stuffed = torch.zeros((batch, c, hs, hs), device="cuda")
        view = stuffed[:, :, e:e + (h - 1) * s + 1:s, e:e + (h - 1) * s + 1:s]
        pb = ConvParam.make(c, k, hs, ks, 1, 0, batch=batch)
        base = ConvLayer(pb, w.flip(2, 3).contiguous(), bias, tuned=True)
        assert pb.output_h == ho
        y_base = torch.empty((batch, k, ho, ho), device="cuda")
        scratch = torch.empty(max(base.buffer_bytes // 4, 1), device="cuda")

        def baseline():
            view.copy_(x)
            base.Forward(stuffed, out=y_base, scratch=scratch)
        ways["baseline: zero-stuffing copy + ConvLayer " + ALGO_NAMES[base.booster.algo]] = baseline
        taps = ks * ks / (s * s)
        c1 = max(16, int(round(c * taps / 16)) * 16)
        p1 = ConvParam.make(c1, k, ho, 1, 1, 0, batch=batch)
        w1 = (torch.rand((k, c1, 1, 1), device="cuda", generator=gen) * 2 - 1) / c1 ** 0.5
        g1 = ConvLayer(p1, w1, bias, tuned=True)
        x1 = torch.rand((batch, c1, ho, ho), device="cuda", generator=gen)
        y1 = torch.empty((batch, k, ho, ho), device="cuda")
        s1 = torch.empty(max(g1.buffer_bytes // 4, 1), device="cuda")
        ways[f"gemm 1x1: {c1} -> {k} @ {ho}, ConvLayer " + ALGO_NAMES[g1.booster.algo]] = lambda: g1.Forward(x1, out=y1, scratch=s1)
        new.Forward(x, out=y_new)
        baseline()
        err = float((y_new - y_base).abs().max() / y_base.abs().max())
        assert err <= 1e-4, f"the two ways disagree: {err}"
    times = {n: [] for n in ways}
    for _ in range(3):
        for n, fn in ways.items():
            timed(fn, inner)
    for _ in range(reps):
        for n, fn in ways.items():
            times[n].append(timed(fn, inner))
    flops = 2.0 * k * cg * ks * ks * h * h * batch
    rows = []
    for n, t in times.items():
        med = statistics.median(t)
        rows.append({"shape": f"{c} -> {k} @ {h}, k{ks} s{s} p{p} op{op}, group {group}, batch {batch}", "way": n, "median_us": round(med * 1e3, 1),
                     "min_us": round(min(t) * 1e3, 1), "max_us": round(max(t) * 1e3, 1), "algorithmic_TFLOPs": round(flops / med / 1e9, 2),
                     "fraction_of_fp32_mfma_peak": round(flops / med / 1e9 / PEAK_TF, 3)})
    if group == 1:
        rows[0]["speedup_over_baseline"] = round(rows[1]["median_us"] / rows[0]["median_us"], 2)
        rows[0]["ranges_disjoint"] = rows[0]["max_us"] < rows[1]["min_us"]
        rows[0]["normalised_difference_of_the_two_ways"] = err
    torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=10)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("deconv_bench.py needs a GPU: nothing is measured without one")
    out = {"device": torch.cuda.get_device_name(0), "fp32_mfma_peak_TFLOPs": PEAK_TF, "rows": []}
    for shape in SHAPES:
        out["rows"] += shape_rows(*shape, a.batch, a.reps, a.inner)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
