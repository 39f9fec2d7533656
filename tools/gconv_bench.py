"""Measure the grouped-convolution route (fhip_gconv_forward, libfeather_gconv.so) on ResNeXt-50 (32x4d)'s grouped 3x3 layers.  A
measurement tool, not a test.

For each of the seven shapes (128 ch @ 56, 256 @ 28, 512 @ 14, 1024 @ 7 at stride 1; 256 @ 56, 512 @ 28, 1024 @ 14 at stride 2; 32 groups)
two ways to run the layer are timed in one process, alternating call by call:
  baseline  what the library offered before this route: the same layer as a dense group == 1 convolution whose weights are the
            block-diagonal expansion, through fhip_conv_forward on the route fhip_conv_select_algo picks;
  new       fhip_gconv_forward.
Every pair is timed twice: "resident" re-runs one input / output pair, "cold" rotates through enough pairs to exceed 1 GiB (four times
the 256 MiB Infinity Cache), so every call streams from HBM.  Torch events around each call, medians with min / max over --reps after a
warm-up.  Reported per row: time, executed FLOPs over algorithmic FLOPs (2 K (C/group) Ho Wo kh kw N), and the fraction of the HBM roof
reached on the compulsory bytes 4 (C H W + K Ho Wo) N.  The outputs of the two ways are compared once (<= 1e-4 normalised).

    python tools/gconv_bench.py [--batch 64] [--reps 30]
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

SHAPES = [(128, 56, 1), (256, 28, 1), (512, 14, 1), (1024, 7, 1), (256, 56, 2), (512, 28, 2), (1024, 14, 2)]
GROUP = 32


class Way:
    def __init__(self, name, layer, xs, ys, flops_ratio):
        self.name, self.layer, self.xs, self.ys, self.flops_ratio, self.times, self.turn = name, layer, xs, ys, flops_ratio, [], 0

    def run(self, record=True):
        import torch
        k = self.turn % len(self.xs)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        self.layer.Forward(self.xs[k], out=self.ys[k])
        b.record()
        b.synchronize()
        self.turn += 1
        if record:
            self.times.append(a.elapsed_time(b))


def shape_rows(c, size, stride, batch, reps, cold, hbm_gbs):
    import torch

    from feathercnn_amd import ALGO_NAMES, ConvLayer, ConvParam, GroupedConvLayer
    cg = c // GROUP
    pg = ConvParam.make(c, c, size, 3, stride, 1, group=GROUP, batch=batch)
    pd = ConvParam.make(c, c, size, 3, stride, 1, group=1, batch=batch)
    gen = torch.Generator(device="cuda").manual_seed(c + size)
    w = (torch.rand((c, cg, 3, 3), device="cuda", generator=gen) * 2 - 1) / (cg * 9) ** 0.5
    bias = torch.rand((c,), device="cuda", generator=gen) * 0.2 - 0.1
    dense = torch.zeros((c, c, 3, 3), device="cuda")
    for g in range(GROUP):
        dense[g * cg:(g + 1) * cg, g * cg:(g + 1) * cg] = w[g * cg:(g + 1) * cg]
    new, base = GroupedConvLayer(pg, w, bias), ConvLayer(pd, dense, bias)
    ho = pg.output_h
    nbytes = 4 * (c * size * size + c * ho * ho) * batch
    sets = max(2, -(-(1 << 30) // nbytes)) if cold else 1
    xs = [torch.rand((batch, c, size, size), device="cuda", generator=gen) * 2 - 1 for _ in range(sets)]
    ys = [torch.empty((batch, c, ho, ho), device="cuda") for _ in range(sets)]
    scratch = torch.empty(max(base.buffer_bytes // 4, 1), device="cuda")
    base_forward = base.Forward
    base.Forward = lambda x, out=None: base_forward(x, out=out, scratch=scratch)
    # one comparison of the two ways on the same input
    ya, yb = new.Forward(xs[0]).clone(), base.Forward(xs[0], out=ys[0]).clone()
    err = float((ya - yb).abs().max() / yb.abs().max())
    assert err <= 1e-4, f"the two ways disagree: {err}"
    ways = [Way("baseline: dense block-diagonal, " + ALGO_NAMES[base.booster.algo], base, xs, ys, float(GROUP)), Way("new: fhip_gconv_forward", new, xs, ys, 1.0)]
    for _ in range(3 * sets):
        for wy in ways:
            wy.run(record=False)
    for _ in range(reps):
        for wy in ways:
            wy.run()
    flops = 2.0 * c * cg * ho * ho * 9 * batch
    rows = []
    for wy in ways:
        med = statistics.median(wy.times)
        rows.append({"shape": f"{c} ch @ {size}, stride {stride}, group {GROUP}, batch {batch}", "buffers": "cold" if cold else "resident",
                     "way": wy.name, "median_us": round(med * 1e3, 1), "min_us": round(min(wy.times) * 1e3, 1),
                     "max_us": round(max(wy.times) * 1e3, 1), "executed_over_algorithmic_flops": wy.flops_ratio,
                     "algorithmic_TFLOPs": round(flops / med / 1e9, 2), "compulsory_bytes": nbytes,
                     "fraction_of_hbm_roof": round(nbytes / med / 1e6 / hbm_gbs, 3)})
    rows[1]["speedup_over_baseline"] = round(rows[0]["median_us"] / rows[1]["median_us"], 2)
    rows[1]["ranges_disjoint"] = rows[1]["max_us"] < rows[0]["min_us"]
    rows[1]["normalised_difference_of_the_two_ways"] = err
    del ways, xs, ys, new, base, scratch
    torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("gconv_bench.py needs a GPU: nothing is measured without one")
    from benchkit import PEAK_HBM_GBS
    out = {"device": torch.cuda.get_device_name(0), "hbm_roof_GBps": PEAK_HBM_GBS, "rows": []}
    for c, size, stride in SHAPES:
        for cold in (False, True):
            out["rows"] += shape_rows(c, size, stride, a.batch, a.reps, cold, PEAK_HBM_GBS)
    out["every_range_disjoint"] = all(r.get("ranges_disjoint", True) for r in out["rows"])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
