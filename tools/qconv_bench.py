#!/usr/bin/env python3
"""tools/qconv_bench.py [--iters N] [--rounds R] [--families vgg16,resnet50,mobilenet_v1] [--nets] [--steps S] -- the kernels of
libfeather_qconv.so on the layers of the nets they are for, against the fp32 route of the same geometry.

Per layer: VGG-16's 3x3 layers at batch 32, ResNet-50's first layer and its 1x1 and 3x3 layers at batch 64, MobileNet-V1's depthwise and pointwise layers at
batch 256.  In one process, the two candidates alternating round by round:
  int8    fhip_qconv_forward (bias + ReLU), the route fhip_qconv_route names
  q8      fhip_q8_forward of libfeather_q8.so, the chain form of the same layer: an int8 tensor in and a requantised int8 tensor out (a
          C = 3 first layer: fp32 in, int8 out), bias + ReLU, on its own ring of int8 tensor sets of more than 256 MiB
  fp32    fhip_conv_forward on the route fhip_conv_select_algo_tuned picks for the geometry (bias + ReLU), with its scratch buffer
Reported per layer: the median over the rounds in microseconds with the least and the largest round; int8 / fp32; the int8 route's achieved
TOPS (2 * N * K * OH * OW * R operations over the median) and that as a fraction of the matrix pipe's int8 peak -- 2x the dense bf16 peak of
~2.5 PF that MI355X_MICROARCH's rate table states, i.e. 5000 TOPS; the depthwise and the generic route do not run on that pipe, the column
says so by being tiny --; the bytes a perfect kernel moves (fp32 input read once, fp32 output written once, packed int8 weights read once)
and the GB/s of that over the median.
Cold: every candidate walks a ring of tensor sets of more than 256 MiB (the Infinity Cache) in all, in order.  Times are device events
around an eager loop of launches.  No figure here is a pass / fail bound of any test: the route is chosen by the model file, not by a
selector, so a slower layer is a finding.
--nets adds vgg16:32, resnet50:64 and mobilenet_v1:256 against their _int8 builds at fusion level 1 (the only level where both run the same
set of launches) and, at fusion level 2, the _int8 build against its _int8_rq build (int8 activations between the int8 layers), hipGraph
replay, the nets alternating.  Prints one JSON line per layer and net, and one at the end."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from benchkit import PEAK_HBM_GBS  # noqa: E402
from feathercnn_amd import ConvLayer, ConvParam, Q8Conv, Q8Param, QuantConv, QuantParam, ReLU, dequant_scales, model_zoo, q8_route, qconv_route  # noqa: E402
from feathercnn_amd.q8 import q8_shape  # noqa: E402
from feathercnn_amd.booster import ALGO_NAMES  # noqa: E402
from feathercnn_amd.net import Net  # noqa: E402

PEAK_I8_TOPS = 5000.0  # 2 x the ~2.5 PF dense bf16 peak (MI355X_MICROARCH.md, matrix-core rate table: I8 = 2x BF16 per clock)
L3 = 256 << 20

# (label, C, K, plane, kernel, stride, group)
LAYERS = {
    "vgg16": (32, [("conv1_1", 3, 64, 224, 3, 1, 1), ("conv1_2", 64, 64, 224, 3, 1, 1), ("conv2_1", 64, 128, 112, 3, 1, 1),
                   ("conv2_2", 128, 128, 112, 3, 1, 1), ("conv3_1", 128, 256, 56, 3, 1, 1), ("conv3_2", 256, 256, 56, 3, 1, 1),
                   ("conv4_1", 256, 512, 28, 3, 1, 1), ("conv4_2", 512, 512, 28, 3, 1, 1), ("conv5_1", 512, 512, 14, 3, 1, 1)]),
    "resnet50": (64, [("conv1 7x7 s2", 3, 64, 224, 7, 2, 1), ("res2 1x1 64-64", 64, 64, 56, 1, 1, 1), ("res2 3x3 64", 64, 64, 56, 3, 1, 1), ("res2 1x1 64-256", 64, 256, 56, 1, 1, 1),
                      ("res2 1x1 256-64", 256, 64, 56, 1, 1, 1), ("res3 3x3 128", 128, 128, 28, 3, 1, 1), ("res3 1x1 128-512", 128, 512, 28, 1, 1, 1),
                      ("res3 1x1 512-128", 512, 128, 28, 1, 1, 1), ("res4 3x3 256", 256, 256, 14, 3, 1, 1), ("res4 1x1 256-1024", 256, 1024, 14, 1, 1, 1),
                      ("res4 1x1 1024-256", 1024, 256, 14, 1, 1, 1), ("res5 3x3 512", 512, 512, 7, 3, 1, 1), ("res5 1x1 512-2048", 512, 2048, 7, 1, 1, 1),
                      ("res5 1x1 2048-512", 2048, 512, 7, 1, 1, 1)]),
    "mobilenet_v1": (256, [("dw 32@112 s1", 32, 32, 112, 3, 1, 32), ("dw 64@112 s2", 64, 64, 112, 3, 2, 64), ("dw 128@56 s1", 128, 128, 56, 3, 1, 128),
                           ("dw 256@28 s1", 256, 256, 28, 3, 1, 256), ("dw 512@14 s1", 512, 512, 14, 3, 1, 512), ("dw 512@14 s2", 512, 512, 14, 3, 2, 512),
                           ("dw 1024@7 s1", 1024, 1024, 7, 3, 1, 1024), ("pw 32-64@112", 32, 64, 112, 1, 1, 1), ("pw 64-128@56", 64, 128, 56, 1, 1, 1),
                           ("pw 128-256@28", 128, 256, 28, 1, 1, 1), ("pw 256-512@14", 256, 512, 14, 1, 1, 1), ("pw 512-512@14", 512, 512, 14, 1, 1, 1),
                           ("pw 1024-1024@7", 1024, 1024, 7, 1, 1, 1)]),
}


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


def layer_row(family, batch, spec, iters, rounds):
    label, c, k, plane, kernel, stride, group = spec
    pad = kernel // 2
    rng = np.random.default_rng(len(label))
    qp = QuantParam.make(c, k, plane, kernel, stride, pad, group=group, bias=True, act=ReLU, batch=batch)
    fp = ConvParam(output_channels=k, input_channels=c, input_h=plane, input_w=plane, kernel_h=kernel, kernel_w=kernel, stride_h=stride, stride_w=stride,
                   pad_left=pad, pad_right=pad, pad_top=pad, pad_bottom=pad, group=group, bias_term=True, activation=ReLU, batch=batch)
    w = torch.from_numpy((rng.standard_normal((k, c // group, kernel, kernel)) * np.sqrt(2.0 / (c // group * kernel * kernel))).astype(np.float32)).cuda()
    bias = torch.from_numpy(rng.uniform(-0.1, 0.1, k).astype(np.float32)).cuda()
    flayer = ConvLayer(fp, w, bias, tuned=True)
    scratch = torch.empty(max(flayer.buffer_bytes // 4, 1), dtype=torch.float32, device="cuda")
    # the int8 layer: per-channel weight scales 127 / absmax, an input scale that puts N(0, 1) inputs at +-4 sigma on +-127
    wq, s_w = model_zoo.quantize_weights(w.cpu().numpy(), k)
    s_in = 127.0 / 4.0
    d = torch.from_numpy(dequant_scales(s_w, s_in)).cuda()
    conv = QuantConv()
    _, packed_bytes = conv.GetBufferSize(qp)
    packed = torch.empty(packed_bytes, dtype=torch.uint8, device="cuda")
    conv.Init(qp, packed, torch.from_numpy(wq.reshape(k, c // group, kernel, kernel)).cuda())
    in_shape, out_shape = (batch, c, plane, plane), (batch, k, qp.output_h, qp.output_w)
    per = (int(np.prod(in_shape)) + int(np.prod(out_shape))) * 4
    ring = max(2, -(-(L3 + (L3 >> 2)) // per))
    sets = [(torch.randn(in_shape, device="cuda"), torch.empty(out_shape, device="cuda")) for _ in range(ring)]
    # the chain form: int8 in (but for a first layer), int8 out at an output scale that keeps the ReLU'd values inside the q range
    in8 = c % 16 == 0 or group > 1
    cp = Q8Param.make(c, k, plane, kernel, stride, pad, group=group, bias=True, act=ReLU, batch=batch, input_int8=in8, output_int8=True)
    chain = Q8Conv()
    _, cpacked_bytes = chain.GetBufferSize(cp)
    cpacked = torch.empty(cpacked_bytes, dtype=torch.uint8, device="cuda")
    chain.Init(cp, cpacked, torch.from_numpy(wq.reshape(k, c // group, kernel, kernel)).cuda())
    cin_shape, cout_shape = (q8_shape(*in_shape) if in8 else in_shape), q8_shape(*out_shape)
    cper = int(np.prod(cin_shape)) * (1 if in8 else 4) + int(np.prod(cout_shape))
    cring = max(2, -(-(L3 + (L3 >> 2)) // cper))
    csets = [((torch.randint(-127, 128, cin_shape, dtype=torch.int8, device="cuda") if in8 else torch.randn(in_shape, device="cuda")),
              torch.empty(cout_shape, dtype=torch.int8, device="cuda")) for _ in range(cring)]
    cands = [("int8", lambda x, y: conv.Forward(qp, y, x, packed, d, bias, s_in), sets), ("q8", lambda x, y: chain.Forward(cp, y, x, cpacked, d, bias, s_in, 16.0), csets),
             ("fp32", lambda x, y: flayer.Forward(x, out=y, scratch=scratch), sets)]
    t = {nm: [] for nm, _, _ in cands}
    for _ in range(rounds):
        for nm, fn, ring_sets in cands:
            t[nm].append(timed(fn, ring_sets, iters))
    med = {nm: statistics.median(v) for nm, v in t.items()}
    # the two routes agree to the quantisation step (a sanity check of the set-up, not a test)
    x, y = sets[0]
    conv.Forward(qp, y, x, packed, d, bias, s_in)
    ref = flayer.Forward(x, scratch=scratch)
    rel = float((y - ref).abs().max() / ref.abs().max())
    ops = 2.0 * batch * k * qp.output_h * qp.output_w * (c // group) * kernel * kernel
    moved = per + packed_bytes
    row = {"family": family, "layer": label, "batch": batch, "route": qconv_route(qp).replace("fhip::", ""), "q8_route": q8_route(cp).replace("fhip::", ""),
           "q8_over_int8": round(med["q8"] / med["int8"], 3), "q8_over_fp32": round(med["q8"] / med["fp32"], 3), "q8_tops": round(ops / med["q8"] / 1e6, 1),
           "q8_of_i8_peak": round(ops / med["q8"] / 1e6 / PEAK_I8_TOPS, 4), "q8_MB_moved": round((cper + cpacked_bytes) / 1e6, 1),
           "q8_gbs": round((cper + cpacked_bytes) / med["q8"] / 1e3), "fp32_route": ALGO_NAMES.get(flayer.booster.algo, str(flayer.booster.algo)),
           "us": {nm: [round(med[nm], 1), round(min(v), 1), round(max(v), 1)] for nm, v in t.items()}, "int8_over_fp32": round(med["int8"] / med["fp32"], 3),
           "int8_tops": round(ops / med["int8"] / 1e6, 1), "of_i8_peak": round(ops / med["int8"] / 1e6 / PEAK_I8_TOPS, 4),
           "MB_moved": round(moved / 1e6, 1), "int8_gbs": round(moved / med["int8"] / 1e3), "max_rel_diff_to_fp32": round(rel, 4)}
    print(json.dumps(row), flush=True)
    del sets, csets, x, y, ref
    torch.cuda.empty_cache()
    return row


def net_row(name, batch, steps, rounds):
    nets = {}
    # the requantised build needs fusion level 2 (its BatchNorm layers exist only folded): it runs next to the int8 build at that level
    for which, build, level in (("fp32", model_zoo.MODELS[name], 1), ("int8", model_zoo.MODELS[name + "_int8"], 1),
                                ("int8_f2", model_zoo.MODELS[name + "_int8"], 2), ("int8_rq_f2", model_zoo.MODELS[name + "_int8_rq"], 2)):
        p, b, i, o = build()
        net = Net(fusion=level, graph=True, tuned=True)
        if which != "fp32":
            net.SetQuantized(True)
        if which == "int8_rq_f2":
            net.SetRequantized(True)
        net.LoadParam(p)
        net.LoadWeights(b)
        del b
        net.FeedInput(i, torch.rand((batch, 3, 224, 224), device="cuda") * 2 - 1)
        for _ in range(3):
            net.Forward()
        torch.cuda.synchronize()
        nets[which] = net
    t = {which: [] for which in nets}
    for _ in range(rounds):
        for which, net in nets.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                net.Forward()
            torch.cuda.synchronize()
            t[which].append((time.perf_counter() - t0) / steps * 1e3)
    med = {k: statistics.median(v) for k, v in t.items()}
    levels = {"fp32": 1, "int8": 1, "int8_f2": 2, "int8_rq_f2": 2}  # the fusion level of each column
    quantised = {k: sum(a == "QCONV" for _, _, a in net.layers()) for k, net in nets.items() if k != "fp32"}
    row = {"net": name, "batch": batch, "fusion": levels, "int8_layers": quantised, "ms": {k: [round(med[k], 3), round(min(v), 3), round(max(v), 3)] for k, v in t.items()},
           "img_s": {k: round(batch / med[k] * 1e3) for k in t}, "int8_over_fp32": round(med["int8"] / med["fp32"], 3),
           "rq_over_int8_f2": round(med["int8_rq_f2"] / med["int8_f2"], 3), "rq_over_fp32": round(med["int8_rq_f2"] / med["fp32"], 3)}
    print(json.dumps(row), flush=True)
    for net in nets.values():
        net.close()
    torch.cuda.empty_cache()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--families", default="vgg16,resnet50,mobilenet_v1")
    ap.add_argument("--nets", action="store_true")
    ap.add_argument("--steps", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("qconv_bench needs a GPU")
    rows, nets = [], []
    for family in [f for f in args.families.split(",") if f]:
        batch, specs = LAYERS[family]
        for spec in specs:
            rows.append(layer_row(family, batch, spec, args.iters, args.rounds))
    if args.nets:
        for name, batch in (("vgg16", 32), ("resnet50", 64), ("mobilenet_v1", 256)):
            nets.append(net_row(name, batch, args.steps, args.rounds))
    print(json.dumps({"qconv_bench": rows, "nets": nets, "peak_i8_tops": PEAK_I8_TOPS, "peak_hbm_gbs": PEAK_HBM_GBS}))


if __name__ == "__main__":
    main()
