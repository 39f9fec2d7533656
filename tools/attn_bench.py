#!/usr/bin/env python3
"""tools/attn_bench.py [--iters N] [--rounds R] [--no-nets] -- the transformer layers on the device (DESIGN.md 3.28 records the figures).

* The attention core of libfeather_attn.so at ViT-B / DeiT shapes: T = 197 and 577 tokens, d = 64, 12 heads (E = 768), batch 1 and 32, read in
  place from a fused [n * T][3E] projection buffer.  Next to the time: the bytes the call must move (q, k, v read once, the output written
  once) at the HBM peak the project uses (benchkit.PEAK_HBM_GBS), its FLOPs (4 n heads T^2 d: two products) at the fp32-MFMA rate the
  project's calibration entry measures in this process (fhip_calibrate_mfma_f32), and torch.nn.functional.scaled_dot_product_attention in
  fp32 on the same card -- an outside yardstick only: no ratio is promised or asserted anywhere.
* LayerNorm (197 n rows of 768) and GELU (197 n x 3072) against a plain hipMemcpyAsync device-to-device copy of the same bytes.
* deit_tiny_patch16_224 at fusion 1 and at fusion 2 (the residual adds run with their LayerNorms), rounds alternating.

Times are device events around an eager loop of calls; microseconds per call, median of the rounds.  No figure here is a pass / fail bound
of any test.  One JSON line per row."""
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
from feathercnn_amd import attn, booster, model_zoo  # noqa: E402
from feathercnn_amd.net import Net  # noqa: E402
from tools.frame_bench import device_copy, timed  # noqa: E402


def attention_rows(iters, rounds, mfma_tflops):
    for n in (1, 32):
        for t in (197, 577):
            heads, d = 12, 64
            e = heads * d
            count = 4 if n == 32 else 16
            sets = []
            for _ in range(count):
                qkv = torch.randn((n, t, 3 * e), device="cuda") * 0.35
                sets.append((qkv, torch.empty((n, t, e), device="cuda")))
            ours = lambda qkv, out: attn.attention(qkv[:, :, :e], qkv[:, :, e:2 * e], qkv[:, :, 2 * e:], heads, out=out)

            def sdpa(qkv, out):
                q, k, v = (qkv[:, :, j * e:(j + 1) * e].reshape(n, t, heads, d).transpose(1, 2) for j in range(3))
                return torch.nn.functional.scaled_dot_product_attention(q, k, v, scale=1.0)

            a, b = [], []
            for _ in range(rounds):
                a.append(timed(ours, sets, iters))
                b.append(timed(sdpa, sets, iters))
            got, ref = ours(*sets[0]), sdpa(*sets[0]).transpose(1, 2).reshape(n, t, e)
            us, tus = statistics.median(a), statistics.median(b)
            moved, flops = 4 * 4 * n * t * e, 4.0 * n * heads * t * t * d
            print(json.dumps({"what": f"attention n{n} T{t} d{d} heads{heads} [{attn.attn_route(attn.ATTENTION, e, heads)}]", "us": round(us, 2), "us_min": round(min(a), 2),
                              "us_max": round(max(a), 2), "MB": round(moved / 1e6, 2), "us_at_hbm_peak": round(moved / PEAK_HBM_GBS / 1e3, 2), "GFLOP": round(flops / 1e9, 3),
                              "TFLOPs": round(flops / us / 1e6, 2), "us_at_mfma_rate": round(flops / mfma_tflops / 1e6, 2), "frac_of_mfma_rate": round(flops / us / 1e6 / mfma_tflops, 3),
                              "torch_sdpa_fp32_us": round(tus, 2), "torch_over_ours": round(tus / us, 3), "max_abs_diff_to_torch": float((got - ref).abs().max())}), flush=True)


def elementwise_rows(iters, rounds):
    copy = device_copy()
    for n in (1, 32):
        for label, shape, fn in ((f"LayerNorm {197 * n} rows of 768", (197 * n, 768), None), (f"GELU {197 * n} x 3072", (197 * n, 3072), lambda o, x: attn.gelu(x, out=o)),
                                 (f"fast GELU {197 * n} x 3072", (197 * n, 3072), lambda o, x: attn.gelu(x, True, out=o))):
            if fn is None:
                gamma, beta = torch.rand(768, device="cuda") + 0.5, torch.rand(768, device="cuda")
                fn = lambda o, x: attn.layer_norm(x, gamma, beta, out=o)
            count = 4 if n == 32 else 16
            sets = [(torch.empty(shape, device="cuda"), torch.randn(shape, device="cuda")) for _ in range(count)]
            copies = [(torch.empty(shape, device="cuda"), torch.randn(shape, device="cuda")) for _ in range(count)]
            a, c = [], []
            for _ in range(rounds):
                a.append(timed(fn, sets, iters))
                c.append(timed(copy, copies, iters))
            us, cus = statistics.median(a), statistics.median(c)
            moved = 8 * int(np.prod(shape))
            print(json.dumps({"what": label, "us": round(us, 2), "us_min": round(min(a), 2), "us_max": round(max(a), 2), "MB": round(moved / 1e6, 2),
                              "GBps": round(moved / us / 1e3, 1), "copy_us": round(cus, 2), "vs_copy": round(cus / us, 3)}), flush=True)


def nets(iters, rounds, batch):
    built = {}
    p, b, i, o = model_zoo.deit_tiny_patch16_224()
    x = np.random.default_rng(0).uniform(-1, 1, (batch, 3, 224, 224)).astype(np.float32)
    for level in (1, 2):
        net = Net(fusion=level)
        net.SetTransformer()
        net.SetDetection(True)
        net.SetFrame()
        net.LoadParam(p)
        net.LoadWeights(b)
        net.FeedInput(i, x)
        for _ in range(3):
            net.Forward()
        torch.cuda.synchronize()
        built[level] = (net, net.Extract(o))
    times = {k: [] for k in built}
    for _ in range(rounds):
        for level, (net, _) in built.items():  # the nets alternate inside a round
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters):
                net.Forward()
            torch.cuda.synchronize()
            times[level].append((time.perf_counter() - t0) * 1e3 / iters)
    for level, (net, _) in built.items():
        t = times[level]
        print(json.dumps({"what": f"deit_tiny_patch16_224 fusion {level}, n{batch}", "layers": len(net.layers()), "ms": round(statistics.median(t), 4), "ms_min": round(min(t), 4),
                          "ms_max": round(max(t), 4)}), flush=True)
    print(json.dumps({"what": "deit_tiny fusion 2 against fusion 1: bit-identical logits", "equal": bool(np.array_equal(built[1][1], built[2][1]))}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--net-batch", type=int, default=8)
    ap.add_argument("--no-nets", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("attn_bench needs the GPU: nothing is measured without one")
    tf, mhz = booster.calibrate_mfma_f32()
    print(json.dumps({"what": "fhip_calibrate_mfma_f32", "TFLOPs": round(tf, 1), "MHz": round(mhz)}), flush=True)
    attention_rows(args.iters, args.rounds, tf)
    elementwise_rows(args.iters, args.rounds)
    if not args.no_nets:
        nets(max(args.iters // 4, 10), args.rounds, args.net_batch)
    print(json.dumps({"done": True}))


if __name__ == "__main__":
    main()
