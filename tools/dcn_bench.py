#!/usr/bin/env python3
"""tools/dcn_bench.py [--batch N] [--iters N] [--rounds R] -- the deformable convolution of libfeather_dcn.so on the three DCN shapes of
CenterNet's ResNet-18 neck (model_zoo.centernet_resdcn18 at 512 px: 512 -> 256 at 16x16, 256 -> 128 at 32x32, 128 -> 64 at 64x64, 3x3, pad 1)
(DESIGN.md 3.31 records the figures).

Per shape: fhip_dcn_forward (DCN v2, offsets U(-2, 2), mask U(0, 1)) on weights packed once; the same call with zero offsets; and the
main library's plain 3x3 convolution of the same shape (the route it picks by itself), which is the floor a DCN with zero offsets could at
best approach -- the outputs of those two are compared.  The fraction is the TFLOP/s of the 2 n K Ho Wo C kh kw operations the layer needs
over what fhip_calibrate_mfma_f32 measures in this process for a kernel of nothing but fp32 matrix instructions.

Times are device events around a loop of calls on buffers allocated once, after a warm-up; microseconds per call, median and maximum of
the rounds.  Every call reuses the same buffers, which stay in the caches.  No figure is a pass / fail bound of any test.  One JSON line
per row."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from feathercnn_amd import ConvLayer, ConvParam, None_, booster, dcn  # noqa: E402
from tools.frame_bench import timed  # noqa: E402

SHAPES = ((512, 256, 16), (256, 128, 32), (128, 64, 64))  # (C, K, plane) of up1_dcn, up2_dcn, up3_dcn


def rounds_of(fn, iters, rounds):
    times = [timed(fn, [()], iters) for _ in range(rounds)]
    return round(statistics.median(times), 1), round(max(times), 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dcn_bench needs the GPU: nothing is measured without one")
    n = args.batch
    torch.manual_seed(0)
    mfma_tflops, mhz = booster.calibrate_mfma_f32()
    print(json.dumps({"measured_fp32_mfma_TFLOPs": round(mfma_tflops, 1), "shader_mhz": round(mhz)}), flush=True)
    for c, k, p in SHAPES:
        x = torch.rand((n, c, p, p), device="cuda") * 2 - 1
        w = (torch.rand((k, c, 3, 3), device="cuda") * 2 - 1) / (c * 9) ** 0.5
        b = torch.rand((k,), device="cuda")
        offset = torch.rand((n, 18, p, p), device="cuda") * 4 - 2
        zero = torch.zeros_like(offset)
        mask = torch.rand((n, 9, p, p), device="cuda")
        packed = dcn.dcn_pack(w)
        y = torch.empty((n, k, p, p), device="cuda")
        us, us_max = rounds_of(lambda: dcn.deform_conv2d(x, offset, mask, w, b, pads=1, out=y, packed=packed), args.iters, args.rounds)
        zus, zus_max = rounds_of(lambda: dcn.deform_conv2d(x, zero, None, w, b, pads=1, out=y, packed=packed), args.iters, args.rounds)
        param = ConvParam(output_channels=k, input_channels=c, input_h=p, input_w=p, kernel_h=3, kernel_w=3, stride_h=1, stride_w=1, pad_left=1, pad_right=1, pad_top=1,
                          pad_bottom=1, group=1, bias_term=True, activation=None_, batch=n)
        layer = ConvLayer(param, w, b)
        yc = torch.empty_like(y)
        scratch = torch.empty(max(layer.buffer_bytes // 4, 1), device="cuda")
        cus, cus_max = rounds_of(lambda: layer.Forward(x, yc, scratch), args.iters, args.rounds)
        tflops = 2.0 * n * k * p * p * c * 9 / us / 1e6
        print(json.dumps({"what": f"DCN {c}->{k} 3x3 at {p}x{p}", "n": n, "kernel": dcn.dcn_route(c, k), "us": us, "us_max": us_max, "TFLOPs": round(tflops, 1),
                          "fraction_of_measured_mfma": round(tflops / mfma_tflops, 3), "zero_offsets_us": zus, "zero_offsets_us_max": zus_max, "plain_conv_us": cus,
                          "plain_conv_us_max": cus_max, "plain_conv_algo": booster.ALGO_NAMES.get(layer.booster.algo, layer.booster.algo), "dcn_over_plain": round(us / cus, 2),
                          "zero_offsets_differ_from_plain_by": float((yc - y).abs().max() / yc.abs().max())}), flush=True)
    print(json.dumps({"done": True}))


if __name__ == "__main__":
    main()
