#!/usr/bin/env python3
"""tools/conv3d_bench.py [--batch N] [--rounds R] [--window MS] [--no-torch] -- the 3-D convolution of libfeather_conv3d.so on five layers of the video nets
of the zoo (DESIGN.md 3.32 records the figures): C3D's conv2 (64 -> 128 at 16 x 56 x 56), conv3b (256 -> 256 at 8 x 28 x 28) and conv5b
(512 -> 512 at 2 x 7 x 7), R3D-18's stem (3 -> 64, 3 x 7 x 7 at stride (1, 2, 2) on 16 x 112 x 112) and its stride-2 3 x 3 x 3 layer (128 -> 256
on 8 x 14 x 14).

Per shape: fhip_conv3d_forward on the kernel the route rule picks, weights packed once; the same call forced onto the direct kernel; and
torch.nn.functional.conv3d in fp32 on the same card, an outside yardstick and no reference for correctness (the outputs are compared all
the same).  The fraction is the TFLOP/s of the 2 n K Do Ho Wo C kd kh kw operations the layer needs over what fhip_calibrate_mfma_f32
measures in this process for a kernel of nothing but fp32 matrix instructions.

Times are device events around a loop of calls on buffers allocated once, after a warm-up, the loop sized to fill --window milliseconds;
microseconds per call, median and maximum of the rounds.  Every call reuses the same buffers.  No figure is a pass / fail bound of any
test.  One JSON line per row."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from feathercnn_amd import booster, conv3d  # noqa: E402
from tools.frame_bench import timed  # noqa: E402

# (what, C, K, (D, H, W), kernel, stride, pads)
SHAPES = (("C3D conv2", 64, 128, (16, 56, 56), 3, 1, 1), ("C3D conv3b", 256, 256, (8, 28, 28), 3, 1, 1), ("C3D conv5b", 512, 512, (2, 7, 7), 3, 1, 1),
          ("R3D-18 stem", 3, 64, (16, 112, 112), (3, 7, 7), (1, 2, 2), (1, 3, 3)), ("R3D-18 l3b0_c1", 128, 256, (8, 14, 14), 3, 2, 1))


def rounds_of(fn, window_ms, rounds):
    once = timed(fn, [()], 3)  # microseconds: sizes the loop
    iters = max(5, int(window_ms * 1e3 / max(once, 1.0)))
    times = [timed(fn, [()], iters) for _ in range(rounds)]
    return round(statistics.median(times), 1), round(max(times), 1), iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=300.0)
    ap.add_argument("--no-torch", action="store_true", help="leave the outside yardstick out")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("conv3d_bench needs the GPU: nothing is measured without one")
    n = args.batch
    torch.manual_seed(0)
    mfma_tflops, mhz = booster.calibrate_mfma_f32()
    print(json.dumps({"measured_fp32_mfma_TFLOPs": round(mfma_tflops, 1), "shader_mhz": round(mhz)}), flush=True)
    for what, c, k, dhw, kernel, stride, pads in SHAPES:
        kern = conv3d._three(kernel)
        x = torch.rand((n, c) + dhw, device="cuda") * 2 - 1
        w = (torch.rand((k, c) + kern, device="cuda") * 2 - 1) / (c * kern[0] * kern[1] * kern[2]) ** 0.5
        b = torch.rand((k,), device="cuda")
        route = conv3d.conv3d_route(c, k, kernel, 1, stride)
        packed = conv3d.pack_weights(w) if "mfma" in route else None
        y = conv3d.conv3d(x, w, b, stride, 1, pads, activation=1, packed=packed)
        yd = torch.empty_like(y)
        us, us_max, iters = rounds_of(lambda: conv3d.conv3d(x, w, b, stride, 1, pads, activation=1, packed=packed, out=y), args.window, args.rounds)
        dus, dus_max, _ = rounds_of(lambda: conv3d.conv3d(x, w, b, stride, 1, pads, activation=1, direct=True, out=yd), args.window, args.rounds)
        flops = 2.0 * y.numel() * c * kern[0] * kern[1] * kern[2]
        print(json.dumps({"what": what, "shape": f"{c}->{k} {kern} at {dhw} stride {stride}", "n": n, "kernel": route, "us": us, "us_max": us_max, "iters": iters,
                          "TFLOPs": round(flops / us / 1e6, 1), "fraction_of_measured_mfma": round(flops / us / 1e6 / mfma_tflops, 3), "direct_us": dus, "direct_us_max": dus_max,
                          "direct_over_chosen": round(dus / us, 2), "differs_from_direct_by": float((y - yd).abs().max() / yd.abs().max())}), flush=True)
        if args.no_torch:
            continue
        torch_pads = conv3d._pads(pads)[0]
        yt = torch.relu_(torch.nn.functional.conv3d(x, w, b, conv3d._three(stride), torch_pads))
        tus, tus_max, _ = rounds_of(lambda: torch.relu_(torch.nn.functional.conv3d(x, w, b, conv3d._three(stride), torch_pads)), args.window, args.rounds)
        print(json.dumps({"what": what, "torch_conv3d_us": tus, "torch_conv3d_us_max": tus_max, "chosen_over_torch": round(us / tus, 2),
                          "differs_from_torch_by": float((y - yt).abs().max() / yt.abs().max())}), flush=True)
    print(json.dumps({"done": True}))


if __name__ == "__main__":
    main()
