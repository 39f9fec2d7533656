#!/usr/bin/env python3
"""tools/inorm_bench.py [--batches 1,4,32] [--iters N] [--routes] -- InstanceNorm (+ReLU) of libfeather_inorm.so on the InstanceNorm shapes
of style_transfer_in and pix2pix_unet, against two yardsticks run in the same process on the same tensors:
  (a) fhip_affine + ReLU: the same 8 bytes per element with free statistics -- the ceiling;
  (b) torch.nn.functional.instance_norm + relu_ of the installed torch -- what a user has without this library.
Warm: the same tensor pair every iteration (it stays in L2 / Infinity Cache where it fits).  Cold: a ring of tensor pairs of more than
256 MiB (the Infinity Cache) in all, however small the shape, walked in order, so that a pair is touched again only after more than the
cache's size of other traffic.  Times are device events around an eager loop of launches (bounded below by the host's cost per enqueue), the best of three rounds in which the three candidates
alternate; bytes are the route's own model (8 B per element for the single-read routes, 12 B for the split-plane route, whose second read
may hit cache).  --routes adds the head-to-head of the routes on either side of each threshold (fhip_instance_norm_forward_route), warm and
cold.  Prints table rows and one JSON line at the end."""
import argparse
import ctypes
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from feathercnn_amd import _lib, instance_norm, instance_norm_route  # noqa: E402
from feathercnn_amd.inorm import CHUNK, scratch_bytes  # noqa: E402

SHAPES = [("st conv1 32x256^2", 32, 256), ("st conv2 64x128^2", 64, 128), ("st res 128x64^2", 128, 64), ("p2p e2/d3 64x64^2", 64, 64),
          ("p2p e3/d4 128x32^2", 128, 32), ("p2p e4/d5 256x16^2", 256, 16), ("p2p e5 256x8^2", 256, 8), ("p2p d2 32x128^2", 32, 128)]
L3 = 256 << 20


def ring_of(shape):
    """Tensor pairs (x, y) whose total size exceeds the Infinity Cache, as slices of two allocations."""
    elems = shape[0] * shape[1] * shape[2] * shape[3]
    ring = max(2, -(-(L3 + (L3 >> 2)) // (elems * 8)))
    xs, ys = torch.randn((ring,) + tuple(shape), device="cuda"), torch.empty((ring,) + tuple(shape), device="cuda")
    return [(xs[k], ys[k]) for k in range(ring)]


def timed(fn, sets, iters):
    """us per call; `sets` is walked in order and whole, so with a ring the re-use distance is the ring's size.  An eager loop: it cannot go
    below the host's cost per enqueue (7 - 9 us from Python), so a row near that figure measures the enqueue, not the kernel."""
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


def best_of(cands, sets, iters, rounds=3):
    best = {}
    for _ in range(rounds):
        for nm, fn in cands:
            t = timed(fn, sets, iters)
            best[nm] = min(best.get(nm, t), t)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,4,32")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--routes", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("inorm_bench needs a GPU")
    lib = _lib.load_library()
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rows, heads = [], []
    print(f"{'shape':20s} {'N':>3s} {'route':38s} {'MB':>7s} | {'warm us':>8s} {'affine':>8s} {'torch':>8s} {'of (a)':>6s} | {'cold us':>8s} {'affine':>8s} {'torch':>8s} {'of (a)':>6s} {'GB/s':>6s}")
    for label, c, size in SHAPES:
        for n in (int(v) for v in args.batches.split(",")):
            shape = (n, c, size, size)
            elems = n * c * size * size
            gamma, beta = torch.rand(c, device="cuda") + 0.5, torch.rand(c, device="cuda") - 0.5
            scratch = torch.empty(max(scratch_bytes(shape) // 4, 2), dtype=torch.float32, device="cuda")
            sets = ring_of(shape)
            route = instance_norm_route(sets[0][0]).replace("fhip::", "")
            moved = elems * (12 if "partial" in route else 8)

            def ours(x, y):
                instance_norm(x, gamma, beta, 1e-3, "relu", out=y, scratch=scratch)

            def affine(x, y):
                lib.fhip_affine(ctypes.c_void_p(y.data_ptr()), ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(gamma.data_ptr()),
                                ctypes.c_void_p(beta.data_ptr()), n, c, size * size, 1, stream())

            def torch_(x, y):
                torch.nn.functional.instance_norm(x, weight=gamma, bias=beta, eps=1e-3).relu_()

            cands = (("ours", ours), ("affine", affine), ("torch", torch_))
            iters = args.iters if elems < (1 << 24) else max(args.iters // 4, 20)
            w, cl = best_of(cands, sets[:1], iters), best_of(cands, sets, iters)
            print(f"{label:20s} {n:3d} {route:38s} {moved / 1e6:7.1f} | {w['ours']:8.1f} {w['affine']:8.1f} {w['torch']:8.1f} {w['affine'] / w['ours']:6.2f} | "
                  f"{cl['ours']:8.1f} {cl['affine']:8.1f} {cl['torch']:8.1f} {cl['affine'] / cl['ours']:6.2f} {moved / cl['ours'] / 1e3:6.0f}", flush=True)
            rows.append({"shape": label, "batch": n, "route": route, "bytes": moved, "ring": len(sets), "warm_us": w, "cold_us": cl})
            del sets
            torch.cuda.empty_cache()
    if args.routes:
        # either side of each threshold: (H = W, plane counts, candidate routes)
        print(f"\n{'plane':>9s} {'planes':>6s} | " + " ".join(f"{r + ' warm':>15s} {r + ' cold':>15s}" for r in ("wave", "block256", "block1024", "split")))
        for size, plane_counts, routes in ((16, (256, 4096), ("wave", "block256")), (32, (128, 512, 4096), ("wave", "block256", "split")),
                                           (64, (64, 128, 512, 4096), ("block256", "block1024", "split")),
                                           (128, (32, 64, 128, 192, 256, 384, 512, 2048), ("block1024", "split"))):
            for planes in plane_counts:
                shape = (1, planes, size, size)
                gamma, beta = torch.rand(planes, device="cuda") + 0.5, torch.rand(planes, device="cuda") - 0.5
                scratch = torch.empty(planes * -(-size * size // CHUNK) * 2, dtype=torch.float32, device="cuda")
                sets = ring_of(shape)
                cands = [(r, (lambda x, y, r=r: instance_norm(x, gamma, beta, 1e-3, "relu", out=y, scratch=scratch, route=r))) for r in routes]
                w, cl = best_of(cands, sets[:1], args.iters), best_of(cands, sets, args.iters)
                cells = " ".join(f"{w[r]:15.1f} {cl[r]:15.1f}" if r in w else f"{'-':>15s} {'-':>15s}" for r in ("wave", "block256", "block1024", "split"))
                print(f"{size:4d}x{size:<4d} {planes:6d} | {cells}", flush=True)
                heads.append({"plane": size, "planes": planes, "warm_us": w, "cold_us": cl})
                del sets
                torch.cuda.empty_cache()
    print(json.dumps({"inorm_bench": rows, "routes": heads}))


if __name__ == "__main__":
    main()
