#!/usr/bin/env python3
"""tools/lrn_bench.py [--iters N] [--rounds R] [--batches 1,32,256] [--nets] -- the kernels of libfeather_lrn.so on the tensors of the nets
they are for: AlexNet's norm1 (96 x 55 x 55) and norm2 (256 x 27 x 27) and GoogLeNet's conv2/norm2 (192 x 56 x 56), LRN 5 / 1e-4 / 0.75
in front of a 3 x 3 / stride-2 max pooling, at batches 1, 32 and 256.

Per shape, in one process, the candidates alternating round by round:
  copy      a device-to-device copy of the same tensor (torch's copy_), the yardstick: reads and writes what a perfect LRN reads and writes
  lrn       fhip_lrn_forward                                   (and lrn_unsplit / lrn_chunk16 / 8 / 4: the channel split given)
  pool      fhip_pooling of libfeather_hip.so on the LRN's output: what fusion levels 0 and 1 run behind it
  fused     fhip_lrn_pool_forward, one launch
Reported per candidate: the median over the rounds in microseconds with the least and the largest round; lrn as a ratio to the copy;
fused as a ratio to lrn + pool of the same run; GB/s of the bytes a perfect kernel moves (LRN: the tensor read and written once; fused:
the tensor read once, the pooled tensor written once).
Cold: every candidate walks a ring of tensor sets of more than 256 MiB (the Infinity Cache) in all, in order.  Times are device events
around an eager loop of launches, bounded below by the host's cost per enqueue: a row near 8 us measures the enqueue, not the kernel
(batch 1 is such a row).  No figure here is a pass / fail bound of any test.
--nets adds alexnet:256 and googlenet:64 at fusion levels 1 and 2 through tools/net_bench.py.  Prints one JSON line per shape and one at
the end."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from benchkit import PEAK_HBM_GBS  # noqa: E402
from feathercnn_amd import _lib, lrn, lrn_pool, lrn_pool_route, lrn_route  # noqa: E402
from feathercnn_amd.booster import _ptr, _stream  # noqa: E402
from feathercnn_amd.net import pool_param  # noqa: E402

# (label, channels, plane)
SHAPES = [("alexnet norm1 96x55^2", 96, 55), ("alexnet norm2 256x27^2", 256, 27), ("googlenet norm2 192x56^2", 192, 56)]
LRN = dict(local_size=5, alpha=1e-4, beta=0.75)
POOL = {"kernel": 3, "stride": 2}
L3 = 256 << 20


def ring_of(shapes):
    """A ring of tensor sets (one tensor per shape) of more than the Infinity Cache in all."""
    per = sum(int(np.prod(s)) * 4 for s in shapes)
    ring = max(2, -(-(L3 + (L3 >> 2)) // per))
    return [tuple(torch.randn(s, device="cuda") for s in shapes) for _ in range(ring)]


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


def rounds_of(cands, sets, iters, rounds):
    """name -> the times of `rounds` rounds, the candidates alternating within a round."""
    t = {nm: [] for nm, _ in cands}
    for _ in range(rounds):
        for nm, fn in cands:
            t[nm].append(timed(fn, sets, iters))
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batches", default="1,32,256")
    ap.add_argument("--nets", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lrn_bench needs a GPU")
    main_lib = _lib.load_library()
    rows = []
    for label, c, plane in SHAPES:
        for n in (int(b) for b in args.batches.split(",")):
            q = pool_param(c, plane, plane, **POOL)
            oh, ow = ctypes.c_int(), ctypes.c_int()
            assert main_lib.fhip_pooling_output_dim(ctypes.byref(q), ctypes.byref(oh), ctypes.byref(ow)) == 0
            full, pooled = (n, c, plane, plane), (n, c, oh.value, ow.value)
            sets = ring_of([full, full, pooled])  # x, the LRN's output, the pooled output
            nbytes, pbytes = int(np.prod(full)) * 4, int(np.prod(pooled)) * 4

            def pool(x, y, z):
                assert main_lib.fhip_pooling(ctypes.byref(q), n, _ptr(z), _ptr(y), _stream()) == 0

            cands = [("copy", lambda x, y, z: y.copy_(x)), ("lrn", lambda x, y, z: lrn(x, out=y, **LRN)), ("pool", pool),
                     ("fused", lambda x, y, z: lrn_pool(x, POOL, out=z, **LRN)), ("lrn_unsplit", lambda x, y, z: lrn(x, out=y, chunk=0, **LRN)),
                     ("lrn_chunk16", lambda x, y, z: lrn(x, out=y, chunk=16, **LRN)), ("lrn_chunk8", lambda x, y, z: lrn(x, out=y, chunk=8, **LRN)),
                     ("lrn_chunk4", lambda x, y, z: lrn(x, out=y, chunk=4, **LRN))]
            t = rounds_of(cands, sets, args.iters, args.rounds)
            med = {nm: statistics.median(v) for nm, v in t.items()}
            x, y, z = sets[0]
            assert torch.equal(lrn_pool(x, POOL, **LRN), _pooled(main_lib, q, n, lrn(x, **LRN), pooled)), "fused != lrn + pooling"
            row = {"shape": label, "batch": n, "MB": nbytes / 1e6, "route": lrn_route(x, LRN["local_size"], out=y).replace("fhip::", ""),
                   "fused_route": lrn_pool_route(x, POOL, LRN["local_size"]).replace("fhip::", ""),
                   "us": {nm: [round(med[nm], 2), round(min(v), 2), round(max(v), 2)] for nm, v in t.items()},
                   "lrn_over_copy": round(med["lrn"] / med["copy"], 3), "fused_over_pair": round(med["fused"] / (med["lrn"] + med["pool"]), 3),
                   "gbs": {"copy": round(2 * nbytes / med["copy"] / 1e3), "lrn": round(2 * nbytes / med["lrn"] / 1e3),
                           "fused": round((nbytes + pbytes) / med["fused"] / 1e3)}}
            print(json.dumps(row), flush=True)
            rows.append(row)
            del sets, x, y, z
            torch.cuda.empty_cache()
    if args.nets:
        import net_bench
        for name, batch in (("alexnet", 256), ("googlenet", 64)):
            for level in (1, 2):
                net_bench.run(name, batch, level)
    print(json.dumps({"lrn_bench": rows, "peak_hbm_gbs": PEAK_HBM_GBS}))


def _pooled(main_lib, q, n, y, shape):
    z = torch.empty(shape, device="cuda")
    assert main_lib.fhip_pooling(ctypes.byref(q), n, _ptr(z), _ptr(y), _stream()) == 0
    return z


if __name__ == "__main__":
    main()
