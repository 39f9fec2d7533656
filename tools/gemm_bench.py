#!/usr/bin/env python3
"""tools/gemm_bench.py [--iters N] [--rounds R] [--only attention|swin|dense|thin] -- libfeather_gemm.so on the device (DESIGN.md 3.36 records
the figures).

* attention: the products of ViT-B un-fused -- 12 heads, T 197 and 577, d 64, n 1 and 32 -- q k^T ([T][d] [T][d]^T) and p v ([T][T] [T][d]),
  at the auto tile and at both forced tiles.
* swin: a window, 49 x 49 x 32 with a batch of 64 windows x 3 heads, both products.
* dense: 2048 x 4096 x 4096 in the four transposes, both tiles.
* thin: 1 and 4 x 4096 x 4096 against a [K][N] and a [N][K] operand, the thin kernel against the matrix kernel at the small tile.
Next to each: torch.matmul in fp32 on the same card, in the same process -- an outside yardstick -- the FLOPs at the fp32-MFMA rate
fhip_calibrate_mfma_f32 measures in this process, and the bytes the call must move at the HBM peak the project uses.

Times are device events around an eager loop of calls on buffers allocated once, after a warm-up, rounds interleaved; microseconds per call,
median, minimum and maximum of the rounds.  No figure here is a pass / fail bound of any test.  One JSON line per row."""
import argparse
import ctypes
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from feathercnn_amd import _lib, booster  # noqa: E402
from feathercnn_amd.booster import _stream  # noqa: E402
from feathercnn_amd.gemm import GemmDesc, gemm_route  # noqa: E402
from tools.decoder_bench import emit, measure  # noqa: E402


def prepared(sets, m, n, k, batch, ta=0, tb=0, tile=0):
    """One description and the library entry, once: the loop then only launches.  sets: (a, b, d) dense tensors -> (fn(index), route)"""
    desc = GemmDesc(m=m, n=n, k=k, batch=batch, trans_a=ta, trans_b=tb, c_broadcast=-1, lda=m if ta else k, ldb=k if tb else n, ldd=n, a_batch_stride=m * k,
                    b_batch_stride=k * n, d_batch_stride=m * n, tile=tile, alpha=1.0)
    fn, ptrs = _lib.load_gemm_library().fhip_gemm_forward, [tuple(ctypes.c_void_p(t.data_ptr()) for t in s) for s in sets]

    def run(i):
        a, b, d = ptrs[i]
        if fn(ctypes.byref(desc), a, b, None, d, _stream()):
            raise RuntimeError(_lib.load_gemm_library().fhip_gemm_last_error().decode())
    return run, gemm_route(desc)


def product(what, m, n, k, batch, ta, tb, tiles, iters, rounds, tf, count=4):
    sets = [(torch.randn((batch, k, m) if ta else (batch, m, k), device="cuda"), torch.randn((batch, n, k) if tb else (batch, k, n), device="cuda"),
             torch.empty((batch, m, n), device="cuda")) for _ in range(count)]
    op = lambda x, t: x.transpose(1, 2) if t else x  # noqa: E731
    fns, routes = {}, {}
    for tile in tiles:
        fns[f"tile{tile}"], routes[f"tile{tile}"] = prepared(sets, m, n, k, batch, ta, tb, tile)
    fns["torch_fp32"] = lambda i: torch.matmul(op(sets[i][0], ta), op(sets[i][1], tb))
    fns["tile%d" % tiles[0]](0)
    diff = float((sets[0][2] - fns["torch_fp32"](0)).abs().max())
    emit(f"{what} {batch} x {m}x{n}x{k} ta{ta} tb{tb}", measure(fns, [(i,) for i in range(count)], iters, rounds), 2.0 * batch * m * n * k, 4.0 * batch * (m * k + k * n + m * n), tf,
         routes=routes, max_abs_diff_to_torch=diff)


def attention(iters, rounds, tf):
    for n in (1, 32):
        for t in (197, 577):
            product("vit q k^T", t, t, 64, 12 * n, 0, 1, (0, 64, 128), iters, rounds, tf)
            product("vit p v", t, 64, t, 12 * n, 0, 0, (0, 64, 128), iters, rounds, tf)


def swin(iters, rounds, tf):
    product("swin q k^T", 49, 49, 32, 64 * 3, 0, 1, (0, 64, 128), iters, rounds, tf)
    product("swin p v", 49, 32, 49, 64 * 3, 0, 0, (0, 64, 128), iters, rounds, tf)


def dense(iters, rounds, tf):
    for ta in (0, 1):
        for tb in (0, 1):
            product("dense", 2048, 4096, 4096, 1, ta, tb, (0, 64), max(iters // 10, 5), rounds, tf, count=2)


def thin(iters, rounds, tf):
    for m in (1, 4):
        for tb in (0, 1):
            product("thin", m, 4096, 4096, 1, 0, tb, (0, 64), iters, rounds, tf)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", choices=("attention", "swin", "dense", "thin"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gemm_bench needs the GPU: nothing is measured without one")
    tf, mhz = booster.calibrate_mfma_f32()
    print(json.dumps({"what": "fhip_calibrate_mfma_f32", "TFLOPs": round(tf, 1), "MHz": round(mhz)}), flush=True)
    for part in (attention, swin, dense, thin):
        if args.only in (None, part.__name__):
            part(args.iters, args.rounds, tf)
    print(json.dumps({"done": True}))


if __name__ == "__main__":
    main()
