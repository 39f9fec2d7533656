"""Tile GEMM + chained boundary of the 64-input-channel layers of VGG-16 (conv1_2 and conv2_1 at batch 32): the main route
(fhip_winograd_f63_tile_gemm + fhip_winograd_f63_output_to_next_input) against libfeather_colpass.so (48-plane M), interleaved round by round
in one process, each launch timed with device events.  Per line V' of the two routes is compared bit for bit.
Usage: python tools/colpass_bench.py [--batch 32] [--rounds 8] [--reps 10] [--lib other/libfeather_colpass.so ...]
Every --lib is one more candidate next to the tree's library (block-shape variants built with -DCOLPASS_WN / _BK / _NBUF)."""
import argparse
import ctypes
import statistics

import numpy as np
import torch

from feathercnn_amd import ConvLayer, ConvParam, _lib
from feathercnn_amd.booster import WINOGRADF63, _ptr, _stream, winograd_plan

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--rounds", type=int, default=8)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--lib", action="append", default=[])
ap.add_argument("--only", default="")
args = ap.parse_args()
dev = torch.device("cuda:0")
main = _lib.load_library()


def candidate(path):
    lib = ctypes.CDLL(path)
    for name, (res, argtypes) in _lib.COLPASS_SIGNATURES.items():
        getattr(lib, name).restype, getattr(lib, name).argtypes = res, argtypes
    return lib


cands = [("colpass", _lib.load_colpass_library())] + [(p.rsplit("/", 1)[-1], candidate(p)) for p in args.lib]
SHAPES = [("conv1_2", 64, 224, True), ("conv2_1", 128, 112, False)]


def prm(ic, oc, h):
    p = ConvParam(output_channels=oc, input_channels=ic, input_h=h, input_w=h, kernel_h=3, kernel_w=3, stride_h=1, stride_w=1, pad_left=1, pad_right=1,
                  pad_top=1, pad_bottom=1, group=1, bias_term=True, activation=1, batch=args.batch)
    p.AssignOutputDim()
    return p


def timed(calls, reps):
    """[(name, f)] run in order `reps` times -> ms per launch, per name."""
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(len(calls) + 1)] for _ in range(reps)]
    for r in range(reps):
        ev[r][0].record()
        for i, (_, f) in enumerate(calls):
            assert f() == 0
            ev[r][i + 1].record()
    torch.cuda.synchronize()
    return [statistics.median(ev[r][i].elapsed_time(ev[r][i + 1]) for r in range(reps)) for i in range(len(calls))]


for name, k, h, pool in SHAPES:
    if args.only and args.only != name:
        continue
    rng = np.random.default_rng(1)
    p, nx = prm(64, k, h), prm(k, k, h // 2 if pool else h)
    pl, pn = winograd_plan(p), winograd_plan(nx)
    w = torch.from_numpy((rng.standard_normal((k, 64, 3, 3)) / 24).astype(np.float32)).to(dev)
    bias = torch.from_numpy(rng.uniform(-0.1, 0.1, k).astype(np.float32)).to(dev)
    u = ConvLayer(p, w, bias, algo=WINOGRADF63).packed
    v = (torch.rand(pl.v_bytes // 4, device=dev) * 2 - 1)
    m = torch.empty(pl.m_bytes // 4, device=dev)
    vn = [torch.zeros(pn.v_bytes // 4, device=dev) for _ in range(2)]
    cp, cn = p._c(), nx._c()
    n = args.batch
    route_main = [("gemm", lambda: main.fhip_winograd_f63_tile_gemm(ctypes.byref(cp), n, _ptr(m), _ptr(u), _ptr(v), _stream())),
                  ("chain", lambda: main.fhip_winograd_f63_output_to_next_input(ctypes.byref(cp), ctypes.byref(cn), n, _ptr(vn[0]), _ptr(m), _ptr(bias), int(pool), _stream()))]

    def route(lib):
        return [("gemm", lambda: lib.fhip_colpass_tile_gemm(ctypes.byref(cp), n, ctypes.byref(pl), _ptr(m), _ptr(u), _ptr(v), _stream())),
                ("chain", lambda: lib.fhip_colpass_output_to_next_input(ctypes.byref(cp), ctypes.byref(cn), n, ctypes.byref(pl), ctypes.byref(pn), _ptr(vn[1]),
                                                                        _ptr(m), _ptr(bias), int(pool), _stream()))]

    timed(route_main, 2)
    for cname, lib in cands:
        vn[1].zero_()
        t = timed(route(lib), 2)
        print(f"{name} {cname}: V' equal to the main route's: {torch.equal(vn[0], vn[1])}", flush=True)
    rows = {c: [] for c in ["main"] + [c for c, _ in cands]}
    for r in range(args.rounds):
        rows["main"].append(timed(route_main, args.reps))
        for cname, lib in cands:
            rows[cname].append(timed(route(lib), args.reps))
    print(f"{name} b{n}: K {k}, {h} px, pool {int(pool)}, columns {pl.columns}; us per launch, median of {args.reps} per round, {args.rounds} interleaved rounds")
    for cname, rr in rows.items():
        pair = [1e3 * (g + c) for g, c in rr]
        print(f"  {cname:28s} gemm {1e3 * statistics.median(g for g, _ in rr):7.1f}  chain {1e3 * statistics.median(c for _, c in rr):7.1f}  "
              f"pair median {statistics.median(pair):7.1f}  min {min(pair):7.1f}  max {max(pair):7.1f}", flush=True)
