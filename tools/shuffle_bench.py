#!/usr/bin/env python3
"""tools/shuffle_bench.py [--batches 1,32,256] [--rounds N] -- the channel map of libfeather_shuffle.so on ShuffleNet v2's unit boundaries
(Concat(a, b) -> ShuffleChannel(2) -> Slice(2) on 2 x 58 x 28^2, 2 x 116 x 14^2, 2 x 232 x 7^2), against yardsticks run in the same process
on the same tensors, the candidates alternating inside every round:
  copy     one device-to-device hipMemcpyAsync of the same byte count: both are one read plus one write;
  map      the collapsed run: one channel-map launch, two sources, two outputs (16-byte accesses where the plane allows, else 4-byte);
  map4     the same launch forced to 4-byte accesses (aligned planes only): what the access width is worth;
  steps    the same three layers through feather::Net at fusion level 0 (two 2-D copies, a shuffle launch, a slice launch) and
  fused    at fusion level 2 (one launch), both as a replayed hipGraph;
  torch    torch.cat + channel_shuffle + split(...).contiguous() of the installed torch, for orientation.
Every candidate but steps / fused is captured REPS times into one hipGraph and timed by device events around a replay, so a figure is the
device's time per call, not the host's cost per enqueue; steps / fused are net Forwards (a graph replay of 4 and 1 nodes each) timed by
the wall clock over REPS back-to-back launches, so they carry one graph launch each.  Warm: the same tensors every call (they stay in L2 / Infinity Cache where they fit).  Prints
median and minimum over the rounds, the ratio to the copy, and one JSON line at the end."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
from feathercnn_amd.net import Net  # noqa: E402
from feathercnn_amd.shuffle import ChannelMap, channel_route  # noqa: E402

SHAPES = [("stage2 2x58x28^2", 58, 28), ("stage3 2x116x14^2", 116, 14), ("stage4 2x232x7^2", 232, 7)]
REPS = 20


def hip_runtime():
    """The HIP runtime torch already mapped (a second copy of the library would be a second runtime)."""
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return ctypes.CDLL(line.split()[-1])
    raise RuntimeError("libamdhip64 is not mapped")


def boundary_tables(half):
    cat = [(0, c) for c in range(half)] + [(1, c) for c in range(half)]
    sh = [cat[k * half + i] for i in range(half) for k in range(2)]
    return [sh[:half], sh[half:]]


def graph_of(fn):
    fn()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            for _ in range(REPS):
                fn()
    return g


def replay_us(g, per=REPS):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    g.replay()
    a.record()
    g.replay()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / per


def net_of(half, hw, n, a, b, fusion):
    param = (f"7767517\n5 6\nInput a 0 1 a 0={hw} 1={hw} 2={half}\nInput b 0 1 b 0={hw} 1={hw} 2={half}\nConcat cat 2 1 a b cat 0=0\n"
             "ShuffleChannel sh 1 1 cat sh 0=2\nSlice sl 1 2 sh keep work -23300=2,-233,-233\n").encode()
    net = Net(fusion=fusion, graph=True)
    net.LoadParam(param)
    net.LoadWeights(b"")
    net.FeedInput("a", a)
    net.FeedInput("b", b)
    for _ in range(3):
        net.Forward()
    torch.cuda.synchronize()
    return net


def net_us(net):
    """The net enqueues on a stream of its own, so this one is wall time over REPS back-to-back graph launches, synchronised at both ends."""
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(REPS):
        net.Forward()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e6 / REPS


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,32,256")
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    hip = hip_runtime()
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    rows = []
    for n in [int(v) for v in args.batches.split(",")]:
        for label, half, hw in SHAPES:
            a, b = torch.randn((n, half, hw, hw), device="cuda"), torch.randn((n, half, hw, hw), device="cuda")
            keep, work = torch.empty_like(a), torch.empty_like(a)
            src, dst = torch.randn((n, 2 * half, hw, hw), device="cuda"), torch.empty((n, 2 * half, hw, hw), device="cuda")
            nbytes = src.numel() * 4
            m = ChannelMap([half, half], boundary_tables(half))

            def copy():
                rc = hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), nbytes, 3, torch.cuda.current_stream().cuda_stream)
                assert rc == 0, rc

            def torch_path():
                s = torch.nn.functional.channel_shuffle(torch.cat([a, b], 1), 2)
                k, w = torch.split(s, [half, half], dim=1)
                return k.contiguous(), w.contiguous()

            cands = {"copy": graph_of(copy), "map": graph_of(lambda: m.forward([a, b], [keep, work])), "torch": graph_of(torch_path)}
            vec = channel_route("map", hw, hw, [a, b, keep, work]).endswith("true>")
            if vec:
                cands["map4"] = graph_of(lambda: m.forward([a, b], [keep, work], "4b"))
            nets = {"steps": net_of(half, hw, n, a, b, 0), "fused": net_of(half, hw, n, a, b, 2)}
            times = {k: [] for k in list(cands) + list(nets)}
            for _ in range(args.rounds):
                for k, g in cands.items():
                    times[k].append(replay_us(g))
                for k, net in nets.items():
                    times[k].append(net_us(net))
            for net in nets.values():
                net.close()
            want = torch.nn.functional.channel_shuffle(torch.cat([a, b], 1), 2)
            assert torch.equal(keep, want[:, :half]) and torch.equal(work, want[:, half:])
            med = {k: statistics.median(v) for k, v in times.items()}
            row = {"batch": n, "shape": label, "bytes": 2 * nbytes, "width": "16b" if vec else "4b",
                   **{k + "_us": [round(med[k], 2), round(min(times[k]), 2), round(max(times[k]), 2)] for k in times},
                   "map_vs_copy": round(med["copy"] / med["map"], 3), "fused_vs_steps": round(med["steps"] / med["fused"], 2),
                   "map_vs_torch": round(med["torch"] / med["map"], 2), "map_GBps": round(2 * nbytes / med["map"] / 1e3, 1),
                   "copy_GBps": round(2 * nbytes / med["copy"] / 1e3, 1)}
            rows.append(row)
            print(f"b{n:<4d} {label:20s} {row['width']:3s} " + "  ".join(f"{k} {med[k]:8.2f} us (min {min(times[k]):.2f}, max {max(times[k]):.2f})" for k in times))
            print(f"      map / copy rate {row['map_vs_copy']:.3f} ({row['map_GBps']} vs {row['copy_GBps']} GB/s), fused vs three steps {row['fused_vs_steps']:.2f}x, "
                  f"map vs torch {row['map_vs_torch']:.2f}x", flush=True)
            m.close()
    print(json.dumps({"shuffle_bench": rows, "reps_per_graph": REPS, "rounds": args.rounds, "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    np.random.seed(0)
    main()
