#!/usr/bin/env python3
"""tools/rnn_bench.py [--iters N] [--rounds R] [--no-nets] -- the recurrent core on the device (DESIGN.md 3.29 records the figures and the
route rule that follows from them).

* libfeather_rnn.so, a bidirectional LSTM (what CRNN runs), over n in {1, 4, 32, 256} x H in {48, 96, 256} x T in {26, 100}: the step route
  (T launches) and, where Wh fits the chip's LDS, the sequence route (one launch), each forced through fhip_rnn_forward_route on buffers
  allocated once -- as an eager loop of calls, and as the replay of a captured graph of one call (what a Net with the graph switch runs:
  the launches cost less there).  Next to them torch.nn.LSTM in fp32 on the same card (input width H, so it also runs the input projection
  that the core leaves to its caller) -- an outside yardstick only: no ratio is promised or asserted anywhere.
* crnn_vgg_bilstm at batch 32 and crnn_lite_lstm at batch 1 and 4, end to end through the Net.

Times are device events around the loop; microseconds per call, median of the rounds, slow ones included.  No figure here is a pass / fail
bound of any test.  One JSON line per row."""
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
from feathercnn_amd import _lib, model_zoo, rnn  # noqa: E402
from feathercnn_amd.net import Net  # noqa: E402
from tools.frame_bench import timed  # noqa: E402

V = ctypes.c_void_p


def core_call(cell, direction, n, t, h, route):
    """-> (a function of no arguments that enqueues one call on the current stream, its output tensor)."""
    lib = _lib.load_rnn_library()
    nd, g = (2 if direction == 2 else 1), rnn.GATES[cell]
    xp = torch.rand((n, t, nd * g * h), device="cuda") * 2 - 1
    wh = (torch.rand((nd, g * h, h), device="cuda") * 2 - 1) / h ** 0.5
    out = torch.empty((n, t, nd * h), device="cuda")
    scratch = torch.empty((nd, n, h), device="cuda")
    keep = (xp, wh, out, scratch)

    def call():
        rc = lib.fhip_rnn_forward_route(cell, direction, n, t, h, V(xp.data_ptr()), nd * g * h, V(wh.data_ptr()), None, None, None, V(out.data_ptr()), nd * h, None, None,
                                        V(scratch.data_ptr()), V(torch.cuda.current_stream().cuda_stream), route)
        if rc:
            raise RuntimeError(lib.fhip_rnn_last_error().decode())
    call.keep = keep
    return call, out


def replayed(call):
    """The call captured once into a graph; -> a function that replays it."""
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        call()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    return graph.replay


def core_rows(iters, rounds):
    for h in (48, 96, 256):
        for t in (26, 100):
            for n in (1, 4, 32, 256):
                row = {"what": f"LSTM bidirectional n{n} H{h} T{t}", "rule": rnn.rnn_route(rnn.LSTM, h, n, t)}
                outs = {}
                for label, route in (("step", rnn.ROUTE_STEP), ("sequence", rnn.ROUTE_SEQUENCE)):
                    if route == rnn.ROUTE_SEQUENCE and not rnn.sequence_fits(rnn.LSTM, h):
                        continue
                    call, out = core_call(rnn.LSTM, 2, n, t, h, route)
                    eager = [timed(call, [()], iters) for _ in range(rounds)]
                    replay = replayed(call)
                    graph = [timed(replay, [()], iters) for _ in range(rounds)]
                    outs[label] = out
                    row.update({f"{label}_us": round(statistics.median(eager), 1), f"{label}_us_max": round(max(eager), 1), f"{label}_graph_us": round(statistics.median(graph), 1),
                                f"{label}_graph_us_max": round(max(graph), 1), f"{label}_kernel": rnn.rnn_route(rnn.LSTM, h, n, t, route)})
                torch.manual_seed(0)
                ref = torch.nn.LSTM(h, h, batch_first=True, bidirectional=True).cuda()
                x = torch.rand((n, t, h), device="cuda")
                with torch.no_grad():
                    theirs = [timed(lambda: ref(x), [()], iters) for _ in range(rounds)]
                row["torch_lstm_fp32_us"] = round(statistics.median(theirs), 1)
                flops = 2.0 * 2 * n * t * 4 * h * h
                row["step_GFLOPs"] = round(flops / row["step_us"] / 1e3, 1)
                print(json.dumps(row), flush=True)


def nets(iters, rounds):
    for fn, batch, width in ((model_zoo.crnn_vgg_bilstm, 32, 100), (model_zoo.crnn_lite_lstm, 1, 100), (model_zoo.crnn_lite_lstm, 4, 100)):
        p, b, i, o = fn()
        x = np.random.default_rng(0).uniform(-1, 1, (batch, 3, 32, width)).astype(np.float32)
        for graph in (False, True):
            net = Net(fusion=2, graph=graph)
            net.SetRecurrent()
            net.SetDetection(True)
            net.SetTransformer()
            net.SetFrame()
            net.LoadParam(p)
            net.LoadWeights(b)
            net.FeedInput(i, x)
            for _ in range(3):
                net.Forward()
            torch.cuda.synchronize()
            times = []
            for _ in range(rounds):
                t0 = time.perf_counter()
                for _ in range(iters):
                    net.Forward()
                torch.cuda.synchronize()
                times.append((time.perf_counter() - t0) * 1e3 / iters)
            out = net.Extract(o)
            print(json.dumps({"what": f"{fn.__name__} n{batch} fusion 2 graph {graph}", "layers": len(net.layers()), "ms": round(statistics.median(times), 4), "ms_min": round(min(times), 4),
                              "ms_max": round(max(times), 4), "output": list(out.shape), "rows_sum_to_one": bool(np.allclose(out.sum(axis=3), 1, atol=1e-4))}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-nets", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rnn_bench needs the GPU: nothing is measured without one")
    core_rows(args.iters, args.rounds)
    if not args.no_nets:
        nets(args.iters, args.rounds)
    print(json.dumps({"done": True}))


if __name__ == "__main__":
    main()
