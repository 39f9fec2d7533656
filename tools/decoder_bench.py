#!/usr/bin/env python3
"""tools/decoder_bench.py [--iters N] [--rounds R] [--only encoder|prefill|decode] -- the attention core of libfeather_decoder.so on the device
(DESIGN.md 3.35 records the figures).

* encoder: the four rows of DESIGN.md 3.28's attention table (T = 197 and 577, d = 64, 12 heads, batch 1 and 32, read in place from a fused
  [n * T][3E] projection buffer, group 1, no mask): fhip_sdpa_forward at row tiles of 64 and 128 against fhip_attention_forward of
  libfeather_attn.so, rounds interleaved, with the spread of each over the rounds.
* prefill: n 1, T 2048, 32 heads, 8 kv heads, d 128, causal against not causal.
* decode: tq 1, tk 1024 / 4096 / 16384, the same heads, read from a cache of capacity tk: the auto split against forced splits 1 .. 256.
Next to each: torch.nn.functional.scaled_dot_product_attention in fp32 on the same card -- an outside yardstick only -- the FLOPs at the
fp32-MFMA rate fhip_calibrate_mfma_f32 measures in this process, and the bytes the call must move at the HBM peak the project uses.

Times are device events around an eager loop of calls on buffers allocated once, after a warm-up; microseconds per call, median, minimum and
maximum of the rounds.  No figure here is a pass / fail bound of any test.  One JSON line per row."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from benchkit import PEAK_HBM_GBS  # noqa: E402
from feathercnn_amd import attn, booster, decoder  # noqa: E402
from tools.frame_bench import timed  # noqa: E402

SDPA = torch.nn.functional.scaled_dot_product_attention


def measure(fns, sets, iters, rounds):
    """{label: (median, min, max) us} of the callables, interleaved inside every round."""
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            times[k].append(timed(fn, sets, iters))
    return {k: (round(statistics.median(t), 2), round(min(t), 2), round(max(t), 2)) for k, t in times.items()}


def emit(what, t, flops, moved, tf, **more):
    row = {"what": what, "GFLOP": round(flops / 1e9, 3), "us_at_mfma_rate": round(flops / tf / 1e6, 2), "MB": round(moved / 1e6, 2), "us_at_hbm_peak": round(moved / PEAK_HBM_GBS / 1e3, 2)}
    row.update({f"{k}_us": v[0] for k, v in t.items()})
    row.update({f"{k}_min_max": v[1:] for k, v in t.items()})
    row.update(more)
    print(json.dumps(row), flush=True)


def prepared(sets, **kw):
    """One prepared call per buffer set (feathercnn_amd.decoder.prepare_sdpa: the loop then only launches) -> fn(index)."""
    runs = [decoder.prepare_sdpa(q, k, v, out=o, **kw)[0] for q, k, v, o in sets]
    return lambda i: runs[i]()


def encoder(iters, rounds, tf):
    heads, d = 12, 64
    e = heads * d
    for n in (1, 32):
        for t in (197, 577):
            count = 4 if n == 32 else 16
            bufs = [(torch.randn((n, t, 3 * e), device="cuda") * 0.35, torch.empty((n, t, e), device="cuda")) for _ in range(count)]
            heads_of = lambda x, j, w: x[:, :, j * e:(j + 1) * e].reshape(n, t, heads, d).transpose(1, 2)  # a view: [n][heads][T][d]
            sets = [(heads_of(qkv, 0, 3), heads_of(qkv, 1, 3), heads_of(qkv, 2, 3), heads_of(out, 0, 1)) for qkv, out in bufs]
            old = lambda i: attn.attention(bufs[i][0][:, :, :e], bufs[i][0][:, :, e:2 * e], bufs[i][0][:, :, 2 * e:], heads, out=bufs[i][1])
            fns = {"attn_old": old, "sdpa_tile64": prepared(sets, scale=1.0, row_tile=64), "sdpa_tile128": prepared(sets, scale=1.0, row_tile=128),
                   "torch_fp32": lambda i: SDPA(*sets[i][:3], scale=1.0)}
            got = {}
            for k in ("attn_old", "sdpa_tile64", "sdpa_tile128"):
                bufs[0][1].zero_()
                fns[k](0)
                got[k] = bufs[0][1].clone()
            times = measure(fns, [(i,) for i in range(count)], iters, rounds)
            emit(f"encoder n{n} T{t} d{d} heads{heads}", times, 4.0 * n * heads * t * t * d, 16.0 * n * t * e, tf,
                 max_abs_diff_new_old=max(float((got[k] - got["attn_old"]).abs().max()) for k in ("sdpa_tile64", "sdpa_tile128")))


def prefill(iters, rounds, tf):
    n, t, heads, kvh, d = 1, 2048, 32, 8, 128
    sets = [tuple(torch.randn((n, h, t, d), device="cuda") * 0.5 for h in (heads, kvh, kvh)) + (torch.empty((n, heads, t, d), device="cuda"),) for _ in range(4)]
    fns = {"sdpa_causal": prepared(sets, causal=True), "sdpa_dense": prepared(sets), "torch_fp32_causal": lambda i: SDPA(*sets[i][:3], is_causal=True, enable_gqa=True),
           "torch_fp32_dense": lambda i: SDPA(*sets[i][:3], enable_gqa=True)}
    q, k, v, o = sets[0]
    diff = float((decoder.sdpa(q, k, v, causal=True) - SDPA(q, k, v, is_causal=True, enable_gqa=True)).abs().max())
    emit(f"prefill n{n} T{t} heads{heads} kv{kvh} d{d} [{decoder.decoder_route(decoder.SDPA, d, heads // kvh * t)}]", measure(fns, [(i,) for i in range(4)], max(iters // 10, 5), rounds),
         4.0 * n * heads * t * t * d, 4.0 * n * t * d * (2 * heads + 2 * kvh), tf, max_abs_diff_to_torch=diff)


def decode(iters, rounds, tf):
    n, heads, kvh, d = 1, 32, 8, 128
    for tk in (1024, 4096, 16384):
        sets = [(torch.randn((n, heads, 1, d), device="cuda") * 0.5, torch.randn((n, kvh, tk, d), device="cuda") * 0.5, torch.randn((n, kvh, tk, d), device="cuda") * 0.5,
                 torch.empty((n, heads, 1, d), device="cuda")) for _ in range(8)]
        scratch = torch.empty((n * kvh * 256 * (heads // kvh) * (d + 2),), device="cuda")
        fns = {"auto": prepared(sets, scratch=scratch), **{f"splits{s}": prepared(sets, splits=s, scratch=scratch) for s in (1, 4, 8, 16, 32, 64, 128, 256) if s <= tk // 32},
               "torch_fp32": lambda i: SDPA(*sets[i][:3], enable_gqa=True)}
        q, k, v, o = sets[0]
        desc = decoder.SdpaDesc(n=n, heads=heads, kv_heads=kvh, tq=1, tk=tk, d=d, q_row_stride=d, k_row_stride=d, v_row_stride=d, out_row_stride=d, scale=1.0)
        diff = float((decoder.sdpa(q, k, v) - SDPA(q, k, v, enable_gqa=True)).abs().max())
        emit(f"decode n{n} tk{tk} heads{heads} kv{kvh} d{d} [{decoder.decoder_route(decoder.SDPA, d, heads // kvh)}]", measure(fns, [(i,) for i in range(8)], iters, rounds),
             4.0 * n * heads * tk * d, 8.0 * n * kvh * tk * d, tf, auto_splits=decoder.sdpa_plan(desc)[1], max_abs_diff_to_torch=diff)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", choices=("encoder", "prefill", "decode"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("decoder_bench needs the GPU: nothing is measured without one")
    tf, mhz = booster.calibrate_mfma_f32()
    print(json.dumps({"what": "fhip_calibrate_mfma_f32", "TFLOPs": round(tf, 1), "MHz": round(mhz)}), flush=True)
    for part in (encoder, prefill, decode):
        if args.only in (None, part.__name__):
            part(args.iters, args.rounds, tf)
    print(json.dumps({"done": True}))


if __name__ == "__main__":
    main()
