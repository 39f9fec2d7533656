#!/usr/bin/env python3
"""tools/stft_bench.py [--batch N] [--seconds S] [--rounds R] [--window MS] [--no-torch] -- the Spectrogram kernel of libfeather_stft.so on
three speech front ends at 16 kHz (DESIGN.md 3.33 records the figures): n_fft 400 / hop 160, 512 / 160 and 1024 / 256, Hann, power 2.

Per shape: the new kernel; its 2 * (2 freqs) * frames * n_fft operations a row over the fp32 matrix rate fhip_calibrate_mfma_f32 measures
in this process, and the bytes it must move (the waveform once, the output once; the basis stays in the caches) at the HBM peak the
project uses -- the two times that bound it; the same arithmetic on what the project offered before, Convolution1D with one input channel,
2 freqs outputs, kw = n_fft, stride = hop on a waveform the caller has padded (the padding is not timed); and torch.stft on the same card
as an outside yardstick.  Times are device events around a loop of calls sized to --window milliseconds on buffers allocated once, after a
warm-up; microseconds per call, median and maximum of the rounds.  The buffers stay in the caches between calls.  No figure is a pass / fail
bound of any test.  One JSON line per row."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from benchkit import PEAK_HBM_GBS  # noqa: E402
from feathercnn_amd import booster, conv1d, stft  # noqa: E402
from tools.conv3d_bench import rounds_of  # noqa: E402

SHAPES = ((400, 160), (512, 160), (1024, 256))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=200.0)
    ap.add_argument("--no-torch", action="store_true", help="leave the outside yardstick out")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("stft_bench needs the GPU: nothing is measured without one")
    n, l = args.batch, int(args.seconds * 16000)
    torch.manual_seed(0)
    mfma_tflops, mhz = booster.calibrate_mfma_f32()
    print(json.dumps({"measured_fp32_mfma_TFLOPs": round(mfma_tflops, 1), "shader_mhz": round(mhz), "hbm_peak_GBs": PEAK_HBM_GBS}), flush=True)
    x = torch.rand((n, l), device="cuda") * 2 - 1
    for n_fft, hop in SHAPES:
        basis = torch.from_numpy(stft.basis(n_fft, n_fft, 1)).cuda()
        y = stft.spectrogram(x, n_fft, 2, hop, n_fft, 1, device_basis=basis)
        _, freqs, frames = y.shape
        us, us_max, iters = rounds_of(lambda: stft.spectrogram(x, n_fft, 2, hop, n_fft, 1, device_basis=basis, out=y), args.window, args.rounds)
        flops, moved = 2.0 * n * 2 * freqs * frames * n_fft, 4.0 * (x.numel() + y.numel())
        row = {"what": f"n_fft {n_fft} hop {hop}", "n": n, "L": l, "freqs": freqs, "frames": frames, "kernel": stft.stft_route(0, n_fft, hop), "us": us, "us_max": us_max,
               "iters": iters, "TFLOPs": round(flops / us / 1e6, 1), "fraction_of_measured_mfma": round(flops / us / 1e6 / mfma_tflops, 3),
               "mfma_bound_us": round(flops / mfma_tflops / 1e6, 1), "hbm_bound_us": round(moved / PEAK_HBM_GBS / 1e3, 1)}
        # the same arithmetic as a Convolution1D: [n][1][L'] * [2 freqs][1][n_fft] at stride hop -> [n][2 freqs][frames]
        xp = torch.nn.functional.pad(x[:, None], (n_fft // 2, n_fft // 2), mode="reflect").contiguous()
        w = basis.reshape(2 * freqs, 1, n_fft)
        yc = conv1d.conv1d(xp, w, None, hop)
        cus, cus_max, _ = rounds_of(lambda: conv1d.conv1d(xp, w, None, hop, out=yc), args.window, args.rounds)
        p = yc[:, 0::2] ** 2 + yc[:, 1::2] ** 2
        row.update({"conv1d_kernel": conv1d.conv1d_route(1, 2 * freqs, n_fft, 1, hop), "conv1d_us": cus, "conv1d_us_max": cus_max, "conv1d_over_stft": round(cus / us, 2),
                    "differs_from_conv1d_by": float((y - p).abs().max() / p.abs().max())})
        if not args.no_torch:
            win = torch.hann_window(n_fft, periodic=True, device="cuda")
            run = lambda: torch.stft(x, n_fft, hop, n_fft, window=win, center=True, pad_mode="reflect", return_complex=True).abs() ** 2
            yt = run()
            tus, tus_max, _ = rounds_of(run, args.window, args.rounds)
            row.update({"torch_stft_us": tus, "torch_stft_us_max": tus_max, "stft_over_torch": round(us / tus, 2),
                        "differs_from_torch_by": float((y - yt).abs().max() / yt.abs().max())})
        print(json.dumps(row), flush=True)
    print(json.dumps({"done": True}))


if __name__ == "__main__":
    main()
