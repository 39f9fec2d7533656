#!/usr/bin/env python3
"""tools/istft_bench.py [--batch N] [--seconds S] [--rounds R] [--window MS] [--no-torch] -- the InverseSpectrogram kernel of
libfeather_istft.so on the inverse of tools/stft_bench.py's three speech front ends at 16 kHz (DESIGN.md 3.34 records the figures): n_fft
400 / hop 160, 512 / 160 and 1024 / 256, Hann, one-sided, centred; the input is the Spectrogram of a random waveform.

Per shape: the new kernel; its dense work, 2 * (2 freqs) * n_fft operations a frame, over the fp32 matrix rate fhip_calibrate_mfma_f32
measures in this process, and the bytes it must move (the spectrogram once, the waveform once; basis and envelope stay in the caches) at
the HBM peak the project uses -- the two times that bound it; and torch.istft on the same input as an outside yardstick.  Times are device
events around a loop of calls sized to --window milliseconds on buffers allocated once, after a warm-up; microseconds per call, median and
maximum of the rounds.  The buffers stay in the caches between calls.  No figure is a pass / fail bound of any test.  One JSON line per row."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from benchkit import PEAK_HBM_GBS  # noqa: E402
from feathercnn_amd import booster, istft, stft  # noqa: E402
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
        raise SystemExit("istft_bench needs the GPU: nothing is measured without one")
    n, l = args.batch, int(args.seconds * 16000)
    torch.manual_seed(0)
    mfma_tflops, mhz = booster.calibrate_mfma_f32()
    print(json.dumps({"measured_fp32_mfma_TFLOPs": round(mfma_tflops, 1), "shader_mhz": round(mhz), "hbm_peak_GBs": PEAK_HBM_GBS}), flush=True)
    wave = torch.rand((n, l), device="cuda") * 2 - 1
    for n_fft, hop in SHAPES:
        x = stft.spectrogram(wave, n_fft, 0, hop, n_fft, 1)
        _, freqs, frames, _ = x.shape
        basis = torch.from_numpy(istft.basis(n_fft, n_fft, 1)).cuda()
        env = torch.from_numpy(istft.envelope(frames, n_fft, hop, n_fft, 1)).cuda()
        run = lambda out=None: istft.inverse_spectrogram(x, n_fft, hop, n_fft, 1, device_basis=basis, device_envelope=env, out=out)
        y = run()
        us, us_max, iters = rounds_of(lambda: run(y), args.window, args.rounds)
        flops, moved = 2.0 * n * 2 * freqs * frames * n_fft, 4.0 * (x.numel() + y.numel())
        row = {"what": f"n_fft {n_fft} hop {hop}", "n": n, "freqs": freqs, "frames": frames, "out_len": y.shape[1], "kernel": istft.istft_route(n_fft, hop), "us": us,
               "us_max": us_max, "iters": iters, "TFLOPs": round(flops / us / 1e6, 1), "fraction_of_measured_mfma": round(flops / us / 1e6 / mfma_tflops, 3),
               "mfma_bound_us": round(flops / mfma_tflops / 1e6, 1), "hbm_bound_us": round(moved / PEAK_HBM_GBS / 1e3, 1),
               "round_trip_differs_by": float((y - wave[:, :y.shape[1]]).abs().max())}
        if not args.no_torch:
            win = torch.hann_window(n_fft, periodic=True, device="cuda")
            xc = torch.view_as_complex(x)
            trun = lambda: torch.istft(xc, n_fft, hop, n_fft, window=win, center=True)
            yt = trun()
            tus, tus_max, _ = rounds_of(trun, args.window, args.rounds)
            row.update({"torch_istft_us": tus, "torch_istft_us_max": tus_max, "istft_over_torch": round(us / tus, 2), "differs_from_torch_by": float((y - yt).abs().max())})
        print(json.dumps(row), flush=True)
    print(json.dumps({"done": True}))


if __name__ == "__main__":
    main()
