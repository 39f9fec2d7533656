"""The tables of InverseSpectrogram's tests (tests/test_istft_cpu.py, tests/test_istft_gpu.py, tests/test_later_contract_cpu.py): the kernel
of libfeather_istft.so and the cases, against the tiles of feather_istft.h: a block owns 128 slots x 64 phases (a wave 64 x 32) and walks
steps of 4 taps x 16 frequencies.  Every case keeps its window envelope above 1e-11; the smallest kept is 0.0064 (Hamming without center)."""
import functools
import os

import numpy as np

import istft_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "feathercnn_amd", "libfeather_istft.so")
F = np.float32
TOL = 1e-4  # the project's bound on max|y - ref| / max|ref| (stft_cases.TOL)

KERNELS = {"istft_mfma_kernel"}
MFMA = "fhip::istft_mfma_kernel"
case_id = lambda c: "-".join(map(str, c))  # noqa: E731


def targets():
    return {MFMA}  # every instantiation of the library, by the names fhip_istft_route reports


# (n, frames, n_fft, hoplen, winlen, window_type, center, normalized, onesided)
CASES = [
    (1, 1, 2, 2, 2, 0, 0, 0, 1),             # one frame, M = 1, out_len 2
    (3, 2, 10, 1, 7, 2, 1, 0, 1),            # hop 1, M = 10 (three tap groups, the last of two), out_len 1, an odd window in an even transform
    (1, 130, 10, 1, 10, 1, 1, 0, 1),         # hop 1 across a slot-tile edge (129 samples)
    (1, 129, 33, 3, 20, 2, 1, 1, 1),         # odd n_fft, odd hop, 17 frequencies (one past a chunk), normalised by n_fft
    (2, 5, 64, 32, 64, 1, 1, 2, 1),          # hop = a wave's 32 phases, 33 frequencies, normalised by the window
    (1, 257, 64, 16, 64, 1, 1, 0, 1),        # 257 frames, M = 4: one full tap group
    (1, 4, 32, 32, 32, 0, 0, 2, 1),          # hop = n_fft, no overlap, not centred
    (3, 6, 34, 33, 34, 2, 0, 0, 0),          # two-sided, a ragged last tap of one row, hop one past a wave's phases
    (1, 131, 400, 160, 400, 1, 1, 0, 1),     # 201 frequencies, three phase tiles, M = 3 with 80 rows in the last tap
    (1, 3, 1024, 256, 1024, 1, 1, 1, 1),     # 513 frequencies, three frames
    (1, 9, 66, 33, 50, 2, 1, 0, 1),          # a window shorter than n_fft
    (3, 6, 66, 65, 66, 2, 0, 0, 0),          # the two-sided case again with hop one past a block's 64 phases
]


def case_kwargs(case):
    _, _, n_fft, hop, winlen, wt, center, norm, ones = case
    return dict(n_fft=n_fft, hoplen=hop, winlen=winlen, window_type=wt, center=center, normalized=norm, onesided=ones)


@functools.lru_cache(maxsize=None)
def case_data(case):
    """-> (x uniform(-1, 1) float32 [n][freqs][frames][2], the float64 result), shared among the tests, which leave them unchanged."""
    n, frames, n_fft = case[:3]
    freqs = n_fft // 2 + 1 if case[8] else n_fft
    x = np.random.default_rng(19000 + CASES.index(case)).uniform(-1, 1, (n, freqs, frames, 2)).astype(F)
    y = R.inverse_spectrogram(x, **case_kwargs(case))
    x.setflags(write=False), y.setflags(write=False)
    return x, y
