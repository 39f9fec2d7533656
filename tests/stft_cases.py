"""The tables of the audio front end's tests (tests/test_stft_cpu.py, tests/test_stft_gpu.py, tests/test_later_contract_cpu.py): the kernel
instantiations of libfeather_stft.so, the Spectrogram and UnaryOp cases and the inputs of the net-level test.

Shapes are the smallest at which the kernel can go wrong, against the tiles of feather_stft.h: a block owns 64 frequencies x 128 frames and
walks chunks of 32 taps.  n_fft 2, 10, 33 (odd, and one tap past a chunk), 34, 64, 400 and 1024 (13 and 32 chunks); frames 1, 127, 129 and 257;
freqs 2, 17, 33 (one past half a tile's rows), 201 (four tiles) and two-sided; hops 1, 3 (odd), 32 (a chunk: every phase row full), 160,
n_fft itself and past n_fft; every pad type, reflect at the shortest legal row; windows shorter than n_fft, odd and even."""
import functools
import os

import numpy as np

import stft_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "feathercnn_amd", "libfeather_stft.so")
F = np.float32
TOL = 1e-4  # tests/test_net_gpu.py's bound on max|y - ref| / max|ref|

KERNELS = {"stft_mfma_kernel", "unary_kernel"}
MFMA, VECTOR, SCALAR = "fhip::stft_mfma_kernel", "fhip::unary_kernel<1>", "fhip::unary_kernel<0>"


def targets():
    """Every instantiation of the library, by the names fhip_stft_route reports."""
    return {MFMA, VECTOR, SCALAR}


# (n, L, n_fft, power, hoplen, winlen, window_type, center, pad_type, normalized, onesided, floats off a 16-byte boundary)
CASES = [
    (1, 2, 2, 0, 1, 2, 0, 0, 2, 0, 1, 0),            # one frame, two frequencies
    (3, 128, 10, 1, 1, 7, 1, 1, 2, 0, 1, 1),         # hop 1, 129 frames, an odd window in an even transform
    (1, 379, 33, 2, 3, 20, 2, 1, 1, 1, 1, 0),        # odd n_fft, one tap past a chunk; 127 frames; replicate
    (1, 8192, 64, 0, 32, 64, 1, 1, 2, 0, 1, 2),      # 33 frequencies, 257 frames, hop = a chunk
    (1, 128, 32, 1, 32, 31, 1, 0, 2, 2, 1, 0),       # 17 frequencies, hop = n_fft, not centred
    (3, 200, 34, 0, 40, 34, 2, 1, 0, 0, 0, 3),       # two-sided, hop past n_fft, zero padding
    (1, 800, 400, 2, 160, 400, 1, 1, 2, 0, 1, 1),    # 201 frequencies, 13 chunks
    (1, 513, 1024, 1, 256, 1024, 1, 1, 2, 1, 1, 0),  # 32 chunks; reflect at the shortest legal row
]
UNARY_OPS = (0, 1, 4, 5, 6, 7, 8, 15, 17)
UNARY_COUNTS = (1, 3, 4, 1027)


def case_id(c):
    return "-".join(str(v) for v in c)


def case_kwargs(case):
    _, _, n_fft, power, hop, winlen, wt, center, pad, norm, ones, _ = case
    return dict(n_fft=n_fft, power=power, hoplen=hop, winlen=winlen, window_type=wt, center=center, pad_type=pad, normalized=norm, onesided=ones)


@functools.lru_cache(maxsize=None)
def spectrogram_case(case):
    """-> (x, the float64 result), shared among the tests, which leave them unchanged."""
    x = np.random.default_rng(16000 + CASES.index(case)).uniform(-1, 1, case[:2]).astype(F)
    y = R.spectrogram(x, **case_kwargs(case))
    x.setflags(write=False), y.setflags(write=False)
    return x, y


@functools.lru_cache(maxsize=None)
def unary_case(op, count):
    """-> (x, the float64 result): positive where the op needs it, away from zero for the reciprocal."""
    x = np.random.default_rng(16500 + 100 * op + count).uniform(0.25, 4, count).astype(F)
    if op in (0, 1, 4, 7, 15):
        x = (x * np.where(np.arange(count) % 2, -1, 1)).astype(F)
    return x, R.unary(op, x)


# ---- net level -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def net_model():
    """-> ((param, bin, input, output), the trace for model_zoo.numpy_forward) of tiny_audio."""
    from feathercnn_amd import model_zoo
    trace = []
    return model_zoo.tiny_audio(trace=trace), trace


@functools.lru_cache(maxsize=None)
def net_input(batch=3):
    """-> (x, every blob of the numpy forward)."""
    from feathercnn_amd import model_zoo
    (p, b, i, o), trace = net_model()
    x = np.random.default_rng(17000 + batch).uniform(-1, 1, (batch, 1, 1, 70)).astype(F)
    return x, model_zoo.numpy_forward(trace, i, x)


NET_SHAPES = {"complex": (9, 18, 2), "magnitude": (1, 6, 24), "power": (1, 12, 15), "floor": (1, 12, 15), "log": (1, 12, 15), "gaps": (1, 5, 7), "root": (1, 5, 7)}
