"""include/feather_hip/feather_stft.h restated in numpy float64: ncnn's Spectrogram (the short-time Fourier transform) and UnaryOp."""
import numpy as np

UNARY = {0: np.abs, 1: np.negative, 4: np.square, 5: np.sqrt, 6: lambda v: 1 / np.sqrt(v), 7: np.exp, 8: np.log, 15: lambda v: 1 / v, 17: np.log10}
PAD_MODES = ("constant", "edge", "reflect")


def window(n_fft, winlen=None, window_type=0):
    """The window, zero-padded to n_fft and centred."""
    winlen = n_fft if winlen is None else winlen
    k = np.arange(winlen, dtype=np.float64)
    w = (np.ones(winlen), 0.5 - 0.5 * np.cos(2 * np.pi * k / winlen), 0.54 - 0.46 * np.cos(2 * np.pi * k / winlen))[window_type]
    out = np.zeros(n_fft)
    out[(n_fft - winlen) // 2:(n_fft - winlen) // 2 + winlen] = w
    return out


def scale(n_fft, win, normalized):
    return (1.0, n_fft ** -0.5, (win ** 2).sum() ** -0.5)[normalized]


def dims(l, n_fft, hoplen=None, center=1, onesided=1):
    """-> (freqs, frames)."""
    hoplen = n_fft // 4 if hoplen is None else hoplen
    return n_fft // 2 + 1 if onesided else n_fft, (l + (2 * (n_fft // 2) if center else 0) - n_fft) // hoplen + 1


def basis(n_fft, winlen=None, window_type=0, normalized=0, onesided=1):
    """[2 freqs][n_fft] in float64: row 2f win cos(2 pi f t / N) norm, row 2f + 1 -win sin(2 pi f t / N) norm."""
    win = window(n_fft, winlen, window_type)
    freqs = dims(n_fft, n_fft, 1, 0, onesided)[0]
    phase = 2 * np.pi * ((np.arange(freqs)[:, None] * np.arange(n_fft)[None, :]) % n_fft) / n_fft
    out = np.empty((2 * freqs, n_fft))
    out[0::2], out[1::2] = np.cos(phase) * win, -np.sin(phase) * win
    return out * scale(n_fft, win, normalized)


def spectrogram(x, n_fft, power=0, hoplen=None, winlen=None, window_type=0, center=1, pad_type=2, normalized=0, onesided=1):
    """x [n][L] -> [n][freqs][frames][2] (power 0) or [n][freqs][frames] (1: magnitude, 2: its square)."""
    hoplen = n_fft // 4 if hoplen is None else hoplen
    x = np.asarray(x, np.float64)
    if center:
        x = np.pad(x, ((0, 0), (n_fft // 2, n_fft // 2)), PAD_MODES[pad_type])
    freqs, frames = dims(x.shape[1], n_fft, hoplen, 0, onesided)
    cut = np.stack([x[:, j * hoplen:j * hoplen + n_fft] for j in range(frames)], axis=1)  # [n][frames][n_fft]
    y = np.einsum("mt,njt->nmj", basis(n_fft, winlen, window_type, normalized, onesided), cut)
    re, im = y[:, 0::2], y[:, 1::2]
    return np.stack([re, im], axis=-1) if power == 0 else (np.sqrt(re * re + im * im) if power == 1 else re * re + im * im)


def unary(op, x):
    return UNARY[op](np.asarray(x, np.float64))
