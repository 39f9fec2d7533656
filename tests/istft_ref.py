"""include/feather_hip/feather_istft.h restated in numpy float64: ncnn's InverseSpectrogram, as the plain overlap-add of windowed inverse
transforms (not the gather the kernel runs)."""
import numpy as np

from stft_ref import scale, window


def basis(n_fft, winlen=None, window_type=0, normalized=0, onesided=1):
    """Binv[n_fft][2 freqs]: column 2f win / N norm c_f cos(2 pi f t / N), column 2f + 1 -win / N norm c_f sin(2 pi f t / N); one-sided, the
    imaginary columns of DC and Nyquist are zeros."""
    win = window(n_fft, winlen, window_type)
    freqs = n_fft // 2 + 1 if onesided else n_fft
    f = np.arange(freqs)
    edge = (f == 0) | (2 * f == n_fft) if onesided else np.zeros(freqs, bool)
    cf = np.where(edge, 1.0, 2.0) if onesided else np.ones(freqs)
    phase = 2 * np.pi * ((np.arange(n_fft)[:, None] * f[None, :]) % n_fft) / n_fft
    out = np.empty((n_fft, 2 * freqs))
    out[:, 0::2], out[:, 1::2] = np.cos(phase) * cf, -np.sin(phase) * np.where(edge, 0.0, cf)
    return out * (win / n_fft / scale(n_fft, win, normalized))[:, None]


def envelope(frames, n_fft, hoplen=None, winlen=None, window_type=0, center=1):
    """env[s0 + i], i < out_len: the sum of the squared windows of the frames that hold the sample (center trims s0 = n_fft / 2 at both ends)."""
    hoplen = n_fft // 4 if hoplen is None else hoplen
    env = np.zeros((frames - 1) * hoplen + n_fft)
    for j in range(frames):
        env[j * hoplen:j * hoplen + n_fft] += window(n_fft, winlen, window_type) ** 2
    s0 = n_fft // 2 if center else 0
    return env[s0:len(env) - s0]


def inverse_spectrogram(x, n_fft, hoplen=None, winlen=None, window_type=0, center=1, normalized=0, onesided=1):
    """x [n][freqs][frames][2] -> [n][out_len]."""
    hoplen = n_fft // 4 if hoplen is None else hoplen
    x = np.asarray(x, np.float64)
    n, freqs, frames, _ = x.shape
    z = np.einsum("tk,nkj->njt", basis(n_fft, winlen, window_type, normalized, onesided), x.transpose(0, 1, 3, 2).reshape(n, 2 * freqs, frames))
    full = np.zeros((n, (frames - 1) * hoplen + n_fft))
    for j in range(frames):
        full[:, j * hoplen:j * hoplen + n_fft] += z[:, j]
    s0 = n_fft // 2 if center else 0
    return full[:, s0:full.shape[1] - s0] / envelope(frames, n_fft, hoplen, winlen, window_type, center)
