/* feather_stft.h -- C-ABI of libfeather_stft.so: ncnn's Spectrogram (the short-time Fourier transform of a waveform) and UnaryOp on the
 * MI355X (gfx950), on fp32 tensors with a leading batch.
 *
 * The reference has neither layer and ncnn's source was not at hand: this text is the definition (the parameter ids are ncnn's
 * Spectrogram as recalled; INTEGRATION.md records that).  tests/stft_ref.py restates it in float64 and is held against torch.stft.
 *
 * Spectrogram    x is [n] rows of L floats, row i at element i * L.  Parameters (ncnn id, default):
 *                  n_fft (0)            transform length, 2 <= n_fft <= FHIP_STFT_MAX_NFFT
 *                  power (1, 0)         0 complex, 1 magnitude, 2 squared magnitude
 *                  hoplen (2, n_fft/4)  samples between frames, >= 1; hoplen > n_fft is legal (frames with gaps)
 *                  winlen (3, n_fft)    1 <= winlen <= n_fft; the window is zero-padded to n_fft, centred: left pad (n_fft - winlen) / 2
 *                  window_type (4, 0)   0 ones, 1 Hann 0.5 - 0.5 cos(2 pi k / winlen), 2 Hamming 0.54 - 0.46 cos(2 pi k / winlen) (periodic)
 *                  center (5, 1)        the signal is padded by n_fft / 2 on both sides first
 *                  pad_type (6, 2)      0 zeros, 1 replicate, 2 reflect (the edge sample not repeated; needs n_fft / 2 < L)
 *                  normalized (7, 0)    0 none, 1 times n_fft^-1/2, 2 times (sum window^2)^-1/2
 *                  onesided (8, 1)      freqs = n_fft / 2 + 1, else n_fft
 *                L' = L + 2 (n_fft / 2) with center, else L; frames = (L' - n_fft) / hoplen + 1;
 *                X[f][j] = sum_t x'[j * hoplen + t] * win[t] * e^(-2 pi i f t / n_fft) * norm.
 *                power 0: y[n][freqs][frames][2] (re, im); power 1: y[n][freqs][frames] = sqrtf(re^2 + im^2); power 2: re^2 + im^2.
 *                The sum is fp32 (v_mfma_f32_32x32x2_f32, an fmaf chain over the taps in a fixed order); re^2 + im^2 is two roundings.
 * Basis          fhip_stft_basis fills, on the HOST, [2 * freqs][n_fft] floats: row 2f is win[t] cos(2 pi f t / n_fft) norm, row 2f + 1 is
 *                -win[t] sin(2 pi f t / n_fft) norm, computed in double with the phase reduced as (f * t) mod n_fft in integers, rounded
 *                once.  It is a pure function; the caller uploads the array once (the Net at Init) and passes the device copy to every
 *                forward call: the window and the normalisation cost nothing at run time.
 * UnaryOp        y[i] = op(x[i]): 0 fabsf, 1 -x, 4 x * x, 5 sqrtf, 6 1 / sqrtf(x), 7 expf, 8 logf, 15 1 / x, 17 log10f (ncnn's op ids; no
 *                others).  y == x (in place) is allowed; any other overlap is refused.
 *
 * Kernels (fhip_stft_route).  One launch per call, nothing allocated, copied or waited for on the host; capturable in a hipGraph.
 *   stft_mfma_kernel   every Spectrogram: a GEMM of the 2 * freqs basis rows x (n * frames) columns over K = n_fft.  A block of four waves owns
 *                      one image, FHIP_STFT_TILE_F frequencies (twice as many basis rows) and FHIP_STFT_TILE_J frames; a wave a 2 x 2 grid of
 *                      32 x 32 tiles.  Per chunk of FHIP_STFT_CHUNK taps it stages the basis rows [2 TILE_F][CHUNK] and the signal SPLIT BY
 *                      PHASE: S[r][q] = x'[(j0 + q) * hop + k0 + r] for r < min(CHUNK, hop) -- the phases a chunk populates -- and
 *                      q < TILE_J + (CHUNK - 1) / hop, so that tap t of frame j is S[t % hop][j + t / hop]: the 32 lanes of a column
 *                      read consecutive words for every hop, a sample is held once however many frames share it, and hop > n_fft needs
 *                      nothing special.  The padding (zero, replicate, reflect) is an index map in that loader; no padded or framed copy
 *                      of the waveform exists.  Taps past n_fft and rows past 2 * freqs are zeros, frames past the last masked stores.
 *                      The next chunk waits in registers while the current one multiplies.  Real and imaginary rows are interleaved,
 *                      so re and im of one (f, j) are adjacent accumulator registers of one lane: the powers are in-lane epilogues and
 *                      the complex form one 8-byte store.
 *   unary_kernel<V>    16 bytes a lane where x and y are 16-byte aligned (V = 1) with a scalar tail, else scalar; the op a uniform switch.
 *
 * Refused with FHIP_E_BADARG before any device call, naming the argument: n_fft < 2 or > FHIP_STFT_MAX_NFFT (the limit of the host
 * basis the callers hold, not of the kernel's LDS, which is independent of n_fft); hoplen < 1; winlen outside [1, n_fft]; an unknown
 * window_type, pad_type, normalized or power; L' < n_fft; reflect with n_fft / 2 >= L; frames other than the definition's; any tensor of
 * 2^31 elements or more; NULL or 4-byte-unaligned pointers; y overlapping x; an unknown UnaryOp id.
 * A sample that is not finite reaches only frames whose window, rounded up to a whole chunk of taps, holds it.
 *
 * Out of scope: InverseSpectrogram, an FFT, bf16 / fp16, a fused mel projection or log, the remaining UnaryOp ids.  The library is separate
 * from libfeather_hip.so and needs nothing from it but the enums of feather_hip.h; it keeps its own last-error slot. */
#ifndef FEATHER_HIP_FEATHER_STFT_H_
#define FEATHER_HIP_FEATHER_STFT_H_

#include <stddef.h>

#include "feather_hip/feather_hip.h"

#ifdef __cplusplus
extern "C"
{
#endif

#define FHIP_STFT_API __attribute__((visibility("default")))

/* Route code fhip_net_layer_info reports for the layers of a net with fhip_net_set_audio (feather_net.h). */
#define FHIP_STFT_NET_ROUTE 118

#define FHIP_STFT_MAX_NFFT 4096 /* the longest transform */
#define FHIP_STFT_TILE_F 64     /* frequencies per block (128 interleaved basis rows: four 32-row tiles) */
#define FHIP_STFT_TILE_J 128    /* frames per block (four 32-column tiles) */
#define FHIP_STFT_CHUNK 32      /* taps staged per step */

#define FHIP_UNARY_ABS 0
#define FHIP_UNARY_NEG 1
#define FHIP_UNARY_SQUARE 4
#define FHIP_UNARY_SQRT 5
#define FHIP_UNARY_RSQRT 6
#define FHIP_UNARY_EXP 7
#define FHIP_UNARY_LOG 8
#define FHIP_UNARY_RECIPROCAL 15
#define FHIP_UNARY_LOG10 17

/* freqs and frames of a Spectrogram of rows of l samples.  FHIP_E_BADARG: what the list above refuses among these arguments. */
FHIP_STFT_API int fhip_stft_output_dim(int l, int n_fft, int hoplen, int center, int pad_type, int onesided, int* freqs, int* frames);

/* The basis defined above into HOST memory basis[2 * freqs][n_fft]; capacity in floats.  A pure function: no device call. */
FHIP_STFT_API int fhip_stft_basis(int n_fft, int winlen, int window_type, int normalized, int onesided, float* basis, long long capacity);

/* y = the Spectrogram of x[n][l] on `stream` (a hipStream_t as void*).  basis: the DEVICE copy of fhip_stft_basis's array for the same
 * n_fft and onesided.  frames: what fhip_stft_output_dim gives.  y: [n][freqs][frames][2] (power 0) or [n][freqs][frames]. */
FHIP_STFT_API int fhip_stft_forward(int n, int l, int n_fft, int power, int hoplen, int center, int pad_type, int onesided, const float* x,
                                    const float* basis, float* y, int frames, void* stream);

/* y[i] = op(x[i]) for i < count on `stream`; y == x is allowed. */
FHIP_STFT_API int fhip_unary_forward(int op, float* y, const float* x, long long count, void* stream);

/* The kernel instantiation a call would launch, as the demangled name without return type and parameters, copied into name[len]:
 *   "fhip::stft_mfma_kernel"   what == 0: a Spectrogram of n_fft = a, hoplen = b (every accepted one: there is no second kernel)
 *   "fhip::unary_kernel<1>"    what == 1: a UnaryOp of op a whose pointers are 16-byte aligned (b != 0)
 *   "fhip::unary_kernel<0>"    what == 1, b == 0
 * FHIP_E_BADARG: NULL name, len < 1, another `what`, arguments the forward call would refuse. */
FHIP_STFT_API int fhip_stft_route(int what, int a, int b, char* name, int len);

/* Message of this thread's last failing call of this library ("" if none). */
FHIP_STFT_API const char* fhip_stft_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* FEATHER_HIP_FEATHER_STFT_H_ */
