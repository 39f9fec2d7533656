/* feather_istft.h -- C-ABI of libfeather_istft.so: ncnn's InverseSpectrogram (the inverse short-time Fourier transform: a complex
 * spectrogram back to a waveform) on the MI355X (gfx950), on fp32 tensors with a leading batch.  The twin of feather_stft.h.
 *
 * The reference has no such layer and ncnn's source was not at hand: this text is the definition (the parameter ids are ncnn's
 * InverseSpectrogram as recalled; INTEGRATION.md records that).  tests/istft_ref.py restates it in float64 and is held against torch.istft.
 *
 * InverseSpectrogram   x is [n][freqs][frames][2] (re, im), Spectrogram's power-0 output.  Parameters (ncnn id, default):
 *                  n_fft (0)            transform length, 2 <= n_fft <= FHIP_ISTFT_MAX_NFFT
 *                  returns (1, 1)       1 the real waveform; 0 (complex) and 2 (imaginary) are refused
 *                  hoplen (2, n_fft/4)  samples between frames, >= 1
 *                  winlen (3, n_fft)    1 <= winlen <= n_fft; the window is zero-padded to n_fft, centred: left pad (n_fft - winlen) / 2
 *                  window_type (4, 0)   0 ones, 1 Hann 0.5 - 0.5 cos(2 pi k / winlen), 2 Hamming 0.54 - 0.46 cos(2 pi k / winlen) (periodic)
 *                  center (5, 1)        n_fft / 2 samples are trimmed from both ends (what Spectrogram's padding added)
 *                  normalized (7, 0)    undoes Spectrogram's: 0 none, 1 times n_fft^1/2, 2 times (sum window^2)^1/2
 *                onesided is an argument here: freqs = n_fft / 2 + 1, else n_fft.  (A net reads it off the bottom's extent.)
 *                z_j[t] = win[t] / n_fft * norm * sum_f c_f (Re X[f][j] cos(2 pi f t / n_fft) - Im X[f][j] sin(2 pi f t / n_fft)), t < n_fft;
 *                two-sided c_f = 1; one-sided c_f = 2 except c_0 = 1 and, for even n_fft, c_(n_fft / 2) = 1, and the imaginary parts of
 *                those two are ignored (as irfft does);
 *                full[s] = sum_j z_j[s - j hoplen];  env[s] = sum_j win[s - j hoplen]^2;  s0 = center ? n_fft / 2 : 0;
 *                out_len = (frames - 1) hoplen + n_fft - (center ? 2 (n_fft / 2) : 0);  y[n][out_len]: y[i] = full[s0 + i] / env[s0 + i].
 * Basis          fhip_istft_basis fills, on the HOST, Binv[n_fft][2 freqs] floats: Binv[t][2f] = win[t] / n_fft norm c_f cos(2 pi f t / n_fft),
 *                Binv[t][2f + 1] = -win[t] / n_fft norm c_f sin(2 pi f t / n_fft), the two ignored columns zeros; computed in double with the
 *                phase reduced as (f * t) mod n_fft in integers, rounded once.  A pure function; the caller uploads it once.
 * Envelope       fhip_istft_envelope fills, on the HOST, inv_env[out_len] = 1 / env[s0 + i] in double, rounded once, and refuses, naming the
 *                first such sample, if a kept env is below 1e-11 (torch.istft's bound): hoplen > winlen, or a Hann window without center.
 *                It depends on frames: a caller re-makes it when the number of frames changes.
 *
 * Kernel (fhip_istft_route).  One launch per call, nothing allocated, copied or waited for on the host; capturable in a hipGraph.
 *   istft_mfma_kernel  With s = q hoplen + r (slot q, phase r < hoplen), M = ceil(n_fft / hoplen) and K = 2 freqs,
 *                        full[q hoplen + r] = sum_{m < M} sum_{k < K} Binv[m hoplen + r][k] X[k][q - m]:
 *                      a 1-D convolution along frames with K input channels, hoplen output channels and M taps, then an interleave of the
 *                      phases.  The overlap-add is the sum over m and happens in the accumulator of v_mfma_f32_32x32x2_f32: no atomics, no
 *                      second pass, no workspace, every output sample written once by one lane.  The k = 2 of the instruction is the (re, im)
 *                      pair of one frequency.  A block of four waves owns one image, FHIP_ISTFT_TILE_Q slots and FHIP_ISTFT_TILE_R phases; a
 *                      wave 64 slots x 32 phases, two 32 x 32 tiles that share the B operand.  The tile is slots x phases, so the 32 lanes
 *                      of a store run along r, the contiguous axis of y.  The reduction is walked in steps of (a group of FHIP_ISTFT_TAPS
 *                      taps) x (a chunk of FHIP_ISTFT_CHUNK frequencies).  Per step the block stages X once, as a re plane and an im
 *                      plane, for the slots q0 - (TAPS - 1) .. q0 + TILE_Q - 1 of the group -- every shift of the group reads that one
 *                      copy at an offset, so a spectrogram value is held once however many output slots share it; M <= TAPS (every hop
 *                      >= n_fft / 4) is one group: X is staged once per chunk -- and the basis rows m hoplen + r of the phases it owns.
 *                      Frames outside [0, frames), rows t >= n_fft (the ragged last tap), phases >= hoplen and frequencies >= freqs
 *                      are zeros in the loaders; no padded or re-laid copy of x exists.  A block walks only the taps that reach its
 *                      phases, ceil((n_fft - r0) / hoplen).  The next step waits in registers while the current one multiplies.  The
 *                      order of the sum (groups, then chunks, then taps, then frequencies) is fixed.  The epilogue multiplies by
 *                      inv_env, applies the center trim as an index shift and stores under a mask.
 *                      Known idle work: hoplen < 32 leaves most of a phase tile idle (hoplen 1: 31 of 32 columns), and the work per
 *                      sample is the dense 2 freqs n_fft multiply-adds where an inverse FFT needs O(log n_fft).  A narrow-hop variant
 *                      and an inverse FFT are out of scope.
 *
 * Refused with FHIP_E_BADARG before any device call, naming the argument: n_fft < 2 or > FHIP_ISTFT_MAX_NFFT; hoplen < 1; winlen outside
 * [1, n_fft]; an unknown window_type or normalized; frames < 1; out_len < 1 (one frame with center) or another out_len than the
 * definition's; a kept envelope sample below 1e-11; any tensor of 2^31 elements or more; NULL or 4-byte-unaligned pointers; y overlapping x.
 *
 * Out of scope: an inverse FFT, returns 0 and 2, a length argument, bf16 / fp16, a narrow-hop kernel, a mask multiply in the loader.  The
 * library is separate from libfeather_hip.so and libfeather_stft.so and needs nothing but the enums of feather_hip.h; it keeps its own
 * last-error slot. */
#ifndef FEATHER_HIP_FEATHER_ISTFT_H_
#define FEATHER_HIP_FEATHER_ISTFT_H_

#include <stddef.h>

#include "feather_hip/feather_hip.h"

#ifdef __cplusplus
extern "C"
{
#endif

#define FHIP_ISTFT_API __attribute__((visibility("default")))

/* Route code fhip_net_layer_info reports for an InverseSpectrogram layer of a net with fhip_net_set_audio (feather_net.h). */
#define FHIP_ISTFT_NET_ROUTE 119

#define FHIP_ISTFT_MAX_NFFT 4096 /* the longest transform */
#define FHIP_ISTFT_TILE_Q 128    /* slots per block (four 32-row tiles) */
#define FHIP_ISTFT_TILE_R 64     /* phases per block (two 32-column tiles) */
#define FHIP_ISTFT_CHUNK 16      /* frequencies staged per step */
#define FHIP_ISTFT_TAPS 4        /* taps (frame shifts) that read one staged copy of X */

/* out_len of an InverseSpectrogram of `frames` frames.  FHIP_E_BADARG: what the list above refuses among these arguments. */
FHIP_ISTFT_API int fhip_istft_output_dim(int frames, int n_fft, int hoplen, int center, int* out_len);

/* The basis defined above into HOST memory basis[n_fft][2 * freqs]; capacity in floats.  A pure function: no device call. */
FHIP_ISTFT_API int fhip_istft_basis(int n_fft, int winlen, int window_type, int normalized, int onesided, float* basis, long long capacity);

/* The inverse envelope defined above into HOST memory inv_env[out_len]; capacity in floats.  A pure function: no device call. */
FHIP_ISTFT_API int fhip_istft_envelope(int frames, int n_fft, int hoplen, int winlen, int window_type, int center, float* inv_env, long long capacity);

/* y[n][out_len] = the InverseSpectrogram of x[n][freqs][frames][2] on `stream` (a hipStream_t as void*).  basis, inv_env: the DEVICE copies
 * of fhip_istft_basis's and fhip_istft_envelope's arrays for the same arguments.  out_len: what fhip_istft_output_dim gives. */
FHIP_ISTFT_API int fhip_istft_forward(int n, int frames, int n_fft, int hoplen, int center, int onesided, const float* x, const float* basis,
                                      const float* inv_env, float* y, int out_len, void* stream);

/* The kernel a call of n_fft and hoplen would launch, as the demangled name without return type and parameters, copied into name[len]:
 * "fhip::istft_mfma_kernel" for every accepted call (there is no second kernel).  FHIP_E_BADARG: NULL name, len < 1, n_fft or hoplen out of range. */
FHIP_ISTFT_API int fhip_istft_route(int n_fft, int hoplen, char* name, int len);

/* Message of this thread's last failing call of this library ("" if none). */
FHIP_ISTFT_API const char* fhip_istft_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* FEATHER_HIP_FEATHER_ISTFT_H_ */
