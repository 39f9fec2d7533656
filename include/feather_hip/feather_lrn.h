/* feather_lrn.h -- C-ABI of libfeather_lrn.so: local response normalisation (Caffe's and ncnn's LRN) of fp32 planes on the MI355X (gfx950),
 * alone and with the Pooling layer behind it in one launch: the layer of AlexNet, CaffeNet and GoogLeNet (Inception v1).
 *
 * The reference has no such layer.  This text is the definition, on dense NCHW fp32 with a leading batch; every image is normalised on its
 * own.
 *
 *   parameters, as ncnn writes them: 0 = region_type (0 across channels, 1 within channel), 1 = local_size (default 5), 2 = alpha (1),
 *                  3 = beta (0.75), 4 = bias (1).  local_size is odd and at least 1: Caffe refuses an even size and ncnn's loop gives an
 *                  even size local_size + 1 taps, so an even size has no agreed meaning.
 *   every step in fp32, each product and sum rounded on its own (no fused multiply-add):
 *                  q = x * x
 *   across         s[c] = the sum of q[c'] over c' in [c - local_size / 2, c + local_size / 2] intersected with [0, C), at the same pixel,
 *                  added in ascending c' starting from 0.f;  a = alpha / local_size
 *   within         s = the sum of q over the local_size x local_size window centred on the pixel, in the same plane; pixels outside the
 *                  plane count as zero; rows ascending, columns ascending within a row, starting from 0.f;
 *                  a = alpha / (local_size * local_size): the divisor is always the full window, as in Caffe and ncnn
 *   both           a is divided on the host in float.   d = bias + a * s  (the product, then the sum)
 *                  y = x * pow(d, -beta)
 *   The order of the sum is part of the definition: every kernel of the library adds in it, so all of them agree with each other bit for
 *   bit (a running add / subtract sum would not).  Squares are not negative, so a tap outside the tensor may be added as 0.f.
 *   pow            the one step that is not pinned to the bit.  In every kernel of the library it is the same function of (d, beta):
 *                  beta == 0.75f:  1.f / (r * sqrtf(r)) with r = sqrtf(d);   beta == 0.5f:  1.f / sqrtf(d);   else the device powf(d, -beta).
 *                  sqrtf and the division are correctly rounded; the two short forms stay within 3 ulp of the exact power, powf within the
 *                  16 ulp OpenCL allows it.
 *   d > 0          is guaranteed statically: bias > 0 and alpha >= 0 are required (with bias <= 0 or alpha < 0 some input makes d <= 0, where
 *                  pow has a pole or no real value), and refused otherwise.
 *
 *   LRN -> Pooling fhip_lrn_pool_forward computes fhip_pooling(fhip_lrn_forward(in)) (feather_net.h) without writing the normalised tensor.
 *                  Every LRN value is computed as above; window, padding quirk (origin = o * stride - pad_top - pad_bottom), clipping,
 *                  ceil-mode output size, the max (`m > v ? m : v` from -FLT_MAX) and the average (sum in rows ascending, columns ascending,
 *                  divided by the number of taps inside the plane) are fhip_pooling's generic kernel's: the result equals the two calls bit
 *                  for bit (a maximum that is zero may differ in sign from fhip_pooling's 3x3 / stride-2 kernel where a window holds
 *                  zeros of both signs).  Global pooling is refused, and so is a window that covers the whole unpadded plane (output 1 x 1, no
 *                  pads, kernel_h >= h and kernel_w >= w): fhip_pooling sums such a window in the order of its plane-reduce kernels, which
 *                  this library does not restate.
 *
 * No atomics: results are bit-identical from run to run.  No entry allocates, copies or synchronises: every one is hipGraph-capturable.
 * Pointers need 4-byte alignment only.  The layer is not in place: out must not overlap in.
 *
 * Size limits (every entry point): FHIP_E_BADARG for a tensor of 2^31 elements or more, input or output; and for a launch of more than
 * 2^24 - 1 blocks (a launch takes fewer than 2^32 lanes): across channels n * ceil(h * w / 1024) blocks -- thin tensors such as
 * [2^24][c][1][1] -- and in fhip_lrn_pool_forward n * chunks of channels * bands of pooled rows; fhip_lrn_forward across channels also for more
 * than 65535 chunks of channels (c above 1048560).
 *
 * The library is separate from libfeather_hip.so and needs nothing from it but the enums of feather_hip.h (fhip_error) and the struct
 * fhip_pool_param of feather_net.h: link or dlopen either or both.  It keeps its own last-error slot. */
#ifndef FEATHER_HIP_FEATHER_LRN_H_
#define FEATHER_HIP_FEATHER_LRN_H_

#include <stddef.h>

#include "feather_hip/feather_hip.h"
#include "feather_hip/feather_net.h"

#ifdef __cplusplus
extern "C"
{
#endif

#define FHIP_LRN_API __attribute__((visibility("default")))

/* `region` of every entry: ncnn's region_type. */
enum fhip_lrn_region
{
    FHIP_LRN_ACROSS_CHANNELS = 0,
    FHIP_LRN_WITHIN_CHANNEL = 1
};

/* Channels one block of the across-channel kernel marches through on a grid that fills the chip (see fhip_lrn_route: 8 or 4 on small
 * grids); likewise the channels of one block of the fused kernel. */
#define FHIP_LRN_CHUNK 16
/* Floats of LDS one block of the fused kernel "fhip::lrn_pool_lds_kernel" holds at most: FHIP_LRN_CHUNK channels of a band of input rows. */
#define FHIP_LRN_POOL_LDS_FLOATS 8192

/* out[n][c][h][w] = LRN(in[n][c][h][w]) as defined above: one launch on `stream` (a hipStream_t as void*).
 * Size limit: 2^31 elements or more (n * c * h * w) is FHIP_E_BADARG.
 * FHIP_E_BADARG: region outside 0 / 1, local_size < 1 or even, alpha / beta / bias not finite, bias <= 0 or alpha < 0 (d > 0 could not be
 * guaranteed), a dimension < 1, 2^31 elements or more, more than 2^24 - 1 blocks or 65535 chunks (the size limits above), NULL out / in, a
 * pointer that is not 4-byte aligned, out overlapping in.
 * FHIP_E_HIP: the launch failed. */
FHIP_LRN_API int fhip_lrn_forward(int region, int local_size, float alpha, float beta, float bias, int n, int c, int h, int w, float* out, const float* in,
                                  void* stream);

/* fhip_lrn_forward across channels with the channel split given instead of selected (measurements and tests): `chunk` = the channels one
 * block marches through, 0 = all of them (no split).  Every value of chunk gives the same bits.  FHIP_E_BADARG in addition: region != 0,
 * chunk < 0, more than 65535 chunks. */
FHIP_LRN_API int fhip_lrn_forward_chunked(int local_size, float alpha, float beta, float bias, int n, int c, int h, int w, int chunk, float* out, const float* in,
                                          void* stream);

/* The kernel instantiation fhip_lrn_forward launches for these arguments (the same selection; the pointers are only looked at for their
 * alignment, NULL counts as aligned), as the demangled name without return type and parameters, copied into name[len]:
 *   "fhip::lrn_across_kernel<V, L>"   across channels.  A lane owns four pixels of an image and marches along the channels, keeping the last
 *                                     L values in registers, so every element is read once, coalesced.  V = 4: the four pixels are adjacent,
 *                                     one 16-byte access, when h * w % 4 == 0 and both pointers are 16-byte aligned; else V = 1: they are
 *                                     256 pixels apart, four 4-byte accesses.  L = local_size for 3 and 5; L = 0 for every other size, which
 *                                     re-reads its taps (they hit the caches).  A block owns 1024 pixels of an image and a chunk of channels:
 *                                     FHIP_LRN_CHUNK (16), halved to 8 and to 4 while the grid n * ceil(h * w / 1024) * ceil(c / chunk) stays
 *                                     below 2048 blocks.  A chunk re-reads a halo of local_size / 2 channels on each side
 *                                     (fhip_lrn_forward_chunked takes another split; every split gives the same bits).
 *   "fhip::lrn_within_kernel"         within channel: one element per lane, a direct sum over the clipped window. */
FHIP_LRN_API int fhip_lrn_route(int region, int local_size, int n, int c, int h, int w, const float* out, const float* in, char* name, int len);

/* out[n][c][oh][ow] = fhip_pooling(pool, LRN(in[n][c][h][w])) bit for bit, in one launch that never writes the normalised tensor; (oh, ow) =
 * fhip_pooling_output_dim(pool).  pool->channels / input_h / input_w must equal c / h / w.
 * Size limit: 2^31 elements or more in `in` or `out` is FHIP_E_BADARG.
 * FHIP_E_BADARG: everything fhip_lrn_forward refuses; pool NULL, its channels / input_h / input_w other than c / h / w, global_pooling set, a
 * kernel or stride < 1, a negative pad, an output dimension < 1, a window that covers the whole unpadded plane, more than 2^24 - 1 blocks.  (out cannot sensibly overlap in either: refused too.) */
FHIP_LRN_API int fhip_lrn_pool_forward(int region, int local_size, float alpha, float beta, float bias, int n, int c, int h, int w,
                                       const fhip_pool_param* pool, float* out, const float* in, void* stream);

/* The instantiation fhip_lrn_pool_forward launches:
 *   "fhip::lrn_pool_lds_kernel<L>"    across channels, where FHIP_LRN_CHUNK channels of kernel_h input rows fit FHIP_LRN_POOL_LDS_FLOATS
 *                                     (16 * kernel_h * w <= 8192).  A block computes the LRN values of a band of input rows for 16 channels
 *                                     into LDS once -- lanes along the pixels of the band, marching along the channels as above, L as above
 *                                     -- and pools from LDS; only the rows two bands share are computed twice.  A band is as many pooled
 *                                     rows B as fit: (B - 1) * stride_h + kernel_h <= 8192 / (16 * w) input rows.  The channels of a block are
 *                                     16, halved to 8 and to 4 while the grid n * bands * ceil(c / channels) stays below 2048 blocks.
 *   "fhip::lrn_pool_direct_kernel"    everything else (within channel; planes too wide for a band): one pooled output per lane, every LRN
 *                                     value of its window computed on the spot. */
FHIP_LRN_API int fhip_lrn_pool_route(int region, int local_size, int n, int c, int h, int w, const fhip_pool_param* pool, const float* out, const float* in,
                                     char* name, int len);

/* Message of this thread's last failing call of this library ("" if none). */
FHIP_LRN_API const char* fhip_lrn_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* FEATHER_HIP_FEATHER_LRN_H_ */
