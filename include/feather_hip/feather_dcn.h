/* feather_dcn.h -- C-ABI of libfeather_dcn.so: deformable convolution (DCN v1 and v2, ncnn's DeformableConv2D) on the MI355X (gfx950), on
 * dense fp32 NCHW tensors with a leading batch.
 *
 * The reference has no such layer: this text is the definition, written from what ncnn's deformableconv2d.cpp does.  tests/dcn_ref.py
 * restates it in float64.
 *
 * Tensors        x [n][C][H][W]; offset [n][G * 2 * kh * kw][Ho][Wo]; mask [n][G * kh * kw][Ho][Wo] or NULL (DCN v1: every mask value is
 *                1); y [n][K][Ho][Wo].  G, the number of offset groups, is >= 1 and divides C: ncnn's layer has G = 1, mmcv's
 *                deform_groups are G > 1.  The convolution group is 1.
 * Output size    Ho = (H + pad_top + pad_bottom - (dil_h * (kh - 1) + 1)) / stride_h + 1, Wo likewise (fhip_dcn_output_dim).
 * Sample         tap t = i * kw + j of input channel c, whose offset group is g = c / (C / G), at output pixel (ho, wo):
 *                  dy = offset[(g * kh * kw + t) * 2][ho][wo], dx = offset[(g * kh * kw + t) * 2 + 1][ho][wo],
 *                  py = float(ho * stride_h - pad_top + i * dil_h) + dy, px = float(wo * stride_w - pad_left + j * dil_w) + dx  (fp32).
 *                The sample is 0 unless py > -1 && px > -1 && py < H && px < W.  Otherwise, with y0 = floor(py), x0 = floor(px),
 *                ly = py - y0, lx = px - x0, it is the sum over the corners (y0, x0), (y0, x0 + 1), (y0 + 1, x0), (y0 + 1, x0 + 1), in that
 *                order, of weight * x[c][corner]; the weights are (1 - ly)(1 - lx), (1 - ly) lx, ly (1 - lx), ly lx.  A corner outside
 *                [0, H) x [0, W) contributes 0, and so does a term whose weight is 0.
 * Sum            y[k][ho][wo] = act(bias[k] + sum_{c, i, j} w[k][c][i][j] * m * sample(c, py, px)), m = mask[g * kh * kw + t][ho][wo] or 1.
 *                The kernel multiplies m into the four corner weights ((wy * wx) * m) before it samples.  The sum is fp32 in an order
 *                fixed per route -- taps outermost, then offset groups, then channels -- with the bias added last.
 * Activation     0 none; 1 max(v, 0); 2 v > 0 ? v : v * a0; 3 min(max(v, a0), a1); 4 1 / (1 + expf(-v)); 5 v * tanhf(logf(1 + expf(v)));
 *                6 v * min(max(v * a0 + a1, 0), 1): exactly those of feather_conv1d.h.
 *
 * Kernels (fhip_dcn_route).  One launch per forward, nothing allocated, copied or waited for on the host; capturable in a hipGraph.
 *   dcn_mfma_kernel<TILE_K>   on v_mfma_f32_32x32x2_f32.  A block of four waves owns FHIP_DCN_TILE_P consecutive output pixels of one image
 *                             (Ho * Wo flattened: a tile may span rows) and TILE_K output channels: the sampled tile is made once and reused
 *                             across up to 128 output channels, and the sampled column matrix never reaches HBM.  The reduction walks taps
 *                             outermost, then offset groups, then chunks of FHIP_DCN_CHUNK_C input channels of the group (the tail
 *                             zero-filled: any C >= 1 runs).
 *                             Tap table, once per (tap, offset group): the 256 lanes are (pixel, corner) pairs; each reads its pixel's dy,
 *                             dx and m and writes one clamped in-plane address and one weight (bilinear weight times m; 0 for a corner
 *                             outside the plane, a sample outside the open range or a pixel past Ho * Wo) to LDS: 64 x 4 x (int, float) =
 *                             2 KiB, two of them.  The coordinate arithmetic is done once per pixel and tap, not once per channel.
 *                             Gather, per chunk: the B operand [CHUNK_C][64] is built in LDS, each lane summing four table-addressed loads
 *                             from its channel's plane times the four table weights; the A operand [TILE_K][CHUNK_C] of the tap is staged
 *                             from the packed weights with 16-byte reads into rows of an odd pitch (17 floats).
 *                             Two buffers: the loads of chunk i + 1 (and the table of the pair after it) are issued before the matrix
 *                             instructions of chunk i, one barrier per chunk.  Epilogue: bias, activation, stores guarded for the pixel and
 *                             the K tails.  Grid (pixel tiles x n, K tiles).
 *   dcn_pack_kernel           the weight re-layout of fhip_dcn_pack_weights, a lane per packed float.
 * TILE_K is 64 where K <= 64 and 128 otherwise.  There is no other kernel: a direct kernel for tiny C is out of scope.
 *
 * Packed weights [kh * kw][K][G][CP], CP = C / G rounded up to FHIP_DCN_CHUNK_C, zero past C / G: the 16 floats of a chunk of one output
 * channel and tap are one 64-byte run.  For G = 1 that is [kh * kw][K][C rounded up to the chunk].  The buffer is 16-byte aligned.
 *
 * Refused with FHIP_E_BADARG, never truncated: an extent, kernel, stride or dilation < 1; a negative pad; G not dividing C; Ho or Wo other
 * than the definition's or < 1; tensors of 2^31 elements or more; more than 65535 K tiles; an activation out of range; NULL or
 * 4-byte-unaligned pointers (bias and mask may be NULL), packed weights off a 16-byte boundary; y overlapping an input.
 *
 * Out of scope: convolution groups > 1, int8, dynamic weights, any fusion, a column-buffer route, DCNv3 / v4, tuning beyond the two tiles.
 * The library is separate from libfeather_hip.so and needs nothing from it but the enums of feather_hip.h; it keeps its own last-error
 * slot. */
#ifndef FEATHER_HIP_FEATHER_DCN_H_
#define FEATHER_HIP_FEATHER_DCN_H_

#include <stddef.h>

#include "feather_hip/feather_hip.h"

#ifdef __cplusplus
extern "C"
{
#endif

#define FHIP_DCN_API __attribute__((visibility("default")))

/* Route code fhip_net_layer_info reports for the layers of a net with fhip_net_set_deformable (feather_net.h). */
#define FHIP_DCN_NET_ROUTE 116

/* The tile of dcn_mfma_kernel<TILE_K>, 256 lanes.  LDS: two tap tables (2 x 2 KiB), two B buffers [CHUNK_C][TILE_P] (2 x 4 KiB) and two A
 * buffers [TILE_K][CHUNK_C + 1] (2 x 4.25 KiB at TILE_K 64, 2 x 8.5 KiB at 128): 20.5 KiB and 29 KiB.  Registers, as the compiler reports
 * them for gfx950: 60 vector and 16 accumulator registers at TILE_K 64, 64 and 32 at 128, no scratch: six and five waves a SIMD.  A block is
 * one wave a SIMD, so a compute unit holds 6 blocks at TILE_K 64 (registers; its 160 KiB of LDS would take 7) and 5 blocks at TILE_K 128
 * (registers and LDS alike). */
#define FHIP_DCN_TILE_P 64       /* consecutive output pixels per block (two 32-column tiles) */
#define FHIP_DCN_TILE_K_SMALL 64 /* output channels per block where K <= 64 (a 32 x 32 tile a wave) */
#define FHIP_DCN_TILE_K_LARGE 128 /* output channels per block otherwise (two 32 x 32 tiles a wave) */
#define FHIP_DCN_CHUNK_C 16      /* input channels per chunk of the reduction */

/* Ho and Wo of the definition.  FHIP_E_BADARG: an extent, kernel, stride or dilation < 1, a negative pad, Ho or Wo < 1, NULL. */
FHIP_DCN_API int fhip_dcn_output_dim(int h, int w, int kernel_h, int kernel_w, int dilation_h, int dilation_w, int stride_h, int stride_w, int pad_top,
                                     int pad_bottom, int pad_left, int pad_right, int* ho, int* wo);

/* The floats of the packed weights, kh * kw * K * G * CP; 0 (and the error set) for values fhip_dcn_pack_weights refuses. */
FHIP_DCN_API long long fhip_dcn_packed_floats(int c, int k, int kernel_h, int kernel_w, int offset_groups);

/* packed = the layout above of w, ncnn's [k][c][kernel_h][kernel_w]: DEVICE to DEVICE, one launch on `stream` (a hipStream_t as void*).
 * packed: fhip_dcn_packed_floats floats, 16-byte aligned, apart from w. */
FHIP_DCN_API int fhip_dcn_pack_weights(int c, int k, int kernel_h, int kernel_w, int offset_groups, const float* w, float* packed, void* stream);

/* y = the deformable convolution defined above, on `stream`.  All pointers DEVICE; mask NULL: DCN v1; bias [k] or NULL; packed: what
 * fhip_dcn_pack_weights wrote; ho, wo: what fhip_dcn_output_dim gives. */
FHIP_DCN_API int fhip_dcn_forward(int n, int c, int h, int w, int k, int kernel_h, int kernel_w, int dilation_h, int dilation_w, int stride_h, int stride_w,
                                  int pad_top, int pad_bottom, int pad_left, int pad_right, int offset_groups, int activation, float a0, float a1, const float* x,
                                  const float* offset, const float* mask, const float* packed, const float* bias, float* y, int ho, int wo, void* stream);

/* The kernel instantiation a forward would launch, as the demangled name without return type and parameters, copied into name[len]:
 *   "fhip::dcn_mfma_kernel<64>"    k <= 64
 *   "fhip::dcn_mfma_kernel<128>"   else
 * FHIP_E_BADARG: NULL name, len < 1, c, k, a kernel extent or offset_groups < 1, offset_groups not dividing c. */
FHIP_DCN_API int fhip_dcn_route(int c, int k, int kernel_h, int kernel_w, int offset_groups, char* name, int len);

/* Message of this thread's last failing call of this library ("" if none). */
FHIP_DCN_API const char* fhip_dcn_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* FEATHER_HIP_FEATHER_DCN_H_ */
