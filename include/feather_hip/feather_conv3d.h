/* feather_conv3d.h -- C-ABI of libfeather_conv3d.so: ncnn's Convolution3D, ConvolutionDepthWise3D and Pooling3D on the MI355X (gfx950),
 * on dense fp32 tensors with a leading batch.
 *
 * The reference has none of these layers: this text is the definition, written from ncnn's documented behaviour (operators.md and the
 * parameter tables of convolution3d, convolutiondepthwise3d and pooling3d).  tests/conv3d_ref.py restates it in float64.
 *
 * Tensors        x is [n][C][D][H][W], y is [n][K][Do][Ho][Wo], both dense; w is [K][C / group][kd][kh][kw] in ncnn's layout.
 * Extents        per axis, with kernel k, dilation d, stride s and the pads lo and hi: ke = d * (k - 1) + 1, out = (in + lo + hi - ke) / s + 1
 *                (fhip_conv3d_output_dim, called once per axis).  lo == -233 (SAME_UPPER) or -234 (SAME_LOWER): the total pad of the axis is
 *                max(0, (ceil(in / s) - 1) * s + ke - in), halved, the odd unit behind for -233 and in front for -234.
 * Convolution    y[k][od][oh][ow] = act(bias[k] + sum_c sum_z sum_i sum_j w[k][c][z][i][j] * xpad[c][od sd + z dd][oh sh + i dh][ow sw + j dw]);
 *                cells of xpad outside the volume hold pad_value.  Output channel k of group g = k / (K / group) sums over the input
 *                channels [g C / group, (g + 1) C / group).  The sum is fp32, the bias added last, in an order fixed per kernel.
 * Activation     0 none; 1 max(v, 0); 2 v > 0 ? v : v * a0; 3 min(max(v, a0), a1); 4 1 / (1 + expf(-v)); 5 v * tanhf(logf(1 + expf(v)));
 *                6 v * min(max(v * a0 + a1, 0), 1)  (ncnn's activation types; a0, a1 = activation_params).
 * Pooling        type 0 max, 1 average over windows of kd x kh x kw cells.  Per axis (fhip_pool3d_output_dim, once per axis) ncnn's
 *                pad_mode: 0 full -- out = ceil((in + lo + hi - k) / s) + 1, the tail window hanging over the end --, 1 valid -- floor --,
 *                2 SAME_UPPER, 3 SAME_LOWER -- total pad max(0, k + (in - 1) / s * s - in), the odd unit behind / in front.  Max: the
 *                maximum of the window's cells inside the volume, -FLT_MAX if there is none.  Average: their sum in ascending order
 *                (depth, row, column), divided by their count, or, with count_include_pad, by the count of the window's cells inside the
 *                padded volume (per axis [-lo, in + hi): the tail cells of full mode never count).  No cell counted: 0.  Adaptive (kernel
 *                0 on every axis): window o of an axis is [floor(o * in / out), ceil((o + 1) * in / out)); global pooling is the adaptive
 *                form onto 1 x 1 x 1.
 * Rank           a volume of the Net runtime is a blob of rank 4, [n][C][D][H][W] (Blob::d).  Global pooling gives ncnn's blob of rank 1
 *                [C], stored as [n][1][1][C], as Pooling1D does.
 *
 * Kernels (fhip_conv3d_route).  One launch per call, nothing allocated, copied or waited for on the host; capturable in a hipGraph.
 *   conv3d_mfma_kernel<TILE_K>  group == 1, kh * kw <= FHIP_CONV3D_MAX_TAPS and a patch plane of at most FHIP_CONV3D_MAX_PLANE cells, on
 *                             v_mfma_f32_32x32x2_f32.  A block of four waves owns one image, one output depth, an 8 x 8 rectangle of
 *                             output pixels and TILE_K output channels (64 where K <= 64, else 128: one or two 32 x 32 accumulator tiles a
 *                             wave).  It walks the depth taps, and per tap chunks of FHIP_CONV3D_CHUNK input channels; per step it stages
 *                             ONCE the input halo patch [CHUNK][(8 - 1) sh + (kh - 1) dh + 1][(8 - 1) sw + (kw - 1) dw + 1] of that input
 *                             depth and the weights of all kh * kw taps [kh kw][TILE_K][CHUNK] (rows of CHUNK + 1 floats) into LDS.  The B
 *                             operand of a tap is the patch read at the tap's offset: no column matrix exists, and a staged input value
 *                             feeds up to kh * kw products.  The next step's patch and weights are fetched into registers before the
 *                             matrix instructions of the current step and written to LDS behind them.  A depth plane wholly in the
 *                             padding is skipped where pad_value == 0 and staged as a constant otherwise.  The weights come from the
 *                             packed buffer [kd kh kw][K][C rounded up to CHUNK] that conv3d_pack_kernel writes once.
 *   conv3d_direct_kernel      everything else -- groups, depthwise, larger kernels and patches --, and any call without a packed buffer:
 *                             a lane per output, the sum over (c, z, i, j) in that order.
 *   pool3d_kernel             a lane per output.
 *   conv3d_pack_kernel        the packed weights, a lane per float.
 *
 * Refused with FHIP_E_BADARG, never truncated: an extent, kernel, stride or dilation < 1; a negative pad; a group that divides not both
 * channel counts; output extents other than the definition's or < 1; tensors of 2^31 elements or more; an activation or pooling type out
 * of range; NULL or 4-byte-unaligned pointers (bias may be NULL; packed must be 16-byte aligned); y overlapping an input.  FHIP_E_UNSUPPORTED:
 * a device whose LDS limit per block is below what the matrix kernel needs.
 *
 * Out of scope: Deconvolution3D, int8 / bf16 / fp16 forms, a 3-D Winograd, dynamic weights, any fusion.  The library is separate from
 * libfeather_hip.so and needs nothing from it but the enums of feather_hip.h; it keeps its own last-error slot. */
#ifndef FEATHER_HIP_FEATHER_CONV3D_H_
#define FEATHER_HIP_FEATHER_CONV3D_H_

#include <stddef.h>

#include "feather_hip/feather_hip.h"

#ifdef __cplusplus
extern "C"
{
#endif

#define FHIP_CONV3D_API __attribute__((visibility("default")))

/* Route code fhip_net_layer_info reports for the layers of a net with fhip_net_set_conv3d (feather_net.h). */
#define FHIP_CONV3D_NET_ROUTE 117

#define FHIP_CONV3D_SAME_UPPER (-233)
#define FHIP_CONV3D_SAME_LOWER (-234)

#define FHIP_CONV3D_TILE_K_SMALL 64  /* output channels per block of the matrix kernel where K <= 64 */
#define FHIP_CONV3D_TILE_K_LARGE 128 /* and where K > 64 */
#define FHIP_CONV3D_TILE_H 8         /* output rows per block */
#define FHIP_CONV3D_TILE_W 8         /* output columns per block */
#define FHIP_CONV3D_CHUNK 8          /* input channels per step */
#define FHIP_CONV3D_MAX_TAPS 9       /* kh * kw the matrix kernel stages at once */
#define FHIP_CONV3D_MAX_PLANE 320    /* cells of one channel's patch plane (17 x 17: a 3 x 3 kernel at stride 2) */

/* The output extent of one axis of a convolution and its pads resolved: pad_lo >= 0 with pad_hi >= 0, or pad_lo -233 / -234 (pad_hi
 * ignored).  FHIP_E_BADARG: an extent < 1, another negative pad, out < 1. */
FHIP_CONV3D_API int fhip_conv3d_output_dim(int extent, int kernel, int dilation, int stride, int pad_lo, int pad_hi, int* lo, int* hi, int* out);

/* The floats of the packed weights of the matrix kernel, kd * kh * kw * k * (c rounded up to FHIP_CONV3D_CHUNK), or 0 where the convolution
 * runs on the direct kernel (which reads w in place) or would be refused. */
FHIP_CONV3D_API long long fhip_conv3d_packed_floats(int c, int k, int kernel_d, int kernel_h, int kernel_w, int dilation_h, int dilation_w,
                                                    int stride_h, int stride_w, int group);

/* packed[(z kh + i) kw + j][k][c'] = w[k][c'][z][i][j], 0 for c' >= c, on `stream`.  w: DEVICE [k][c][kd][kh][kw]; packed: DEVICE, 16-byte
 * aligned, fhip_conv3d_packed_floats floats. */
FHIP_CONV3D_API int fhip_conv3d_pack_weights(int c, int k, int kernel_d, int kernel_h, int kernel_w, const float* w, float* packed, void* stream);

/* y = the convolution defined above, on `stream` (a hipStream_t as void*).  Pads: resolved (>= 0), in the order front, behind, top, bottom,
 * left, right.  w: DEVICE [k][c / group][kd][kh][kw]; packed: what fhip_conv3d_pack_weights wrote, or NULL -- the call then runs on the
 * direct kernel whatever fhip_conv3d_route says for a packed call; bias: DEVICE [k] or NULL.  od, oh, ow: what fhip_conv3d_output_dim gives. */
FHIP_CONV3D_API int fhip_conv3d_forward(int n, int c, int d, int h, int w, int k, int kernel_d, int kernel_h, int kernel_w, int dilation_d,
                                        int dilation_h, int dilation_w, int stride_d, int stride_h, int stride_w, int pad_front, int pad_behind,
                                        int pad_top, int pad_bottom, int pad_left, int pad_right, float pad_value, int group, int activation,
                                        float a0, float a1, const float* x, const float* wt, const float* packed, const float* bias, float* y,
                                        int od, int oh, int ow, void* stream);

/* The output extent of one axis of a pooling and its pads resolved: pad_mode 0 full, 1 valid, 2 SAME_UPPER, 3 SAME_LOWER (the pads given are
 * ignored for 2, 3). */
FHIP_CONV3D_API int fhip_pool3d_output_dim(int extent, int kernel, int stride, int pad_lo, int pad_hi, int pad_mode, int* lo, int* hi, int* out);

/* y[rows][od][oh][ow] = the pooling defined above of x[rows][d][h][w] (rows = n * C).  kernel_d == kernel_h == kernel_w == 0: adaptive
 * onto od x oh x ow cells (strides and pads ignored). */
FHIP_CONV3D_API int fhip_pool3d_forward(int type, int rows, int d, int h, int w, int kernel_d, int kernel_h, int kernel_w, int stride_d, int stride_h,
                                        int stride_w, int pad_front, int pad_behind, int pad_top, int pad_bottom, int pad_left, int pad_right,
                                        int count_include_pad, const float* x, float* y, int od, int oh, int ow, void* stream);

/* The kernel instantiation a convolution with packed weights would launch, as the demangled name without return type and parameters:
 *   "fhip::conv3d_mfma_kernel<64>"    group == 1, kh * kw <= MAX_TAPS, ((8 - 1) sh + (kh - 1) dh + 1) * ((8 - 1) sw + (kw - 1) dw + 1) <= MAX_PLANE, k <= 64
 *   "fhip::conv3d_mfma_kernel<128>"   the same with k > 64
 *   "fhip::conv3d_direct_kernel"      else, and with direct != 0 (a call without packed weights)
 * k == 0 asks for the pooling: "fhip::pool3d_kernel".  FHIP_E_BADARG: NULL name, len < 1, extents the forward call would refuse. */
FHIP_CONV3D_API int fhip_conv3d_route(int c, int k, int kernel_d, int kernel_h, int kernel_w, int dilation_h, int dilation_w, int stride_h,
                                      int stride_w, int group, int direct, char* name, int len);

/* Message of this thread's last failing call of this library ("" if none). */
FHIP_CONV3D_API const char* fhip_conv3d_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* FEATHER_HIP_FEATHER_CONV3D_H_ */
