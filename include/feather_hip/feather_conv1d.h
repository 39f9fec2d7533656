/* feather_conv1d.h -- C-ABI of libfeather_conv1d.so: ncnn's Convolution1D, ConvolutionDepthWise1D and Pooling1D on the MI355X (gfx950),
 * on fp32 tensors with a leading batch.
 *
 * The reference has none of these layers: this text is the definition, written from what ncnn's convolution1d.cpp,
 * convolutiondepthwise1d.cpp and pooling1d.cpp do.  tests/conv1d_ref.py restates it in float64.
 *
 * Tensors        x is [n][C] rows of L floats, row (i, c) at element (i * C + c) * x_stride (x_stride >= L); y is [n][K] rows of Lo floats,
 *                row (i, k) at (i * K + k) * y_stride (y_stride >= Lo): a tensor may sit inside a wider buffer.  Floats between the rows
 *                are neither read nor written.
 * Convolution    kw taps, dilation d, stride s, pads pl and pr: ke = d * (kw - 1) + 1, Lo = (L + pl + pr - ke) / s + 1.  pl == -233
 *                (SAME_UPPER) or -234 (SAME_LOWER): the total pad is max(0, (ceil(L / s) - 1) * s + ke - L), halved, the odd unit on
 *                the right for -233 and on the left for -234 (fhip_conv1d_output_dim resolves them).
 *                y[k][l] = act(bias[k] + sum_c sum_t w[k][c][t] * xpad[c][l * s + t * d]); cells of xpad outside [0, L) hold pad_value.
 *                Weights [K][C / group][kw] in ncnn's layout, read in place: output channel k of group g = k / (K / group) sums over the
 *                input channels [g * C / group, (g + 1) * C / group).  The sum is fp32, the bias added last, in an order fixed per route.
 * Activation     0 none; 1 max(v, 0); 2 v > 0 ? v : v * a0; 3 min(max(v, a0), a1); 4 1 / (1 + expf(-v)); 5 v * tanhf(logf(1 + expf(v)));
 *                6 v * min(max(v * a0 + a1, 0), 1)  (ncnn's activation types; a0, a1 = activation_params).
 * Pooling        type 0 max, 1 average over windows of kw cells at stride s of the row padded by pl and pr (fhip_pool1d_output_dim
 *                resolves ncnn's pad_mode: 0 full -- Lo = ceil((L + pl + pr - kw) / s) + 1, the tail window hanging over the end --, 1
 *                valid -- floor --, 2 SAME_UPPER, 3 SAME_LOWER -- total pad max(0, kw + (L - 1) / s * s - L), the odd unit right / left).
 *                Max: the maximum of the window's cells inside [0, L), -FLT_MAX if there is none.  Average: their sum in ascending
 *                order, divided by their count, or, with count_include_pad, by the count of the window's cells inside the padded row
 *                [-pl, L + pr): the tail cells of full mode never count.  No cell counted: 0.  Adaptive (kw == 0): window l is
 *                [floor(l * L / Lo), ceil((l + 1) * L / Lo)); global pooling is the adaptive form with Lo = 1.
 * Rank           a 1-D blob of the Net runtime is rank 2, [n][1][C][L].  Global pooling gives ncnn's blob of rank 1 [C], stored as
 *                [n][1][1][C] with Blob::dims 1, the form MemoryData writes and InnerProduct and Reshape behind it accept (they flatten).
 *
 * Kernels (fhip_conv1d_route).  One launch per call, nothing allocated, copied or waited for on the host; capturable in a hipGraph.
 *   conv1d_mfma_kernel<LDS>   dense and grouped convolution on v_mfma_f32_32x32x2_f32.  A block of four waves owns FHIP_CONV1D_TILE_K
 *                             output channels x FHIP_CONV1D_TILE_L output positions of one image and one group.  Per chunk of CC input
 *                             channels it stages ONCE the input slab [CC][(TILE_L - 1) * s + (kw - 1) * d + 1] and the weights
 *                             [TILE_K][CC * kw] into LDS; the reduction walks channel pairs and taps, the B operand of tap t being the
 *                             slab read at offset t * d: an input element leaves HBM once per block, not kw times.  The slab is stored
 *                             SPLIT BY PHASE, cell p at (p % s) * PW + p / s with PW = ceil(slab / s): the 32 lanes of a column read
 *                             p = l * s + t * d, which is phase (t * d) % s -- the same for all lanes -- at l + (t * d) / s: consecutive
 *                             words for every stride, so no stride has a bank conflict (a padded row would fix odd strides only).
 *                             Weight rows have an odd pitch.  Two buffers: chunk i + 1 is staged while chunk i multiplies, one barrier
 *                             per chunk.  LDS is 8192 floats (32 KiB, five blocks a compute unit) where a chunk of at least
 *                             two channels fits, else 24576 floats (96 KiB, one block): fhip_conv1d_chunk below is the rule.
 *   conv1d_direct_kernel      every other convolution: fewer than FHIP_CONV1D_MFMA_MIN_C input channels per group (raw audio), slabs
 *                             past the budget.  A lane owns one output position and FHIP_CONV1D_DIRECT_K output channels, the taps are
 *                             wave-uniform operands.  A body of its own: csrc_side/direct_conv.h walks 2-D windows with pads of zero.
 *   conv1d_depthwise_kernel   group == C == K > 1 where the segment fits: a block owns FHIP_CONV1D_DW_SEGMENT outputs of one row, the
 *                             segment plus halo in LDS, a lane FHIP_CONV1D_DW_LANE consecutive outputs in registers; at s == d == 1 a
 *                             16-byte LDS read feeds four taps of four outputs.  Input read once, output written once.
 *   pool1d_kernel             a lane per output.
 *
 * Refused with FHIP_E_BADARG, never truncated: an extent, kernel, stride or dilation < 1; a negative pad; a group that divides not
 * both channel counts; Lo other than the definition's or < 1; a stride below its row; tensors of 2^31 elements or more (strides included);
 * an activation or pooling type out of range; NULL or 4-byte-unaligned pointers (bias may be NULL); y overlapping x.
 *
 * Out of scope: Deconvolution1D, GLU, dynamic weights, int8, any fusion, tuning beyond the one tile.  The library is separate from
 * libfeather_hip.so and needs nothing from it but the enums of feather_hip.h; it keeps its own last-error slot. */
#ifndef FEATHER_HIP_FEATHER_CONV1D_H_
#define FEATHER_HIP_FEATHER_CONV1D_H_

#include <stddef.h>

#include "feather_hip/feather_hip.h"

#ifdef __cplusplus
extern "C"
{
#endif

#define FHIP_CONV1D_API __attribute__((visibility("default")))

/* Route code fhip_net_layer_info reports for the layers of a net with fhip_net_set_conv1d (feather_net.h). */
#define FHIP_CONV1D_NET_ROUTE 115

#define FHIP_CONV1D_SAME_UPPER (-233)
#define FHIP_CONV1D_SAME_LOWER (-234)

#define FHIP_CONV1D_TILE_K 64         /* output channels per block of the matrix kernel (two 32-row tiles) */
#define FHIP_CONV1D_TILE_L 64         /* output positions per block of the matrix kernel (two 32-column tiles) */
#define FHIP_CONV1D_MFMA_MIN_C 3      /* input channels per group from which the matrix kernel is taken */
#define FHIP_CONV1D_LDS_SMALL 8192    /* floats: 32 KiB, five blocks on a compute unit's 160 KiB */
#define FHIP_CONV1D_LDS_LARGE 24576   /* floats: 96 KiB, one block; what a filter of 87 taps needs for a chunk of two channels */
#define FHIP_CONV1D_DIRECT_K 4        /* output channels per lane of the direct kernel */
#define FHIP_CONV1D_DW_SEGMENT 1024   /* outputs per block of the depthwise kernel */
#define FHIP_CONV1D_DW_LANE 4         /* consecutive outputs per lane of it */
#define FHIP_CONV1D_DW_LDS 8192       /* floats: the segment plus halo, (SEGMENT - 1) * s + (kw - 1) * d + 1, must fit (8 floats spare) */

/* The rule of the matrix kernel: the channels per chunk, CC, for a budget of lds_floats, or 0 if no chunk fits.  Two buffers, each the
 * weights [TILE_K][CC * kw | 1] (odd pitch) and the slab [CC][s * PW], PW = ceil(((TILE_L - 1) * s + (kw - 1) * d + 1) / s).  The largest
 * CC of 16, 8, 4, 2 that fits.  feathercnn_amd/conv1d.py restates it. */
static inline int fhip_conv1d_chunk(int kw, int s, int d, int lds_floats)
{
    const long long slab = 63ll * s + (long long)(kw - 1) * d + 1, sp = (slab + s - 1) / s * s;
    int cc;
    for (cc = 16; cc >= 2; cc /= 2)
        if (2 * (64 * (((long long)cc * kw) | 1) + cc * sp) <= lds_floats) return cc;
    return 0;
}

/* Lo, and the pads resolved, of a convolution: pad_left >= 0 with pad_right >= 0, or pad_left -233 / -234 (pad_right ignored).
 * FHIP_E_BADARG: an extent < 1, another negative pad, Lo < 1. */
FHIP_CONV1D_API int fhip_conv1d_output_dim(int l, int kernel_w, int dilation, int stride, int pad_left, int pad_right, int* left, int* right,
                                           int* lo);

/* y = the convolution defined above, on `stream` (a hipStream_t as void*).  pad_left, pad_right: resolved (>= 0).  w: DEVICE
 * [k][c / group][kernel_w]; bias: DEVICE [k] or NULL.  lo: what fhip_conv1d_output_dim gives. */
FHIP_CONV1D_API int fhip_conv1d_forward(int n, int c, int l, int k, int kernel_w, int dilation, int stride, int pad_left, int pad_right,
                                        float pad_value, int group, int activation, float a0, float a1, const float* x, int x_stride,
                                        const float* w, const float* bias, float* y, int y_stride, int lo, void* stream);

/* Lo, and the pads resolved, of a pooling: pad_mode 0 full, 1 valid, 2 SAME_UPPER, 3 SAME_LOWER (the pads given are ignored for 2, 3). */
FHIP_CONV1D_API int fhip_pool1d_output_dim(int l, int kernel_w, int stride, int pad_left, int pad_right, int pad_mode, int* left, int* right,
                                           int* lo);

/* y[rows][lo] = the pooling defined above of x[rows][l] (rows = n * C).  kernel_w == 0: adaptive onto lo cells (stride and pads ignored). */
FHIP_CONV1D_API int fhip_pool1d_forward(int type, int rows, int l, int kernel_w, int stride, int pad_left, int pad_right, int count_include_pad,
                                        const float* x, int x_stride, float* y, int y_stride, int lo, void* stream);

/* The kernel instantiation a convolution would launch, as the demangled name without return type and parameters, copied into name[len]:
 *   "fhip::conv1d_depthwise_kernel"     group == c == k > 1 and (SEGMENT - 1) * s + (kw - 1) * d + 9 <= FHIP_CONV1D_DW_LDS
 *   "fhip::conv1d_mfma_kernel<8192>"    else, c / group >= FHIP_CONV1D_MFMA_MIN_C and fhip_conv1d_chunk(.., FHIP_CONV1D_LDS_SMALL) > 0
 *   "fhip::conv1d_mfma_kernel<24576>"   else, c / group >= FHIP_CONV1D_MFMA_MIN_C and fhip_conv1d_chunk(.., FHIP_CONV1D_LDS_LARGE) > 0
 *   "fhip::conv1d_direct_kernel"        else
 * kernel_w == 0 asks for the pooling: "fhip::pool1d_kernel".  FHIP_E_BADARG: NULL name, len < 1, extents the forward call would refuse. */
FHIP_CONV1D_API int fhip_conv1d_route(int c, int k, int kernel_w, int dilation, int stride, int group, char* name, int len);

/* Message of this thread's last failing call of this library ("" if none). */
FHIP_CONV1D_API const char* fhip_conv1d_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* FEATHER_HIP_FEATHER_CONV1D_H_ */
