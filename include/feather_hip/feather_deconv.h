/* feather_deconv.h -- C-ABI of libfeather_deconv.so: transposed convolution (ncnn's Deconvolution / DeconvolutionDepthWise) on the
 * MI355X (gfx950).
 *
 * The reference has no such layer.  The definition (this text is the contract): dense NCHW fp32 with a leading batch, C = input_channels
 * and K = output_channels of the WHOLE layer, group divides both, weights [K][C/group][kh][kw] (the .bin order ncnn's converters emit, the
 * order of this project's Convolution reader), bias [K].  Output channel k belongs to group g = k / (K / group).
 *
 *     Ho = (H - 1) * sh + kh - pad_top  - pad_bottom + output_pad_bottom
 *     Wo = (W - 1) * sw + kw - pad_left - pad_right  + output_pad_right
 *     y[n][k][oy][ox] = act(bias[k] + sum w[k][c][i][j] * x[n][g * C/group + c][iy][ix])
 *         over c < C/group, i < kh, j < kw with  oy + pad_top - i = iy * sh,  ox + pad_left - j = ix * sw,  0 <= iy < H,  0 <= ix < W
 *
 * The kernel is NOT flipped (scatter form: input pixel (iy, ix) adds w[k][c][i][j] * x to output (iy * sh + i - pad_top,
 * ix * sw + j - pad_left)).  torch.nn.functional.conv_transpose2d keeps [C][K/group][kh][kw]: per group, swap the first two axes.
 *
 * The library is separate from libfeather_hip.so and needs nothing from it but the enums of feather_hip.h (fhip_error,
 * fhip_activation): link or dlopen either or both.  It keeps its own last-error slot.  Inputs and weights must be finite: the MFMA
 * route pads the shallower x-phase of a pair with zero weights, and 0 * Inf is NaN. */
#ifndef FEATHER_HIP_FEATHER_DECONV_H_
#define FEATHER_HIP_FEATHER_DECONV_H_

#include <stddef.h>

#include "feather_hip/feather_hip.h"

#ifdef __cplusplus
extern "C"
{
#endif

#define FHIP_DECONV_API __attribute__((visibility("default")))

/* The fields of fhip_conv_param (which stays field for field the reference's) plus the two output pads.  input_* is the SMALL tensor. */
typedef struct fhip_deconv_param
{
    int output_channels; /* K of the whole layer */
    int input_channels;  /* C of the whole layer */
    int input_h;
    int input_w;
    int kernel_h;
    int kernel_w;
    int output_h; /* set by fhip_deconv_assign_output_dim */
    int output_w;
    int stride_h;
    int stride_w;
    int pad_left;
    int pad_bottom;
    int pad_right;
    int pad_top;
    int group;
    int bias_term;
    int activation; /* enum fhip_activation */
    int output_pad_right;
    int output_pad_bottom;
} fhip_deconv_param;

/* output_h / output_w from the formula above.  FHIP_E_BADARG: NULL, or a result < 1. */
FHIP_DECONV_API int fhip_deconv_assign_output_dim(fhip_deconv_param* param);

/* 1 when the layer is one this library runs, else 0 (and the reason in fhip_deconv_last_error).  Refused: channels / input size / kernel /
 * stride < 1, negative pads, a group that does not divide both channel counts, output_pad >= stride, output_pad_bottom > pad_bottom or
 * output_pad_right > pad_right (only there would an output lie outside the full scatter range, where the formula gives act(bias) and
 * ncnn, which crops or pads the scatter result, may give 0), output_h / output_w other than fhip_deconv_assign_output_dim's, an
 * activation other than None / ReLU.  Every other entry point refuses the same params with FHIP_E_BADARG. */
FHIP_DECONV_API int fhip_deconv_supported(const fhip_deconv_param* param);

/* Bytes of the scratch buffer (always 0) and of the packed weights.  Cheap, pure, no device call.
 * FHIP_E_BADARG: NULL pointers, batch < 1, a refused param. */
FHIP_DECONV_API int fhip_deconv_get_buffer_size(const fhip_deconv_param* param, int batch, size_t* scratch_bytes, size_t* packed_bytes);

/* kernel [K][C/group][kh][kw] (device) -> packed (device, packed_bytes): one launch on `stream`, every packed word is written, so the
 * call is idempotent.  FHIP_E_BADARG: NULL or not 4-byte aligned pointers (packed: 16-byte aligned), a refused param. */
FHIP_DECONV_API int fhip_deconv_init(const fhip_deconv_param* param, float* packed, const float* kernel, void* stream);

/* out[batch][K][output_h][output_w] = act(deconv(in[batch][C][input_h][input_w]) + bias): one launch on `stream` (a hipStream_t as
 * void*), no allocation, no copy, no synchronisation: hipGraph-capturable.  `scratch` is unused (may be NULL); `bias` is [K], read only
 * with bias_term.  FHIP_E_BADARG: a refused param, batch < 1, NULL out / in / packed, NULL bias with bias_term, a pointer that is not
 * 4-byte aligned (packed: 16-byte), a tensor of 2^31 elements or more.  FHIP_E_HIP: the launch failed. */
/* Size limits: FHIP_E_BADARG for an input or output tensor of 2^31 elements or more, for 2^30 GEMM columns or more on the MFMA routes (not
 * reachable: the element limit refuses first), for more than 65535 chunks of 4 output channels on the generic route; fhip_deconv_init for 2^31
 * packed floats or more; fhip_deconv_assign_output_dim for an output side of 2^31 or more. */
FHIP_DECONV_API int fhip_deconv_forward(const fhip_deconv_param* param, int batch, float* out, const float* in, const float* packed, float* scratch,
                                        const float* bias, void* stream);

/* The kernel instantiation fhip_deconv_forward launches for this layer (the same selection function), as the demangled name without
 * return type and parameters, e.g. "fhip::deconv_generic_kernel<4>", copied into name[len]. */
FHIP_DECONV_API int fhip_deconv_route(const fhip_deconv_param* param, char* name, int len);

/* Message of this thread's last failing call of this library ("" if none). */
FHIP_DECONV_API const char* fhip_deconv_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* FEATHER_HIP_FEATHER_DECONV_H_ */
