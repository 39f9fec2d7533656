/* feather_qconv.h -- C-ABI of libfeather_qconv.so: ncnn-style int8 convolution on the MI355X (gfx950), fp32 in and out.
 *
 * The reference refuses int8 layers (conv_layer.h:50-55); this library is the route of its own that runs a Convolution,
 * ConvolutionDepthWise or InnerProduct layer whose weights are int8 (int8_scale_term 1 or 2 of an ncnn model).  The text below follows
 * ncnn's int8 inference as the maintainers know it; where ncnn differs, THIS TEXT HOLDS: it is the contract, and tests/qconv_ref.py
 * restates it in numpy.  Every result is defined to the bit: the sum is an exact integer sum, so its order is free.
 *
 * Layout and scales.  Dense NCHW fp32 with a leading batch, in and out.  C = input_channels and K = output_channels of the WHOLE layer;
 * group is 1, or equal to both C and K (depthwise).  Weights are signed char [K][C/group][kh][kw], weight scales s_w[K], one input scale
 * s_in, bias[K] or none.
 *
 *     OH = (H + pad_top  + pad_bottom - kh) / stride_h + 1      (floor)
 *     OW = (W + pad_left + pad_right  - kw) / stride_w + 1      (floor)
 *
 * Quantise an input value x:   t = x * s_in                     (one fp32 rounding)
 *                              r = roundf(t)                    (halves away from zero: ncnn's float2int8)
 *                              q = r clamped to [-127, 127]     (NaN gives 0, +-inf gives +-127)
 *   A tap outside the plane is q = 0: its address is clamped into the plane and the value replaced (a select), so a non-finite input
 *   pixel only reaches the outputs whose window holds it.
 * Accumulate:                  acc = sum over the R = (C/group) * kh * kw products q * w, exact in int32.  R > 133144 is refused:
 *                              127 * 127 * R must stay below 2^31.
 * Dequantise:                  y = act(float(acc) * d[k] + b[k])
 *   float(acc) rounds to nearest even (|acc| may exceed 2^24); the product and the sum are rounded each on its own (no FMA); without a
 *   bias there is no addition; act is None or ReLU (fmaxf(y, 0)).
 *   d[k] = 1.0f / (s_in * s_w[k]) in fp32 on the host -- the product rounded, then the reciprocal rounded -- and d[k] = 0 where
 *   s_w[k] == 0 (ncnn's convention).  fhip_qconv_dequant_scales computes it, so that every caller gets the same bits.
 * A folded BatchNorm / Scale (y * mul[k] + add[k] behind the layer, the Net runtime's fusion level 2) cannot go into int8 weights; it
 *   goes into the dequantisation: d'[k] = d[k] * mul[k], b'[k] = b[k] * mul[k] + add[k], each operation rounded in fp32, b = 0 when the
 *   layer has no bias (a fold creates one).  The layer then computes act(float(acc) * d'[k] + b'[k]).
 *
 * Refused: s_in that is not finite or not > 0; s_w[k] that is not finite or < 0; a partial group (1 < group < C); any dilation other
 * than 1; negative (automatic) pads; int8_scale_term > 100 (requantised int8 output).
 *
 * The library is separate from libfeather_hip.so and needs nothing from it but the enums of feather_hip.h (fhip_error,
 * fhip_activation): link or dlopen either or both.  It keeps its own last-error slot. */
#ifndef FEATHER_HIP_FEATHER_QCONV_H_
#define FEATHER_HIP_FEATHER_QCONV_H_

#include <stddef.h>

#include "feather_hip/feather_hip.h"

#ifdef __cplusplus
extern "C"
{
#endif

#define FHIP_QCONV_API __attribute__((visibility("default")))

/* 127 * 127 * R < 2^31 */
#define FHIP_QCONV_MAX_REDUCTION 133144

/* The fields of fhip_atrous_param in the same order (the dilations must be 1), plus the model's int8_scale_term (0 .. 100). */
typedef struct fhip_qconv_param
{
    int output_channels; /* K of the whole layer */
    int input_channels;  /* C of the whole layer */
    int input_h;
    int input_w;
    int kernel_h;
    int kernel_w;
    int output_h; /* set by fhip_qconv_assign_output_dim */
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
    int dilation_h;
    int dilation_w;
    int int8_scale_term;
} fhip_qconv_param;

/* output_h / output_w from the formula above.  FHIP_E_BADARG: NULL, sizes / strides < 1, a kernel larger than the padded input. */
FHIP_QCONV_API int fhip_qconv_assign_output_dim(fhip_qconv_param* param);

/* 1 when the layer is one this library runs, else 0 (and the reason in fhip_qconv_last_error).  Refused: channels / input size / kernel /
 * stride < 1, a dilation other than 1, negative pads, a group that is neither 1 nor equal to both channel counts, int8_scale_term < 0 or
 * > 100, a reduction length R > 133144, a kernel larger than the padded input, output_h / output_w other than
 * fhip_qconv_assign_output_dim's, an activation other than None / ReLU, an input or output image of 2^31 elements or more.  Every other
 * entry point refuses the same params with FHIP_E_BADARG. */
FHIP_QCONV_API int fhip_qconv_supported(const fhip_qconv_param* param);

/* Bytes of the scratch buffer (always 0) and of the packed weights.  Cheap, pure, no device call. */
FHIP_QCONV_API int fhip_qconv_get_buffer_size(const fhip_qconv_param* param, int batch, size_t* scratch_bytes, size_t* packed_bytes);

/* kernel: signed char [K][C/group][kh][kw] (device) -> packed (device, packed_bytes, 16-byte aligned): one launch on `stream`, every
 * packed byte is written, so the call is idempotent.  FHIP_E_BADARG: NULL pointers, a packed pointer that is not 16-byte aligned, a
 * refused param, 2^31 packed bytes or more. */
FHIP_QCONV_API int fhip_qconv_init(const fhip_qconv_param* param, void* packed, const signed char* kernel, void* stream);

/* d[k] = s_w[k] == 0 ? 0 : 1.0f / (s_in * s_w[k]) for k < K, on the host (all pointers are host pointers).
 * FHIP_E_BADARG: NULL, K < 1, s_in not finite or not > 0, an s_w[k] that is not finite or < 0. */
FHIP_QCONV_API int fhip_qconv_dequant_scales(float* d, const float* s_w, int K, float s_in);

/* out[batch][K][output_h][output_w] = act(float(acc) * d[k] + bias[k]), acc the int8 convolution of quantise(in[batch][C][H][W]; s_in):
 * one launch on `stream` (a hipStream_t as void*), no allocation, no copy, no synchronisation: hipGraph-capturable.  The input is
 * quantised while it is loaded: no int8 copy of it exists in memory.  `scratch` is unused (may be NULL); d is [K] (device), bias [K]
 * (device), read only with bias_term.
 * FHIP_E_BADARG: a refused param, batch < 1, NULL out / in / packed / d, NULL bias with bias_term, a pointer that is not 4-byte aligned
 * (packed: 16-byte), s_in not finite or not > 0.  FHIP_E_HIP: the launch failed.
 * Size limits: FHIP_E_BADARG for 2^31 elements or more in one image (every entry point: fhip_qconv_supported is 0) or in a whole tensor, for
 * 2^30 GEMM columns or more on an MFMA route, for more than 65535 chunks of 4 (16) output channels on the generic routes; fhip_qconv_init for 2^31
 * packed bytes or more. */
FHIP_QCONV_API int fhip_qconv_forward(const fhip_qconv_param* param, int batch, float* out, const float* in, const void* packed, float* scratch,
                                      const float* d, const float* bias, float s_in, void* stream);

/* out[i] = quantise(in[i]; s_in) for i < count, by the rule above, as a kernel of its own (the convolution routes never call it: they
 * quantise in their loaders).  One launch, capturable.  FHIP_E_BADARG: NULL, count < 1 or >= 2^31, `in` not 4-byte aligned, a bad s_in. */
FHIP_QCONV_API int fhip_quantize_forward(signed char* out, const float* in, size_t count, float s_in, void* stream);

/* The kernel instantiation fhip_qconv_forward launches for this layer (the same selection function), as the demangled name without
 * return type and parameters, e.g. "fhip::qconv_generic_kernel<4>", copied into name[len].  The routes:
 *   fhip::qconv_mfma_kernel<4, 1> / <2, 2>   group 1, C % 16 == 0: implicit GEMM on v_mfma_i32_16x16x64_i8, 128 / 64 output channels per block
 *   fhip::qconv_dw3x3_kernel<1> / <2>        group == C == K, 3x3, stride 1 / 2 in both directions
 *   fhip::qconv_generic_kernel<16> / <4>     everything else: 16 output channels per lane from 16 output channels per group on, else 4 */
FHIP_QCONV_API int fhip_qconv_route(const fhip_qconv_param* param, char* name, int len);

/* The three calls above for a NAMED route instead of the selected one.  The packed layout belongs to the route: pack with
 * fhip_qconv_init_route under the same name.  FHIP_E_BADARG: an unknown name; FHIP_E_UNSUPPORTED: a route that cannot run this layer. */
FHIP_QCONV_API int fhip_qconv_get_buffer_size_route(const fhip_qconv_param* param, int batch, const char* route, size_t* scratch_bytes,
                                                    size_t* packed_bytes);
FHIP_QCONV_API int fhip_qconv_init_route(const fhip_qconv_param* param, void* packed, const signed char* kernel, void* stream, const char* route);
FHIP_QCONV_API int fhip_qconv_forward_route(const fhip_qconv_param* param, int batch, float* out, const float* in, const void* packed, float* scratch,
                                            const float* d, const float* bias, float s_in, void* stream, const char* route);

/* Message of this thread's last failing call of this library ("" if none). */
FHIP_QCONV_API const char* fhip_qconv_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* FEATHER_HIP_FEATHER_QCONV_H_ */
