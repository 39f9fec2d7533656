/* feather_q8.h -- C-ABI of libfeather_q8.so: int8 convolution whose input, output or both are int8 TENSORS on the MI355X (gfx950): the
 * activation between two int8 layers of an ncnn model stays int8 in memory (ncnn's requantised output, int8_scale_term 101 .. 200).
 *
 * This text is the contract, as feather_qconv.h is for the fp32-in / fp32-out form; tests/q8_ref.py restates it in numpy and every result
 * is defined to the bit.  Everything feather_qconv.h defines holds here unchanged: "Quantise an input value", "Accumulate", "Dequantise",
 * d[k], the BatchNorm / Scale fold into d'[k] and b'[k], the refusals.  What this header adds:
 *
 * The q8 tensor.  signed char [n][CB][h][w][16] with CB = ceil(C / 16): channel c is byte c & 15 of block c >> 4, so the 16 channels of one
 *   pixel are 16 adjacent bytes (one 16-byte load: one B-fragment row of v_mfma_i32_16x16x64_i8).  The bytes of channels >= C are 0: every
 *   producer of this library writes them as 0, and no consumer's result depends on them (the packers zero the weights of the pad channels).
 *   Values lie in [-127, 127]; a -128 a caller made is used as it is, and the int32 sum may then wrap.  fhip_q8_tensor_bytes gives the size
 *   = n * CB * h * w * 16; 2^31 bytes or more is refused.  A q8 tensor is 16-byte aligned.  The tensor carries no scale.
 *
 * Int8 input (input_int8 = 1).  The layer takes q from the tensor as it is: there is no quantise.  A tap outside the plane is 0.
 *   d[k] = 1 / (s_in * s_w[k]) uses the layer's own s_in (fhip_q8_dequant_scales == fhip_qconv_dequant_scales).
 *
 * Requantised output (output_int8 = 1).  y = act(float(acc) * d[k] + b[k]) exactly as feather_qconv.h defines it -- the same roundings,
 *   the same d[k], the same fold, act None or ReLU -- and then q_out = quantise(y; s_out) by the quantise rule of feather_qconv.h: one
 *   fp32 product, roundf, clamp to +-127, NaN -> 0.  y is never stored.  s_out must be finite and > 0.
 *   In an ncnn model such a layer has int8_scale_term 101 .. 200 (the base term is the value - 100) and, behind the weights, bias, K weight
 *   scales and the input scale its .bin holds today, one more raw fp32: s_out.  Above 200 is refused.
 *
 * quantise is monotone, odd and maps 0 to 0, so it commutes with ReLU and, for finite values, with max: a ReLU or a max pooling on a q8
 *   tensor (fhip_q8_relu_forward, fhip_q8_max_pool_forward) gives the bytes the fp32 layer followed by the quantise would give, and a net
 *   whose readers all have s_in == s_out of their producer equals, bit for bit on every fp32 blob, the same net with fp32 activations.
 *
 * fp32 in AND fp32 out is not this library's job (libfeather_qconv.so): fhip_q8_supported is 0.
 *
 * The library is separate from libfeather_hip.so and libfeather_qconv.so and needs nothing from them but the enums and fhip_pool_param of
 * feather_hip.h / feather_net.h: link or dlopen any of them.  It keeps its own last-error slot. */
#ifndef FEATHER_HIP_FEATHER_Q8_H_
#define FEATHER_HIP_FEATHER_Q8_H_

#include <stddef.h>

#include "feather_hip/feather_hip.h"
#include "feather_hip/feather_net.h"

#ifdef __cplusplus
extern "C"
{
#endif

#define FHIP_Q8_API __attribute__((visibility("default")))

/* The fields of fhip_qconv_param in the same order (int8_scale_term: 0 .. 200), plus the form of the input and of the output: 0 = dense
 * NCHW fp32, 1 = a q8 tensor. */
typedef struct fhip_q8_param
{
    int output_channels; /* K of the whole layer */
    int input_channels;  /* C of the whole layer */
    int input_h;
    int input_w;
    int kernel_h;
    int kernel_w;
    int output_h; /* set by fhip_q8_assign_output_dim */
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
    int input_int8;
    int output_int8;
} fhip_q8_param;

/* *bytes = batch * ceil(channels / 16) * h * w * 16.  FHIP_E_BADARG: NULL, a size < 1, 2^31 bytes or more. */
FHIP_Q8_API int fhip_q8_tensor_bytes(int batch, int channels, int h, int w, size_t* bytes);

/* output_h / output_w by the formula of feather_qconv.h.  FHIP_E_BADARG: NULL, sizes / strides < 1, a kernel larger than the padded input. */
FHIP_Q8_API int fhip_q8_assign_output_dim(fhip_q8_param* param);

/* 1 when the layer is one this library runs, else 0 (and the reason in fhip_q8_last_error).  Refused: everything fhip_qconv_supported
 * refuses (int8_scale_term: < 0 or > 200), input_int8 / output_int8 other than 0 / 1 or both 0, a q8 input or output image of 2^31 bytes or
 * more.  Every other entry point refuses the same params with FHIP_E_BADARG. */
FHIP_Q8_API int fhip_q8_supported(const fhip_q8_param* param);

/* Bytes of the scratch buffer (always 0) and of the packed weights.  Cheap, pure, no device call. */
FHIP_Q8_API int fhip_q8_get_buffer_size(const fhip_q8_param* param, int batch, size_t* scratch_bytes, size_t* packed_bytes);

/* kernel: signed char [K][C/group][kh][kw] (device) -> packed (device, packed_bytes, 16-byte aligned): one launch on `stream`, every
 * packed byte is written (the weights of pad channels as 0), so the call is idempotent.  FHIP_E_BADARG: NULL pointers, a packed pointer
 * that is not 16-byte aligned, a refused param, 2^31 packed bytes or more. */
FHIP_Q8_API int fhip_q8_init(const fhip_q8_param* param, void* packed, const signed char* kernel, void* stream);

/* fhip_qconv_dequant_scales, compiled from the same host function. */
FHIP_Q8_API int fhip_q8_dequant_scales(float* d, const float* s_w, int K, float s_in);

/* The layer: `in` is float [batch][C][H][W] or a q8 tensor (input_int8), `out` float [batch][K][OH][OW] or a q8 tensor (output_int8).
 * One launch on `stream` (a hipStream_t as void*), no allocation, no copy, no synchronisation: hipGraph-capturable.  `scratch` is unused
 * (may be NULL); d is [K] (device), bias [K] (device), read only with bias_term.  s_in is read only with an fp32 input (an int8 input is
 * taken as it is; its scale is in d), s_out only with an int8 output.
 * FHIP_E_BADARG: a refused param, batch < 1, NULL out / in / packed / d, NULL bias with bias_term, an fp32 tensor / d / bias that is not
 * 4-byte aligned, a q8 tensor or packed that is not 16-byte aligned, s_in (fp32 input) or s_out (int8 output) not finite or not > 0, an fp32
 * tensor of 2^31 elements or more, a q8 tensor of 2^31 bytes or more, 2^30 GEMM columns or more on an MFMA route, more than 65535 channel
 * blocks on the other routes.  FHIP_E_HIP: the launch failed. */
FHIP_Q8_API int fhip_q8_forward(const fhip_q8_param* param, int batch, void* out, const void* in, const void* packed, void* scratch, const float* d,
                                const float* bias, float s_in, float s_out, void* stream);

/* The kernel instantiation fhip_q8_forward launches for this layer, as the demangled name without return type and parameters.  The
 * template arguments end with <input is int8>, <output is int8>:
 *   fhip::q8_mfma_kernel<4, 1, I, O> / <2, 2, I, O>   group 1: the implicit GEMM of feather_qconv.h on v_mfma_i32_16x16x64_i8, 128 / 64
 *                                                     output channels per block (K > 64 / K <= 64); int8 in: any C; fp32 in: C % 16 == 0, int8 out
 *   fhip::q8_dw_kernel<O>                             int8 in, group == C == K, any kernel and stride: 16 channels per lane
 *   fhip::q8_generic_kernel<DW>                       fp32 in, int8 out, everything else: one pixel and 16 output channels per lane; DW: depthwise */
FHIP_Q8_API int fhip_q8_route(const fhip_q8_param* param, char* name, int len);

/* The three calls above for a NAMED route instead of the selected one.  The packed layout belongs to the route: pack with
 * fhip_q8_init_route under the same name.  FHIP_E_BADARG: an unknown name; FHIP_E_UNSUPPORTED: a route that cannot run this layer. */
FHIP_Q8_API int fhip_q8_get_buffer_size_route(const fhip_q8_param* param, int batch, const char* route, size_t* scratch_bytes, size_t* packed_bytes);
FHIP_Q8_API int fhip_q8_init_route(const fhip_q8_param* param, void* packed, const signed char* kernel, void* stream, const char* route);
FHIP_Q8_API int fhip_q8_forward_route(const fhip_q8_param* param, int batch, void* out, const void* in, const void* packed, void* scratch,
                                      const float* d, const float* bias, float s_in, float s_out, void* stream, const char* route);

/* out (q8 tensor of [batch][channels][h][w]) = quantise(in (float, dense NCHW); s), pad bytes 0.  One launch, capturable.
 * FHIP_E_BADARG: NULL, sizes < 1, a misaligned pointer, a bad s, 2^31 elements / bytes or more. */
FHIP_Q8_API int fhip_q8_quantize_forward(void* out, const float* in, int batch, int channels, int h, int w, float s, void* stream);

/* out (float, dense NCHW) = float(q) / s (one fp32 division, correctly rounded) of the q8 tensor `in`.  Same refusals. */
FHIP_Q8_API int fhip_q8_dequantize_forward(float* out, const void* in, int batch, int channels, int h, int w, float s, void* stream);

/* out = max(q, 0) byte for byte over `bytes` (a whole q8 tensor: a multiple of 16, below 2^31); out == in is allowed.  One launch. */
FHIP_Q8_API int fhip_q8_relu_forward(void* out, const void* in, size_t bytes, void* stream);

/* Max pooling of a q8 tensor into a q8 tensor: the byte-wise max over the taps inside the plane, with the geometry of fhip_pooling
 * (feather_net.h): the output size of fhip_pooling_output_dim, the window origin oy * stride - (pad_top + pad_bottom) (both pads), the
 * window clipped to the plane, global_pooling = the whole plane.  An empty window gives -127.  The pad bytes stay 0.
 * FHIP_E_BADARG: NULL, batch / channels / sizes < 1, pooling_type other than 0 (max), an empty output, a misaligned pointer, a tensor of
 * 2^31 bytes or more. */
FHIP_Q8_API int fhip_q8_max_pool_forward(const fhip_pool_param* param, int batch, void* out, const void* in, void* stream);

/* Message of this thread's last failing call of this library ("" if none). */
FHIP_Q8_API const char* fhip_q8_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* FEATHER_HIP_FEATHER_Q8_H_ */
