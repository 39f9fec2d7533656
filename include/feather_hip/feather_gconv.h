/* feather_gconv.h -- C-ABI of libfeather_gconv.so: grouped convolution, 1 < group < C, on the MI355X (gfx950).
 *
 * The reference refuses such a layer (ConvBooster::SelectAlgo returns -1, avx/booster.cpp:304-308) and so does fhip_conv_select_algo;
 * this library is the route of its own that runs it.  The definition is Caffe's / ncnn's: with C = input_channels and K = output_channels
 * of the WHOLE layer, output channel k belongs to group g = k / (K / group) and reads input channels [g * C / group, (g + 1) * C / group):
 *
 *     y[n][k][oy][ox] = act(bias[k] + sum_{c < C/group, i < kh, j < kw} w[k][c][i][j] * x[n][g * C/group + c][oy * sh - pt + i][ox * sw - pl + j])
 *
 * Tensors are dense NCHW fp32 with a leading batch; weights [K][C/group][kh][kw]; bias [K].  The library is separate from
 * libfeather_hip.so and needs nothing from it but the types of feather_hip.h (fhip_conv_param, fhip_error, fhip_activation): link or
 * dlopen either or both.  It keeps its own last-error slot. */
#ifndef FEATHER_HIP_FEATHER_GCONV_H_
#define FEATHER_HIP_FEATHER_GCONV_H_

#include <stddef.h>

#include "feather_hip/feather_hip.h"

#ifdef __cplusplus
extern "C"
{
#endif

#define FHIP_GCONV_API __attribute__((visibility("default")))

/* 1 when the layer is one this library runs, else 0 (and the reason in fhip_gconv_last_error):
 *   1 < group < input_channels (group == 1 and group == input_channels are refused on purpose: those layers have tuned routes in
 *   libfeather_hip.so), input_channels % group == 0, output_channels % group == 0, channels / input size / kernel / stride >= 1,
 *   pads >= 0, a kernel no larger than the padded input, output_h / output_w equal to what fhip_conv_assign_output_dim gives,
 *   activation None or ReLU.  Every other entry point refuses the same params with FHIP_E_BADARG. */
FHIP_GCONV_API int fhip_gconv_supported(const fhip_conv_param* param);

/* Bytes of the scratch buffer (0: the kernels need none) and of the packed weights.  Cheap, pure, no device call.
 * FHIP_E_BADARG: NULL pointers, batch < 1, a param fhip_gconv_supported refuses. */
FHIP_GCONV_API int fhip_gconv_get_buffer_size(const fhip_conv_param* param, int batch, size_t* scratch_bytes, size_t* packed_bytes);

/* kernel [K][C/group][kh][kw] (device) -> packed (device, packed_bytes): one launch on `stream`, every packed word is written, so the
 * call is idempotent.  FHIP_E_BADARG: NULL or not 4-byte aligned pointers, a refused param. */
FHIP_GCONV_API int fhip_gconv_init(const fhip_conv_param* param, float* packed, const float* kernel, void* stream);

/* out[batch][K][output_h][output_w] = act(conv(in[batch][C][input_h][input_w]) + bias): one launch on `stream` (a hipStream_t as void*),
 * no allocation, no copy, no synchronisation: hipGraph-capturable.  `scratch` is unused (may be NULL); `bias` is [K], read only with
 * bias_term.  FHIP_E_BADARG: a refused param, batch < 1, NULL out / in / packed, NULL bias with bias_term, a pointer that is not 4-byte
 * aligned, more than 2^31 lanes.  FHIP_E_HIP: the launch failed. */
/* Size limits: FHIP_E_BADARG at 2^31 lanes or more (batch * Ho * strips of the output row: 4 outputs per strip on the tuned routes, 1 on the
 * generic one) and for more than 65535 channel chunks; fhip_gconv_init for 2^31 packed floats or more.  Tensors beyond 2^31 elements are
 * supported within that (64-bit offsets). */
FHIP_GCONV_API int fhip_gconv_forward(const fhip_conv_param* param, int batch, float* out, const float* in, const float* packed, float* scratch,
                                      const float* bias, void* stream);

/* The kernel instantiation fhip_gconv_forward launches for these arguments (the same selection function), as the demangled name without
 * return type and parameters, e.g. "fhip::gconv3x3_kernel<16, 1, true>", copied into name[len].  Same refusals as fhip_gconv_forward. */
FHIP_GCONV_API int fhip_gconv_route(const fhip_conv_param* param, const float* out, const float* in, char* name, int len);

/* Message of this thread's last failing call of this library ("" if none). */
FHIP_GCONV_API const char* fhip_gconv_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* FEATHER_HIP_FEATHER_GCONV_H_ */
