/* feather_atrous.h -- C-ABI of libfeather_atrous.so: dilated (atrous) convolution on the MI355X (gfx950).
 *
 * The reference has no dilation (ConvParam carries none) and fhip_conv_param stays field for field the reference's; this library is the
 * route of its own that runs a Convolution layer with dilation > 1.  The definition (this text is the contract): dense NCHW fp32 with a
 * leading batch, C = input_channels and K = output_channels of the WHOLE layer, group divides both, weights [K][C/group][kh][kw], bias
 * [K].  Output channel k belongs to group g = k / (K / group).
 *
 *     OH = (H + pad_top  + pad_bottom - (dilation_h * (kh - 1) + 1)) / stride_h + 1      (floor)
 *     OW = (W + pad_left + pad_right  - (dilation_w * (kw - 1) + 1)) / stride_w + 1      (floor)
 *     y[n][k][oy][ox] = act(bias[k] + sum_{c < C/group, i < kh, j < kw}
 *                           w[k][c][i][j] * x[n][g * C/group + c][oy * sh - pad_top + i * dh][ox * sw - pad_left + j * dw])
 *
 * Taps outside the plane contribute nothing: their addresses are clamped into the plane and the value is replaced by 0 (a select, never
 * a multiplication by a zero weight), so a non-finite input pixel only reaches the outputs whose window holds it.
 *
 * The library is separate from libfeather_hip.so and needs nothing from it but the enums of feather_hip.h (fhip_error,
 * fhip_activation): link or dlopen either or both.  It keeps its own last-error slot. */
#ifndef FEATHER_HIP_FEATHER_ATROUS_H_
#define FEATHER_HIP_FEATHER_ATROUS_H_

#include <stddef.h>

#include "feather_hip/feather_hip.h"

#ifdef __cplusplus
extern "C"
{
#endif

#define FHIP_ATROUS_API __attribute__((visibility("default")))

/* The fields of fhip_conv_param in the same order, plus the two dilations. */
typedef struct fhip_atrous_param
{
    int output_channels; /* K of the whole layer */
    int input_channels;  /* C of the whole layer */
    int input_h;
    int input_w;
    int kernel_h;
    int kernel_w;
    int output_h; /* set by fhip_atrous_assign_output_dim */
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
} fhip_atrous_param;

/* output_h / output_w from the formula above.  FHIP_E_BADARG: NULL, sizes / strides / dilations < 1, or a result < 1. */
FHIP_ATROUS_API int fhip_atrous_assign_output_dim(fhip_atrous_param* param);

/* 1 when the layer is one this library runs, else 0 (and the reason in fhip_atrous_last_error).  Refused: dilation_h == dilation_w == 1
 * (on purpose: those layers have tuned routes in libfeather_hip.so and libfeather_gconv.so), a dilation < 1, channels / input size /
 * kernel / stride < 1, a group that does not divide both channel counts, negative pads, a dilated kernel extent larger than the padded
 * input, output_h / output_w other than fhip_atrous_assign_output_dim's, an activation other than None / ReLU, an input or output image
 * of 2^31 elements or more.  Every other entry point refuses the same params with FHIP_E_BADARG. */
FHIP_ATROUS_API int fhip_atrous_supported(const fhip_atrous_param* param);

/* Bytes of the scratch buffer (always 0) and of the packed weights.  Cheap, pure, no device call.
 * FHIP_E_BADARG: NULL pointers, batch < 1, a refused param. */
FHIP_ATROUS_API int fhip_atrous_get_buffer_size(const fhip_atrous_param* param, int batch, size_t* scratch_bytes, size_t* packed_bytes);

/* kernel [K][C/group][kh][kw] (device) -> packed (device, packed_bytes): one launch on `stream`, every packed word is written, so the
 * call is idempotent.  FHIP_E_BADARG: NULL or not 4-byte aligned pointers (packed: 16-byte aligned), a refused param. */
FHIP_ATROUS_API int fhip_atrous_init(const fhip_atrous_param* param, float* packed, const float* kernel, void* stream);

/* out[batch][K][output_h][output_w] = act(conv(in[batch][C][input_h][input_w]) + bias): one launch on `stream` (a hipStream_t as void*),
 * no allocation, no copy, no synchronisation: hipGraph-capturable.  `scratch` is unused (may be NULL); `bias` is [K], read only with
 * bias_term.  FHIP_E_BADARG: a refused param, batch < 1, NULL out / in / packed, NULL bias with bias_term, a pointer that is not 4-byte
 * aligned (packed: 16-byte), a tensor of 2^31 elements or more.  FHIP_E_HIP: the launch failed. */
/* Size limits: FHIP_E_BADARG for 2^31 elements or more in one image (every entry point: fhip_atrous_supported is 0) or in a whole tensor, for
 * 2^30 GEMM columns or more on an MFMA route, for more than 65535 chunks of 4 output channels on the generic route, for an output plane of more
 * than 65535 blocks of 256 lanes on the depthwise routes; fhip_atrous_init for 2^31 packed floats or more; fhip_atrous_assign_output_dim for an
 * output side of 2^31 or more. */
FHIP_ATROUS_API int fhip_atrous_forward(const fhip_atrous_param* param, int batch, float* out, const float* in, const float* packed, float* scratch,
                                        const float* bias, void* stream);

/* The kernel instantiation fhip_atrous_forward launches for this layer (the same selection function), as the demangled name without
 * return type and parameters, e.g. "fhip::atrous_generic_kernel<4>", copied into name[len]. */
FHIP_ATROUS_API int fhip_atrous_route(const fhip_atrous_param* param, char* name, int len);

/* The three calls above for a NAMED route (a name fhip_atrous_route can return) instead of the selected one, so that routes can be timed
 * and checked against each other.  The packed layout belongs to the route: pack with fhip_atrous_init_route under the same name.
 * FHIP_E_BADARG: an unknown name; FHIP_E_UNSUPPORTED: a route that cannot run this layer (the MFMA forms need group 1 and
 * input_channels % 16 == 0, ROW4 stride_w 1, output_w % 4 == 0 and input_w >= 4, tap skipping at most 16 taps; the depthwise forms
 * group == C == K, a 3x3 kernel and their stride; their 16-byte forms output_w % 4 == 0 (stride 1: and input_w >= 4)). */
FHIP_ATROUS_API int fhip_atrous_get_buffer_size_route(const fhip_atrous_param* param, int batch, const char* route, size_t* scratch_bytes,
                                                      size_t* packed_bytes);
FHIP_ATROUS_API int fhip_atrous_init_route(const fhip_atrous_param* param, float* packed, const float* kernel, void* stream, const char* route);
FHIP_ATROUS_API int fhip_atrous_forward_route(const fhip_atrous_param* param, int batch, float* out, const float* in, const float* packed,
                                              float* scratch, const float* bias, void* stream, const char* route);

/* Message of this thread's last failing call of this library ("" if none). */
FHIP_ATROUS_API const char* fhip_atrous_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* FEATHER_HIP_FEATHER_ATROUS_H_ */
