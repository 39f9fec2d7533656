/* feather_inorm.h -- C-ABI of libfeather_inorm.so: ncnn's InstanceNorm and the element-wise activations of generative nets (leaky ReLU,
 * PReLU, Sigmoid, TanH, Clip) on the MI355X (gfx950).
 *
 * The reference has none of these layers.  The definitions (this text is the contract), dense NCHW fp32 with a leading batch, HW = h * w:
 *
 *   InstanceNorm   per (n, c) plane:  mean = sum(x) / HW,  var = sum((x - mean)^2) / HW  (biased),  a = gamma[c] / sqrt(var + eps),
 *                  y = act((x - mean) * a + beta[c]);  gamma == NULL is 1, beta == NULL is 0 (ncnn's affine = 0).
 *                  ncnn .param: 0=channels, 1=eps (default 0.001), 2=affine (default 1); .bin: gamma[channels], beta[channels], raw fp32,
 *                  only when affine.  A plane of one pixel is legal (var = 0, y = act(beta)).  eps = 0 is accepted as ncnn accepts it; a
 *                  constant plane is then undefined (0 * inf).  With eps > 0 a constant plane gives act(beta) exactly.
 *   ReLU           0=slope (default 0):                   y = x > 0 ? x : slope * x
 *   PReLU          0=num_slope, .bin slope[num_slope]:    y = x > 0 ? x : slope[num_slope == 1 ? 0 : c] * x
 *   Sigmoid                                               y = 1 / (1 + exp(-x))
 *   TanH                                                  y = tanh(x)
 *   Clip           0=min, 1=max (defaults -/+FLT_MAX):    y = min(max(x, min), max)
 *
 * The variance is never E[x^2] - E[x]^2: every plane (or chunk of a plane) is held on chip, its mean is taken first, then the sums of
 * (x - mean) and (x - mean)^2 (the corrected two-pass form); chunks of a split plane are merged with Chan's formula in chunk order.  No
 * floating-point atomics anywhere: results are bit-identical from run to run.
 *
 * The library is separate from libfeather_hip.so and needs nothing from it but the enums of feather_hip.h (fhip_error): link or dlopen
 * either or both.  It keeps its own last-error slot. */
#ifndef FEATHER_HIP_FEATHER_INORM_H_
#define FEATHER_HIP_FEATHER_INORM_H_

#include <stddef.h>

#include "feather_hip/feather_hip.h"

#ifdef __cplusplus
extern "C"
{
#endif

#define FHIP_INORM_API __attribute__((visibility("default")))

/* `act` of fhip_instance_norm_forward: applied in the store.  NONE and RELU are fhip_activation's values. */
enum fhip_inorm_act
{
    FHIP_INORM_ACT_NONE = 0,
    FHIP_INORM_ACT_RELU = 1,
    FHIP_INORM_ACT_LEAKY = 2 /* y > 0 ? y : slope * y */
};

/* `kind` of fhip_activation_forward. */
enum fhip_activation_kind
{
    FHIP_ACTIVATION_LEAKY_RELU = 0, /* slope = slope_or_min */
    FHIP_ACTIVATION_PRELU = 1,      /* slope_vector[c] (device); NULL: the shared slope slope_or_min */
    FHIP_ACTIVATION_SIGMOID = 2,
    FHIP_ACTIVATION_TANH = 3,
    FHIP_ACTIVATION_CLIP = 4        /* min = slope_or_min, max = max */
};

/* Bytes of scratch fhip_instance_norm_forward needs for this shape: 0 for the routes that read a plane once, 8 bytes per chunk of every
 * plane for the split-plane route.  Cheap, pure, no device call.  FHIP_E_BADARG: a dimension < 1, 2^31 elements or more, NULL. */
FHIP_INORM_API int fhip_instance_norm_get_buffer_size(int n, int c, int h, int w, size_t* scratch_bytes);

/* out[n][c][h][w] = act(instance_norm(in)): one launch (two for the split-plane route) on `stream` (a hipStream_t as void*), no
 * allocation, no copy, no synchronisation: hipGraph-capturable.  gamma / beta are [c] on the device or NULL; `scratch` holds
 * fhip_instance_norm_get_buffer_size bytes (may be NULL when that is 0) and must be 8-byte aligned; out must not overlap in.  16-byte
 * accesses when h * w is a multiple of 4 and out and in are 16-byte aligned, 4-byte accesses otherwise.
 * FHIP_E_BADARG: a dimension < 1, 2^31 elements or more, NULL out / in, NULL scratch where some is needed, a pointer that is not 4-byte
 * aligned, eps < 0 or not finite, an unknown act.  FHIP_E_HIP: a launch failed. */
/* Size limit (every entry point of this header): FHIP_E_BADARG for a tensor of 2^31 elements or more (n * c * h * w). */
FHIP_INORM_API int fhip_instance_norm_forward(int n, int c, int h, int w, float* out, const float* in, const float* gamma, const float* beta,
                                              float eps, int act, float slope, float* scratch, void* stream);

/* fhip_instance_norm_forward with the route given instead of selected: 0 one wave per plane (h * w <= 1024), 1 one 256-thread block per
 * plane (<= 4096), 2 one 1024-thread block per plane (<= 16384), 3 split planes (any size; scratch = 8 bytes per 4096-float chunk of every
 * plane, whatever fhip_instance_norm_get_buffer_size says for the selected route).  The same result up to rounding.  For measuring the
 * thresholds between the routes (tools/inorm_bench.py --routes) and for tests.  FHIP_E_BADARG also: an unknown route, a plane that does
 * not fit it. */
FHIP_INORM_API int fhip_instance_norm_forward_route(int route, int n, int c, int h, int w, float* out, const float* in, const float* gamma,
                                                    const float* beta, float eps, int act, float slope, float* scratch, void* stream);

/* The kernel instantiation fhip_instance_norm_forward launches for this shape and these pointers (the same selection function; the
 * pointers are only looked at for their alignment), as the demangled name without return type and parameters, e.g.
 * "fhip::inorm_plane_kernel<256, 64, true>", copied into name[len].  The split-plane route names its first kernel
 * (fhip::inorm_partial_kernel<..>); fhip::inorm_apply_kernel<..> with the same argument follows it. */
FHIP_INORM_API int fhip_instance_norm_route(int n, int c, int h, int w, const float* out, const float* in, char* name, int len);

/* out[n][c][hw] = f(in) element by element (see the table above); out may be in.  One launch on `stream`, no allocation.
 * FHIP_E_BADARG: a dimension < 1, 2^31 elements or more, NULL out / in, misaligned pointers, an unknown kind, Clip with min > max. */
FHIP_INORM_API int fhip_activation_forward(int kind, float* out, const float* in, int n, int c, int hw, float slope_or_min, float max,
                                           const float* slope_vector, void* stream);

/* Message of this thread's last failing call of this library ("" if none). */
FHIP_INORM_API const char* fhip_inorm_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* FEATHER_HIP_FEATHER_INORM_H_ */
