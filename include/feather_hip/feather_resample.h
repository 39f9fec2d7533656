/* feather_resample.h -- C-ABI of libfeather_resample.so: Interp (nearest and bilinear resize of fp32 planes) and HardSwish on the MI355X
 * (gfx950): the up-sampling layer of segmentation and detection decoders (DeepLab, FPN, YOLOv3, bilinear U-Nets, LR-ASPP) and the
 * activation of MobileNet-V3.
 *
 * The reference has neither layer; it holds ncnn's resize convention for uint8 images (src/ncnn/mat_pixel_resize.cpp:33-68), which
 * feathercnn_amd/csrc/pixel_resample.h restates.  This text is the definition, on dense NCHW fp32 with a leading batch; every (n, c)
 * plane is resized on its own.
 *
 *   Interp parameters, as ncnn writes them: 0 = resize_type (1 nearest, 2 bilinear), 1 = height_scale, 2 = width_scale,
 *                  3 = output_height, 4 = output_width, 6 = align_corner.  Bicubic (3) and dynamic_target_size (5) are left out.
 *   output size    out_h = output_height if that is non-zero, else (int)(in_h * height_scale) with the product in fp32; the same across.
 *                  A layer with a second bottom takes that blob's height and width ("the size was given").
 *   nearest        out[dy][dx] = in[sy][sx],  sy = min((int)(dy * hs), in_h - 1),  sx = min((int)(dx * ws), in_w - 1), the products in
 *                  fp32;  hs = in_h / (float)out_h when the size was given, else 1.f / height_scale;  ws likewise.  align_corner is not
 *                  looked at.
 *   bilinear       per axis, for dx in 0 .. out_w - 1 (mat_pixel_resize.cpp:51-68; the double expression is rounded to fp32 once):
 *                      fx = (float)((dx + 0.5) * ((double)in_w / out_w) - 0.5)
 *                      align_corner:  fx = (float)(dx * ((double)(in_w - 1) / (out_w - 1))),  the factor 0 when out_w = 1
 *                      sx = floor(fx);  fx -= sx;
 *                      if (sx < 0)         { sx = 0;        fx = 0.f; }
 *                      if (sx >= in_w - 1) { sx = in_w - 2; fx = 1.f; }
 *                  The taps are columns max(sx, 0) and min(sx + 1, in_w - 1): a plane one pixel wide or high replicates and nothing
 *                  outside the plane is read.  With rows S0 (tap max(sy, 0)) and S1 (tap min(sy + 1, in_h - 1)):
 *                      r0  = S0[x0] * (1.f - fx) + S0[x1] * fx
 *                      r1  = S1[x0] * (1.f - fx) + S1[x1] * fx
 *                      out = r0 * (1.f - fy) + r1 * fy
 *                  Every difference, product and sum is rounded to fp32 on its own (no fused multiply-add): the result is defined bit
 *                  for bit, and tests/resample_ref.py restates it in numpy.
 *   residual, relu out = relu(fl(interp + residual)): the sum is rounded on its own and the ReLU follows it, so the fused call equals
 *                  the resize followed by fhip_add (and fhip_relu) bit for bit.
 *   HardSwish      ncnn's ids 0 = alpha, 1 = beta, defaults 0.2 and 0.5 (MobileNet-V3 writes 1/6 and 0.5).  In fp32:
 *                      lower = -beta / alpha,  upper = 1.f / alpha + lower
 *                      y = 0 if x < lower;  x if x > upper;  else x * (x * alpha + beta), the product and the sum rounded separately.
 *
 * No atomics: results are bit-identical from run to run.  No entry allocates, copies or synchronises: every one is hipGraph-capturable.
 * Pointers need 4-byte alignment only; the 16-byte paths are chosen by looking at the pointers and the widths (fhip_interp_route).
 *
 * Size limit (every entry point): FHIP_E_BADARG for a tensor of 2^31 elements or more, input or output.
 *
 * The library is separate from libfeather_hip.so and needs nothing from it but the enums of feather_hip.h (fhip_error): link or dlopen
 * either or both.  It keeps its own last-error slot. */
#ifndef FEATHER_HIP_FEATHER_RESAMPLE_H_
#define FEATHER_HIP_FEATHER_RESAMPLE_H_

#include <stddef.h>

#include "feather_hip/feather_hip.h"

#ifdef __cplusplus
extern "C"
{
#endif

#define FHIP_RESAMPLE_API __attribute__((visibility("default")))

/* `mode` of the Interp entries: ncnn's resize_type. */
enum fhip_interp_mode
{
    FHIP_INTERP_NEAREST = 1,
    FHIP_INTERP_BILINEAR = 2
};

/* The output size of an Interp layer as defined above.  output_height / output_width 0: the scale decides, and must be finite and
 * positive; non-zero: the size is taken and the scale of that axis is not looked at.  Cheap, pure, no device call.
 * FHIP_E_BADARG: an input dimension < 1, a scale (that is used) not finite or not positive, an output dimension < 1 or of 2^31 or more,
 * NULL out_h / out_w. */
FHIP_RESAMPLE_API int fhip_interp_output_dim(int in_h, int in_w, float height_scale, float width_scale, int output_height, int output_width,
                                             int* out_h, int* out_w);

/* out[n][c][out_h][out_w] = relu?( interp(in[n][c][in_h][in_w]) [+ residual[n][c][out_h][out_w]] ) as defined above: one launch on `stream`
 * (a hipStream_t as void*).  height_scale / width_scale: the layer's scale where it decided the output size, 0 where the size was given
 * (read by NEAREST only).  residual may be NULL; relu is 0 or 1.  out may be residual; out must not overlap in.
 * FHIP_E_BADARG: an unknown mode, a dimension < 1, 2^31 elements or more in either tensor, NULL out / in, a pointer that is not 4-byte
 * aligned, out overlapping in, a scale that is neither 0 nor finite and positive, relu outside 0 / 1.  FHIP_E_HIP: the launch failed. */
FHIP_RESAMPLE_API int fhip_interp_forward(int mode, int align_corner, int n, int c, int in_h, int in_w, int out_h, int out_w, float height_scale,
                                          float width_scale, float* out, const float* in, const float* residual, int relu, void* stream);

/* The kernel instantiation fhip_interp_forward launches for these arguments (the same selection; the pointers are only looked at for
 * their alignment, NULL counts as aligned), as the demangled name without return type and parameters, copied into name[len]:
 *   "fhip::interp_nearest2x_kernel"   NEAREST, out = 2 x in on both axes with steps of exactly 0.5, in_w even, out and residual 16-byte
 *                                     and in 8-byte aligned: a lane turns two input pixels into one 16-byte store on each of two rows
 *   "fhip::interp_vec4_kernel<M>"     M = 1 nearest, 2 bilinear: out_w a multiple of 4, out and residual 16-byte aligned, no axis
 *                                     scaled down: a lane produces four adjacent outputs of a row for one 16-byte store, on four rows
 *   "fhip::interp_gather_kernel<M>"   everything else: one output column per lane, four rows, 4-byte accesses */
FHIP_RESAMPLE_API int fhip_interp_route(int mode, int n, int c, int in_h, int in_w, int out_h, int out_w, float height_scale, float width_scale,
                                        const float* out, const float* in, const float* residual, char* name, int len);

/* out[n][c][hw] = HardSwish(in; alpha, beta) element by element as defined above; out may be in.  One grid-strided launch, 16-byte accesses
 * when the element count is a multiple of 4 and both pointers are 16-byte aligned, 4-byte accesses otherwise.
 * FHIP_E_BADARG: a dimension < 1, 2^31 elements or more, NULL out / in, a pointer that is not 4-byte aligned, alpha or beta not finite,
 * alpha = 0. */
FHIP_RESAMPLE_API int fhip_hardswish_forward(float* out, const float* in, int n, int c, int hw, float alpha, float beta, void* stream);

/* The instantiation fhip_hardswish_forward launches: "fhip::hardswish_kernel<true>" (16-byte) or "fhip::hardswish_kernel<false>". */
FHIP_RESAMPLE_API int fhip_hardswish_route(const float* out, const float* in, int n, int c, int hw, char* name, int len);

/* Message of this thread's last failing call of this library ("" if none). */
FHIP_RESAMPLE_API const char* fhip_resample_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* FEATHER_HIP_FEATHER_RESAMPLE_H_ */
