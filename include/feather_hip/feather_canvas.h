/* feather_canvas.h -- C-ABI of libfeather_canvas.so: the Winograd F(6x6,3x3) transforms of chained layers whose V and M hold 2x2 IMAGE
 * CANVASES instead of images (MI355X, gfx950).
 *
 * F(6x6,3x3) computes whole 6 x 6 output tiles: a 14-pixel plane takes 3 x 3 tiles (18 pixels, 1.65 x the work needed), a 56-pixel plane
 * 10 x 10 (60 pixels, 1.15 x).  Four images of one channel on one canvas with a two-pixel zero seam between them,
 *
 *        +--------+--+--------+      canvas side 2H + 2:   14 + 2 + 14 = 30 = 5 tiles   (25 tiles for four images instead of 36)
 *        | n % 4  |  | n % 4  |                            56 + 2 + 56 = 114 = 19 tiles (361 instead of 400)
 *        |  = 0   |  |  = 1   |
 *        +--------+  +--------+      the seam is the pad-1 zero border of both neighbours, and it keeps every image at an even offset,
 *        +--------+  +--------+      so a 2 x 2 pooling cell never straddles a tile
 *        |  = 2   |  |  = 3   |
 *        +--------+--+--------+      image n of the batch is quadrant n % 4 of canvas n / 4
 *
 * is an ordinary pad-1 image of 2H + 2 pixels per side as far as the transforms' arithmetic and the tile GEMM go:
 * fhip_winograd_f63_canvas_param / fhip_winograd_f63_plan_canvas (feather_hip.h) give that image's geometry and plan, and
 * fhip_winograd_f63_tile_gemm runs on it unchanged at batch / 4.  What is not ordinary are the layer boundaries, which this library holds:
 *
 *   FHIP_CANVAS_ENTRY   a plain layer, 2x2 max pooling, then a canvas layer: the four pooled images go to their quadrants
 *   FHIP_CANVAS_INSIDE  canvas layer to canvas layer: the convolution's values on the seam are junk and are written as zeros
 *   FHIP_CANVAS_EXIT    a canvas layer, 2x2 max pooling, then a plain layer: every pooled quadrant becomes a zero-bordered image of its own
 *   fhip_canvas_output_transform   the last layer of a run: canvas tiles back to the ordinary [N][K][H][W] tensor (pooled or not)
 *
 * Same butterflies, the same fp32 values in the same order as the plain transforms (csrc/wino_butterfly.h): V', M and the output are
 * bit-identical to the plain stage kernels run on host-assembled canvases whose seam is zeroed between layers.
 *
 * The library is separate from libfeather_hip.so and needs nothing from it but the types of feather_hip.h; the Net runtime opens it at
 * run time when a run qualifies (fusion level 3, batch a multiple of 4).  It keeps its own last-error slot. */
#ifndef FEATHER_HIP_FEATHER_CANVAS_H_
#define FEATHER_HIP_FEATHER_CANVAS_H_

#include <stddef.h>

#include "feather_hip/feather_hip.h"

#ifdef __cplusplus
extern "C"
{
#endif

#define FHIP_CANVAS_API __attribute__((visibility("default")))

enum fhip_canvas_form
{
    FHIP_CANVAS_ENTRY = 1,
    FHIP_CANVAS_INSIDE = 2,
    FHIP_CANVAS_EXIT = 3
};

/* The chained transform of one boundary: layer `param`'s M -> [bias, ReLU, 2x2 max pooling for ENTRY and EXIT] -> layer `next`'s V'.
 * `param` and `next` are the layers' own (per-image) geometries, `batch` the number of images (a multiple of 4).  `plan` / `plan_next`
 * are the plans the two layers RUN with: fhip_winograd_f63_plan(layer, batch) for a plain one, fhip_winograd_f63_plan_canvas(layer,
 * batch, 2) for a canvas one (ENTRY: plain, canvas; INSIDE: canvas, canvas; EXIT: canvas, plain).  One launch on `stream`, no allocation.
 * FHIP_E_BADARG: NULL pointers, plans that do not belong to the layers.  FHIP_E_UNSUPPORTED: a pair this form does not take. */
/* Size limits: FHIP_E_BADARG at 2^31 canvas planes or more (batch / 4 * output_channels); fhip_canvas_output_transform returns FHIP_E_UNSUPPORTED
 * for more than 65535 output channels. */
FHIP_CANVAS_API int fhip_canvas_output_to_next_input(int form, const fhip_conv_param* param, const fhip_conv_param* next, int batch,
                                                     const fhip_winograd_plan* plan, const fhip_winograd_plan* plan_next, float* v_next,
                                                     const float* m, const float* bias, void* stream);

/* The output transform of a canvas layer: M (plan = fhip_winograd_f63_plan_canvas(param, batch, 2)) -> output[batch][K][H][W], or
 * [batch][K][H/2][W/2] behind the 2x2 max pooling when pool = 1.  The seam is dropped. */
FHIP_CANVAS_API int fhip_canvas_output_transform(const fhip_conv_param* param, int batch, const fhip_winograd_plan* plan, float* output,
                                                 const float* m, const float* bias, int pool, void* stream);

/* Message of this thread's last failing call of this library ("" if none). */
FHIP_CANVAS_API const char* fhip_canvas_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* FEATHER_HIP_FEATHER_CANVAS_H_ */
