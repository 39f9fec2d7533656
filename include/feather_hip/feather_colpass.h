/* feather_colpass.h -- C-ABI of libfeather_colpass.so: the Winograd F(6x6,3x3) tile GEMM of 64-input-channel layers that writes the
 * COLUMN-PASSED M (48 planes instead of 64), and the chained transform that reads it (MI355X, gfx950).
 *
 * Every reader of M begins with the column pass of the output transform, tmp[a][j] = at6(m[0][j] .. m[7][j]) (8 -> 6, csrc/wino_butterfly.h),
 * which combines the eight frequency points xi = 8 i + j of one j, element for element.  A GEMM block that computes those eight xi for
 * its rows and columns holds the eight accumulators of one element in the same lane and register: it applies at6 across them and stores
 * six planes.  M48 is in wino_layout(K, Pp, BP, 48), plane 8 a + j -- three quarters of M on the write and again on the read, which is what
 * the HBM-bound 224- and 112-pixel layers of VGG-16 pay for.
 *
 * at6 multiplies by powers of two only: every product is exact, so contraction into FMAs cannot change a bit.  The GEMM is the main
 * library's instruction in the main library's k order from a zero start.  tmp, V' and everything behind them are bit-identical to
 * fhip_winograd_f63_tile_gemm followed by fhip_winograd_f63_output_to_next_input.
 *
 * The library is separate from libfeather_hip.so and needs nothing from it but the types of feather_hip.h; the Net runtime opens it at
 * run time when a layer qualifies (fhip_net_set_colpass).  It keeps its own last-error slot. */
#ifndef FEATHER_HIP_FEATHER_COLPASS_H_
#define FEATHER_HIP_FEATHER_COLPASS_H_

#include <stddef.h>

#include "feather_hip/feather_hip.h"

#ifdef __cplusplus
extern "C"
{
#endif

#define FHIP_COLPASS_API __attribute__((visibility("default")))

/* FHIP_OK if this layer at this batch runs here: a 3x3 / stride-1 / group-1 convolution on the F(6x6,3x3) route (not the 7- and 8-pixel
 * planes of F(4x4,3x3)) with input_channels == 64 and output_channels a multiple of 64, within the main route's 32-bit limit
 * (batch * tiles per image at most 0x7fffff00).  FHIP_E_UNSUPPORTED with a message otherwise, FHIP_E_BADARG for NULL or batch < 1. */
FHIP_COLPASS_API int fhip_colpass_supported(const fhip_conv_param* param, int batch);

/* The tile GEMM: u = the main library's packed filter as it is ([64][Cp][Kp], fhip_winograd_f63_transform_kernel), v in the layout of
 * `plan` = fhip_winograd_f63_plan(param, batch), m48 = 48 planes in wino_layout(K, columns_padded, column_block, 48): 48 * K *
 * columns_padded floats, which fit the m_bytes of `plan`.  One launch on `stream`, no allocation.
 * FHIP_E_BADARG: NULL pointers, a plan that does not belong to the layer.  FHIP_E_UNSUPPORTED: as fhip_colpass_supported. */
FHIP_COLPASS_API int fhip_colpass_tile_gemm(const fhip_conv_param* param, int batch, const fhip_winograd_plan* plan, float* m48, const float* u,
                                            const float* v, void* stream);

/* The chained transform of one boundary from m48: row pass, bias, ReLU, the 2x2 / stride-2 max pooling when pool != 0, then B^T d B of
 * `next` (3x3 / stride-1 / pad-1, next.input_channels == param.output_channels) into its V' (plan_next = fhip_winograd_f63_plan(next,
 * batch)), in fhip_winograd_f63_output_to_next_input's order.  Forms: pooled (any plane the consumer's block holds; output dims even) and
 * unpooled with at most 512 tiles per plane.  FHIP_E_BADARG at 2^31 planes (batch * output_channels) or more. */
FHIP_COLPASS_API int fhip_colpass_output_to_next_input(const fhip_conv_param* param, const fhip_conv_param* next, int batch,
                                                       const fhip_winograd_plan* plan, const fhip_winograd_plan* plan_next, float* v_next,
                                                       const float* m48, const float* bias, int pool, void* stream);

/* Message of this thread's last failing call of this library ("" if none). */
FHIP_COLPASS_API const char* fhip_colpass_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* FEATHER_HIP_FEATHER_COLPASS_H_ */
