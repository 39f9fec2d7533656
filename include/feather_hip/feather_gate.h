/* feather_gate.h -- C-ABI of libfeather_gate.so: squeeze-and-excitation (SE) channel gating and the activations of the nets built on it
 * (Swish, HardSigmoid) on the MI355X (gfx950).
 *
 * The reference has none of these layers.  The definitions (this text is the contract), dense NCHW fp32 with a leading batch, HW = h * w:
 *
 *   channel gate   out[n][c][i] = act( fl(in[n][c][i] * gate[n][c]) [+ residual[n][c][i]] ),  act NONE or RELU.  The product and the sum
 *                  are rounded separately (no fused multiply-add): the call equals a multiply followed by fhip_add bit for bit.
 *                  ncnn writes the multiply as `BinaryOp 0=2` with two bottoms or as `Scale 0=-233` with two bottoms.
 *   squeeze        mean[n][c] = sum(in[n][c][:]) / HW (ncnn's global average Pooling).  The order of the sum is fixed by the shape and the
 *                  alignment alone.
 *   excite         per image:  gate = gact( W2 . mact( W1 . mean + b1 ) + b2 ),  W1 [R][C], W2 [C][R], b1 [R], b2 [C], row-major: the .bin
 *                  order of an InnerProduct and of a 1x1 Convolution alike.  mact NONE, RELU or SWISH; gact SIGMOID or HARDSIGMOID.
 *   Swish          y = x / (1 + exp(-x))                          (ncnn: no params)
 *   HardSigmoid    y = min(max(alpha * x + beta, 0), 1)           (ncnn: 0=alpha, 1=beta, defaults 0.2 and 0.5); the product and the sum
 *                  are rounded separately.
 *
 * No floating-point atomics anywhere: results are bit-identical from run to run.  No entry allocates, copies or synchronises: every one
 * is hipGraph-capturable.
 *
 * The library is separate from libfeather_hip.so and needs nothing from it but the enums of feather_hip.h (fhip_error): link or dlopen
 * either or both.  It keeps its own last-error slot. */
#ifndef FEATHER_HIP_FEATHER_GATE_H_
#define FEATHER_HIP_FEATHER_GATE_H_

#include <stddef.h>

#include "feather_hip/feather_hip.h"

#ifdef __cplusplus
extern "C"
{
#endif

#define FHIP_GATE_API __attribute__((visibility("default")))

/* `act` of fhip_channel_gate_forward: fhip_activation's values. */
enum fhip_gate_act
{
    FHIP_GATE_ACT_NONE = 0,
    FHIP_GATE_ACT_RELU = 1
};

/* `kind` of fhip_gate_activation_forward. */
enum fhip_gate_kind
{
    FHIP_GATE_SWISH = 0,
    FHIP_GATE_HARDSIGMOID = 1
};

/* `mact` / `gact` of fhip_excite_forward. */
enum fhip_excite_mact
{
    FHIP_EXCITE_MACT_NONE = 0,
    FHIP_EXCITE_MACT_RELU = 1,
    FHIP_EXCITE_MACT_SWISH = 2
};
enum fhip_excite_gact
{
    FHIP_EXCITE_GACT_SIGMOID = 0,
    FHIP_EXCITE_GACT_HARDSIGMOID = 1 /* alpha, beta */
};

/* `op` of fhip_gate_route. */
enum fhip_gate_op
{
    FHIP_GATE_OP_APPLY = 0,
    FHIP_GATE_OP_SQUEEZE = 1,
    FHIP_GATE_OP_EXCITE = 2,
    FHIP_GATE_OP_ACTIVATION = 3
};

/* out = act(in * gate [+ residual]) as defined above: one launch on `stream` (a hipStream_t as void*).  gate is [n][c] on the device;
 * residual is [n][c][h][w] or NULL; out may be in or residual.  16-byte accesses when h * w is a multiple of 4 and out, in and residual
 * are 16-byte aligned, 4-byte accesses otherwise.
 * FHIP_E_BADARG: a dimension < 1, 2^31 elements or more, NULL out / in / gate, a pointer that is not 4-byte aligned, an unknown act.
 * FHIP_E_HIP: a launch failed. */
/* Size limit (every entry point of this header): FHIP_E_BADARG for a tensor of 2^31 elements or more (n * c * h * w; n * c and c * r for
 * fhip_excite_forward, whose n is at most 65535).  The kernels index elements in unsigned 32-bit arithmetic up to that limit. */
FHIP_GATE_API int fhip_channel_gate_forward(int n, int c, int h, int w, float* out, const float* in, const float* gate, const float* residual, int act,
                                            void* stream);

/* Bytes of scratch fhip_squeeze_forward needs for this shape: 0 for planes of up to 16384 floats (read by one block, or by a group of
 * lanes of one wave up to 4096), 4 bytes per 16384-float chunk of every plane for larger ones (the split route).  Cheap, pure, no device
 * call.  FHIP_E_BADARG: a dimension < 1, 2^31 elements or more, NULL. */
FHIP_GATE_API int fhip_squeeze_get_buffer_size(int n, int c, int h, int w, size_t* scratch_bytes);

/* mean[n][c] = sum(in[n][c][:]) / HW: one launch (two on the split route: chunk sums to `scratch`, then their sum in chunk order).
 * `scratch` holds fhip_squeeze_get_buffer_size bytes (may be NULL when that is 0).  16-byte accesses when h * w is a multiple of 4 and in
 * is 16-byte aligned, 4-byte accesses otherwise.
 * FHIP_E_BADARG: a dimension < 1, 2^31 elements or more, NULL mean / in, NULL scratch where some is needed, a pointer that is not 4-byte
 * aligned. */
FHIP_GATE_API int fhip_squeeze_forward(int n, int c, int h, int w, float* mean, const float* in, float* scratch, void* stream);

/* gate[n][c] = gact(W2 . mact(W1 . mean[n] + b1) + b2) as defined above: one launch; the output channels of an image are dealt out to
 * 1 .. 8 blocks, chosen from n.  c, r >= 1, any values; b1 and b2 may be NULL; alpha and beta are read for HARDSIGMOID only.  gate must not overlap mean.
 * FHIP_E_BADARG: a dimension < 1 (n above 65535), 2^31 elements or more in a tensor or a weight matrix, NULL gate / mean / w1 / w2, a
 * pointer that is not 4-byte aligned, an unknown mact / gact, alpha or beta that is not finite. */
FHIP_GATE_API int fhip_excite_forward(int n, int c, int r, float* gate, const float* mean, const float* w1, const float* b1, const float* w2,
                                      const float* b2, int mact, int gact, float alpha, float beta, void* stream);

/* fhip_excite_forward with the output channels of an image dealt out to `slices` blocks (1 .. 1024, at most c), each of which recomputes
 * the hidden vector.  The same result bit for bit.  For measuring the split (tools/gate_bench.py) and for tests. */
FHIP_GATE_API int fhip_excite_forward_slices(int slices, int n, int c, int r, float* gate, const float* mean, const float* w1, const float* b1,
                                             const float* w2, const float* b2, int mact, int gact, float alpha, float beta, void* stream);

/* out[n][c][hw] = f(in) element by element, f = Swish or HardSigmoid(alpha, beta); out may be in.  One launch, no allocation.
 * FHIP_E_BADARG: a dimension < 1, 2^31 elements or more, NULL out / in, misaligned pointers, an unknown kind, alpha or beta not finite. */
FHIP_GATE_API int fhip_gate_activation_forward(int kind, float* out, const float* in, int n, int c, int hw, float alpha, float beta, void* stream);

/* The kernel instantiation the entry named by `op` launches for this shape and these pointers (the same selection; the pointers are only
 * looked at for their alignment, NULL counts as aligned), as the demangled name without return type and parameters, e.g.
 * "fhip::gate_apply_kernel<true>", copied into name[len].  APPLY looks at out, in and residual; SQUEEZE at in (the split route names
 * fhip::squeeze_block_kernel<..>, fhip::squeeze_merge_kernel follows it); EXCITE at nothing ("fhip::excite_kernel"); ACTIVATION at out
 * and in, with h * w as its hw. */
FHIP_GATE_API int fhip_gate_route(int op, int n, int c, int h, int w, const float* out, const float* in, const float* residual, char* name, int len);

/* Message of this thread's last failing call of this library ("" if none). */
FHIP_GATE_API const char* fhip_gate_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* FEATHER_HIP_FEATHER_GATE_H_ */
