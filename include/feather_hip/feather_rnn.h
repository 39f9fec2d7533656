/* feather_rnn.h -- C-ABI of libfeather_rnn.so: the recurrent core of ncnn's LSTM, GRU and RNN layers on the MI355X (gfx950), on fp32
 * tensors with a leading batch of sequences.
 *
 * The reference has no recurrent layer: this text is the definition, written from what ncnn's lstm.cpp, gru.cpp and rnn.cpp do.
 * tests/rnn_ref.py restates it line by line in float64.
 *
 * Notation       H = num_output; nd = 1 for direction 0 (forward) or 1 (reverse), 2 for direction 2 (bidirectional); G = 4 (LSTM), 3 (GRU),
 *                1 (RNN); sigmoid(x) = 1 / (1 + expf(-x)), tanh = tanhf: both give +-1, 0 or 1 for pre-activations of +-80 and never NaN.
 * Input          xp is [n][T] rows of nd * G * H floats, row (i, t) at element (i * T + t) * xp_stride (xp_stride >= nd * G * H).  It holds the
 *                input projections with the bias already added: xp[i][t][d][g][j] = Wx[d][g * H + j] . x[i][t] + b[d][g][j].  The caller
 *                computes them (one GEMM for all steps and both directions).
 * LSTM           gate rows in ncnn's order I, F, O, G.  For t along the direction: a[g] = xp[..][g][j] + Wh[d][g * H + j] . h_prev;
 *                I, F, O = sigmoid(a[0 .. 2]); Gt = tanh(a[3]); c = F * c_prev + I * Gt; h = O * tanh(c).
 * GRU            gate rows R, U, N.  ncnn's bias has four rows per direction, R, U, WN and BN: the first three are in xp, BN is passed as
 *                bn[nd][H].  R = sigmoid(a[0]); U = sigmoid(a[1]); N = tanh(xp[..][2][j] + R * (Wh[d][2H + j] . h_prev + bn[d][j]));
 *                h = (1 - U) * N + U * h_prev.
 * RNN            h = tanh(a[0]).
 * Output         out is [n][T][nd * H], row (i, t) at element (i * T + t) * out_stride (out_stride >= nd * H): columns [0, H) hold the
 *                forward direction, [H, 2H) the reverse one.  A reverse direction walks t = T - 1 .. 0 and writes its h at position t.
 * State          h0, c0: NULL (zeros) or [n][nd][H].  hn, cn: NULL or [n][nd][H]; they receive the state after the last step walked
 *                (t = T - 1 forward, t = 0 reverse).  c0 and cn are ignored for GRU and RNN.
 * Weights        Wh is [nd][G * H][H] fp32 in ncnn's layout, read in place (no packed form).
 * Arithmetic     products and sums are fp32, in an order that is fixed per route: the result is a function of the input.  The dot product
 *                Wh . h_prev is summed first and xp added to it.
 *
 * Routes (fhip_rnn_route).  No kernel of this library waits for another block: there is no grid barrier, no flag and no spin.  Work that
 * must be ordered across blocks is ordered by launch boundaries on the stream.
 *   the step route        ONE LAUNCH PER TIME STEP, enqueued by the one fhip_rnn_forward call: the entry is T launches, both directions in
 *                         the same launch.  A block owns FHIP_RNN_UNIT_TILE hidden units with all G gates of those units, and
 *                         FHIP_RNN_SEQ_TILE sequences, of one direction, so the pointwise part needs no second pass: it reads h_prev in
 *                         place from `out` at the previous position (h0 at the first step), runs Wh . h_prev over K = H, adds xp, applies
 *                         the gates, writes h to `out` and updates c in the caller's [nd][n][H] scratch, each element of which one block
 *                         owns.  H a multiple of FHIP_RNN_MFMA_MULTIPLE runs the product on v_mfma_f32_32x32x2_f32 (a wave per gate), every
 *                         other H on a direct kernel of the same ownership on plain multiply-adds.
 *   the sequence route    ONE LAUNCH.  A block owns (FHIP_RNN_SEQUENCE_TILE sequences, a direction) and walks all T steps itself: Wh of that
 *                         direction, h and c are resident on the chip, __syncthreads separates the steps.  It applies only where
 *                         fhip_rnn_sequence_fits(cell, H): G * H * H + 2 * FHIP_RNN_SEQUENCE_TILE * H <= FHIP_RNN_SEQUENCE_LDS_FLOATS.  It
 *                         exists for small H (the mobile recognisers' 48 .. 96), where T launches of a small kernel cost more than the
 *                         arithmetic.  fhip_rnn_forward takes it where it fits and n <= FHIP_RNN_SEQUENCE_MAX_N
 *                         (DESIGN.md 3.29 has the table the number came from).
 *
 * Refused with FHIP_E_BADARG, never truncated: an extent < 1; a stride below its row; tensors of 2^31 elements or more (strides included);
 * a cell, direction or route code out of range; NULL or 4-byte-unaligned pointers (bn for the GRU, the cell scratch for the LSTM; h0, c0,
 * hn and cn may be NULL); `out` overlapping xp; a forced sequence route that does not fit.  fhip_rnn_forward allocates nothing, copies
 * nothing and waits for nothing on the host; it may be captured in a hipGraph.
 *
 * Out of scope: an LSTM projection (hidden_size != num_output), int8 recurrent weights, sequences of different lengths within a batch, CTC
 * decoding (the application takes the argmax of the [T][classes] blob), any fusion into or across these layers, tuning beyond the route rule.
 * The library is separate from libfeather_hip.so and needs nothing from it but the enums of feather_hip.h; it keeps its own last-error slot. */
#ifndef FEATHER_HIP_FEATHER_RNN_H_
#define FEATHER_HIP_FEATHER_RNN_H_

#include <stddef.h>

#include "feather_hip/feather_hip.h"

#ifdef __cplusplus
extern "C"
{
#endif

#define FHIP_RNN_API __attribute__((visibility("default")))

/* Route code fhip_net_layer_info reports for the LSTM, GRU and RNN layers of a net with fhip_net_set_recurrent (feather_net.h). */
#define FHIP_RNN_NET_ROUTE 114

/* cell */
#define FHIP_RNN_LSTM 0
#define FHIP_RNN_GRU 1
#define FHIP_RNN_RNN 2

/* route of fhip_rnn_forward_route and fhip_rnn_route */
#define FHIP_RNN_ROUTE_AUTO 0     /* the rule below */
#define FHIP_RNN_ROUTE_STEP 1     /* T launches */
#define FHIP_RNN_ROUTE_SEQUENCE 2 /* one launch; refused where fhip_rnn_sequence_fits says 0 */

#define FHIP_RNN_UNIT_TILE 32    /* hidden units per block of the step route (the rows of one 32x32 matrix tile) */
#define FHIP_RNN_SEQ_TILE 32     /* sequences per block of the step route (its columns) */
#define FHIP_RNN_MFMA_MULTIPLE 4 /* the step route runs on the matrix instruction where H is a multiple of this, else on the direct kernel */
#define FHIP_RNN_SEQUENCE_TILE 4 /* sequences per block of the sequence route */
/* The sequence route's bound.  A workgroup of gfx950 may declare 160 KiB of LDS = 40960 floats.  The block keeps Wh of its direction
 * (G * H * H floats, k-major) and h of its FHIP_RNN_SEQUENCE_TILE sequences twice (read at step t, written for step t + 1); c lives in
 * registers.  So: G * H * H + 2 * FHIP_RNN_SEQUENCE_TILE * H <= 40960, which is H <= 100 (LSTM), 115 (GRU), 198 (RNN). */
#define FHIP_RNN_SEQUENCE_LDS_FLOATS 40960
#define FHIP_RNN_SEQUENCE_MAX_H_LSTM 100
#define FHIP_RNN_SEQUENCE_MAX_H_GRU 115
#define FHIP_RNN_SEQUENCE_MAX_H_RNN 198
/* The rule where both routes apply: the sequence route up to this many sequences, the step route above.  tools/rnn_bench.py measured both
 * over n in {1, 4, 32, 256} x H in {48, 96} x T in {26, 100} (DESIGN.md 3.29 has the table): the sequence route was 1.6 to 2.8 times faster
 * in every row, so the bound is the largest batch measured.  Above it the blocks outnumber the compute units (one block of 160 KiB a unit),
 * which nobody has measured. */
#define FHIP_RNN_SEQUENCE_MAX_N 256

/* 1 where G * H * H + 2 * FHIP_RNN_SEQUENCE_TILE * H <= FHIP_RNN_SEQUENCE_LDS_FLOATS for the cell, else 0 (also for a cell out of range or h < 1). */
FHIP_RNN_API int fhip_rnn_sequence_fits(int cell, int h);

/* out[n][t][nd * h] = the recurrence over xp as defined above, on `stream` (a hipStream_t as void*): T launches on the step route, one on the
 * sequence route.  wh: DEVICE [nd][G * h][h].  bn: DEVICE [nd][h], GRU only (ignored otherwise).  cell_scratch: DEVICE [nd][n][h] floats, LSTM
 * only (ignored otherwise; never read before it is written).  FHIP_E_BADARG as listed above. */
FHIP_RNN_API int fhip_rnn_forward(int cell, int direction, int n, int t, int h, const float* xp, int xp_stride, const float* wh, const float* bn,
                                  const float* h0, const float* c0, float* out, int out_stride, float* hn, float* cn, float* cell_scratch,
                                  void* stream);

/* The same with the route named (FHIP_RNN_ROUTE_*): what tools/rnn_bench.py measures both routes with. */
FHIP_RNN_API int fhip_rnn_forward_route(int cell, int direction, int n, int t, int h, const float* xp, int xp_stride, const float* wh,
                                        const float* bn, const float* h0, const float* c0, float* out, int out_stride, float* hn, float* cn,
                                        float* cell_scratch, void* stream, int route);

/* The kernel instantiation a call would launch (T times on the step route), as the demangled name without return type and parameters,
 * copied into name[len]; CELL is the cell code:
 *   "fhip::rnn_sequence_kernel<CELL>"      route SEQUENCE, or AUTO where it fits and n <= FHIP_RNN_SEQUENCE_MAX_N
 *   "fhip::rnn_step_mfma_kernel<CELL>"     else, where h % FHIP_RNN_MFMA_MULTIPLE == 0
 *   "fhip::rnn_step_direct_kernel<CELL>"   else
 * FHIP_E_BADARG: NULL name, len < 1, arguments the forward call would refuse. */
FHIP_RNN_API int fhip_rnn_route(int cell, int h, int n, int t, int route, char* name, int len);

/* Message of this thread's last failing call of this library ("" if none). */
FHIP_RNN_API const char* fhip_rnn_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* FEATHER_HIP_FEATHER_RNN_H_ */
