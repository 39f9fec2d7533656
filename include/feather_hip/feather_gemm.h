/* feather_gemm.h -- C-ABI of libfeather_gemm.so: the product of two RUN-TIME matrices on the MI355X (gfx950) -- ncnn's Gemm and MatMul --
 * batched, with either operand transposed, at arbitrary M, N, K, on fp32 row-major tensors.
 *
 * This text is the definition; tests/gemm_ref.py restates it in float64.  For b in [0, batch):
 *
 *      D[b] = alpha * op(A[b]) * op(B[b]) + beta * bcast(C[b])
 *
 *   op(A) is M x K, stored [M][K] (row m at m * lda) or, with trans_a, [K][M] (row k at k * lda).
 *   op(B) is K x N, stored [K][N] (row k at k * ldb) or, with trans_b, [N][K] (row n at n * ldb).
 *   D     is M x N, stored [M][N] (row m at m * ldd) or, with out_transpose, D^T as [N][M] (row n at n * ldd).
 *   C     by c_broadcast:  -1 none (the pointer is not read, beta is ignored)      0 a scalar, C[0]
 *                           1 a value per row, C[m] of M floats                     2 the same as [M][1]
 *                           3 the full [M][N], row m at m * ldc                     4 a value per column, C[n] of N floats
 *         C is always addressed by the (m, n) of the UNtransposed D, whatever out_transpose says.
 *   A leading dimension may exceed the row length (a view cut out of a larger buffer); ldc is read for c_broadcast 3 only.
 *   Matrix b of an operand lies b * <x>_batch_stride floats behind matrix 0; a stride of 0 broadcasts the operand to every b (not D's, unless
 *   batch is 1).
 *
 * On the matrix pipe each element of D is ONE accumulation chain over k in increasing order in fp32 (v_mfma_f32_32x32x2_f32 takes two k a
 * step).  The thin kernel splits k in a fixed way -- a lane takes every 64th group of four k and the 64 lanes are added in a fixed tree, or
 * a lane takes every 16th k and the 16 slices are added in order -- so its sums are as reproducible.  Then alpha * acc (+ beta * c), each
 * product and sum rounded.  No result depends on the grid, the tile rule or the batch.
 *
 * Kernels.  min(M, N) <= FHIP_GEMM_THIN_MAX: gemm_thin_kernel, no matrix instruction (a vector times a matrix, a decoding step).  Else
 * gemm_kernel on the matrix pipe: a block of four waves owns FHIP_GEMM_TILE_WIDE^2 of D where that still gives FHIP_GEMM_WIDE_BLOCKS blocks
 * (two a CU on 256 CUs) and both M and N exceed FHIP_GEMM_TILE_SMALL (measured: p v with N = 64 loses a quarter at the wide tile), else
 * FHIP_GEMM_TILE_SMALL^2.  `tile` of the description forces a tile (and the matrix kernel): a measuring aid
 * (tools/gemm_bench.py) and what lets a test reach each tile at a small shape.  out_transpose and the orientation of the thin kernel cost
 * nothing: D^T = op(B)^T op(A)^T, the host swaps the operands.  No padded copy of an operand is made anywhere.
 *
 * Limits, refused with FHIP_E_BADARG and never truncated: M, N, K, batch >= 1; a leading dimension below its row length; a negative batch
 * stride; a D batch stride of 0 with batch > 1; every tensor -- (batch - 1) * batch_stride + (rows - 1) * ld + row length -- below
 * FHIP_GEMM_MAX_ELEMENTS = 2^31 floats, so that every offset inside a tensor fits 32 bits; batch * blocks below 2^31; flags outside 0 / 1;
 * c_broadcast outside -1 .. 4; alpha or beta not finite; NULL (C only where c_broadcast is -1) or unaligned pointers.  FHIP_E_UNSUPPORTED: a
 * `tile` other than 0, 64, 128.  No entry allocates, copies or synchronises; the forward is ONE launch and hipGraph-capturable.  Pointers
 * need 4-byte alignment; 16-byte loads are used per operand where its pointer, leading dimension and batch stride are multiples of 4
 * floats, 4-byte ones otherwise.  D must not overlap an input.  The library is separate from libfeather_hip.so and needs nothing from it
 * but the enums of feather_hip.h; it keeps its own last-error slot. */
#ifndef FEATHER_HIP_FEATHER_GEMM_H_
#define FEATHER_HIP_FEATHER_GEMM_H_

#include <stddef.h>

#include "feather_hip/feather_hip.h"

#ifdef __cplusplus
extern "C"
{
#endif

#define FHIP_GEMM_API __attribute__((visibility("default")))

/* Route code fhip_net_layer_info reports for the layers of a net with fhip_net_set_gemm (feather_net.h): Gemm, MatMul. */
#define FHIP_GEMM_NET_ROUTE 121

#define FHIP_GEMM_TILE_SMALL 64    /* rows and columns of D a block owns: four waves of 32 x 32 */
#define FHIP_GEMM_TILE_WIDE 128    /* four waves of 64 x 64 (2 x 2 matrix tiles, 64 accumulator registers) */
#define FHIP_GEMM_K_STEP 16        /* k per LDS buffer */
#define FHIP_GEMM_WIDE_BLOCKS 512  /* auto: the wide tile where batch * ceil(M / 128) * ceil(N / 128) reaches this and min(M, N) > 64 */
#define FHIP_GEMM_THIN_MAX 8       /* auto: min(M, N) up to this takes the thin kernel */
#define FHIP_GEMM_MAX_ELEMENTS 2147483648ll /* every tensor, strides included, stays below this many floats */

/* What fhip_gemm_forward computes, by address; leading dimensions and batch strides in floats.  (Anonymous: the ctypes mirror is
 * feathercnn_amd.gemm.GemmDesc, which tests/test_gemm_cpu.py holds against this text field by field.) */
typedef struct
{
    int m, n, k, batch;
    int trans_a, trans_b, out_transpose; /* 0 or 1 */
    int c_broadcast;                     /* -1 .. 4 as above */
    int lda, ldb, ldc, ldd;
    int a_batch_stride, b_batch_stride, c_batch_stride, d_batch_stride;
    int tile;                            /* 0: the auto rule; FHIP_GEMM_TILE_SMALL or FHIP_GEMM_TILE_WIDE: the matrix kernel at that tile */
    float alpha, beta;
} fhip_gemm_desc;

/* D = alpha op(A) op(B) + beta bcast(C) as defined above, one launch on `stream`.  c may be NULL where c_broadcast is -1. */
FHIP_GEMM_API int fhip_gemm_forward(const fhip_gemm_desc* desc, const float* a, const float* b, const float* c, float* d, void* stream);

/* The kernel instantiation a call would launch, as the demangled name without return type and parameters, copied into name[len]:
 *   "fhip::gemm_kernel<TA, TB, TILE>"  the operands AS LAUNCHED (with out_transpose they are swapped and TA = !trans_b, TB = !trans_a);
 *                                      TILE 1 wide, 0 small
 *   "fhip::gemm_thin_kernel<TB>"       TB: the large operand as launched is [N][K] (a wave reduces along K), else [K][N] (a lane owns four
 *                                      columns); the thin side is M after the swap (M <= N: as given, else swapped), on top of out_transpose
 * The same refusals as the forward call, pointers apart; FHIP_E_BADARG also for a NULL name or len < 1. */
FHIP_GEMM_API int fhip_gemm_route(const fhip_gemm_desc* desc, char* name, int len);

/* Message of this thread's last failing call of this library ("" if none). */
FHIP_GEMM_API const char* fhip_gemm_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* FEATHER_HIP_FEATHER_GEMM_H_ */
