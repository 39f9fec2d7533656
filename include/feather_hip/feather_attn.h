/* feather_attn.h -- C-ABI of libfeather_attn.so: the layers of a Vision Transformer encoder on the MI355X (gfx950) -- the attention core of
 * ncnn's MultiHeadAttention, LayerNorm, GELU and the element-wise BinaryOp -- on fp32 tensors with a leading batch.
 *
 * The reference has none of these layers: this text is the definition, written from what ncnn's multiheadattention.cpp, layernorm.cpp,
 * gelu.cpp and binaryop.cpp do.  tests/attn_ref.py restates it line by line.
 *
 * Attention      q is [n][Tq] rows and k, v are [n][Tk] rows of E floats each; row r of a tensor starts at element r * stride (stride >= E, in
 *                floats), so one fused [n * T][3E] projection buffer is read in place (q = buf, k = buf + E, v = buf + 2E, stride 3E).
 *                Per image i and head h of width d = E / heads, over the columns [h * d, (h + 1) * d):
 *                   s[t][u]   = sum_c q[i][t][h * d + c] * k[i][u][h * d + c]            (no scale: the caller folds it into q)
 *                   p[t][u]   = exp(s[t][u] - max_u s[t][u]) / sum_u exp(s[t][u] - max_u s[t][u])
 *                   out[i][t][h * d + c] = sum_u p[t][u] * v[i][u][h * d + c]            out is dense: [n][Tq][E]
 *                Products, sums and the softmax are fp32; exp is the device's expf.  The Tq x Tk scores never leave the chip: a block owns
 *                (image, head, a tile of queries), walks the keys in tiles staged in LDS and keeps a running maximum and sum per query
 *                (an online softmax), so the order of the sums differs from the text above and the result from it by fp32 rounding.
 *                Two routes (fhip_attn_route): d a multiple of 4 and <= 128 runs both products on the fp32 matrix instruction
 *                (v_mfma_f32_32x32x2_f32); every other d <= FHIP_ATTN_DIRECT_MAX_D runs on a direct kernel, a wave per query.
 *
 * LayerNorm      rows of L contiguous floats:  mean = sum(x) / L;  var = sum((x - mean)^2) / L  (the biased variance of the centred
 *                row, never E[x^2] - E[x]^2);  y = (x - mean) / sqrt(var + eps) * gamma + beta, gamma and beta of L floats, each optional.
 *                The device sums x - x[0] and centres that (the same numbers: mean = x[0] + sum(x - x[0]) / L), so a row of mean 10^4 and
 *                spread 1 keeps its spread, which no float32 mean could resolve.
 *                One wave per row where L <= FHIP_ATTN_LN_WAVE_MAX, one block of 256 lanes per row above it.
 *                fhip_add_layer_norm_forward computes s = a + b, writes s, and writes LayerNorm(s): bit for bit fhip_binary_forward (add)
 *                followed by fhip_layer_norm_forward.
 *
 * GELU           fast = 0:  y = 0.5 * x * (1 + erff(0.70710678 * x));  fast = 1:  y = 0.5 * x * (1 + tanhf(0.79788452 * (x + 0.044715 * x^3))).
 *                Both as the formula gives them: -inf yields NaN (0 * inf) in the first form, NaN stays NaN.
 *
 * Binary         out = x op y with op 0 add, 1 sub, 2 mul, 3 div, 4 max (fmaxf), 5 min (fminf) -- ncnn's BinaryOp 0=0..5; every other op code
 *                is refused.  y is, by `form`: a scalar passed by value; a tensor of the same `count` elements; or `per` elements (one
 *                image's worth, count % per == 0) broadcast over the batch: y[i % per].  swap = 1 computes y op x.  16-byte accesses where
 *                every pointer is 16-byte aligned (and per % 4 == 0 for the broadcast), a scalar tail behind them.
 *
 * Limits, refused with FHIP_E_BADARG and never truncated: every extent >= 1, fewer than 2^31 elements in every tensor (strides
 * included), E % heads == 0.  No entry allocates, copies or synchronises: every device entry is one launch and hipGraph-capturable.
 * Pointers need 4-byte alignment.  Only the Binary forms and fhip_add_layer_norm_forward (sum == a or sum == b) may run in place.  The library is
 * separate from libfeather_hip.so and needs nothing from it but the enums of feather_hip.h; it keeps its own last-error slot. */
#ifndef FEATHER_HIP_FEATHER_ATTN_H_
#define FEATHER_HIP_FEATHER_ATTN_H_

#include <stddef.h>

#include "feather_hip/feather_hip.h"

#ifdef __cplusplus
extern "C"
{
#endif

#define FHIP_ATTN_API __attribute__((visibility("default")))

/* Route code fhip_net_layer_info reports for the layers of a net with fhip_net_set_transformer (feather_net.h): MemoryData, LayerNorm, GELU,
 * MultiHeadAttention and the element-wise BinaryOp.  The token-wise InnerProduct reports FHIP_IM2COL, as every InnerProduct does. */
#define FHIP_ATTN_NET_ROUTE 113

#define FHIP_ATTN_MFMA_MAX_D 128    /* the widest head of the matrix route */
#define FHIP_ATTN_DIRECT_MAX_D 4096 /* the widest head of the direct route: q and the output row of one query live in LDS */
#define FHIP_ATTN_QUERY_TILE 64     /* queries per block of the matrix route (two waves of 32) */
#define FHIP_ATTN_KEY_TILE 32       /* keys per LDS tile of the matrix route */
#define FHIP_ATTN_LN_WAVE_MAX 256   /* LayerNorm: rows up to this length take a wave each, longer ones a block each */

/* op of fhip_binary_forward (ncnn's BinaryOp 0=) */
#define FHIP_BINARY_ADD 0
#define FHIP_BINARY_SUB 1
#define FHIP_BINARY_MUL 2
#define FHIP_BINARY_DIV 3
#define FHIP_BINARY_MAX 4
#define FHIP_BINARY_MIN 5

/* form of fhip_binary_forward */
#define FHIP_BINARY_SCALAR 0    /* y = the scalar argument */
#define FHIP_BINARY_TENSOR 1    /* y = b[i] */
#define FHIP_BINARY_BROADCAST 2 /* y = b[i % per] */

/* `what` of fhip_attn_route */
enum fhip_attn_op
{
    FHIP_ATTN_ATTENTION = 0,  /* a = E, b = heads */
    FHIP_ATTN_LAYER_NORM = 1, /* a = L, b = 1 for fhip_add_layer_norm_forward */
    FHIP_ATTN_GELU = 2,       /* a = fast, b = 1 where both pointers are 16-byte aligned */
    FHIP_ATTN_BINARY = 3      /* a = form, b = 1 where every pointer is 16-byte aligned (and per % 4 == 0 for the broadcast) */
};

/* out[n][tq][e] = attention of q (n * tq rows), k and v (n * tk rows each) as defined above: one launch on `stream` (a hipStream_t as void*).
 * FHIP_E_BADARG: n, heads, tq or e < 1, tk < 1, e % heads != 0, a stride below e, a tensor of 2^31 elements or more (rows * stride), a head
 * wider than FHIP_ATTN_DIRECT_MAX_D on the direct route, NULL or unaligned (4 bytes) pointers. */
FHIP_ATTN_API int fhip_attention_forward(int n, int heads, int tq, int tk, int e, const float* q, int q_stride, const float* k, int k_stride,
                                         const float* v, int v_stride, float* out, void* stream);

/* y[rows][l] = LayerNorm(x[rows][l]); gamma, beta: NULL or DEVICE arrays of l floats.  One launch.  FHIP_E_BADARG: rows or l < 1, 2^31
 * elements or more, eps that is negative or not finite, NULL or unaligned x / y. */
FHIP_ATTN_API int fhip_layer_norm_forward(int rows, int l, const float* gamma, const float* beta, float eps, float* y, const float* x, void* stream);

/* sum = a + b and y = LayerNorm(sum), one launch; sum may be a or b, y may not overlap anything.  The same refusals. */
FHIP_ATTN_API int fhip_add_layer_norm_forward(int rows, int l, const float* gamma, const float* beta, float eps, float* sum, float* y, const float* a,
                                              const float* b, void* stream);

/* out[count] = GELU(in[count]), fast = 0 or 1.  One launch.  FHIP_E_BADARG: count < 1 or >= 2^31, fast outside 0 / 1, NULL or unaligned pointers. */
FHIP_ATTN_API int fhip_gelu_forward(int fast, float* out, const float* in, size_t count, void* stream);

/* out[count] = a op y as defined above (b is ignored for the scalar form, `scalar` for the others; per only for the broadcast).  One
 * launch.  FHIP_E_BADARG: an op outside 0 .. 5, a form outside 0 .. 2, swap outside 0 / 1, count < 1 or >= 2^31, per < 1 or count % per != 0,
 * NULL or unaligned pointers. */
FHIP_ATTN_API int fhip_binary_forward(int op, int form, int swap, float* out, const float* a, const float* b, float scalar, size_t count, size_t per,
                                      void* stream);

/* The kernel instantiation a call would launch, as the demangled name without return type and parameters, copied into name[len]:
 *   FHIP_ATTN_ATTENTION   "fhip::attention_mfma_kernel<DC>" where d = a / b is a multiple of 4 and <= 128, DC = ceil(d / 32) the 32-column
 *                         chunks of a head; else "fhip::attention_direct_kernel"
 *   FHIP_ATTN_LAYER_NORM  "fhip::layer_norm_kernel<B, A>": B = 0 a wave per row (L <= FHIP_ATTN_LN_WAVE_MAX), 1 a block per row; A = 1 with the add
 *   FHIP_ATTN_GELU        "fhip::gelu_kernel<F, V>": F = fast, V = 1 with 16-byte accesses
 *   FHIP_ATTN_BINARY      "fhip::binary_kernel<FORM, V>"
 * FHIP_E_BADARG: an unknown `what`, NULL name, len < 1, arguments the forward call would refuse. */
FHIP_ATTN_API int fhip_attn_route(int what, int a, int b, char* name, int len);

/* Message of this thread's last failing call of this library ("" if none). */
FHIP_ATTN_API const char* fhip_attn_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* FEATHER_HIP_FEATHER_ATTN_H_ */
