/* feather_decoder.h -- C-ABI of libfeather_decoder.so: the layers of a decoder-only language model on the MI355X (gfx950) -- masked scaled
 * dot-product attention with grouped-query heads, a key/value cache, a split-KV route for decoding, and the small layers around it
 * (key/value concatenation, RMSNorm, rotary embedding, token embedding) -- on fp32 tensors with a leading batch.
 *
 * The reference has none of these layers and ncnn's sources were not at hand: this text is the definition, written from what ncnn's SDPA,
 * RMSNorm, RotaryEmbed and Embed layers do.  Where it and ncnn differ, this text holds.  tests/decoder_ref.py restates it in float64.
 *
 * SDPA           n images, `heads` query heads, `kv_heads` key/value heads (heads % kv_heads == 0, group = heads / kv_heads: query head h
 *                reads key/value head h / group), tq queries, tk keys, head width d.  Element (i, h, t, c) of a tensor lies at
 *                base + i * image_stride + h * head_stride + t * row_stride + c (strides in floats, columns contiguous), so one entry reads
 *                head-major blobs [n][heads][T][d] (row d, head T d, image heads T d), a fused token-major projection buffer (row 3E,
 *                head d, image T 3E), and a view of a preallocated cache (row d, head capacity * d, tk the filled length).
 *                   s[t][u]   = scale * sum_c q[i][h][t][c] * k[i][h / group][u][c]      (+ mask[i][h][t][u] where a mask is given)
 *                   key u is VISIBLE to query t  iff  (not causal or u <= t + (tk - tq))  and  s[t][u] > -inf
 *                   p[t][u]   = exp(s[t][u] - max_u s[t][u]) / sum_u exp(s[t][u] - max_u s[t][u])        over the visible keys
 *                   out[i][h][t][c] = sum_u p[t][u] * v[i][h / group][u][c]
 *                A row with no visible key yields ZEROS, not NaN: the one deliberate difference from ncnn and torch, whose softmax of a
 *                row of -inf is NaN.  The mask is additive fp32 [tq][tk] rows, dense, with a head stride and an image stride of its own
 *                (0: broadcast); -inf entries are allowed; NaN and +inf entries, and scores that overflow to +inf, are not (they give NaN).
 *                tq * tk must stay below 2^31 whether a mask is given or not (the description cannot see the pointer).
 *                Products, sums and the softmax are fp32 on v_mfma_f32_32x32x2_f32; exp is the device's expf.  Per (image, kv head) the
 *                problem is an R x tk attention with R = group * tq STACKED rows (row r = query head r / tq of the group, query r % tq): a
 *                block owns a tile of FHIP_DECODER_ROW_TILE_* stacked rows and walks the keys in tiles of FHIP_DECODER_KEY_TILE through two
 *                LDS buffers, so one staged K/V tile serves every head of the group; it keeps a running maximum and sum per row (an online
 *                softmax), so the order of the sums differs from the text above and the result from it by fp32 rounding.  Key tiles no row
 *                of the block can see (causal) are not loaded.  With splits > 1 the visible key tiles of every block are divided over
 *                `splits` blocks that write unnormalised partial results to `scratch`, and a second launch combines them (two launches, no
 *                flags, no waiting); an empty or fully masked split carries max = -inf and weight 0.
 *                d % 4 == 0 and d <= FHIP_DECODER_MAX_D; every other d is FHIP_E_UNSUPPORTED: there is no direct fallback.
 *
 * KV concat      present[n][kv_heads][tp + tn][d] = past[n][kv_heads][tp][d] followed by fresh[n][kv_heads][tn][d], dense, a bit copy; tp = 0
 *                (past ignored) is allowed.
 * RMSNorm        rows of L contiguous floats: y = x / sqrt(sum(x^2) / L + eps) * gamma; gamma of L floats, optional.
 *                One wave per row where L <= FHIP_DECODER_RMS_WAVE_MAX, one block of 256 lanes per row above it.
 * Rotary         x[n][heads][T][d] dense, d even; cos, sin [T][d / 2] with an image stride (0: shared by the batch).  Pair j of a row is
 *                (a, b) = (x[j], x[j + d / 2]), or (x[2j], x[2j + 1]) when interleaved; a' = a cos[t][j] - b sin[t][j],
 *                b' = a sin[t][j] + b cos[t][j].  y may be x.
 * Embed          ids[rows] int32; out[rows][E] = weight[clamp(id, 0, vocab - 1)][E] (+ bias[E] where given).  Without a bias a bit copy.
 *
 * Limits, refused with FHIP_E_BADARG and never truncated: every extent >= 1 (tp >= 0), every tensor below 2^31 elements (strides included),
 * a row stride below d.  No entry allocates, copies or synchronises; every device entry is one launch (SDPA with splits > 1: two) and
 * hipGraph-capturable.  Pointers need 4-byte alignment; 16-byte accesses are used where pointers and strides allow, 4-byte ones otherwise.
 * The elements `out` addresses must be distinct and must not overlap an input (Rotary excepted).  The library is separate from
 * libfeather_hip.so and needs nothing from it but the enums of feather_hip.h; it keeps its own last-error slot. */
#ifndef FEATHER_HIP_FEATHER_DECODER_H_
#define FEATHER_HIP_FEATHER_DECODER_H_

#include <stddef.h>

#include "feather_hip/feather_hip.h"

#ifdef __cplusplus
extern "C"
{
#endif

#define FHIP_DECODER_API __attribute__((visibility("default")))

/* Route code fhip_net_layer_info reports for the layers of a net with fhip_net_set_decoder (feather_net.h): SDPA, RMSNorm, RotaryEmbed, Embed. */
#define FHIP_DECODER_NET_ROUTE 120

#define FHIP_DECODER_MAX_D 128        /* the widest head */
#define FHIP_DECODER_KEY_TILE 32      /* keys per LDS tile */
#define FHIP_DECODER_ROW_TILE_FEW 32  /* stacked rows per block where R <= 32 (one wave): decoding */
#define FHIP_DECODER_ROW_TILE_MID 64  /* where R <= 64 (two waves) */
#define FHIP_DECODER_ROW_TILE_WIDE 128 /* above (four waves) */
#define FHIP_DECODER_MAX_SPLITS 256   /* the most blocks the keys of one row tile are divided over */
#define FHIP_DECODER_SPLIT_BLOCKS 128 /* auto: split only where n * kv_heads * row tiles is below this (half the card's 256 CUs) */
#define FHIP_DECODER_SPLIT_TARGET 512 /* auto: as many splits as bring the grid to this many blocks ... */
#define FHIP_DECODER_SPLIT_MIN_TILES 2 /* ... but no split of fewer key tiles than this */
#define FHIP_DECODER_RMS_WAVE_MAX 256 /* RMSNorm: rows up to this length take a wave each, longer ones a block each */

/* What fhip_sdpa_forward computes, by value; every stride in floats.  (Anonymous: the ctypes mirror is feathercnn_amd.decoder.SdpaDesc,
 * which tests/test_decoder_cpu.py holds against this text field by field.) */
typedef struct
{
    int n, heads, kv_heads, tq, tk, d;
    int q_image_stride, q_head_stride, q_row_stride;
    int k_image_stride, k_head_stride, k_row_stride;
    int v_image_stride, v_head_stride, v_row_stride;
    int out_image_stride, out_head_stride, out_row_stride;
    int mask_image_stride, mask_head_stride; /* read only with a mask; 0: the same [tq][tk] rows for every image / head */
    int causal;                              /* 0 or 1 */
    int splits;                              /* 0: the auto rule below; else forced, clamped to the key tiles and FHIP_DECODER_MAX_SPLITS */
    int row_tile;                            /* 0: by R as above; else 32, 64 or 128 forced (a measuring aid: tools/decoder_bench.py) */
    float scale;                             /* applied to the scores; finite */
} fhip_sdpa_desc;

/* `what` of fhip_decoder_route */
enum fhip_decoder_op
{
    FHIP_DECODER_SDPA = 0,      /* a = d, b = R = group * tq, c = row_tile (0: auto) */
    FHIP_DECODER_COMBINE = 1,   /* the second launch of a split call */
    FHIP_DECODER_KV_CONCAT = 2, /* a = 1 where d % 4 == 0 and every pointer is 16-byte aligned */
    FHIP_DECODER_RMS_NORM = 3,  /* a = L */
    FHIP_DECODER_ROTARY = 4,    /* a = interleaved */
    FHIP_DECODER_EMBED = 5
};

/* bytes = what `scratch` of fhip_sdpa_forward must hold for this description (0 without a split), splits (may be NULL) = the number of
 * splits the call will use.  The auto rule (splits == 0): with B = n * kv_heads * row tiles and KT = ceil(tk / FHIP_DECODER_KEY_TILE),
 * 1 where B >= FHIP_DECODER_SPLIT_BLOCKS, else min(ceil(FHIP_DECODER_SPLIT_TARGET / B), KT / FHIP_DECODER_SPLIT_MIN_TILES, FHIP_DECODER_MAX_SPLITS),
 * at least 1.  The rule was measured at B = 8 only; for every other B it is extrapolation.  The same refusals as the forward
 * call, pointers apart. */
FHIP_DECODER_API int fhip_sdpa_get_buffer_size(const fhip_sdpa_desc* desc, size_t* bytes, int* splits);

/* out = SDPA(q, k, v, mask) as defined above; mask may be NULL; scratch: NULL where fhip_sdpa_get_buffer_size gives 0 bytes, else DEVICE
 * memory of that size, 16-byte aligned, whose contents before and after the call mean nothing.  FHIP_E_BADARG: an extent < 1,
 * heads % kv_heads != 0, causal outside 0 / 1, splits < 0, a row_tile other than 0, 32, 64, 128, a scale that is not finite, a row stride
 * below d, a negative stride, a tensor of 2^31 elements or more, NULL or unaligned pointers.  FHIP_E_UNSUPPORTED: d % 4 != 0 or
 * d > FHIP_DECODER_MAX_D. */
FHIP_DECODER_API int fhip_sdpa_forward(const fhip_sdpa_desc* desc, const float* q, const float* k, const float* v, const float* mask, float* out,
                                       void* scratch, void* stream);

/* present = past followed by fresh, as defined above.  One launch.  FHIP_E_BADARG: n, kv_heads, tn or d < 1, tp < 0, 2^31 elements or
 * more, NULL (past only where tp > 0) or unaligned pointers. */
FHIP_DECODER_API int fhip_kv_concat_forward(int n, int kv_heads, int tp, int tn, int d, const float* past, const float* fresh, float* present, void* stream);

/* y[rows][l] = RMSNorm(x[rows][l]); gamma: NULL or a DEVICE array of l floats.  One launch.  FHIP_E_BADARG: rows or l < 1, 2^31 elements or
 * more, eps that is negative or not finite, NULL or unaligned x / y. */
FHIP_DECODER_API int fhip_rms_norm_forward(int rows, int l, const float* gamma, float eps, float* y, const float* x, void* stream);

/* y = Rotary(x) as defined above; cs_image_stride in floats (0: shared, else >= t * d / 2).  One launch.  FHIP_E_BADARG: an extent < 1, odd d,
 * interleaved outside 0 / 1, a negative stride, 2^31 elements or more, NULL or unaligned pointers. */
FHIP_DECODER_API int fhip_rotary_forward(int n, int heads, int t, int d, int interleaved, const float* cos, const float* sin, int cs_image_stride,
                                         float* y, const float* x, void* stream);

/* out[rows][e] = weight[clamp(ids[i], 0, vocab - 1)] (+ bias); ids: DEVICE int32.  One launch.  FHIP_E_BADARG: rows, e or vocab < 1, 2^31
 * elements or more (rows * e, vocab * e), NULL (bias excepted) or unaligned pointers. */
FHIP_DECODER_API int fhip_embed_forward(int rows, int e, int vocab, const int* ids, const float* weight, const float* bias, float* out, void* stream);

/* The kernel instantiation a call would launch, as the demangled name without return type and parameters, copied into name[len]:
 *   FHIP_DECODER_SDPA       "fhip::sdpa_kernel<DC, RW>": DC = ceil(d / 32) the 32-column chunks of a head, RW = row tile / 32 the waves of a block
 *   FHIP_DECODER_COMBINE    "fhip::sdpa_combine_kernel"
 *   FHIP_DECODER_KV_CONCAT  "fhip::kv_concat_kernel<V>": V = 1 with 16-byte accesses
 *   FHIP_DECODER_RMS_NORM   "fhip::rms_norm_kernel<B>": B = 0 a wave per row (L <= FHIP_DECODER_RMS_WAVE_MAX), 1 a block per row
 *   FHIP_DECODER_ROTARY     "fhip::rotary_kernel<I>": I = interleaved
 *   FHIP_DECODER_EMBED      "fhip::embed_kernel"
 * FHIP_E_BADARG: an unknown `what`, NULL name, len < 1, arguments the forward call would refuse; FHIP_E_UNSUPPORTED: a d the core refuses. */
FHIP_DECODER_API int fhip_decoder_route(int what, int a, int b, int c, char* name, int len);

/* Message of this thread's last failing call of this library ("" if none). */
FHIP_DECODER_API const char* fhip_decoder_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* FEATHER_HIP_FEATHER_DECODER_H_ */
