// libfeather_decoder.so: the layers of a decoder-only language model on gfx950 (include/feather_hip/feather_decoder.h is the contract and the
// definition; DESIGN.md 3.35 the design and its measurements).
//
//   sdpa_kernel<DC, RW>           a block of RW waves owns (image, kv head, 32 RW STACKED rows, one split of the keys); a wave owns 32 rows.
//                                 Row r of the R = group * tq stacked rows is (query head r / tq of the group, query r % tq): only the Q load,
//                                 the mask lookup, the causal limit and the store know it, and one staged K/V tile serves every head of the
//                                 group.  Keys come in tiles of 32 through TWO LDS buffers: the 16-byte global loads of tile i + 1 are issued
//                                 into registers before the products of tile i and written to the other buffer behind them, one barrier a
//                                 tile.  Both products run TRANSPOSED on v_mfma_f32_32x32x2_f32 (S^T = K Q^T, O^T += V^T P^T), so a lane's 16
//                                 accumulator registers hold 16 keys of ONE row (column = lane & 31): the online softmax is in-lane plus one
//                                 exchange with lane ^ 32, and P^T is already the B operand of the second product (register s holds key
//                                 8 (s >> 2) + 4 (lane >> 5) + (s & 3)).  K rows are padded by 4 floats and read 16 bytes at a time.  Key
//                                 tiles past the causal limit of the block's last row are never loaded; a wave skips the products of tiles
//                                 past its own.  A row whose running maximum is still -inf has seen no key: it keeps sum 0 and ends as zeros.
//                                 With splits > 1 the block writes its unnormalised accumulator, maximum and sum to scratch instead.
//   sdpa_combine_kernel           a lane per (stacked row, 4 columns): the maximum over the splits, then the weighted sums; -inf weighs 0.
//   kv_concat_kernel<V>           a bit copy, V = 1: 16 bytes a lane
//   rms_norm_kernel<B>            B = 0: a wave per row, 4 rows a block; B = 1: a block of 256 lanes per row.  Two passes, the second from cache.
//   rotary_kernel<I>              a lane per pair
//   embed_kernel                  a lane per element
//
// Contraction is off for the whole file: a * b + c is two roundings wherever the text of the header says so.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>

#include "feather_hip/feather_decoder.h"
#include "side_error.h"

#pragma clang fp contract(off)

namespace fhip
{

typedef long long i64;
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kKT = FHIP_DECODER_KEY_TILE;
constexpr unsigned kMaxBlocks = 16384;

struct SdpaArgs
{
    const float *q, *k, *v, *mask;
    float *out, *acc, *ml; // scratch of a split call: acc [b][split][R][d], ml [b][split][R][2] (maximum, sum); b = image * kv_heads + kv head
    i64 q_is, q_hs, q_rs, k_is, k_hs, k_rs, v_is, v_hs, v_rs, o_is, o_hs, o_rs, m_is, m_hs;
    int kv_heads, group, tq, tk, d, R, row_tiles, splits, causal, vec_kv, vec_out;
    float scale;
};

__device__ __forceinline__ float xor32(float x) { return __shfl_xor(x, 32, 64); }

__device__ __forceinline__ float wave_max(float x)
{
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) x = fmaxf(x, __shfl_xor(x, s, 64));
    return x;
}

__device__ __forceinline__ float wave_sum(float x)
{
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) x += __shfl_xor(x, s, 64);
    return x;
}

// where the stacked row r of (image, kv head) lies in `out`
__device__ __forceinline__ float* out_row(const SdpaArgs& g, unsigned img, unsigned kvh, int r)
{
    const int hg = r / g.tq, t = r - hg * g.tq;
    return g.out + (i64)img * g.o_is + ((i64)kvh * g.group + hg) * g.o_hs + (i64)t * g.o_rs;
}

// blockIdx.x runs over (image, kv head, row tile), blockIdx.z over the splits.  LDS: two K tiles [32][32 DC + 4] and two V tiles [32][32 DC]
// (columns past d zero; rows of keys past tk zero, their scores masked).
template <int DC, int RW>
__global__ __launch_bounds__(64 * RW) void sdpa_kernel(SdpaArgs g)
{
    constexpr int W = 32 * DC, LDK = W + 4, LDV = W, HALF = 16 * DC, NT = 64 * RW, RT = 32 * RW, Q4 = W / 4, PER = kKT * Q4 / NT;
    __shared__ __attribute__((aligned(16))) float Ks[2][kKT * LDK];
    __shared__ __attribute__((aligned(16))) float Vs[2][kKT * LDV];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 31, hi = lane >> 5;
    const unsigned tile = blockIdx.x % (unsigned)g.row_tiles, b = blockIdx.x / (unsigned)g.row_tiles;
    const unsigned kvh = b % (unsigned)g.kv_heads, img = b / (unsigned)g.kv_heads;
    const int split = blockIdx.z;

    // this lane's stacked row: column `col` of S^T and O^T
    const int r = (int)tile * RT + wave * 32 + col;
    const bool have_q = r < g.R;
    const int hg = have_q ? r / g.tq : 0, t = have_q ? r - hg * g.tq : 0;
    const int past = g.tk - g.tq;
    const int klim = g.causal && have_q ? t + past : g.tk - 1; // the last key this row sees; below 0: none
    const bool wave_live = (int)tile * RT + wave * 32 < g.R;
    const int wave_klim = (int)wave_max((float)klim); // exact: below 2^24 keys (checked by the host)
    const float* mrow = g.mask && have_q ? g.mask + (i64)img * g.m_is + ((i64)kvh * g.group + hg) * g.m_hs + (i64)t * g.tk : nullptr;

    // the key tiles the block walks: those its last row can see, then this split's share of them
    int tile_begin, tile_end;
    {
        const int r0 = (int)tile * RT, r1 = min(g.R, r0 + RT) - 1;
        const int t_last = r0 / g.tq == r1 / g.tq ? r1 % g.tq : g.tq - 1;
        const int total = (g.tk + kKT - 1) / kKT, limit = t_last + past;
        const int visible = g.causal ? (limit < 0 ? 0 : min(total, limit / kKT + 1)) : total;
        const int per = (visible + g.splits - 1) / g.splits;
        tile_begin = min(visible, split * per), tile_end = min(visible, tile_begin + per);
    }

    // Q^T as the B operand of S^T = K Q^T: step s of the product takes k index hi * HALF + s from both operands
    float qr[HALF];
    {
        const float* qrow = g.q + (i64)img * g.q_is + ((i64)kvh * g.group + hg) * g.q_hs + (i64)t * g.q_rs;
#pragma unroll
        for (int s = 0; s < HALF; ++s)
        {
            const int c = hi * HALF + s;
            qr[s] = have_q && c < g.d ? qrow[c] : 0.f;
        }
    }
    f32x16 o[DC];
#pragma unroll
    for (int j = 0; j < DC; ++j)
#pragma unroll
        for (int i = 0; i < 16; ++i) o[j][i] = 0.f;
    float m = -INFINITY, l = 0.f;

    const float* kbase = g.k + (i64)img * g.k_is + (i64)kvh * g.k_hs;
    const float* vbase = g.v + (i64)img * g.v_is + (i64)kvh * g.v_hs;
    float4 pk[PER], pv[PER];
    auto fetch = [&](int key0) { // global -> registers: quad `at` of the tile is row at / Q4, columns 4 (at % Q4) ..
#pragma unroll
        for (int i = 0; i < PER; ++i)
        {
            const int at = (int)threadIdx.x + i * NT, row = at / Q4, c = 4 * (at - row * Q4), key = key0 + row;
            pk[i] = pv[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (key < g.tk && c < g.d) // d is a multiple of 4: the whole quad or none of it
            {
                const float* kp = kbase + (i64)key * g.k_rs + c;
                const float* vp = vbase + (i64)key * g.v_rs + c;
                if (g.vec_kv)
                    pk[i] = *reinterpret_cast<const float4*>(kp), pv[i] = *reinterpret_cast<const float4*>(vp);
                else
                    pk[i] = make_float4(kp[0], kp[1], kp[2], kp[3]), pv[i] = make_float4(vp[0], vp[1], vp[2], vp[3]);
            }
        }
    };
    auto stage = [&](int buf) { // registers -> LDS
#pragma unroll
        for (int i = 0; i < PER; ++i)
        {
            const int at = (int)threadIdx.x + i * NT, row = at / Q4, c = 4 * (at - row * Q4);
            *reinterpret_cast<float4*>(&Ks[buf][row * LDK + c]) = pk[i];
            *reinterpret_cast<float4*>(&Vs[buf][row * LDV + c]) = pv[i];
        }
    };

    if (tile_begin < tile_end)
    {
        fetch(tile_begin * kKT);
        stage(0);
    }
    __syncthreads();
    for (int kt = tile_begin; kt < tile_end; ++kt) // block-uniform bounds: every wave meets every barrier
    {
        const int buf = (kt - tile_begin) & 1, key0 = kt * kKT;
        const bool more = kt + 1 < tile_end;
        if (more) fetch(key0 + kKT); // in flight under the products below

        if (wave_live && key0 <= wave_klim)
        {
            // S^T[key][row]: A = K (row = key `col` of the tile), B = Q^T
            f32x16 st;
#pragma unroll
            for (int i = 0; i < 16; ++i) st[i] = 0.f;
            const float* krow = &Ks[buf][col * LDK + hi * HALF];
#pragma unroll
            for (int s = 0; s < HALF; s += 4)
            {
                const float4 kk = *reinterpret_cast<const float4*>(krow + s);
                st = __builtin_amdgcn_mfma_f32_32x32x2f32(kk.x, qr[s], st, 0, 0, 0);
                st = __builtin_amdgcn_mfma_f32_32x32x2f32(kk.y, qr[s + 1], st, 0, 0, 0);
                st = __builtin_amdgcn_mfma_f32_32x32x2f32(kk.z, qr[s + 2], st, 0, 0, 0);
                st = __builtin_amdgcn_mfma_f32_32x32x2f32(kk.w, qr[s + 3], st, 0, 0, 0);
            }

            // register i holds key 8 * (i >> 2) + 4 * hi + (i & 3) of the tile for this lane's row
            float tmax = -INFINITY;
#pragma unroll
            for (int i = 0; i < 16; ++i)
            {
                const int key = key0 + 8 * (i >> 2) + 4 * hi + (i & 3);
                float s = st[i] * g.scale;
                if (mrow && key < g.tk) s = s + mrow[key];
                s = key <= klim ? s : -INFINITY; // klim < tk
                st[i] = s;
                tmax = fmaxf(tmax, s);
            }
            tmax = fmaxf(tmax, xor32(tmax));
            const float m_new = fmaxf(m, tmax);
            const float m_ref = m_new == -INFINITY ? 0.f : m_new; // no key seen so far: every exp below is exp(-inf) = 0, never exp(nan)
            const float alpha = expf(m - m_ref);                  // 0 while m = -inf
            float psum = 0.f;
#pragma unroll
            for (int i = 0; i < 16; ++i)
            {
                st[i] = expf(st[i] - m_ref); // a masked key: exp(-inf) = 0
                psum += st[i];
            }
            psum += xor32(psum);
            l = l * alpha + psum;
            m = m_new;
#pragma unroll
            for (int j = 0; j < DC; ++j)
#pragma unroll
                for (int i = 0; i < 16; ++i) o[j][i] *= alpha;

            // O^T[column][row] += V^T P^T: step s takes the key register s holds; A = V^T (row = column 32 j + col of the head)
#pragma unroll
            for (int s = 0; s < 16; ++s)
            {
                const float* vrow = &Vs[buf][(8 * (s >> 2) + 4 * hi + (s & 3)) * LDV + col];
#pragma unroll
                for (int j = 0; j < DC; ++j) o[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(vrow[32 * j], st[s], o[j], 0, 0, 0);
            }
        }

        if (more) stage(buf ^ 1); // read last a tile ago, before the barrier that ended it
        __syncthreads();
    }

    if (!have_q) return;
    if (g.splits > 1)
    {
        const i64 at = ((i64)b * g.splits + split) * g.R + r;
        float* arow = g.acc + at * g.d;
        if (hi == 0) g.ml[2 * at] = m, g.ml[2 * at + 1] = l;
#pragma unroll
        for (int j = 0; j < DC; ++j)
#pragma unroll
            for (int gq = 0; gq < 4; ++gq)
            {
                const int c = 32 * j + 8 * gq + 4 * hi;
                if (c < g.d) *reinterpret_cast<float4*>(arow + c) = make_float4(o[j][4 * gq], o[j][4 * gq + 1], o[j][4 * gq + 2], o[j][4 * gq + 3]);
            }
        return;
    }
    const float inv = l > 0.f ? 1.f / l : 0.f; // no visible key: zeros
    float* orow = out_row(g, img, kvh, r);
#pragma unroll
    for (int j = 0; j < DC; ++j)
#pragma unroll
        for (int gq = 0; gq < 4; ++gq)
        {
            const int c = 32 * j + 8 * gq + 4 * hi; // registers 4 gq .. 4 gq + 3: four consecutive columns (d is a multiple of 4)
            if (c >= g.d) continue;
            const float r0 = o[j][4 * gq] * inv, r1 = o[j][4 * gq + 1] * inv, r2 = o[j][4 * gq + 2] * inv, r3 = o[j][4 * gq + 3] * inv;
            if (g.vec_out)
                *reinterpret_cast<float4*>(orow + c) = make_float4(r0, r1, r2, r3);
            else
                orow[c] = r0, orow[c + 1] = r1, orow[c + 2] = r2, orow[c + 3] = r3;
        }
}

// a lane per (b, stacked row, quad of columns); `quads` of them
__global__ __launch_bounds__(256) void sdpa_combine_kernel(SdpaArgs g, unsigned quads)
{
    const unsigned id = blockIdx.x * 256u + threadIdx.x;
    if (id >= quads) return;
    const unsigned dq = (unsigned)g.d / 4, c = 4 * (id % dq), rb = id / dq;
    const int r = (int)(rb % (unsigned)g.R);
    const unsigned b = rb / (unsigned)g.R, kvh = b % (unsigned)g.kv_heads, img = b / (unsigned)g.kv_heads;
    float top = -INFINITY;
    for (int s = 0; s < g.splits; ++s) top = fmaxf(top, g.ml[2 * (((i64)b * g.splits + s) * g.R + r)]);
    float4 num = make_float4(0.f, 0.f, 0.f, 0.f);
    float den = 0.f;
    if (top != -INFINITY) // else no split saw a key: zeros
        for (int s = 0; s < g.splits; ++s)
        {
            const i64 at = ((i64)b * g.splits + s) * g.R + r;
            const float w = expf(g.ml[2 * at] - top); // an empty or fully masked split: exp(-inf) = 0
            const float4 a = *reinterpret_cast<const float4*>(g.acc + at * g.d + c);
            den += w * g.ml[2 * at + 1];
            num.x += w * a.x, num.y += w * a.y, num.z += w * a.z, num.w += w * a.w;
        }
    const float inv = den > 0.f ? 1.f / den : 0.f;
    float* orow = out_row(g, img, kvh, r) + c;
    if (g.vec_out)
        *reinterpret_cast<float4*>(orow) = make_float4(num.x * inv, num.y * inv, num.z * inv, num.w * inv);
    else
        orow[0] = num.x * inv, orow[1] = num.y * inv, orow[2] = num.z * inv, orow[3] = num.w * inv;
}

// ---- the small kernels -----------------------------------------------------------------------------------------------------------------
// present[b][tp + tn][d] = past[b][tp][d] | fresh[b][tn][d], b over (image, kv head); `count` units of 4 (V) or 1 floats, d a multiple of it
template <int V>
__global__ __launch_bounds__(256) void kv_concat_kernel(uint32_t* __restrict__ present, const uint32_t* __restrict__ past, const uint32_t* __restrict__ fresh, unsigned count,
                                                        unsigned past_row, unsigned fresh_row)
{
    constexpr unsigned U = V ? 4 : 1;
    const unsigned row = past_row + fresh_row; // units per (image, kv head) of present
    for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < count; i += gridDim.x * 256u)
    {
        const unsigned b = i / row, at = i - b * row;
        const uint32_t* from = at < past_row ? past + ((i64)b * past_row + at) * U : fresh + ((i64)b * fresh_row + (at - past_row)) * U;
        if constexpr (V)
            reinterpret_cast<uint4*>(present)[i] = *reinterpret_cast<const uint4*>(from);
        else
            present[i] = *from;
    }
}

template <int B>
__global__ __launch_bounds__(256) void rms_norm_kernel(float* __restrict__ y, const float* __restrict__ x, const float* __restrict__ gamma, float eps, int rows, int L)
{
    __shared__ float part[4];
    constexpr int STEP = B ? 256 : 64;
    const int lane = B ? threadIdx.x : (threadIdx.x & 63);
    const i64 row = B ? (i64)blockIdx.x : (i64)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (!B && row >= rows) return; // a whole wave: no barrier follows in this form
    const float* px = x + row * L;
    float acc = 0.f;
    for (int i = lane; i < L; i += STEP) acc += px[i] * px[i];
    acc = wave_sum(acc);
    if constexpr (B)
    {
        if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
        __syncthreads();
        acc = (part[0] + part[1]) + (part[2] + part[3]);
    }
    const float scale = 1.f / sqrtf(acc / (float)L + eps);
    float* py = y + row * L;
    for (int i = lane; i < L; i += STEP)
    {
        float r = px[i] * scale;
        if (gamma) r = r * gamma[i];
        py[i] = r;
    }
}

// a lane per pair; y may be x (no __restrict__): a pair is read before it is written, by the same lane
template <int I>
__global__ __launch_bounds__(256) void rotary_kernel(float* y, const float* x, const float* __restrict__ cs, const float* __restrict__ sn, unsigned pairs, unsigned heads,
                                                     unsigned T, unsigned half, i64 cs_is)
{
    for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < pairs; i += gridDim.x * 256u)
    {
        const unsigned j = i % half, row = i / half, t = row % T, img = row / T / heads;
        const i64 base = (i64)row * 2 * half, ia = base + (I ? 2 * j : j), ib = base + (I ? 2 * j + 1 : j + half);
        const i64 at = (i64)img * cs_is + (i64)t * half + j;
        const float a = x[ia], b = x[ib], c = cs[at], s = sn[at];
        y[ia] = a * c - b * s;
        y[ib] = a * s + b * c;
    }
}

__global__ __launch_bounds__(256) void embed_kernel(float* __restrict__ out, const int* __restrict__ ids, const float* __restrict__ weight, const float* __restrict__ bias,
                                                    unsigned count, unsigned E, int vocab)
{
    for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < count; i += gridDim.x * 256u)
    {
        const unsigned row = i / E, c = i - row * E;
        const int id = min(max(ids[row], 0), vocab - 1);
        const float w = weight[(i64)id * E + c];
        out[i] = bias ? w + bias[c] : w;
    }
}

// ---- host checks -----------------------------------------------------------------------------------------------------------------------
constexpr i64 kMaxElements = 1ll << 31;

static unsigned grid_for(size_t count) { return (unsigned)std::min<size_t>((count + 255) / 256, kMaxBlocks); }

static int check_width(int d)
{
    if (d < 1) return fail(FHIP_E_BADARG, "d < 1");
    if (d % 4 || d > FHIP_DECODER_MAX_D) return fail(FHIP_E_UNSUPPORTED, "SDPA needs a head width d that is a multiple of 4 and <= FHIP_DECODER_MAX_D (128): there is no direct route");
    return FHIP_OK;
}

static int row_tile_for(int R, int forced)
{
    if (forced) return forced;
    return R <= FHIP_DECODER_ROW_TILE_FEW ? FHIP_DECODER_ROW_TILE_FEW : (R <= FHIP_DECODER_ROW_TILE_MID ? FHIP_DECODER_ROW_TILE_MID : FHIP_DECODER_ROW_TILE_WIDE);
}

// one past the last element of a tensor [n][heads][rows][d] with these strides, or -1 for a stride the header refuses
static i64 extent(int n, int heads, int rows, int d, int is, int hs, int rs)
{
    if (is < 0 || hs < 0 || rs < d) return -1;
    return (i64)(n - 1) * is + (i64)(heads - 1) * hs + (i64)(rows - 1) * rs + d;
}

struct SdpaPlan
{
    int R, row_tile, row_tiles, splits;
    i64 blocks;
    size_t bytes;
};

static int plan_sdpa(const fhip_sdpa_desc* p, SdpaPlan& plan)
{
    if (!p) return fail(FHIP_E_BADARG, "null description");
    if (p->n < 1 || p->heads < 1 || p->kv_heads < 1 || p->tq < 1 || p->tk < 1) return fail(FHIP_E_BADARG, "n, heads, kv_heads, tq or tk < 1");
    if (const int rc = check_width(p->d)) return rc;
    if (p->heads % p->kv_heads) return fail(FHIP_E_BADARG, "the number of heads is no multiple of the number of key/value heads (heads % kv_heads != 0)");
    if (p->causal != 0 && p->causal != 1) return fail(FHIP_E_BADARG, "causal must be 0 or 1");
    if (p->splits < 0) return fail(FHIP_E_BADARG, "splits < 0");
    if (p->row_tile != 0 && p->row_tile != 32 && p->row_tile != 64 && p->row_tile != 128) return fail(FHIP_E_BADARG, "row_tile must be 0 (auto), 32, 64 or 128");
    if (!isfinite(p->scale)) return fail(FHIP_E_BADARG, "scale must be finite");
    const i64 eq = extent(p->n, p->heads, p->tq, p->d, p->q_image_stride, p->q_head_stride, p->q_row_stride);
    const i64 ek = extent(p->n, p->kv_heads, p->tk, p->d, p->k_image_stride, p->k_head_stride, p->k_row_stride);
    const i64 ev = extent(p->n, p->kv_heads, p->tk, p->d, p->v_image_stride, p->v_head_stride, p->v_row_stride);
    const i64 eo = extent(p->n, p->heads, p->tq, p->d, p->out_image_stride, p->out_head_stride, p->out_row_stride);
    if (eq < 0 || ek < 0 || ev < 0 || eo < 0) return fail(FHIP_E_BADARG, "a negative stride, or a row stride below the head width d");
    if (p->mask_image_stride < 0 || p->mask_head_stride < 0) return fail(FHIP_E_BADARG, "a negative mask stride");
    const i64 em = (i64)(p->n - 1) * p->mask_image_stride + (i64)(p->heads - 1) * p->mask_head_stride + (i64)p->tq * p->tk;
    const i64 R = (i64)(p->heads / p->kv_heads) * p->tq;
    if (eq >= kMaxElements || ek >= kMaxElements || ev >= kMaxElements || eo >= kMaxElements || em >= kMaxElements || R >= kMaxElements || p->tk >= (1 << 24))
        return fail(FHIP_E_BADARG, "tensors of 2^31 elements or more (2^24 keys or more) are not supported");
    plan.R = (int)R;
    plan.row_tile = row_tile_for(plan.R, p->row_tile);
    plan.row_tiles = (plan.R + plan.row_tile - 1) / plan.row_tile;
    plan.blocks = (i64)p->n * p->kv_heads * plan.row_tiles;
    if (plan.blocks >= kMaxElements) return fail(FHIP_E_BADARG, "tensors of 2^31 elements or more are not supported");
    const int key_tiles = (p->tk + kKT - 1) / kKT;
    int s = p->splits;
    if (s == 0) // the auto rule of the header
        s = plan.blocks >= FHIP_DECODER_SPLIT_BLOCKS ? 1 : (int)std::min<i64>((FHIP_DECODER_SPLIT_TARGET + plan.blocks - 1) / plan.blocks, key_tiles / FHIP_DECODER_SPLIT_MIN_TILES);
    plan.splits = std::max(1, std::min(s, std::min(key_tiles, FHIP_DECODER_MAX_SPLITS)));
    const i64 rows = (i64)p->n * p->kv_heads * plan.splits * plan.R; // rows of the scratch
    if (plan.splits > 1 && rows * p->d >= kMaxElements) return fail(FHIP_E_BADARG, "the scratch of the split route would hold 2^31 elements or more");
    plan.bytes = plan.splits > 1 ? (size_t)rows * (p->d + 2) * sizeof(float) : 0;
    return FHIP_OK;
}

template <int DC>
static void launch_sdpa(int rw, dim3 grid, hipStream_t s, const SdpaArgs& g)
{
    if (rw == 1) hipLaunchKernelGGL((sdpa_kernel<DC, 1>), grid, dim3(64), 0, s, g);
    else if (rw == 2) hipLaunchKernelGGL((sdpa_kernel<DC, 2>), grid, dim3(128), 0, s, g);
    else hipLaunchKernelGGL((sdpa_kernel<DC, 4>), grid, dim3(256), 0, s, g);
}

static int check_rows(int rows, int l, float eps)
{
    if (rows < 1 || l < 1) return fail(FHIP_E_BADARG, "rows or l < 1");
    if ((i64)rows * l >= kMaxElements) return fail(FHIP_E_BADARG, "tensors of 2^31 elements or more are not supported");
    if (!(eps >= 0.f) || !isfinite(eps)) return fail(FHIP_E_BADARG, "eps must be finite and >= 0");
    return FHIP_OK;
}

} // namespace fhip

using namespace fhip;

extern "C"
{

int fhip_sdpa_get_buffer_size(const fhip_sdpa_desc* desc, size_t* bytes, int* splits)
{
    SdpaPlan plan;
    if (const int rc = plan_sdpa(desc, plan)) return rc;
    if (!bytes) return fail(FHIP_E_BADARG, "null pointer");
    *bytes = plan.bytes;
    if (splits) *splits = plan.splits;
    return FHIP_OK;
}

int fhip_sdpa_forward(const fhip_sdpa_desc* p, const float* q, const float* k, const float* v, const float* mask, float* out, void* scratch, void* stream)
{
    SdpaPlan plan;
    if (const int rc = plan_sdpa(p, plan)) return rc;
    if (!q || !k || !v || !out) return fail(FHIP_E_BADARG, "null pointer");
    if (!aligned(q, 4) || !aligned(k, 4) || !aligned(v, 4) || !aligned(out, 4) || !aligned(mask, 4)) return fail(FHIP_E_BADARG, "pointers must be 4-byte aligned");
    if (plan.splits > 1 && (!scratch || !aligned(scratch, 16))) return fail(FHIP_E_BADARG, "the split route needs a 16-byte aligned scratch of fhip_sdpa_get_buffer_size bytes");
    SdpaArgs g;
    g.q = q, g.k = k, g.v = v, g.mask = mask, g.out = out;
    g.acc = (float*)scratch; // [rows][d], then [rows][2]: d is a multiple of 4, so both stay 16-byte aligned
    g.ml = g.acc ? g.acc + (size_t)p->n * p->kv_heads * plan.splits * plan.R * p->d : nullptr;
    g.q_is = p->q_image_stride, g.q_hs = p->q_head_stride, g.q_rs = p->q_row_stride;
    g.k_is = p->k_image_stride, g.k_hs = p->k_head_stride, g.k_rs = p->k_row_stride;
    g.v_is = p->v_image_stride, g.v_hs = p->v_head_stride, g.v_rs = p->v_row_stride;
    g.o_is = p->out_image_stride, g.o_hs = p->out_head_stride, g.o_rs = p->out_row_stride;
    g.m_is = p->mask_image_stride, g.m_hs = p->mask_head_stride;
    g.kv_heads = p->kv_heads, g.group = p->heads / p->kv_heads, g.tq = p->tq, g.tk = p->tk, g.d = p->d, g.R = plan.R;
    g.row_tiles = plan.row_tiles, g.splits = plan.splits, g.causal = p->causal, g.scale = p->scale;
    const auto quads = [](const void* at, int is, int hs, int rs) { return aligned(at, 16) && is % 4 == 0 && hs % 4 == 0 && rs % 4 == 0; };
    g.vec_kv = quads(k, p->k_image_stride, p->k_head_stride, p->k_row_stride) && quads(v, p->v_image_stride, p->v_head_stride, p->v_row_stride);
    g.vec_out = quads(out, p->out_image_stride, p->out_head_stride, p->out_row_stride);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)plan.blocks, 1, (unsigned)plan.splits);
    const int rw = plan.row_tile / 32;
    switch ((p->d + 31) / 32)
    {
    case 1: launch_sdpa<1>(rw, grid, s, g); break;
    case 2: launch_sdpa<2>(rw, grid, s, g); break;
    case 3: launch_sdpa<3>(rw, grid, s, g); break;
    default: launch_sdpa<4>(rw, grid, s, g); break;
    }
    FHIP_CHECK_HIP(hipGetLastError());
    if (plan.splits > 1)
    {
        const i64 quads_all = (i64)p->n * p->kv_heads * plan.R * (p->d / 4); // <= the output's elements < 2^31
        hipLaunchKernelGGL(sdpa_combine_kernel, dim3((unsigned)((quads_all + 255) / 256)), dim3(256), 0, s, g, (unsigned)quads_all);
        FHIP_CHECK_HIP(hipGetLastError());
    }
    return FHIP_OK;
}

int fhip_kv_concat_forward(int n, int kv_heads, int tp, int tn, int d, const float* past, const float* fresh, float* present, void* stream)
{
    if (n < 1 || kv_heads < 1 || tn < 1 || d < 1 || tp < 0) return fail(FHIP_E_BADARG, "n, kv_heads, tn or d < 1, or tp < 0");
    const i64 count = (i64)n * kv_heads * ((i64)tp + tn) * d;
    if (count >= kMaxElements) return fail(FHIP_E_BADARG, "tensors of 2^31 elements or more are not supported");
    if (!fresh || !present || (tp > 0 && !past)) return fail(FHIP_E_BADARG, "null pointer");
    if (!aligned(fresh, 4) || !aligned(present, 4) || !aligned(past, 4)) return fail(FHIP_E_BADARG, "pointers must be 4-byte aligned");
    const bool v = d % 4 == 0 && aligned(fresh, 16) && aligned(present, 16) && (tp == 0 || aligned(past, 16));
    const unsigned unit = v ? 4 : 1, units = (unsigned)(count / unit), past_row = (unsigned)((i64)tp * d / unit), fresh_row = (unsigned)((i64)tn * d / unit);
    hipStream_t s = (hipStream_t)stream;
    if (v) hipLaunchKernelGGL(kv_concat_kernel<1>, dim3(grid_for(units)), dim3(256), 0, s, (uint32_t*)present, (const uint32_t*)past, (const uint32_t*)fresh, units, past_row, fresh_row);
    else hipLaunchKernelGGL(kv_concat_kernel<0>, dim3(grid_for(units)), dim3(256), 0, s, (uint32_t*)present, (const uint32_t*)past, (const uint32_t*)fresh, units, past_row, fresh_row);
    FHIP_CHECK_HIP(hipGetLastError());
    return FHIP_OK;
}

int fhip_rms_norm_forward(int rows, int l, const float* gamma, float eps, float* y, const float* x, void* stream)
{
    if (const int rc = check_rows(rows, l, eps)) return rc;
    if (!y || !x) return fail(FHIP_E_BADARG, "null pointer");
    if (!aligned(y, 4) || !aligned(x, 4) || !aligned(gamma, 4)) return fail(FHIP_E_BADARG, "pointers must be 4-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    if (l <= FHIP_DECODER_RMS_WAVE_MAX) hipLaunchKernelGGL(rms_norm_kernel<0>, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, y, x, gamma, eps, rows, l);
    else hipLaunchKernelGGL(rms_norm_kernel<1>, dim3((unsigned)rows), dim3(256), 0, s, y, x, gamma, eps, rows, l);
    FHIP_CHECK_HIP(hipGetLastError());
    return FHIP_OK;
}

int fhip_rotary_forward(int n, int heads, int t, int d, int interleaved, const float* cos, const float* sin, int cs_image_stride, float* y, const float* x, void* stream)
{
    if (n < 1 || heads < 1 || t < 1 || d < 1) return fail(FHIP_E_BADARG, "n, heads, t or d < 1");
    if (d % 2) return fail(FHIP_E_BADARG, "the rotary embedding needs an even head width d");
    if (interleaved != 0 && interleaved != 1) return fail(FHIP_E_BADARG, "interleaved must be 0 or 1");
    if (cs_image_stride < 0) return fail(FHIP_E_BADARG, "a negative stride");
    if ((i64)n * heads * t * d >= kMaxElements || (i64)(n - 1) * cs_image_stride + (i64)t * (d / 2) >= kMaxElements)
        return fail(FHIP_E_BADARG, "tensors of 2^31 elements or more are not supported");
    if (!cos || !sin || !y || !x) return fail(FHIP_E_BADARG, "null pointer");
    if (!aligned(cos, 4) || !aligned(sin, 4) || !aligned(y, 4) || !aligned(x, 4)) return fail(FHIP_E_BADARG, "pointers must be 4-byte aligned");
    const unsigned pairs = (unsigned)((i64)n * heads * t * (d / 2));
    hipStream_t s = (hipStream_t)stream;
    if (interleaved) hipLaunchKernelGGL(rotary_kernel<1>, dim3(grid_for(pairs)), dim3(256), 0, s, y, x, cos, sin, pairs, (unsigned)heads, (unsigned)t, (unsigned)(d / 2), (i64)cs_image_stride);
    else hipLaunchKernelGGL(rotary_kernel<0>, dim3(grid_for(pairs)), dim3(256), 0, s, y, x, cos, sin, pairs, (unsigned)heads, (unsigned)t, (unsigned)(d / 2), (i64)cs_image_stride);
    FHIP_CHECK_HIP(hipGetLastError());
    return FHIP_OK;
}

int fhip_embed_forward(int rows, int e, int vocab, const int* ids, const float* weight, const float* bias, float* out, void* stream)
{
    if (rows < 1 || e < 1 || vocab < 1) return fail(FHIP_E_BADARG, "rows, e or vocab < 1");
    if ((i64)rows * e >= kMaxElements || (i64)vocab * e >= kMaxElements) return fail(FHIP_E_BADARG, "tensors of 2^31 elements or more are not supported");
    if (!ids || !weight || !out) return fail(FHIP_E_BADARG, "null pointer");
    if (!aligned(ids, 4) || !aligned(weight, 4) || !aligned(bias, 4) || !aligned(out, 4)) return fail(FHIP_E_BADARG, "pointers must be 4-byte aligned");
    const unsigned count = (unsigned)((i64)rows * e);
    hipLaunchKernelGGL(embed_kernel, dim3(grid_for(count)), dim3(256), 0, (hipStream_t)stream, out, ids, weight, bias, count, (unsigned)e, vocab);
    FHIP_CHECK_HIP(hipGetLastError());
    return FHIP_OK;
}

int fhip_decoder_route(int what, int a, int b, int c, char* name, int len)
{
    if (!name || len < 1) return fail(FHIP_E_BADARG, "null name");
    switch (what)
    {
    case FHIP_DECODER_SDPA:
    {
        if (const int rc = check_width(a)) return rc;
        if (b < 1) return fail(FHIP_E_BADARG, "R < 1");
        if (c != 0 && c != 32 && c != 64 && c != 128) return fail(FHIP_E_BADARG, "row_tile must be 0 (auto), 32, 64 or 128");
        snprintf(name, (size_t)len, "fhip::sdpa_kernel<%d, %d>", (a + 31) / 32, row_tile_for(b, c) / 32);
        return FHIP_OK;
    }
    case FHIP_DECODER_COMBINE: snprintf(name, (size_t)len, "fhip::sdpa_combine_kernel"); return FHIP_OK;
    case FHIP_DECODER_KV_CONCAT: snprintf(name, (size_t)len, "fhip::kv_concat_kernel<%d>", a ? 1 : 0); return FHIP_OK;
    case FHIP_DECODER_RMS_NORM:
        if (a < 1) return fail(FHIP_E_BADARG, "l < 1");
        snprintf(name, (size_t)len, "fhip::rms_norm_kernel<%d>", a <= FHIP_DECODER_RMS_WAVE_MAX ? 0 : 1);
        return FHIP_OK;
    case FHIP_DECODER_ROTARY:
        if (a != 0 && a != 1) return fail(FHIP_E_BADARG, "interleaved must be 0 or 1");
        snprintf(name, (size_t)len, "fhip::rotary_kernel<%d>", a);
        return FHIP_OK;
    case FHIP_DECODER_EMBED: snprintf(name, (size_t)len, "fhip::embed_kernel"); return FHIP_OK;
    default: return fail(FHIP_E_BADARG, "unknown operation");
    }
}

const char* fhip_decoder_last_error(void) { return last_error(); }

} // extern "C"
