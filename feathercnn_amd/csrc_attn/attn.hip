// libfeather_attn.so: the layers of a Vision Transformer encoder on gfx950 (include/feather_hip/feather_attn.h is the contract and the
// definition; DESIGN.md 3.28 the design and its measurements).
//
//   attention_mfma_kernel<DC>     a block of two waves owns (image, head, 64 queries), a wave 32 of them.  Keys come in tiles of 32 through
//                                 LDS.  Both products run TRANSPOSED on v_mfma_f32_32x32x2_f32, so that a lane's 16 accumulator registers hold
//                                 16 keys of ONE query (column = lane & 31): S^T = K Q^T, then O^T += V^T P^T.  The row maximum and sum of
//                                 the online softmax are then in-lane reductions plus one exchange with lane ^ 32, and P^T is already the B
//                                 operand of the second product -- the k index of step s of that product is the key register s holds
//                                 (8 * (s >> 2) + 4 * (lane >> 5) + (s & 3)), which is legal because A and B agree on it.  DC = ceil(d / 32):
//                                 the 32-column chunks of a head; columns past d are zero in LDS and in the Q registers.
//   attention_direct_kernel       a wave per (image, head, query): every other head width.  Keys in chunks of 64, a lane a key; the query row
//                                 and the running output row live in LDS; the same online softmax.
//   layer_norm_kernel<B, A>       B = 0: a wave per row, 4 rows a block; B = 1: a block of 256 lanes per row.  Three passes over the row (sum of
//                                 x - x[0], centred squares, write), the second and third from cache.  A = 1: the row is a + b, written on the way.
//   gelu_kernel<F, V>             element-wise; V = 1: 16 bytes a lane, the tail scalar
//   binary_kernel<FORM, V>        element-wise, the op a uniform switch
//
// Contraction is off for the whole file: a * b + c is two roundings wherever the text of the header says so.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>

#include "feather_hip/feather_attn.h"
#include "side_error.h"

#pragma clang fp contract(off)

namespace fhip
{

typedef long long i64;
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kQT = FHIP_ATTN_QUERY_TILE, kKT = FHIP_ATTN_KEY_TILE;
constexpr unsigned kMaxBlocks = 16384;

struct AttnArgs
{
    const float *q, *k, *v;
    float* out;
    int heads, tq, tk, e, d, qs, ks, vs, q_tiles, vec_out;
};

__device__ __forceinline__ float xor32(float x) { return __shfl_xor(x, 32, 64); }

// blockIdx.x runs over (image, head, query tile).  LDS: K tile [32][32 DC + 1] (columns past d zero), V tile [32][32 DC + 1] likewise; rows
// of keys past tk are zero in both, their scores masked.
template <int DC>
__global__ __launch_bounds__(128) void attention_mfma_kernel(AttnArgs g)
{
    constexpr int W = 32 * DC, LD = W + 1, HALF = 16 * DC;
    __shared__ float Ks[kKT * LD];
    __shared__ float Vs[kKT * LD];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 31, hi = lane >> 5;
    const unsigned tile = blockIdx.x % (unsigned)g.q_tiles, ih = blockIdx.x / (unsigned)g.q_tiles;
    const unsigned head = ih % (unsigned)g.heads, img = ih / (unsigned)g.heads;
    const int c0 = (int)head * g.d;
    const int query = (int)tile * kQT + wave * 32 + col; // this lane's query: column `col` of S^T and O^T
    const bool have_q = query < g.tq;

    // Q^T as the B operand of S^T = K Q^T: step s of the product takes k index hi * HALF + s from both operands
    float qr[HALF];
    {
        const float* qrow = g.q + ((i64)img * g.tq + (have_q ? query : 0)) * g.qs + c0;
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

    const float* kbase = g.k + (i64)img * g.tk * g.ks + c0;
    const float* vbase = g.v + (i64)img * g.tk * g.vs + c0;
    for (int key0 = 0; key0 < g.tk; key0 += kKT)
    {
        __syncthreads(); // the previous tile has been read
        for (int at = threadIdx.x; at < kKT * W; at += 128)
        {
            const int r = at / W, c = at - r * W;
            const bool have = key0 + r < g.tk && c < g.d;
            Ks[r * LD + c] = have ? kbase[(i64)(key0 + r) * g.ks + c] : 0.f;
            Vs[r * LD + c] = have ? vbase[(i64)(key0 + r) * g.vs + c] : 0.f;
        }
        __syncthreads();

        // S^T[key][query]: A = K (row = key `col` of the tile), B = Q^T
        f32x16 st;
#pragma unroll
        for (int i = 0; i < 16; ++i) st[i] = 0.f;
        const float* krow = Ks + col * LD + hi * HALF;
#pragma unroll
        for (int s = 0; s < HALF; ++s) st = __builtin_amdgcn_mfma_f32_32x32x2f32(krow[s], qr[s], st, 0, 0, 0);

        // register i holds key 8 * (i >> 2) + 4 * hi + (i & 3) of the tile for this lane's query
        float tmax = -INFINITY;
#pragma unroll
        for (int i = 0; i < 16; ++i)
        {
            const int key = key0 + 8 * (i >> 2) + 4 * hi + (i & 3);
            st[i] = key < g.tk ? st[i] : -INFINITY;
            tmax = fmaxf(tmax, st[i]);
        }
        tmax = fmaxf(tmax, xor32(tmax));
        const float m_new = fmaxf(m, tmax); // finite from the first tile on: key0 itself is a key
        const float alpha = expf(m - m_new); // 0 at the first tile (m = -inf)
        float psum = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i)
        {
            st[i] = expf(st[i] - m_new); // a masked key: exp(-inf) = 0
            psum += st[i];
        }
        psum += xor32(psum);
        l = l * alpha + psum;
        m = m_new;
#pragma unroll
        for (int j = 0; j < DC; ++j)
#pragma unroll
            for (int i = 0; i < 16; ++i) o[j][i] *= alpha;

        // O^T[column][query] += V^T P^T: step s takes the key register s holds; A = V^T (row = column 32 j + col of the head)
#pragma unroll
        for (int s = 0; s < 16; ++s)
        {
            const float* vrow = Vs + (8 * (s >> 2) + 4 * hi + (s & 3)) * LD + col;
#pragma unroll
            for (int j = 0; j < DC; ++j) o[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(vrow[32 * j], st[s], o[j], 0, 0, 0);
        }
    }

    if (!have_q) return;
    const float inv = 1.f / l;
    float* orow = g.out + ((i64)img * g.tq + query) * g.e + c0;
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

// blockIdx.x runs over (image, head, query); one wave.  d <= FHIP_ATTN_DIRECT_MAX_D.
__global__ __launch_bounds__(64) void attention_direct_kernel(AttnArgs g)
{
    __shared__ float qs[FHIP_ATTN_DIRECT_MAX_D];
    __shared__ float os[FHIP_ATTN_DIRECT_MAX_D];
    __shared__ float ps[64];
    const int lane = threadIdx.x;
    const unsigned query = blockIdx.x % (unsigned)g.tq, ih = blockIdx.x / (unsigned)g.tq;
    const unsigned head = ih % (unsigned)g.heads, img = ih / (unsigned)g.heads;
    const int c0 = (int)head * g.d;
    const float* qrow = g.q + ((i64)img * g.tq + query) * g.qs + c0;
    for (int c = lane; c < g.d; c += 64) qs[c] = qrow[c], os[c] = 0.f;
    __syncthreads();
    const float* kbase = g.k + (i64)img * g.tk * g.ks + c0;
    const float* vbase = g.v + (i64)img * g.tk * g.vs + c0;
    float m = -INFINITY, l = 0.f;
    for (int key0 = 0; key0 < g.tk; key0 += 64)
    {
        const int key = key0 + lane;
        float s = -INFINITY;
        if (key < g.tk)
        {
            const float* krow = kbase + (i64)key * g.ks;
            s = 0.f;
            for (int c = 0; c < g.d; ++c) s += qs[c] * krow[c];
        }
        const float m_new = fmaxf(m, wave_max(s));
        const float alpha = expf(m - m_new);
        const float p = expf(s - m_new);
        l = l * alpha + wave_sum(p);
        m = m_new;
        __syncthreads(); // ps of the previous chunk has been read
        ps[lane] = p;
        __syncthreads();
        const int here = min(64, g.tk - key0);
        for (int c = lane; c < g.d; c += 64)
        {
            float acc = os[c] * alpha;
            for (int j = 0; j < here; ++j) acc += ps[j] * vbase[(i64)(key0 + j) * g.vs + c];
            os[c] = acc; // column c is this lane's alone
        }
    }
    const float inv = 1.f / l;
    float* orow = g.out + ((i64)img * g.tq + query) * g.e + c0;
    for (int c = lane; c < g.d; c += 64) orow[c] = os[c] * inv;
}

// ---- LayerNorm ---------------------------------------------------------------------------------------------------------------------------
// the sum of one value per lane over the row's lanes: a wave (B = 0), or the block's 4 waves through LDS (B = 1), the same order every time
template <int B>
__device__ __forceinline__ float row_sum(float x, float* part)
{
    x = wave_sum(x);
    if constexpr (B)
    {
        __syncthreads(); // `part` of the previous reduction has been read
        if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = x;
        __syncthreads();
        x = (part[0] + part[1]) + (part[2] + part[3]);
    }
    return x;
}

template <int B, int A>
__global__ __launch_bounds__(256) void layer_norm_kernel(float* __restrict__ y, float* sum, const float* a, const float* b, const float* __restrict__ gamma,
                                                         const float* __restrict__ beta, float eps, int rows, int L)
{
    __shared__ float part[4];
    constexpr int STEP = B ? 256 : 64;
    const int lane = B ? threadIdx.x : (threadIdx.x & 63);
    const i64 row = B ? (i64)blockIdx.x : (i64)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (!B && row >= rows) return; // a whole wave: no barrier follows in this form
    const float* pa = a + row * L;
    const float* pb = A ? b + row * L : nullptr;
    // the row is shifted by its first element before it is summed: x - pivot is exact for a row of large mean and small spread, whose mean no
    // float holds to the precision its spread asks for
    const float pivot = A ? pa[0] + pb[0] : pa[0];
    float acc = 0.f;
    for (int i = lane; i < L; i += STEP) acc += (A ? pa[i] + pb[i] : pa[i]) - pivot;
    const float mean = row_sum<B>(acc, part) / (float)L; // of x - pivot
    acc = 0.f;
    for (int i = lane; i < L; i += STEP)
    {
        const float c = ((A ? pa[i] + pb[i] : pa[i]) - pivot) - mean;
        acc += c * c;
    }
    const float var = row_sum<B>(acc, part) / (float)L;
    const float scale = 1.f / sqrtf(var + eps);
    float* py = y + row * L;
    for (int i = lane; i < L; i += STEP)
    {
        const float x = A ? pa[i] + pb[i] : pa[i];
        if constexpr (A) sum[row * L + i] = x; // may be a or b: this lane has read element i for the last time
        float r = ((x - pivot) - mean) * scale;
        if (gamma) r = r * gamma[i];
        if (beta) r = r + beta[i];
        py[i] = r;
    }
}

// ---- GELU, Binary ------------------------------------------------------------------------------------------------------------------------
template <int F>
__device__ __forceinline__ float gelu(float x)
{
    if constexpr (F) return 0.5f * x * (1.f + tanhf(0.79788452f * (x + 0.044715f * x * x * x)));
    return 0.5f * x * (1.f + erff(0.70710678f * x));
}

template <int F, int V>
__global__ __launch_bounds__(256) void gelu_kernel(float* __restrict__ out, const float* __restrict__ in, unsigned count)
{
    const unsigned tid = blockIdx.x * 256u + threadIdx.x, step = gridDim.x * 256u;
    const unsigned quads = V ? count / 4 : 0;
    for (unsigned i = tid; i < quads; i += step)
    {
        float4 t = reinterpret_cast<const float4*>(in)[i];
        t.x = gelu<F>(t.x), t.y = gelu<F>(t.y), t.z = gelu<F>(t.z), t.w = gelu<F>(t.w);
        reinterpret_cast<float4*>(out)[i] = t;
    }
    for (unsigned i = quads * 4 + tid; i < count; i += step) out[i] = gelu<F>(in[i]);
}

__device__ __forceinline__ float binary(int op, float x, float y)
{
    switch (op)
    {
    case FHIP_BINARY_ADD: return x + y;
    case FHIP_BINARY_SUB: return x - y;
    case FHIP_BINARY_MUL: return x * y;
    case FHIP_BINARY_DIV: return x / y;
    case FHIP_BINARY_MAX: return fmaxf(x, y);
    default: return fminf(x, y);
    }
}

// out and a may be the same buffer (no __restrict__): an element is read before it is written, by the same lane
template <int FORM, int V>
__global__ __launch_bounds__(256) void binary_kernel(float* out, const float* a, const float* b, float scalar, int op, int swap, unsigned count, unsigned per)
{
    const unsigned tid = blockIdx.x * 256u + threadIdx.x, step = gridDim.x * 256u;
    const unsigned quads = V ? count / 4 : 0;
    for (unsigned i = tid; i < quads; i += step)
    {
        const float4 x = reinterpret_cast<const float4*>(a)[i];
        float4 y = make_float4(scalar, scalar, scalar, scalar);
        if constexpr (FORM == FHIP_BINARY_TENSOR) y = reinterpret_cast<const float4*>(b)[i];
        if constexpr (FORM == FHIP_BINARY_BROADCAST) y = reinterpret_cast<const float4*>(b)[i % (per / 4)]; // per % 4 == 0 in this form
        float4 r;
        r.x = swap ? binary(op, y.x, x.x) : binary(op, x.x, y.x);
        r.y = swap ? binary(op, y.y, x.y) : binary(op, x.y, y.y);
        r.z = swap ? binary(op, y.z, x.z) : binary(op, x.z, y.z);
        r.w = swap ? binary(op, y.w, x.w) : binary(op, x.w, y.w);
        reinterpret_cast<float4*>(out)[i] = r;
    }
    for (unsigned i = quads * 4 + tid; i < count; i += step)
    {
        const float x = a[i];
        const float y = FORM == FHIP_BINARY_TENSOR ? b[i] : (FORM == FHIP_BINARY_BROADCAST ? b[i % per] : scalar);
        out[i] = swap ? binary(op, y, x) : binary(op, x, y);
    }
}

// ---- host checks -----------------------------------------------------------------------------------------------------------------------
constexpr i64 kMaxElements = 1ll << 31;

static bool overlap(const void* a, size_t na, const void* b, size_t nb)
{
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}

static bool mfma_route(int d) { return d % 4 == 0 && d <= FHIP_ATTN_MFMA_MAX_D; }

static int check_attention(int n, int heads, int tq, int tk, int e)
{
    if (tk < 1) return fail(FHIP_E_BADARG, "attention needs at least one key (tk < 1)");
    if (n < 1 || heads < 1 || tq < 1 || e < 1) return fail(FHIP_E_BADARG, "n, heads, tq or e < 1");
    if (e % heads) return fail(FHIP_E_BADARG, "the embedding width is no multiple of the number of heads (E % heads != 0)");
    if (!mfma_route(e / heads) && e / heads > FHIP_ATTN_DIRECT_MAX_D)
        return fail(FHIP_E_BADARG, "a head wider than FHIP_ATTN_DIRECT_MAX_D (4096) that is no multiple of 4 <= 128 is not supported");
    return FHIP_OK;
}

static unsigned elementwise_blocks(size_t count, int v) { return (unsigned)std::min<size_t>((count / (v ? 4 : 1) + 255) / 256 + 1, kMaxBlocks); }

static int check_layer_norm(int rows, int l, float eps)
{
    if (rows < 1 || l < 1) return fail(FHIP_E_BADARG, "rows or l < 1");
    if ((i64)rows * l >= kMaxElements) return fail(FHIP_E_BADARG, "tensors of 2^31 elements or more are not supported");
    if (!(eps >= 0.f) || !isfinite(eps)) return fail(FHIP_E_BADARG, "eps must be finite and >= 0");
    return FHIP_OK;
}

template <int A>
static void launch_layer_norm(int rows, int l, float* y, float* sum, const float* a, const float* b, const float* gamma, const float* beta, float eps, hipStream_t s)
{
    if (l <= FHIP_ATTN_LN_WAVE_MAX)
        hipLaunchKernelGGL((layer_norm_kernel<0, A>), dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, y, sum, a, b, gamma, beta, eps, rows, l);
    else
        hipLaunchKernelGGL((layer_norm_kernel<1, A>), dim3((unsigned)rows), dim3(256), 0, s, y, sum, a, b, gamma, beta, eps, rows, l);
}

} // namespace fhip

using namespace fhip;

extern "C"
{

int fhip_attention_forward(int n, int heads, int tq, int tk, int e, const float* q, int q_stride, const float* k, int k_stride, const float* v, int v_stride,
                           float* out, void* stream)
{
    const int rc = check_attention(n, heads, tq, tk, e);
    if (rc) return rc;
    if (q_stride < e || k_stride < e || v_stride < e) return fail(FHIP_E_BADARG, "a row stride below the embedding width");
    if ((i64)n * tq * q_stride >= kMaxElements || (i64)n * tk * k_stride >= kMaxElements || (i64)n * tk * v_stride >= kMaxElements ||
        (i64)n * tq * e >= kMaxElements || (i64)n * tq >= kMaxElements || (i64)n * tk >= kMaxElements)
        return fail(FHIP_E_BADARG, "tensors of 2^31 elements or more are not supported");
    if (!q || !k || !v || !out) return fail(FHIP_E_BADARG, "null pointer");
    if (!aligned(q, 4) || !aligned(k, 4) || !aligned(v, 4) || !aligned(out, 4)) return fail(FHIP_E_BADARG, "pointers must be 4-byte aligned");
    AttnArgs g;
    g.q = q, g.k = k, g.v = v, g.out = out;
    g.heads = heads, g.tq = tq, g.tk = tk, g.e = e, g.d = e / heads, g.qs = q_stride, g.ks = k_stride, g.vs = v_stride;
    g.q_tiles = (tq + kQT - 1) / kQT;
    g.vec_out = aligned(out, 16) && e % 4 == 0;
    hipStream_t s = (hipStream_t)stream;
    if (mfma_route(g.d))
    {
        const i64 blocks = (i64)n * heads * g.q_tiles;
        if (blocks >= kMaxElements) return fail(FHIP_E_BADARG, "tensors of 2^31 elements or more are not supported");
        switch ((g.d + 31) / 32)
        {
        case 1: hipLaunchKernelGGL(attention_mfma_kernel<1>, dim3((unsigned)blocks), dim3(128), 0, s, g); break;
        case 2: hipLaunchKernelGGL(attention_mfma_kernel<2>, dim3((unsigned)blocks), dim3(128), 0, s, g); break;
        case 3: hipLaunchKernelGGL(attention_mfma_kernel<3>, dim3((unsigned)blocks), dim3(128), 0, s, g); break;
        default: hipLaunchKernelGGL(attention_mfma_kernel<4>, dim3((unsigned)blocks), dim3(128), 0, s, g); break;
        }
    }
    else
    {
        const i64 blocks = (i64)n * heads * tq; // <= n * tq * e < 2^31
        hipLaunchKernelGGL(attention_direct_kernel, dim3((unsigned)blocks), dim3(64), 0, s, g);
    }
    FHIP_CHECK_HIP(hipGetLastError());
    return FHIP_OK;
}

int fhip_layer_norm_forward(int rows, int l, const float* gamma, const float* beta, float eps, float* y, const float* x, void* stream)
{
    const int rc = check_layer_norm(rows, l, eps);
    if (rc) return rc;
    if (!y || !x) return fail(FHIP_E_BADARG, "null pointer");
    if (!aligned(y, 4) || !aligned(x, 4) || !aligned(gamma, 4) || !aligned(beta, 4)) return fail(FHIP_E_BADARG, "pointers must be 4-byte aligned");
    const size_t bytes = (size_t)rows * l * 4;
    if (overlap(y, bytes, x, bytes)) return fail(FHIP_E_BADARG, "y must not overlap x");
    launch_layer_norm<0>(rows, l, y, nullptr, x, nullptr, gamma, beta, eps, (hipStream_t)stream);
    FHIP_CHECK_HIP(hipGetLastError());
    return FHIP_OK;
}

int fhip_add_layer_norm_forward(int rows, int l, const float* gamma, const float* beta, float eps, float* sum, float* y, const float* a, const float* b,
                                void* stream)
{
    const int rc = check_layer_norm(rows, l, eps);
    if (rc) return rc;
    if (!y || !sum || !a || !b) return fail(FHIP_E_BADARG, "null pointer");
    if (!aligned(y, 4) || !aligned(sum, 4) || !aligned(a, 4) || !aligned(b, 4) || !aligned(gamma, 4) || !aligned(beta, 4))
        return fail(FHIP_E_BADARG, "pointers must be 4-byte aligned");
    const size_t bytes = (size_t)rows * l * 4;
    if (overlap(y, bytes, a, bytes) || overlap(y, bytes, b, bytes) || overlap(y, bytes, sum, bytes)) return fail(FHIP_E_BADARG, "y must not overlap a, b or sum");
    if ((sum != a && overlap(sum, bytes, a, bytes)) || (sum != b && overlap(sum, bytes, b, bytes)))
        return fail(FHIP_E_BADARG, "sum must be a, b or a buffer that overlaps neither");
    launch_layer_norm<1>(rows, l, y, sum, a, b, gamma, beta, eps, (hipStream_t)stream);
    FHIP_CHECK_HIP(hipGetLastError());
    return FHIP_OK;
}

int fhip_gelu_forward(int fast, float* out, const float* in, size_t count, void* stream)
{
    if (fast != 0 && fast != 1) return fail(FHIP_E_BADARG, "fast_gelu must be 0 or 1");
    if (count < 1 || count >= (size_t)kMaxElements) return fail(FHIP_E_BADARG, "count < 1, or tensors of 2^31 elements or more");
    if (!out || !in) return fail(FHIP_E_BADARG, "null pointer");
    if (!aligned(out, 4) || !aligned(in, 4)) return fail(FHIP_E_BADARG, "pointers must be 4-byte aligned");
    if (overlap(out, count * 4, in, count * 4)) return fail(FHIP_E_BADARG, "out must not overlap in");
    const int v = aligned(out, 16) && aligned(in, 16);
    const unsigned blocks = elementwise_blocks(count, v);
    hipStream_t s = (hipStream_t)stream;
    if (fast)
    {
        if (v) hipLaunchKernelGGL((gelu_kernel<1, 1>), dim3(blocks), dim3(256), 0, s, out, in, (unsigned)count);
        else hipLaunchKernelGGL((gelu_kernel<1, 0>), dim3(blocks), dim3(256), 0, s, out, in, (unsigned)count);
    }
    else
    {
        if (v) hipLaunchKernelGGL((gelu_kernel<0, 1>), dim3(blocks), dim3(256), 0, s, out, in, (unsigned)count);
        else hipLaunchKernelGGL((gelu_kernel<0, 0>), dim3(blocks), dim3(256), 0, s, out, in, (unsigned)count);
    }
    FHIP_CHECK_HIP(hipGetLastError());
    return FHIP_OK;
}

int fhip_binary_forward(int op, int form, int swap, float* out, const float* a, const float* b, float scalar, size_t count, size_t per, void* stream)
{
    if (op < FHIP_BINARY_ADD || op > FHIP_BINARY_MIN) return fail(FHIP_E_BADARG, "the binary op must be 0 (add), 1 (sub), 2 (mul), 3 (div), 4 (max) or 5 (min)");
    if (form < FHIP_BINARY_SCALAR || form > FHIP_BINARY_BROADCAST) return fail(FHIP_E_BADARG, "the operand form must be 0 (scalar), 1 (tensor) or 2 (broadcast)");
    if (swap != 0 && swap != 1) return fail(FHIP_E_BADARG, "swap must be 0 or 1");
    if (count < 1 || count >= (size_t)kMaxElements) return fail(FHIP_E_BADARG, "count < 1, or tensors of 2^31 elements or more");
    if (form == FHIP_BINARY_BROADCAST && (per < 1 || per > count || count % per)) return fail(FHIP_E_BADARG, "the broadcast operand must divide the tensor (count % per != 0)");
    if (!out || !a || (form != FHIP_BINARY_SCALAR && !b)) return fail(FHIP_E_BADARG, "null pointer");
    if (!aligned(out, 4) || !aligned(a, 4) || (form != FHIP_BINARY_SCALAR && !aligned(b, 4))) return fail(FHIP_E_BADARG, "pointers must be 4-byte aligned");
    if (out != a && overlap(out, count * 4, a, count * 4)) return fail(FHIP_E_BADARG, "out must be a or not overlap it");
    if (form == FHIP_BINARY_TENSOR && out != b && overlap(out, count * 4, b, count * 4)) return fail(FHIP_E_BADARG, "out must be b or not overlap it");
    if (form == FHIP_BINARY_BROADCAST && overlap(out, count * 4, b, per * 4)) return fail(FHIP_E_BADARG, "out must not overlap the broadcast operand");
    const int v = aligned(out, 16) && aligned(a, 16) && (form == FHIP_BINARY_SCALAR || aligned(b, 16)) && (form != FHIP_BINARY_BROADCAST || per % 4 == 0);
    const unsigned blocks = elementwise_blocks(count, v), cnt = (unsigned)count, pr = (unsigned)per;
    hipStream_t s = (hipStream_t)stream;
#define FHIP_BINARY_LAUNCH(FORM)                                                                                                        \
    if (v) hipLaunchKernelGGL((binary_kernel<FORM, 1>), dim3(blocks), dim3(256), 0, s, out, a, b, scalar, op, swap, cnt, pr);            \
    else hipLaunchKernelGGL((binary_kernel<FORM, 0>), dim3(blocks), dim3(256), 0, s, out, a, b, scalar, op, swap, cnt, pr)
    if (form == FHIP_BINARY_SCALAR) { FHIP_BINARY_LAUNCH(FHIP_BINARY_SCALAR); }
    else if (form == FHIP_BINARY_TENSOR) { FHIP_BINARY_LAUNCH(FHIP_BINARY_TENSOR); }
    else { FHIP_BINARY_LAUNCH(FHIP_BINARY_BROADCAST); }
#undef FHIP_BINARY_LAUNCH
    FHIP_CHECK_HIP(hipGetLastError());
    return FHIP_OK;
}

int fhip_attn_route(int what, int a, int b, char* name, int len)
{
    if (!name || len < 1) return fail(FHIP_E_BADARG, "null name");
    switch (what)
    {
    case FHIP_ATTN_ATTENTION:
    {
        const int rc = check_attention(1, b, 1, 1, a);
        if (rc) return rc;
        const int d = a / b;
        if (mfma_route(d)) snprintf(name, (size_t)len, "fhip::attention_mfma_kernel<%d>", (d + 31) / 32);
        else snprintf(name, (size_t)len, "fhip::attention_direct_kernel");
        return FHIP_OK;
    }
    case FHIP_ATTN_LAYER_NORM:
        if (a < 1) return fail(FHIP_E_BADARG, "l < 1");
        snprintf(name, (size_t)len, "fhip::layer_norm_kernel<%d, %d>", a <= FHIP_ATTN_LN_WAVE_MAX ? 0 : 1, b ? 1 : 0);
        return FHIP_OK;
    case FHIP_ATTN_GELU:
        if (a != 0 && a != 1) return fail(FHIP_E_BADARG, "fast_gelu must be 0 or 1");
        snprintf(name, (size_t)len, "fhip::gelu_kernel<%d, %d>", a, b ? 1 : 0);
        return FHIP_OK;
    case FHIP_ATTN_BINARY:
        if (a < FHIP_BINARY_SCALAR || a > FHIP_BINARY_BROADCAST) return fail(FHIP_E_BADARG, "the operand form must be 0, 1 or 2");
        snprintf(name, (size_t)len, "fhip::binary_kernel<%d, %d>", a, b ? 1 : 0);
        return FHIP_OK;
    default: return fail(FHIP_E_BADARG, "unknown operation");
    }
}

const char* fhip_attn_last_error(void) { return last_error(); }

} // extern "C"
