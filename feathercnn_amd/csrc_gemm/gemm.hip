// libfeather_gemm.so: the product of two run-time matrices on gfx950 -- ncnn's Gemm and MatMul (include/feather_hip/feather_gemm.h is the
// contract and the definition; DESIGN.md 3.36 the design, its resource table and its measurements).
//
//   gemm_kernel<TA, TB, TILE>     a block of four waves owns BT x BT of D (BT = 128: a wave owns 64 x 64, 2 x 2 tiles of
//                                 v_mfma_f32_32x32x2_f32, 64 accumulator registers; BT = 64: a wave owns 32 x 32).  K is walked in steps of 16
//                                 through TWO LDS buffers: the global loads of step i + 1 go into registers before the products of step i
//                                 and into the other buffer behind them, one barrier a step.  Global loads are 16 bytes along whichever
//                                 dimension is contiguous for that operand and flag; both operands land in LDS k-major, [k][BT + 4], so the
//                                 matrix instruction reads 32 consecutive floats per half-wave for either flag.  The transposition happens
//                                 once, on the register-to-LDS store: a K-contiguous quad goes out as four 4-byte stores, lane -> (row =
//                                 lane % 16 (+ 16 wave), quad = lane / 16), which with a row of BT + 4 = 4 (mod 16) floats puts the 64 lanes
//                                 of a store on 64 different banks (and its halves on 32 different ones); an M- or N-contiguous quad goes
//                                 out as one aligned 16-byte store to consecutive addresses.  Rows, columns and k past the extent are
//                                 zero-filled on load and skipped on store; a quad that crosses the extent is read float by float.  An
//                                 accumulator lane holds one column of D, so rows store coalesced; alpha, beta and the C broadcast are
//                                 applied in registers.
//   gemm_thin_kernel<TB>          min(M, N) <= 8, no matrix instruction; the host orients the problem so that the thin side is M.
//                                 TB = 1, the large operand is [N][K]: a wave owns a column, a lane every 64th quad of k, up to 8 partial
//                                 sums a lane, a fixed xor tree over the lanes.  TB = 0, [K][N]: a lane owns four columns and every 16th
//                                 k, a block 64 columns; the 16 k-slices are added in order through LDS.
//
// Contraction is off for the whole file: a * b + c is two roundings outside the matrix instruction.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>

#include "feather_hip/feather_gemm.h"
#include "side_error.h"

#pragma clang fp contract(off)

namespace fhip
{

typedef long long i64;
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kKS = FHIP_GEMM_K_STEP;
constexpr int kThin = FHIP_GEMM_THIN_MAX;

// The problem AS LAUNCHED (after the host's swap): D'(m, n) = alpha sum_k A'(m, k) B'(k, n) + beta C'(m, n).
struct GemmArgs
{
    const float *a, *b, *c;
    float* d;
    i64 a_bs, b_bs, c_bs, d_bs; // batch strides
    int lda, ldb;               // gemm_kernel: the leading dimensions of A' and B'
    int a_rs, a_ks;             // gemm_thin_kernel: A'(m, k) at m * a_rs + k * a_ks
    int d_rs, d_cs, c_rs, c_cs; // D'(m, n) at m * d_rs + n * d_cs (gemm_kernel: d_cs = 1); C' likewise, 0 where it broadcasts
    int M, N, K, mt, nt;        // mt, nt: the tiles (gemm_kernel) or 1 and the column groups (gemm_thin_kernel)
    int vec_a, vec_b, has_c;
    float alpha, beta;
};

// `left` >= 1 floats at p belong to the tensor: the 16-byte load only where all four do
__device__ __forceinline__ float4 load_quad(const float* p, int left, int vec)
{
    if (vec && left >= 4) return *reinterpret_cast<const float4*>(p);
    float4 v = make_float4(p[0], 0.f, 0.f, 0.f);
    if (left > 1) v.y = p[1];
    if (left > 2) v.z = p[2];
    if (left > 3) v.w = p[3];
    return v;
}

// One operand's share of a k-step, global -> registers.  The tile is BT rows (of M or N, from r0, extent R) by 16 k (from k0, extent K).
// CK: the operand is K-contiguous ([rows][K]), a quad is four k of one row; else it is row-contiguous ([K][rows]), a quad four rows of one k.
template <int CK, int BT, int PER>
__device__ __forceinline__ void fetch_tile(float4 (&q)[PER], const float* x, int ld, int r0, int R, int k0, int K, int vec, int tid)
{
#pragma unroll
    for (int i = 0; i < PER; ++i)
    {
        q[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        if constexpr (CK)
        {
            const int r = r0 + (tid & 15) + 16 * ((tid >> 6) + 4 * i), k = k0 + 4 * ((tid >> 4) & 3);
            if (r < R && k < K) q[i] = load_quad(x + r * ld + k, K - k, vec);
        }
        else
        {
            const int at = tid + 256 * i, kk = at / (BT / 4), r = r0 + 4 * (at - kk * (BT / 4)), k = k0 + kk;
            if (r < R && k < K) q[i] = load_quad(x + k * ld + r, R - r, vec);
        }
    }
}

// registers -> LDS [16][BT + 4], by the same maps
template <int CK, int BT, int PER>
__device__ __forceinline__ void stage_tile(float* s, const float4 (&q)[PER], int tid)
{
    constexpr int LD = BT + 4;
#pragma unroll
    for (int i = 0; i < PER; ++i)
    {
        if constexpr (CK)
        {
            float* at = s + 4 * ((tid >> 4) & 3) * LD + (tid & 15) + 16 * ((tid >> 6) + 4 * i);
            at[0] = q[i].x, at[LD] = q[i].y, at[2 * LD] = q[i].z, at[3 * LD] = q[i].w;
        }
        else
        {
            const int at = tid + 256 * i, kk = at / (BT / 4);
            *reinterpret_cast<float4*>(s + kk * LD + 4 * (at - kk * (BT / 4))) = q[i];
        }
    }
}

// blockIdx.x runs over (batch, row tile, column tile).  TA: A' is [K][M]; TB: B' is [N][K].
template <int TA, int TB, int TILE>
__global__ __launch_bounds__(256) void gemm_kernel(GemmArgs g)
{
    constexpr int BT = TILE ? FHIP_GEMM_TILE_WIDE : FHIP_GEMM_TILE_SMALL, LD = BT + 4, MI = BT / 64, PER = BT * kKS / 4 / 256;
    __shared__ __attribute__((aligned(16))) float As[2][kKS * LD];
    __shared__ __attribute__((aligned(16))) float Bs[2][kKS * LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, hi = lane >> 5;
    unsigned id = blockIdx.x;
    const unsigned tn = id % (unsigned)g.nt;
    id /= (unsigned)g.nt;
    const unsigned tm = id % (unsigned)g.mt, batch = id / (unsigned)g.mt;
    const int m0 = (int)tm * BT, n0 = (int)tn * BT, wm = (wave >> 1) * 32 * MI, wn = (wave & 1) * 32 * MI;
    const float* A = g.a + (i64)batch * g.a_bs;
    const float* B = g.b + (i64)batch * g.b_bs;

    f32x16 acc[MI][MI];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < MI; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    float4 qa[PER], qb[PER];
    const int steps = (g.K + kKS - 1) / kKS;
    fetch_tile<!TA, BT, PER>(qa, A, g.lda, m0, g.M, 0, g.K, g.vec_a, tid);
    fetch_tile<TB, BT, PER>(qb, B, g.ldb, n0, g.N, 0, g.K, g.vec_b, tid);
    stage_tile<!TA, BT, PER>(As[0], qa, tid);
    stage_tile<TB, BT, PER>(Bs[0], qb, tid);
    __syncthreads();
    for (int s = 0; s < steps; ++s) // block-uniform: every wave meets every barrier
    {
        const int buf = s & 1;
        const bool more = s + 1 < steps;
        if (more) // in flight under the products below
        {
            fetch_tile<!TA, BT, PER>(qa, A, g.lda, m0, g.M, (s + 1) * kKS, g.K, g.vec_a, tid);
            fetch_tile<TB, BT, PER>(qb, B, g.ldb, n0, g.N, (s + 1) * kKS, g.K, g.vec_b, tid);
        }
        const float* as = &As[buf][hi * LD + wm + col]; // the A operand: lane -> (row = lane % 32, k = lane / 32)
        const float* bs = &Bs[buf][hi * LD + wn + col]; // the B operand: lane -> (k = lane / 32, column = lane % 32)
#pragma unroll
        for (int kk = 0; kk < kKS / 2; ++kk)
        {
            float av[MI], bv[MI];
#pragma unroll
            for (int i = 0; i < MI; ++i) av[i] = as[2 * kk * LD + 32 * i], bv[i] = bs[2 * kk * LD + 32 * i];
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int j = 0; j < MI; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i], bv[j], acc[i][j], 0, 0, 0);
        }
        if (more) // the other buffer was read last a step ago, before the barrier that ended it
        {
            stage_tile<!TA, BT, PER>(As[buf ^ 1], qa, tid);
            stage_tile<TB, BT, PER>(Bs[buf ^ 1], qb, tid);
        }
        __syncthreads();
    }

    // register r of a lane is row 8 (r / 4) + 4 (lane / 32) + r % 4, column lane % 32 of its 32 x 32 tile
    float* D = g.d + (i64)batch * g.d_bs;
    const float* C = g.has_c ? g.c + (i64)batch * g.c_bs : nullptr;
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < MI; ++j)
        {
            const int n = n0 + wn + 32 * j + col;
            if (n >= g.N) continue;
#pragma unroll
            for (int r = 0; r < 16; ++r)
            {
                const int m = m0 + wm + 32 * i + 8 * (r >> 2) + 4 * hi + (r & 3);
                if (m >= g.M) continue;
                float v = g.alpha * acc[i][j][r];
                if (C) v = v + g.beta * C[m * g.c_rs + n * g.c_cs];
                D[m * g.d_rs + n] = v;
            }
        }
}

// blockIdx.x runs over (batch, column group).  M <= 8.  TB: B' is [N][K], a group is 4 columns (a wave each); else [K][N], 64 columns.
template <int TB>
__global__ __launch_bounds__(256) void gemm_thin_kernel(GemmArgs g)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned grp = blockIdx.x % (unsigned)g.nt, batch = blockIdx.x / (unsigned)g.nt;
    const float* A = g.a + (i64)batch * g.a_bs;
    const float* B = g.b + (i64)batch * g.b_bs;
    float* D = g.d + (i64)batch * g.d_bs;
    const float* C = g.has_c ? g.c + (i64)batch * g.c_bs : nullptr;
    if constexpr (TB)
    {
        const int n = (int)grp * 4 + wave;
        if (n >= g.N) return; // a whole wave: no barrier follows in this form
        const float* brow = B + n * g.ldb;
        float acc[kThin];
#pragma unroll
        for (int m = 0; m < kThin; ++m) acc[m] = 0.f;
        for (int k = 4 * lane; k < g.K; k += 256)
        {
            const int left = min(4, g.K - k);
            const float4 q = load_quad(brow + k, left, g.vec_b);
            const float bq[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int m = 0; m < kThin; ++m)
                if (m < g.M)
                {
                    const float* ap = A + m * g.a_rs + k * g.a_ks;
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (j < left) acc[m] += ap[j * g.a_ks] * bq[j];
                }
        }
#pragma unroll
        for (int m = 0; m < kThin; ++m)
        {
            if (m >= g.M) break; // wave-uniform
            float x = acc[m];
#pragma unroll
            for (int s = 32; s >= 1; s >>= 1) x += __shfl_xor(x, s, 64); // a fixed tree: every lane ends with the same sum
            if (lane == m)
            {
                float v = g.alpha * x;
                if (C) v = v + g.beta * C[m * g.c_rs + n * g.c_cs];
                D[m * g.d_rs + n * g.d_cs] = v;
            }
        }
    }
    else
    {
        __shared__ float red[16][kThin][64];
        const int cq = tid & 15, ks = tid >> 4, n = (int)grp * 64 + 4 * cq;
        float acc[kThin][4];
#pragma unroll
        for (int m = 0; m < kThin; ++m) acc[m][0] = acc[m][1] = acc[m][2] = acc[m][3] = 0.f;
        if (n < g.N)
            for (int k = ks; k < g.K; k += 16)
            {
                const float4 q = load_quad(B + k * g.ldb + n, g.N - n, g.vec_b); // columns past N: zeros, never stored
#pragma unroll
                for (int m = 0; m < kThin; ++m)
                    if (m < g.M)
                    {
                        const float a = A[m * g.a_rs + k * g.a_ks];
                        acc[m][0] += a * q.x, acc[m][1] += a * q.y, acc[m][2] += a * q.z, acc[m][3] += a * q.w;
                    }
            }
#pragma unroll
        for (int m = 0; m < kThin; ++m)
#pragma unroll
            for (int j = 0; j < 4; ++j) red[ks][m][4 * cq + j] = acc[m][j];
        __syncthreads();
        for (int o = tid; o < g.M * 64; o += 256)
        {
            const int m = o >> 6, c = o & 63, nn = (int)grp * 64 + c;
            if (nn >= g.N) continue;
            float x = red[0][m][c];
#pragma unroll
            for (int s = 1; s < 16; ++s) x += red[s][m][c]; // the 16 k-slices in order
            float v = g.alpha * x;
            if (C) v = v + g.beta * C[m * g.c_rs + nn * g.c_cs];
            D[m * g.d_rs + nn * g.d_cs] = v;
        }
    }
}

// ---- host: checks, the swap, the rule ----------------------------------------------------------------------------------------------------
struct Plan
{
    bool swap, thin;
    int ta, tb, tile; // as launched; tile: 1 wide, 0 small
    GemmArgs g;       // everything but the pointers and the 16-byte flags
    i64 blocks;
};

// one past the last float of a tensor of `batch` matrices [rows][cols] with these strides, or -1 for strides the header refuses
static i64 extent(int batch, int rows, int cols, int ld, int bs)
{
    if (ld < cols || bs < 0) return -1;
    return (i64)(batch - 1) * bs + (i64)(rows - 1) * ld + cols;
}

static int plan_gemm(const fhip_gemm_desc* p, Plan& pl)
{
    if (!p) return fail(FHIP_E_BADARG, "null description");
    if (p->m < 1 || p->n < 1 || p->k < 1 || p->batch < 1) return fail(FHIP_E_BADARG, "m, n, k or batch < 1");
    if ((p->trans_a | p->trans_b | p->out_transpose) & ~1) return fail(FHIP_E_BADARG, "trans_a, trans_b and out_transpose must be 0 or 1");
    if (p->c_broadcast < -1 || p->c_broadcast > 4) return fail(FHIP_E_BADARG, "c_broadcast must be -1 (no C) .. 4");
    if (p->tile != 0 && p->tile != FHIP_GEMM_TILE_SMALL && p->tile != FHIP_GEMM_TILE_WIDE) return fail(FHIP_E_UNSUPPORTED, "tile must be 0 (auto), 64 or 128");
    if (!isfinite(p->alpha) || !isfinite(p->beta)) return fail(FHIP_E_BADARG, "alpha and beta must be finite");
    const int M = p->m, N = p->n, K = p->k, cb = p->c_broadcast;
    const i64 ea = extent(p->batch, p->trans_a ? K : M, p->trans_a ? M : K, p->lda, p->a_batch_stride);
    const i64 eb = extent(p->batch, p->trans_b ? N : K, p->trans_b ? K : N, p->ldb, p->b_batch_stride);
    const i64 ed = extent(p->batch, p->out_transpose ? N : M, p->out_transpose ? M : N, p->ldd, p->d_batch_stride);
    i64 ec = 0;
    if (cb == 3) ec = extent(p->batch, M, N, p->ldc, p->c_batch_stride);
    else if (cb >= 0) ec = extent(p->batch, 1, cb == 0 ? 1 : (cb == 4 ? N : M), cb == 0 ? 1 : (cb == 4 ? N : M), p->c_batch_stride);
    if (ea < 0 || eb < 0 || ec < 0 || ed < 0) return fail(FHIP_E_BADARG, "a leading dimension below its row length, or a negative batch stride");
    if (p->batch > 1 && p->d_batch_stride == 0) return fail(FHIP_E_BADARG, "the batch stride of D must not be 0 where batch > 1");
    if (ea >= FHIP_GEMM_MAX_ELEMENTS || eb >= FHIP_GEMM_MAX_ELEMENTS || ec >= FHIP_GEMM_MAX_ELEMENTS || ed >= FHIP_GEMM_MAX_ELEMENTS)
        return fail(FHIP_E_BADARG, "tensors of 2^31 elements or more (strides included) are not supported");

    // the problem as given, by strides
    int a_rs = p->trans_a ? 1 : p->lda, a_ks = p->trans_a ? p->lda : 1, b_ks = p->trans_b ? 1 : p->ldb, b_ns = p->trans_b ? p->ldb : 1;
    int d_rs = p->out_transpose ? 1 : p->ldd, d_cs = p->out_transpose ? p->ldd : 1;
    int c_rs = cb == 1 || cb == 2 ? 1 : (cb == 3 ? p->ldc : 0), c_cs = cb == 3 || cb == 4 ? 1 : 0;
    pl.thin = p->tile == 0 && std::min(M, N) <= kThin;
    pl.swap = pl.thin ? N < M : p->out_transpose != 0; // D^T = op(B)^T op(A)^T: the thin side becomes M; a transposed D becomes row-major
    GemmArgs& g = pl.g;
    memset(&g, 0, sizeof(g));
    g.M = M, g.N = N, g.K = K;
    g.a_bs = p->a_batch_stride, g.b_bs = p->b_batch_stride, g.c_bs = p->c_batch_stride, g.d_bs = p->d_batch_stride;
    g.lda = p->lda, g.ldb = p->ldb;
    pl.ta = p->trans_a, pl.tb = p->trans_b;
    if (pl.swap)
    {
        std::swap(g.M, g.N), std::swap(g.a_bs, g.b_bs), std::swap(g.lda, g.ldb);
        std::swap(d_rs, d_cs), std::swap(c_rs, c_cs);
        const int rs = b_ns, ks = b_ks;
        b_ns = a_rs, b_ks = a_ks, a_rs = rs, a_ks = ks;
        pl.ta = !p->trans_b, pl.tb = !p->trans_a;
    }
    g.a_rs = a_rs, g.a_ks = a_ks, g.d_rs = d_rs, g.d_cs = d_cs, g.c_rs = c_rs, g.c_cs = c_cs;
    g.has_c = cb >= 0, g.alpha = p->alpha, g.beta = p->beta;
    if (pl.thin)
    {
        pl.tile = 0;
        g.mt = 1, g.nt = pl.tb ? (g.N + 3) / 4 : (g.N + 63) / 64;
    }
    else
    {
        const i64 wide = (i64)p->batch * ((g.M + 127) / 128) * ((g.N + 127) / 128);
        pl.tile = p->tile ? p->tile == FHIP_GEMM_TILE_WIDE : wide >= FHIP_GEMM_WIDE_BLOCKS && std::min(g.M, g.N) > FHIP_GEMM_TILE_SMALL;
        const int bt = pl.tile ? FHIP_GEMM_TILE_WIDE : FHIP_GEMM_TILE_SMALL;
        g.mt = (g.M + bt - 1) / bt, g.nt = (g.N + bt - 1) / bt;
    }
    pl.blocks = (i64)p->batch * g.mt * g.nt;
    if (pl.blocks >= FHIP_GEMM_MAX_ELEMENTS) return fail(FHIP_E_BADARG, "batch * blocks reaches 2^31");
    return FHIP_OK;
}

template <int TA, int TB>
static void launch_gemm(int tile, dim3 grid, hipStream_t s, const GemmArgs& g)
{
    if (tile) hipLaunchKernelGGL((gemm_kernel<TA, TB, 1>), grid, dim3(256), 0, s, g);
    else hipLaunchKernelGGL((gemm_kernel<TA, TB, 0>), grid, dim3(256), 0, s, g);
}

} // namespace fhip

using namespace fhip;

extern "C"
{

int fhip_gemm_forward(const fhip_gemm_desc* p, const float* a, const float* b, const float* c, float* d, void* stream)
{
    Plan pl;
    if (const int rc = plan_gemm(p, pl)) return rc;
    if (!a || !b || !d || (p->c_broadcast >= 0 && !c)) return fail(FHIP_E_BADARG, "null pointer");
    if (!aligned(a, 4) || !aligned(b, 4) || !aligned(c, 4) || !aligned(d, 4)) return fail(FHIP_E_BADARG, "pointers must be 4-byte aligned");
    GemmArgs g = pl.g;
    g.a = pl.swap ? b : a, g.b = pl.swap ? a : b, g.c = p->c_broadcast >= 0 ? c : nullptr, g.d = d;
    g.vec_a = aligned(g.a, 16) && g.lda % 4 == 0 && g.a_bs % 4 == 0;
    g.vec_b = aligned(g.b, 16) && g.ldb % 4 == 0 && g.b_bs % 4 == 0;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)pl.blocks);
    if (pl.thin)
    {
        if (pl.tb) hipLaunchKernelGGL(gemm_thin_kernel<1>, grid, dim3(256), 0, s, g);
        else hipLaunchKernelGGL(gemm_thin_kernel<0>, grid, dim3(256), 0, s, g);
    }
    else if (pl.ta)
        pl.tb ? launch_gemm<1, 1>(pl.tile, grid, s, g) : launch_gemm<1, 0>(pl.tile, grid, s, g);
    else
        pl.tb ? launch_gemm<0, 1>(pl.tile, grid, s, g) : launch_gemm<0, 0>(pl.tile, grid, s, g);
    FHIP_CHECK_HIP(hipGetLastError());
    return FHIP_OK;
}

int fhip_gemm_route(const fhip_gemm_desc* p, char* name, int len)
{
    if (!name || len < 1) return fail(FHIP_E_BADARG, "null name");
    Plan pl;
    if (const int rc = plan_gemm(p, pl)) return rc;
    if (pl.thin) snprintf(name, (size_t)len, "fhip::gemm_thin_kernel<%d>", pl.tb);
    else snprintf(name, (size_t)len, "fhip::gemm_kernel<%d, %d, %d>", pl.ta, pl.tb, pl.tile);
    return FHIP_OK;
}

const char* fhip_gemm_last_error(void) { return last_error(); }

} // extern "C"
