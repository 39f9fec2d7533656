// libfeather_rnn.so: the recurrent core of ncnn's LSTM, GRU and RNN on gfx950 (include/feather_hip/feather_rnn.h is the contract and the
// definition; DESIGN.md 3.29 the design and its measurements).  CELL: 0 LSTM (G = 4 gates), 1 GRU (3), 2 RNN (1).
//
//   rnn_step_mfma_kernel<CELL>    ONE TIME STEP.  A block of four waves owns (32 hidden units, 32 sequences, a direction) with all G gates of
//                                 those units.  K = H comes in chunks of 32 through LDS: the G x 32 rows of Wh and the 32 rows of h_prev (read in
//                                 place from `out` at the previous position, h0 at the first step).  Wave g < G runs gate g's product
//                                 Wh_g h_prev^T on v_mfma_f32_32x32x2_f32 (rows = units, columns = sequences), then the waves exchange their
//                                 tiles through LDS and every lane finishes four (unit, sequence) elements: adds xp, applies the gates, writes
//                                 h and updates c in the caller's scratch.  No element is touched by two blocks, and no block waits for another:
//                                 the steps are ordered by the launches.
//   rnn_step_direct_kernel<CELL>  the same ownership, staging and pointwise part; the product on plain multiply-adds, each lane its four
//                                 elements.  Every H that is no multiple of FHIP_RNN_MFMA_MULTIPLE.
//   rnn_sequence_kernel<CELL>     THE WHOLE SEQUENCE.  A block owns (4 sequences, a direction): Wh of the direction lies k-major in LDS, h of
//                                 the four sequences twice (read / written), c in registers; lane j < H owns unit j.  __syncthreads separates
//                                 the steps.
//
// Contraction is off for the whole file: a * b + c is two roundings, so a route's sums are the same numbers wherever it runs.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>

#include "feather_hip/feather_rnn.h"
#include "side_error.h"

#pragma clang fp contract(off)

namespace fhip
{

typedef long long i64;
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kUT = FHIP_RNN_UNIT_TILE, kST = FHIP_RNN_SEQ_TILE, kKC = 32, kLD = kKC + 1, kQT = FHIP_RNN_SEQUENCE_TILE;
static_assert(kUT == 32 && kST == 32, "the tiles are those of one 32x32 matrix instruction");

struct RnnArgs
{
    const float *xp, *wh, *bn, *h0, *c0;
    float *out, *hn, *cn, *cs;
    int n, T, H, nd, dir, xs, os, unit_tiles, seq_tiles;
};

template <int CELL>
struct Cell
{
    static constexpr int G = CELL == FHIP_RNN_LSTM ? 4 : (CELL == FHIP_RNN_GRU ? 3 : 1);
};

__device__ __forceinline__ float sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

// One (unit, sequence) element of one step, given the G dot products Wh[g] . h_prev: the text of the header.  h_prev is read only by the GRU,
// c_prev and *c only by the LSTM.
template <int CELL>
__device__ __forceinline__ float pointwise(const float* dot, const float* x, int H, float bn, float h_prev, float c_prev, float* c)
{
    if constexpr (CELL == FHIP_RNN_LSTM)
    {
        const float I = sigmoid(x[0] + dot[0]), F = sigmoid(x[H] + dot[1]), O = sigmoid(x[2 * H] + dot[2]), Gt = tanhf(x[3 * H] + dot[3]);
        *c = F * c_prev + I * Gt;
        return O * tanhf(*c);
    }
    else if constexpr (CELL == FHIP_RNN_GRU)
    {
        const float R = sigmoid(x[0] + dot[0]), U = sigmoid(x[H] + dot[1]);
        const float N = tanhf(x[2 * H] + R * (dot[2] + bn));
        return (1.f - U) * N + U * h_prev;
    }
    else
        return tanhf(x[0] + dot[0]);
}

// The step kernels.  blockIdx.x runs over (direction slot, sequence tile, unit tile).  LDS: Ws[G * 32][33] the rows of Wh of this chunk of K
// (rows past H and columns past H zero), Hs[32][33] the rows of h_prev likewise (sequences past n zero); after the last chunk Ws holds the
// exchanged products, [G][32 sequences][33].
template <int CELL, bool MFMA>
__device__ __forceinline__ void rnn_step(const RnnArgs& a, int step)
{
    constexpr int G = Cell<CELL>::G;
    __shared__ float Ws[G * kUT * kLD];
    __shared__ float Hs[kST * kLD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, hi = lane >> 5;
    const unsigned ut = blockIdx.x % (unsigned)a.unit_tiles, rest = blockIdx.x / (unsigned)a.unit_tiles;
    const unsigned st = rest % (unsigned)a.seq_tiles;
    const int d = (int)(rest / (unsigned)a.seq_tiles); // < nd
    const int u0 = (int)ut * kUT, s0 = (int)st * kST, H = a.H;
    const bool reverse = a.dir == 1 || (a.dir == 2 && d == 1);
    const int t = reverse ? a.T - 1 - step : step, tp = reverse ? t + 1 : t - 1;
    // row of h_prev of sequence i: in `out` at the previous position, in h0 (or nowhere: zeros) at the first step
    const float* hp_base = step ? a.out + (i64)tp * a.os + (i64)d * H : (a.h0 ? a.h0 + (i64)d * H : nullptr);
    const i64 hp_seq = step ? (i64)a.T * a.os : (i64)a.nd * H;
    const float* wd = a.wh + (i64)d * G * H * H;

    f32x16 acc;
    float dacc[4][G];
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int g = 0; g < G; ++g) dacc[j][g] = 0.f;

    for (int k0 = 0; k0 < H; k0 += kKC)
    {
        __syncthreads(); // the previous chunk has been read
        for (int at = tid; at < G * kUT * kKC; at += 256)
        {
            const int r = at >> 5, kk = at & 31, g = r >> 5, unit = u0 + (r & 31), k = k0 + kk;
            Ws[r * kLD + kk] = unit < H && k < H ? wd[((i64)g * H + unit) * H + k] : 0.f;
        }
        for (int at = tid; at < kST * kKC; at += 256)
        {
            const int s = at >> 5, kk = at & 31, seq = s0 + s, k = k0 + kk;
            Hs[s * kLD + kk] = hp_base && seq < a.n && k < H ? hp_base[(i64)seq * hp_seq + k] : 0.f;
        }
        __syncthreads();
        if constexpr (MFMA)
        {
            if (wave < G) // wave-uniform: gate `wave`; A = Wh (row = unit `col`), B = h_prev^T (column = sequence `col`), k = kk + hi
            {
                const float* wrow = Ws + (wave * kUT + col) * kLD + hi;
                const float* hrow = Hs + col * kLD + hi;
#pragma unroll
                for (int kk = 0; kk < kKC; kk += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wrow[kk], hrow[kk], acc, 0, 0, 0);
            }
        }
        else
        {
            const int u = tid & 31;
#pragma unroll
            for (int j = 0; j < 4; ++j)
            {
                const float* hrow = Hs + ((tid >> 5) + 8 * j) * kLD;
#pragma unroll
                for (int g = 0; g < G; ++g)
                {
                    const float* wrow = Ws + (g * kUT + u) * kLD;
                    float s = dacc[j][g];
                    for (int kk = 0; kk < kKC; ++kk) s += wrow[kk] * hrow[kk];
                    dacc[j][g] = s;
                }
            }
        }
    }
    if constexpr (MFMA)
    {
        __syncthreads(); // the last chunk has been read: Ws becomes the exchange [G][sequence][unit]
        if (wave < G)
#pragma unroll
            for (int i = 0; i < 16; ++i) Ws[(wave * kST + col) * kLD + 8 * (i >> 2) + 4 * hi + (i & 3)] = acc[i]; // register i: unit row 8 (i >> 2) + 4 hi + (i & 3)
        __syncthreads();
    }

    const int u = tid & 31, unit = u0 + u;
#pragma unroll
    for (int j = 0; j < 4; ++j)
    {
        const int s = (tid >> 5) + 8 * j, seq = s0 + s;
        if (unit >= H || seq >= a.n) continue;
        float dot[G];
#pragma unroll
        for (int g = 0; g < G; ++g) dot[g] = MFMA ? Ws[(g * kST + s) * kLD + u] : dacc[j][g];
        const float* x = a.xp + ((i64)seq * a.T + t) * a.xs + (i64)d * G * H + unit;
        const i64 state = ((i64)seq * a.nd + d) * H + unit; // h0, c0, hn, cn: [n][nd][H]
        const i64 cell = ((i64)d * a.n + seq) * H + unit;   // the scratch: [nd][n][H]
        float h_prev = 0.f, c_prev = 0.f, c = 0.f, bn = 0.f;
        if constexpr (CELL == FHIP_RNN_GRU)
        {
            h_prev = hp_base ? hp_base[(i64)seq * hp_seq + unit] : 0.f;
            bn = a.bn[(i64)d * H + unit];
        }
        if constexpr (CELL == FHIP_RNN_LSTM) c_prev = step ? a.cs[cell] : (a.c0 ? a.c0[state] : 0.f);
        const float h = pointwise<CELL>(dot, x, H, bn, h_prev, c_prev, &c);
        a.out[((i64)seq * a.T + t) * a.os + (i64)d * H + unit] = h;
        if constexpr (CELL == FHIP_RNN_LSTM) a.cs[cell] = c;
        if (step == a.T - 1)
        {
            if (a.hn) a.hn[state] = h;
            if constexpr (CELL == FHIP_RNN_LSTM)
                if (a.cn) a.cn[state] = c;
        }
    }
}

template <int CELL>
__global__ __launch_bounds__(256) void rnn_step_mfma_kernel(RnnArgs a, int step)
{
    rnn_step<CELL, true>(a, step);
}

template <int CELL>
__global__ __launch_bounds__(256) void rnn_step_direct_kernel(RnnArgs a, int step)
{
    rnn_step<CELL, false>(a, step);
}

// blockIdx.x runs over (sequence tile of 4, direction slot).  LDS: Wt[H][G * H] (k-major: lanes of consecutive units read consecutive
// banks), hs[2][H][4].  G * H * H + 8 H <= FHIP_RNN_SEQUENCE_LDS_FLOATS (the host has checked), so H <= 198 < 256: lane j owns unit j.
template <int CELL>
__global__ __launch_bounds__(256) void rnn_sequence_kernel(RnnArgs a)
{
    constexpr int G = Cell<CELL>::G;
    __shared__ float lds[FHIP_RNN_SEQUENCE_LDS_FLOATS];
    const int tid = threadIdx.x, H = a.H, GH = G * H;
    const int d = (int)(blockIdx.x % (unsigned)a.nd), s0 = (int)(blockIdx.x / (unsigned)a.nd) * kQT;
    const bool reverse = a.dir == 1 || (a.dir == 2 && d == 1);
    float* Wt = lds;
    float* hs = lds + (((size_t)GH * H + 3) & ~(size_t)3); // 16-byte aligned: a step reads the four sequences of a k at once
    const float* wd = a.wh + (i64)d * GH * H;
    for (int at = tid; at < GH * H; at += 256)
    {
        const int row = at / H, k = at - row * H;
        Wt[k * GH + row] = wd[at];
    }
    for (int at = tid; at < H * kQT; at += 256)
    {
        const int k = at / kQT, s = at - k * kQT, seq = s0 + s;
        hs[at] = a.h0 && seq < a.n ? a.h0[((i64)seq * a.nd + d) * H + k] : 0.f;
    }
    const int j = tid;
    const bool owner = j < H;
    float c[kQT], h[kQT], bn = 0.f;
#pragma unroll
    for (int s = 0; s < kQT; ++s)
    {
        const int seq = s0 + s;
        c[s] = CELL == FHIP_RNN_LSTM && owner && a.c0 && seq < a.n ? a.c0[((i64)seq * a.nd + d) * H + j] : 0.f;
        h[s] = 0.f;
    }
    if (CELL == FHIP_RNN_GRU && owner) bn = a.bn[(i64)d * H + j];
    __syncthreads();
    for (int step = 0; step < a.T; ++step)
    {
        const int t = reverse ? a.T - 1 - step : step;
        const float* cur = hs + (step & 1) * H * kQT;
        float* nxt = hs + ((step & 1) ^ 1) * H * kQT;
        if (owner)
        {
            float x[kQT][G]; // asked for before the product, needed behind it
#pragma unroll
            for (int s = 0; s < kQT; ++s)
#pragma unroll
                for (int g = 0; g < G; ++g) x[s][g] = s0 + s < a.n ? a.xp[((i64)(s0 + s) * a.T + t) * a.xs + (i64)d * GH + g * H + j] : 0.f;
            float dot[kQT][G];
#pragma unroll
            for (int s = 0; s < kQT; ++s)
#pragma unroll
                for (int g = 0; g < G; ++g) dot[s][g] = 0.f;
            for (int k = 0; k < H; ++k)
            {
                const float4 hv = *reinterpret_cast<const float4*>(cur + k * kQT);
                const float hk[kQT] = {hv.x, hv.y, hv.z, hv.w};
#pragma unroll
                for (int g = 0; g < G; ++g)
                {
                    const float w = Wt[k * GH + g * H + j];
#pragma unroll
                    for (int s = 0; s < kQT; ++s) dot[s][g] += w * hk[s];
                }
            }
#pragma unroll
            for (int s = 0; s < kQT; ++s)
            {
                const float h_prev = cur[j * kQT + s];
                h[s] = pointwise<CELL>(dot[s], x[s], 1, bn, h_prev, c[s], &c[s]); // x[s] with a gate stride of 1
                nxt[j * kQT + s] = h[s];
                if (s0 + s < a.n) a.out[((i64)(s0 + s) * a.T + t) * a.os + (i64)d * H + j] = h[s];
            }
        }
        __syncthreads(); // nxt is complete, cur has been read
    }
    if (!owner) return;
#pragma unroll
    for (int s = 0; s < kQT; ++s)
    {
        const int seq = s0 + s;
        if (seq >= a.n) continue;
        const i64 state = ((i64)seq * a.nd + d) * H + j;
        if (a.hn) a.hn[state] = h[s];
        if (CELL == FHIP_RNN_LSTM && a.cn) a.cn[state] = c[s];
    }
}

// ---- host checks -----------------------------------------------------------------------------------------------------------------------
constexpr i64 kMaxElements = 1ll << 31;

static bool overlap(const void* a, size_t na, const void* b, size_t nb)
{
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}

static int gates(int cell) { return cell == FHIP_RNN_LSTM ? 4 : (cell == FHIP_RNN_GRU ? 3 : 1); }

static bool sequence_fits(int cell, int h)
{
    if (cell < FHIP_RNN_LSTM || cell > FHIP_RNN_RNN || h < 1 || h > FHIP_RNN_SEQUENCE_MAX_H_RNN) return false;
    // (Wh rounded up to 16 bytes, which moves no H across the bound: the sums next to it are 40800, 40595 and 40788)
    return (((i64)gates(cell) * h * h + 3) & ~3ll) + 2ll * kQT * h <= FHIP_RNN_SEQUENCE_LDS_FLOATS;
}

// 0 and *route resolved to STEP or SEQUENCE, or the refusal
static int check_route(int cell, int h, int n, int t, int* route)
{
    if (cell < FHIP_RNN_LSTM || cell > FHIP_RNN_RNN) return fail(FHIP_E_BADARG, "the cell must be 0 (LSTM), 1 (GRU) or 2 (RNN)");
    if (h < 1 || n < 1 || t < 1) return fail(FHIP_E_BADARG, "n, t or h < 1");
    if (*route < FHIP_RNN_ROUTE_AUTO || *route > FHIP_RNN_ROUTE_SEQUENCE) return fail(FHIP_E_BADARG, "the route must be 0 (auto), 1 (step) or 2 (sequence)");
    if (*route == FHIP_RNN_ROUTE_SEQUENCE && !sequence_fits(cell, h))
        return fail(FHIP_E_BADARG, "the sequence route needs G * H * H + 2 * FHIP_RNN_SEQUENCE_TILE * H <= FHIP_RNN_SEQUENCE_LDS_FLOATS");
    if (*route == FHIP_RNN_ROUTE_AUTO) *route = sequence_fits(cell, h) && n <= FHIP_RNN_SEQUENCE_MAX_N ? FHIP_RNN_ROUTE_SEQUENCE : FHIP_RNN_ROUTE_STEP;
    return FHIP_OK;
}

template <int CELL>
static void launch(const RnnArgs& a, int route, hipStream_t s)
{
    if (route == FHIP_RNN_ROUTE_SEQUENCE)
    {
        const unsigned blocks = (unsigned)(((i64)a.n + kQT - 1) / kQT * a.nd);
        hipLaunchKernelGGL(rnn_sequence_kernel<CELL>, dim3(blocks), dim3(256), 0, s, a);
        return;
    }
    const unsigned blocks = (unsigned)((i64)a.unit_tiles * a.seq_tiles * a.nd); // <= n * h * nd / 1 < 2^31
    for (int step = 0; step < a.T; ++step)
    {
        if (a.H % FHIP_RNN_MFMA_MULTIPLE == 0) hipLaunchKernelGGL(rnn_step_mfma_kernel<CELL>, dim3(blocks), dim3(256), 0, s, a, step);
        else hipLaunchKernelGGL(rnn_step_direct_kernel<CELL>, dim3(blocks), dim3(256), 0, s, a, step);
    }
}

} // namespace fhip

using namespace fhip;

extern "C"
{

int fhip_rnn_sequence_fits(int cell, int h) { return sequence_fits(cell, h) ? 1 : 0; }

int fhip_rnn_forward_route(int cell, int direction, int n, int t, int h, const float* xp, int xp_stride, const float* wh, const float* bn, const float* h0,
                           const float* c0, float* out, int out_stride, float* hn, float* cn, float* cell_scratch, void* stream, int route)
{
    const int rc = check_route(cell, h, n, t, &route);
    if (rc) return rc;
    if (direction < 0 || direction > 2) return fail(FHIP_E_BADARG, "the direction must be 0 (forward), 1 (reverse) or 2 (bidirectional)");
    const int nd = direction == 2 ? 2 : 1, G = gates(cell);
    const i64 xrow = (i64)nd * G * h, orow = (i64)nd * h;
    if (xrow >= kMaxElements || xrow * h >= kMaxElements) return fail(FHIP_E_BADARG, "tensors of 2^31 elements or more are not supported");
    if (xp_stride < xrow) return fail(FHIP_E_BADARG, "xp_stride is below its row of nd * G * h floats");
    if (out_stride < orow) return fail(FHIP_E_BADARG, "out_stride is below its row of nd * h floats");
    const i64 rows = (i64)n * t;
    if (rows >= kMaxElements || rows * xp_stride >= kMaxElements || rows * out_stride >= kMaxElements || (i64)n * orow >= kMaxElements)
        return fail(FHIP_E_BADARG, "tensors of 2^31 elements or more are not supported");
    const bool lstm = cell == FHIP_RNN_LSTM, gru = cell == FHIP_RNN_GRU;
    if (!xp || !wh || !out || (gru && !bn) || (lstm && !cell_scratch)) return fail(FHIP_E_BADARG, "null pointer (xp, wh, out; bn for the GRU; the cell scratch for the LSTM)");
    if (!aligned(xp, 4) || !aligned(wh, 4) || !aligned(out, 4) || !aligned(bn, 4) || !aligned(h0, 4) || !aligned(c0, 4) || !aligned(hn, 4) || !aligned(cn, 4) ||
        !aligned(cell_scratch, 4))
        return fail(FHIP_E_BADARG, "pointers must be 4-byte aligned");
    if (overlap(out, (size_t)(rows * out_stride) * 4, xp, (size_t)(rows * xp_stride) * 4)) return fail(FHIP_E_BADARG, "out must not overlap xp");
    RnnArgs a;
    a.xp = xp, a.wh = wh, a.bn = gru ? bn : nullptr, a.h0 = h0, a.c0 = lstm ? c0 : nullptr;
    a.out = out, a.hn = hn, a.cn = lstm ? cn : nullptr, a.cs = lstm ? cell_scratch : nullptr;
    a.n = n, a.T = t, a.H = h, a.nd = nd, a.dir = direction, a.xs = xp_stride, a.os = out_stride;
    a.unit_tiles = (h + kUT - 1) / kUT, a.seq_tiles = (n + kST - 1) / kST;
    hipStream_t s = (hipStream_t)stream;
    if (lstm) launch<FHIP_RNN_LSTM>(a, route, s);
    else if (gru) launch<FHIP_RNN_GRU>(a, route, s);
    else launch<FHIP_RNN_RNN>(a, route, s);
    FHIP_CHECK_HIP(hipGetLastError());
    return FHIP_OK;
}

int fhip_rnn_forward(int cell, int direction, int n, int t, int h, const float* xp, int xp_stride, const float* wh, const float* bn, const float* h0,
                     const float* c0, float* out, int out_stride, float* hn, float* cn, float* cell_scratch, void* stream)
{
    return fhip_rnn_forward_route(cell, direction, n, t, h, xp, xp_stride, wh, bn, h0, c0, out, out_stride, hn, cn, cell_scratch, stream, FHIP_RNN_ROUTE_AUTO);
}

int fhip_rnn_route(int cell, int h, int n, int t, int route, char* name, int len)
{
    if (!name || len < 1) return fail(FHIP_E_BADARG, "null name");
    const int rc = check_route(cell, h, n, t, &route);
    if (rc) return rc;
    const char* kernel = route == FHIP_RNN_ROUTE_SEQUENCE ? "sequence" : (h % FHIP_RNN_MFMA_MULTIPLE == 0 ? "step_mfma" : "step_direct");
    snprintf(name, (size_t)len, "fhip::rnn_%s_kernel<%d>", kernel, cell);
    return FHIP_OK;
}

const char* fhip_rnn_last_error(void) { return last_error(); }

} // extern "C"
