// libfeather_colpass.so: the Winograd F(6x6,3x3) tile GEMM of 64-input-channel layers that applies the output transform's column pass to
// its accumulators and writes 48 planes of M instead of 64, and the chained transform that reads them
// (include/feather_hip/feather_colpass.h is the contract; DESIGN.md 3.24 the design and its measurements).
//
// colpass_gemm_kernel is the main library's tile GEMM loop (csrc/wino_gemm_glds.h: LDS-DMA operand staging, counted waits, raw barriers,
// v_mfma_f32_32x32x2_f32 in ascending k from a zero start, the per-wave LDS transpose in front of 16-byte row stores) with another block
// shape: a block owns the EIGHT frequency points xi = 8 i + j of one j for 64 output channels and one column tile, one accumulator
// per xi.  colpass_chain_kernel is csrc/winograd_f63.hip's wino_chain_kernel without its column pass.  The butterflies are
// csrc/wino_butterfly.h's, so every value equals the main route's.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <string>

#include "feather_hip/feather_colpass.h"
#include "side_error.h"
#include "wino_butterfly.h"
#include "wino_layout.h"

namespace fhip
{

typedef __attribute__((address_space(3))) void lds_void;

// M stores carry `nt` when the 64-plane M of the layer would have at least this many bytes (csrc/wino_gemm_policy.h FHIP_M_NT_BYTES: the
// size from which nothing written here is still in a cache when the next launch reads it)
constexpr size_t kBigM = (size_t)150u << 20;

struct ColGemm
{
    const float* U; // [64 xi][64][Kp]
    const float* V; // Lv: 64 planes of 64 rows
    float* M;       // Lm: 48 planes of K rows, plane 8 a + j
    int Kp, m_tiles, n_tiles;
    WinoLayout Lv, Lm;
};

template <int N>
__device__ __forceinline__ void wait_stage()
{
    asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(N) : "memory");
}

// The block shape the product runs (measured against the others with tools/colpass_bench.py --lib: DESIGN.md 3.24, EXPERIMENTS.md): WN
// waves along the columns, BK rows of both operands per stage, NBUF LDS buffers (48 KB: three blocks per CU, 40 KB of requests in flight
// per block)
#ifndef COLPASS_WN
#define COLPASS_WN 2
#endif
#ifndef COLPASS_BK
#define COLPASS_BK 16
#endif
#ifndef COLPASS_NBUF
#define COLPASS_NBUF 6
#endif
#ifndef COLPASS_OCC
#define COLPASS_OCC 3 // blocks of 256 lanes per CU the register budget is cut for
#endif

// 64 rows x 32 WN columns x 8 xi per block, 2 x WN waves of one 32 x 32 tile each: eight f32x16 accumulators per wave.  A stage is BK of the
// 64 rows of U_xi (BK x 64 floats) and of V_xi (BK x BN); NBUF - 1 stages are in flight under the MFMAs of the current one.
// NT bit 0: V pieces are requested with the non-temporal hint (one row tile covers K: every V element is read by one block); bit 1: M48
// leaves through `nt` stores.
// Ordering (cdna_hip_programming.md, LDS-DMA; as wino_gemm_glds.h): a wave waits vmcnt for ITS pieces of stage s + 1, then the barrier;
// readers touch that buffer only behind the barrier; a buffer is re-filled only after every wave waited lgkmcnt(0) for its reads of it and
// passed the barrier.
template <int WN, int BK, int NBUF, int NT>
__global__ __launch_bounds__(128 * WN, COLPASS_OCC * WN / 2) void colpass_gemm_kernel(const ColGemm g)
{
    constexpr int C = 64, BM = 64, BN = 32 * WN, NW = 2 * WN, EPI_LD = 36;
    constexpr int KT = C / BK, S = 8 * KT; // stages per frequency point, stages per block
    constexpr int BUF = BK * (BM + BN);    // A [BK][64] then B [BK][BN]
    constexpr int A_PIECES = BK / 4 / NW;  // 1-KB pieces (4 rows of A) per wave and stage
    constexpr int B_LPR = BN / 4, B_RPP = 64 / B_LPR, B_PIECES = BK / B_RPP / NW; // lanes per row of B, rows per piece, pieces per wave
    constexpr int PPS = A_PIECES + B_PIECES;
    constexpr int LDSF = NBUF * BUF > NW * 32 * EPI_LD ? NBUF * BUF : NW * 32 * EPI_LD;
    static_assert(A_PIECES >= 1 && B_PIECES >= 1 && A_PIECES * 4 * NW == BK && B_PIECES * B_RPP * NW == BK, "stage pieces");
    static_assert(NBUF >= 2 && NBUF <= S, "buffers");
    __shared__ __attribute__((aligned(16))) float lds[LDSF];

    int vid = xcd_remap(blockIdx.x, 8 * g.m_tiles * g.n_tiles);
    // j fastest: the eight blocks of a column tile run next to each other on one XCD and read all 64 frequency points of the same columns
    // (conv1_2 b32: 263 against 271 us with j slowest, tools/colpass_bench.py)
    const int j = vid & 7;
    vid >>= 3;
    const int mt = vid % g.m_tiles;
    const int nt = vid / g.m_tiles;
    const int m0 = mt * BM, n0 = nt * BN;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int l31 = lane & 31, half = lane >> 5;

    // per-lane sources of frequency point j, stage 0; xi = 8 i + j is 8 i planes further
    const float* srcA = g.U + (size_t)j * C * g.Kp + (size_t)(wave * A_PIECES * 4 + (lane >> 4)) * g.Kp + m0 + (lane & 15) * 4;
    const float* srcB = g.V + (size_t)j * g.Lv.xis + g.Lv.col(n0) + (size_t)(wave * B_PIECES * B_RPP + lane / B_LPR) * g.Lv.bp + (lane % B_LPR) * 4;
    const size_t a_xi = (size_t)8 * C * g.Kp, b_xi = (size_t)8 * g.Lv.xis;

    auto issue = [&](int s, int buf) {
        const int i = s / KT, kt = s - i * KT;
        float* base = lds + buf * BUF;
        const float* a = srcA + (size_t)i * a_xi + (size_t)(kt * BK) * g.Kp;
        const float* b = srcB + (size_t)i * b_xi + (size_t)(kt * BK) * g.Lv.bp;
#pragma unroll
        for (int p = 0; p < A_PIECES; ++p)
            __builtin_amdgcn_global_load_lds(a + (size_t)(4 * p) * g.Kp, (lds_void*)(base + (wave * A_PIECES + p) * 256), 16, 0, 0);
#pragma unroll
        for (int p = 0; p < B_PIECES; ++p)
            __builtin_amdgcn_global_load_lds(b + (size_t)(B_RPP * p) * g.Lv.bp, (lds_void*)(base + BK * BM + (wave * B_PIECES + p) * 256), 16, 0,
                                             (NT & 1) ? 2 : 0);
    };

    f32x16 acc[8];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;

#pragma unroll
    for (int s = 0; s < NBUF - 1; ++s) issue(s, s);
    wait_stage<(NBUF - 2) * PPS>();
    __builtin_amdgcn_s_barrier();

    const int a_off = half * BM + wm * 32 + l31;
    const int b_off = BK * BM + half * BN + wn * 32 + l31;
#pragma unroll
    for (int s = 0; s < S; ++s)
    {
        const bool more = s + NBUF - 1 < S;
        if (more) issue(s + NBUF - 1, (s + NBUF - 1) % NBUF);
        const float* as = lds + (s % NBUF) * BUF + a_off;
        const float* bs = lds + (s % NBUF) * BUF + b_off;
#pragma unroll
        for (int kp = 0; kp < BK / 2; ++kp) acc[s / KT] = __builtin_amdgcn_mfma_f32_32x32x2f32(as[(2 * kp) * BM], bs[(2 * kp) * BN], acc[s / KT], 0, 0, 0);
        // my pieces of the NEXT stage have landed (the stages behind it may stay in flight), my LDS reads are done
        if (more)
            wait_stage<(NBUF - 2) * PPS>();
        else
            wait_stage<0>();
        __builtin_amdgcn_s_barrier();
    }

    // the column pass, lane-wise across the eight accumulators: plane a of the six lands in acc[a]
#pragma unroll
    for (int r = 0; r < 16; ++r)
    {
        float s0, s1, s2, s3, s4, s5;
        at6(acc[0][r], acc[1][r], acc[2][r], acc[3][r], acc[4][r], acc[5][r], acc[6][r], acc[7][r], s0, s1, s2, s3, s4, s5);
        acc[0][r] = s0;
        acc[1][r] = s1;
        acc[2][r] = s2;
        acc[3][r] = s3;
        acc[4][r] = s4;
        acc[5][r] = s5;
    }

    // epilogue (csrc/gemm_core.h): per-wave LDS transpose in the operand buffers, free behind the last barrier; 16-byte row stores.
    // K is a multiple of 64 and Pp of the column tile: every row and column of the tile exists.
    float* const scr = lds + wave * (32 * EPI_LD);
    const int e_row = lane >> 3, e_c4 = (lane & 7) * 4;
    float* const mbase = g.M + (size_t)j * g.Lm.xis + g.Lm.col(n0 + wn * 32) + e_c4 + (size_t)(m0 + wm * 32 + e_row) * g.Lm.bp;
#pragma unroll
    for (int a = 0; a < 6; ++a)
    {
#pragma unroll
        for (int r = 0; r < 16; ++r) scr[((r & 3) + 8 * (r >> 2) + 4 * half) * EPI_LD + l31] = acc[a][r];
        float* const mp = mbase + (size_t)(8 * a) * g.Lm.xis;
#pragma unroll
        for (int q = 0; q < 4; ++q)
        {
            const float4 v = *reinterpret_cast<const float4*>(&scr[(q * 8 + e_row) * EPI_LD + e_c4]);
            if constexpr ((NT & 2) != 0)
                stg4_nt(mp + (size_t)(q * 8) * g.Lm.bp, v);
            else
                *reinterpret_cast<float4*>(mp + (size_t)(q * 8) * g.Lm.bp) = v;
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// csrc/winograd_f63.hip's WinoChain and wino_chain_kernel, reading tmp[6][8] = the column-passed M: 48 loads per lane instead of 64 and no
// column pass; row pass, bias, ReLU, pooling, the LDS plane, B^T d B and the V' stores as there, in the same order.
struct ColChain
{
    int K, N;         // channels of the plane set (layer L's output = the consumer's input channels), images
    int TX, T;        // layer L's tiling (M columns p = n*T + ty*TX + tx)
    int AH, AW;       // activation the consumer sees: OH x OW, or OH/2 x OW/2 behind the fused pooling
    int TX2, T2;      // the consumer's tiling
    int planes;       // K * N, image index fastest
    int ppb;          // planes per block
    int LDW, LDH;     // LDS plane: (AH + 2 rows) x LDW floats, 2 border columns left, >= 2 right
    WinoLayout Lm, Lv2; // layer L's M48 (rows = K, 48 planes) and the consumer's V' (rows = K)
};

template <bool HAS_BIAS, bool RELU, bool POOL, bool MULTI>
__global__ __launch_bounds__(512, 3) void colpass_chain_kernel(float* __restrict__ Vn, const float* __restrict__ M, const float* __restrict__ bias,
                                                               const ColChain g, const int units)
{
    extern __shared__ __attribute__((aligned(16))) float smem[]; // [ppb][LDH][LDW]
    const int tid = threadIdx.x, nthreads = blockDim.x;
    const int plane_floats = g.LDH * g.LDW;
    // phase 1 writes rows 1 .. AH x the columns layer L's tiles cover and nothing else: the consumer's padding is zeroed once per block
    for (int i = tid; i < g.ppb * plane_floats; i += nthreads) smem[i] = 0.f;
    const int n1 = MULTI ? (g.T + nthreads - 1) / nthreads : 1;
    int pl = MULTI ? 0 : tid / g.T, t = tid - pl * g.T; // phase 1: layer L's tile (ty, tx) of plane pl of the unit
    bool lane_on = MULTI ? t < g.T : pl < g.ppb;
    int ty = t / g.TX, tx = t - ty * g.TX;
    const int pl2 = tid / g.T2, t2 = tid - pl2 * g.T2; // phase 2: the consumer's tile
    const bool lane_on2 = pl2 < g.ppb;
    const int ty2 = t2 / g.TX2, tx2 = t2 - ty2 * g.TX2;
    // unit order: as wino_chain_kernel (the XCD blockIdx % 8 owns a contiguous eighth of the units)
    const int xcd = blockIdx.x & 7, j = blockIdx.x >> 3, xcd_blocks = (gridDim.x + 7 - xcd) >> 3;
    const int u_lo = (int)((long long)units * xcd / 8), u_hi = (int)((long long)units * (xcd + 1) / 8);
    const size_t xi_stride = g.Lm.xis, xi_stride2 = g.Lv2.xis;
    float* const lp1 = smem + pl * plane_floats;

    float tmp[6][8];
    auto fetch = [&](int unit, int tile) {
        // clamped and unconditional (a load under a branch is waited for on the spot)
        const int plane = min(unit * g.ppb + (lane_on ? pl : 0), g.planes - 1);
        const int k = plane / g.N, n = plane - k * g.N;
        const float* mp = M + (size_t)k * g.Lm.bp + g.Lm.col(n * g.T + min(tile, g.T - 1));
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) tmp[a][jj] = mp[(size_t)(a * 8 + jj) * xi_stride];
    };
    int unit = u_lo + j;
    if (unit < u_hi) fetch(unit, t);
    __syncthreads();
    for (; unit < u_hi; unit += xcd_blocks)
    {
        const int plane = unit * g.ppb + pl;
        const int k = min(plane, g.planes - 1) / g.N;
        // ---- phase 1: layer L's tiles -> activation plane(s) in LDS
        for (int it = 0; it < n1; ++it)
        {
            if (MULTI)
            {
                t = tid + it * nthreads;
                lane_on = t < g.T;
                ty = t / g.TX;
                tx = t - ty * g.TX;
            }
            if (lane_on && plane < g.planes)
            {
                const float b = HAS_BIAS ? bias[k] : 0.f;
                float prev0 = 0.f, prev1 = 0.f, prev2 = 0.f;
#pragma unroll
                for (int a = 0; a < 6; ++a)
                {
                    float y[6];
                    at6(tmp[a][0], tmp[a][1], tmp[a][2], tmp[a][3], tmp[a][4], tmp[a][5], tmp[a][6], tmp[a][7], y[0], y[1], y[2], y[3], y[4], y[5]);
#pragma unroll
                    for (int bb = 0; bb < 6; ++bb)
                    {
                        float v = y[bb] + b;
                        if (RELU) v = fmaxf(v, 0.f);
                        y[bb] = v;
                    }
                    if (POOL)
                    {
                        // OH, OW even: a 2x2 cell never straddles the image edge; a whole cell is inside or outside
                        const float h0 = fmaxf(y[0], y[1]), h1 = fmaxf(y[2], y[3]), h2 = fmaxf(y[4], y[5]);
                        if ((a & 1) == 0)
                        {
                            prev0 = h0;
                            prev1 = h1;
                            prev2 = h2;
                        }
                        else
                        {
                            const int ay = 3 * ty + (a >> 1);
                            if (ay < g.AH)
                            {
                                float* row = lp1 + (size_t)(ay + 1) * g.LDW + 2 + 3 * tx;
                                row[0] = (3 * tx < g.AW) ? fmaxf(prev0, h0) : 0.f;
                                row[1] = (3 * tx + 1 < g.AW) ? fmaxf(prev1, h1) : 0.f;
                                row[2] = (3 * tx + 2 < g.AW) ? fmaxf(prev2, h2) : 0.f;
                            }
                        }
                        continue;
                    }
                    const int ay = 6 * ty + a;
                    if (ay < g.AH)
                    {
                        float* row = lp1 + (size_t)(ay + 1) * g.LDW + 2 + 6 * tx; // even offset: 8-byte aligned pairs
#pragma unroll
                        for (int bb = 0; bb < 6; bb += 2)
                        {
                            const float v0 = (6 * tx + bb < g.AW) ? y[bb] : 0.f, v1 = (6 * tx + bb + 1 < g.AW) ? y[bb + 1] : 0.f;
                            *reinterpret_cast<float2*>(row + bb) = make_float2(v0, v1);
                        }
                    }
                }
            }
            if (MULTI && it + 1 < n1) fetch(unit, tid + (it + 1) * nthreads);
        }
        __syncthreads();
        // ---- the next unit's tiles: in flight through phase 2
        if (unit + xcd_blocks < u_hi) fetch(unit + xcd_blocks, MULTI ? tid : t);
        __builtin_amdgcn_sched_barrier(0); // hipcc would sink the loads to their uses
        // ---- phase 2: the consumer's tiles: LDS rows 6ty .. 6ty+7, columns 6tx+1 .. 6tx+8
        const int plane2 = unit * g.ppb + pl2;
        if (lane_on2 && plane2 < g.planes)
        {
            const int k2 = plane2 / g.N, n2 = plane2 - k2 * g.N;
            const float* lp = smem + pl2 * plane_floats + (size_t)(6 * ty2) * g.LDW + 6 * tx2 + 1;
            float d[8][8];
#pragma unroll
            for (int i = 0; i < 8; ++i)
#pragma unroll
                for (int jj = 0; jj < 8; ++jj) d[i][jj] = lp[(size_t)i * g.LDW + jj];
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) bt8(d[0][jj], d[1][jj], d[2][jj], d[3][jj], d[4][jj], d[5][jj], d[6][jj], d[7][jj]);
#pragma unroll
            for (int i = 0; i < 8; ++i) bt8(d[i][0], d[i][1], d[i][2], d[i][3], d[i][4], d[i][5], d[i][6], d[i][7]);
            float* vp = Vn + (size_t)k2 * g.Lv2.bp + g.Lv2.col(n2 * g.T2 + t2);
#pragma unroll
            for (int i = 0; i < 8; ++i)
#pragma unroll
                for (int jj = 0; jj < 8; ++jj) vp[(size_t)(i * 8 + jj) * xi_stride2] = d[i][jj];
        }
        __syncthreads(); // the windows are read: the next phase 1 may overwrite the planes
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
static int device_limits(int* cus, size_t* lds)
{
    static thread_local int dev_cached = -1, cus_cached = 0;
    static thread_local size_t lds_cached = 0;
    int dev = 0;
    FHIP_CHECK_HIP(hipGetDevice(&dev));
    if (dev != dev_cached)
    {
        hipDeviceProp_t prop;
        FHIP_CHECK_HIP(hipGetDeviceProperties(&prop, dev));
        cus_cached = prop.multiProcessorCount;
        lds_cached = prop.maxSharedMemoryPerMultiProcessor;
        dev_cached = dev;
    }
    *cus = cus_cached;
    *lds = lds_cached;
    return FHIP_OK;
}

static bool k3s1(const fhip_conv_param& c) { return c.kernel_h == 3 && c.kernel_w == 3 && c.stride_h <= 1 && c.stride_w <= 1 && c.group <= 1; }

// the planes the main library runs on F(4x4,3x3) (csrc/winograd_f63.hip wino_f43): 7 and 8 output pixels per side
static bool f43_plane(const fhip_conv_param& p)
{
    const int oh = p.input_h + p.pad_top + p.pad_bottom - 2, ow = p.input_w + p.pad_left + p.pad_right - 2;
    if (oh < 1 || ow < 1 || oh > 8 || ow > 8 || (oh < 7 && ow < 7)) return false;
    return ((oh + 3) / 4) * ((ow + 3) / 4) * 36 < ((oh + 5) / 6) * ((ow + 5) / 6) * 64;
}

static int supported(const fhip_conv_param& p, int batch)
{
    if (batch < 1) return fail(FHIP_E_BADARG, "batch < 1");
    if (!k3s1(p)) return fail(FHIP_E_UNSUPPORTED, "the column-passed tile GEMM needs a 3x3 stride-1 group-1 convolution");
    const int hp = p.input_h + p.pad_top + p.pad_bottom, wp = p.input_w + p.pad_left + p.pad_right;
    if (hp < 3 || wp < 3) return fail(FHIP_E_BADARG, "input smaller than the kernel");
    if (f43_plane(p)) return fail(FHIP_E_UNSUPPORTED, "a plane of 7 or 8 pixels runs on F(4x4,3x3), which has no column-passed form");
    if (p.input_channels != 64) return fail(FHIP_E_UNSUPPORTED, "the column-passed tile GEMM holds the whole depth of a stage on chip: input_channels must be 64");
    if (p.output_channels < 64 || (p.output_channels & 63)) return fail(FHIP_E_UNSUPPORTED, "output_channels must be a multiple of 64 (the row tile)");
    const long long P = (long long)((wp + 3) / 6) * ((hp + 3) / 6) * batch;
    if (P > 0x7fffff00LL) return fail(FHIP_E_BADARG, "too many Winograd tiles for 32-bit column indices: N * tiles per image above 0x7fffff00");
    return FHIP_OK;
}

// is `pl` the F(6,3) plan of layer `p` at `batch` images?
static bool plan_is(const fhip_winograd_plan& pl, const fhip_conv_param& p, int batch)
{
    const int tx = (p.input_w + p.pad_left + p.pad_right + 3) / 6, ty = (p.input_h + p.pad_top + p.pad_bottom + 3) / 6;
    if (pl.frequency_points != 64 || pl.tiles_x != tx || pl.tiles_y != ty || pl.tiles_per_image != tx * ty) return false;
    if ((long long)pl.columns != (long long)tx * ty * batch || pl.columns_padded < pl.columns || (pl.columns_padded & 127)) return false;
    const int bp = pl.column_block;
    return bp == pl.columns_padded || (bp >= 128 && (bp & (bp - 1)) == 0 && pl.columns_padded % bp == 0);
}

static int tile_gemm(const fhip_conv_param& p, int batch, const fhip_winograd_plan& pl, float* m48, const float* u, const float* v, hipStream_t s)
{
    if (const int rc = supported(p, batch)) return rc;
    if (!plan_is(pl, p, batch) || pl.in_channels_padded != 64 || pl.out_channels_padded < p.output_channels || (pl.out_channels_padded & 63))
        return fail(FHIP_E_BADARG, "the plan does not belong to this layer and batch (fhip_winograd_f63_plan)");
    if (!aligned(m48, 16) || !aligned(u, 16) || !aligned(v, 16)) return fail(FHIP_E_BADARG, "m48, u and v must be 16-byte aligned");
    constexpr int WN = COLPASS_WN, BK = COLPASS_BK, NBUF = COLPASS_NBUF, BN = 32 * WN;
    ColGemm g;
    g.U = u;
    g.V = v;
    g.M = m48;
    g.Kp = pl.out_channels_padded;
    g.m_tiles = p.output_channels / 64;
    g.n_tiles = (pl.columns + BN - 1) / BN; // Pp is a multiple of the column tile: no pure-padding tiles, every tile inside one column block
    g.Lv = wino_layout(64, pl.columns_padded, pl.column_block, 64);
    g.Lm = wino_layout(p.output_channels, pl.columns_padded, pl.column_block, 48);
    const long long blocks = 8LL * g.m_tiles * g.n_tiles;
    if (blocks > 0x7fffffffLL) return fail(FHIP_E_BADARG, "2^31 blocks or more");
    const bool big_m = (size_t)64 * p.output_channels * pl.columns_padded * sizeof(float) >= kBigM;
    const dim3 grid((unsigned)blocks), threads(128 * WN);
    // V with `nt` only while one row tile covers all of K: with more, every V element is read by m_tiles blocks and must stay cached
    if (g.m_tiles == 1 && big_m) hipLaunchKernelGGL((colpass_gemm_kernel<WN, BK, NBUF, 3>), grid, threads, 0, s, g);
    else if (g.m_tiles == 1) hipLaunchKernelGGL((colpass_gemm_kernel<WN, BK, NBUF, 1>), grid, threads, 0, s, g);
    else if (big_m) hipLaunchKernelGGL((colpass_gemm_kernel<WN, BK, NBUF, 2>), grid, threads, 0, s, g);
    else hipLaunchKernelGGL((colpass_gemm_kernel<WN, BK, NBUF, 0>), grid, threads, 0, s, g);
    FHIP_CHECK_HIP(hipGetLastError());
    return FHIP_OK;
}

static int chain(const fhip_conv_param& p, const fhip_conv_param& next, int batch, const fhip_winograd_plan& pl, const fhip_winograd_plan& pn,
                 float* vn, const float* m48, const float* bias, int pool, hipStream_t s)
{
    if (const int rc = supported(p, batch)) return rc;
    if (!k3s1(next) || next.pad_left != 1 || next.pad_right != 1 || next.pad_top != 1 || next.pad_bottom != 1 ||
        next.input_channels != p.output_channels || f43_plane(next))
        return fail(FHIP_E_UNSUPPORTED, "the consumer must be a 3x3 / stride-1 / pad-1 F(6x6,3x3) layer on this layer's output channels");
    if (pool && ((p.output_h & 1) || (p.output_w & 1))) return fail(FHIP_E_UNSUPPORTED, "fused max pooling needs even output dims");
    const int ah = pool ? p.output_h / 2 : p.output_h, aw = pool ? p.output_w / 2 : p.output_w;
    if (next.input_h != ah || next.input_w != aw) return fail(FHIP_E_UNSUPPORTED, "the consumer's input is not this layer's (pooled) output");
    if (p.activation != FHIP_ACT_NONE && p.activation != FHIP_ACT_RELU) return fail(FHIP_E_UNSUPPORTED, "activation other than none / ReLU");
    if (!plan_is(pl, p, batch) || !plan_is(pn, next, batch))
        return fail(FHIP_E_BADARG, "the plans do not belong to these layers and this batch (fhip_winograd_f63_plan)");
    if (p.output_h != p.input_h + p.pad_top + p.pad_bottom - 2 || p.output_w != p.input_w + p.pad_left + p.pad_right - 2)
        return fail(FHIP_E_BADARG, "output dims are not those of the geometry (fhip_conv_assign_output_dim)");
    const bool has_bias = p.bias_term != 0, relu = p.activation == FHIP_ACT_RELU;
    if (has_bias && !bias) return fail(FHIP_E_BADARG, "bias_term set but bias is NULL");
    ColChain g;
    g.K = p.output_channels;
    g.N = batch;
    g.TX = pl.tiles_x;
    g.T = pl.tiles_per_image;
    g.AH = ah;
    g.AW = aw;
    g.TX2 = pn.tiles_x;
    g.T2 = pn.tiles_per_image;
    g.Lm = wino_layout(g.K, pl.columns_padded, pl.column_block, 48);
    g.Lv2 = wino_layout(g.K, pn.columns_padded, pn.column_block, 64);
    const long long planes = (long long)batch * g.K;
    if (planes > 0x7fffffffLL) return fail(FHIP_E_BADARG, "N*K too large: 2^31 planes or more");
    g.planes = (int)planes;
    g.LDH = 6 * pn.tiles_y + 2;
    g.LDW = 6 * pn.tiles_x + 4;
    const size_t plane_bytes = (size_t)g.LDH * g.LDW * sizeof(float);
    if (plane_bytes > 64 * 1024) return fail(FHIP_E_UNSUPPORTED, "the consumer's plane does not fit a block's LDS");
    // one tile per lane, as many planes per block as 256 lanes and 48 KB of LDS take (wino_chain_kernel's rule)
    const int work = std::max(g.T, g.T2);
    int ppb = std::max(1, 256 / work);
    ppb = (int)std::min<size_t>(ppb, std::max<size_t>(1, (48 * 1024) / plane_bytes));
    g.ppb = (int)std::min<long long>(ppb, planes);
    const bool multi = work > 512;
    if (multi && !pool) return fail(FHIP_E_UNSUPPORTED, "an unpooled plane of more than 512 tiles");
    const unsigned threads = std::max(256u, (unsigned)((multi ? g.T2 : work) + 63) / 64 * 64);
    if (threads > 512u) return fail(FHIP_E_UNSUPPORTED, "the consumer's plane has more than 512 tiles");
    const size_t lds = plane_bytes * g.ppb;
    const long long units = (planes + g.ppb - 1) / g.ppb;
    int cus;
    size_t dev_lds;
    if (const int rc = device_limits(&cus, &dev_lds)) return rc;
    const int bpc = std::max(1, std::min((int)(dev_lds / lds), 12 / (int)(threads / 64)));
    const unsigned grid = ((unsigned)std::min<long long>(units, (long long)cus * bpc) + 7u) & ~7u;
#define FHIP_COLPASS_CHAIN(P_, M_)                                                                                                              \
    do                                                                                                                                          \
    {                                                                                                                                           \
        if (has_bias && relu) hipLaunchKernelGGL((colpass_chain_kernel<true, true, P_, M_>), dim3(grid), dim3(threads), lds, s, vn, m48, bias, g, (int)units); \
        else if (has_bias) hipLaunchKernelGGL((colpass_chain_kernel<true, false, P_, M_>), dim3(grid), dim3(threads), lds, s, vn, m48, bias, g, (int)units);   \
        else if (relu) hipLaunchKernelGGL((colpass_chain_kernel<false, true, P_, M_>), dim3(grid), dim3(threads), lds, s, vn, m48, bias, g, (int)units);       \
        else hipLaunchKernelGGL((colpass_chain_kernel<false, false, P_, M_>), dim3(grid), dim3(threads), lds, s, vn, m48, bias, g, (int)units);                \
    } while (0)
    if (pool && multi) FHIP_COLPASS_CHAIN(true, true);
    else if (pool) FHIP_COLPASS_CHAIN(true, false);
    else FHIP_COLPASS_CHAIN(false, false);
#undef FHIP_COLPASS_CHAIN
    FHIP_CHECK_HIP(hipGetLastError());
    return FHIP_OK;
}

} // namespace fhip

extern "C"
{

int fhip_colpass_supported(const fhip_conv_param* param, int batch)
{
    if (!param) return fhip::fail(FHIP_E_BADARG, "bad argument");
    return fhip::supported(*param, batch);
}

int fhip_colpass_tile_gemm(const fhip_conv_param* param, int batch, const fhip_winograd_plan* plan, float* m48, const float* u, const float* v,
                           void* stream)
{
    if (!param || !plan || !m48 || !u || !v) return fhip::fail(FHIP_E_BADARG, "bad argument");
    return fhip::tile_gemm(*param, batch, *plan, m48, u, v, (hipStream_t)stream);
}

int fhip_colpass_output_to_next_input(const fhip_conv_param* param, const fhip_conv_param* next, int batch, const fhip_winograd_plan* plan,
                                      const fhip_winograd_plan* plan_next, float* v_next, const float* m48, const float* bias, int pool, void* stream)
{
    if (!param || !next || !plan || !plan_next || !v_next || !m48) return fhip::fail(FHIP_E_BADARG, "bad argument");
    return fhip::chain(*param, *next, batch, *plan, *plan_next, v_next, m48, bias, pool, (hipStream_t)stream);
}

const char* fhip_colpass_last_error(void) { return fhip::last_error(); }

} // extern "C"
