// q8.hip -- libfeather_q8.so: int8 convolution whose input, output or both are q8 tensors (include/feather_hip/feather_q8.h is the
// definition), and the layers that live between two such convolutions.  A library of its own: the kernel sets of libfeather_hip.so and
// libfeather_qconv.so are closed.  The arithmetic rules are those of libfeather_qconv.so, from the one header both include (int8_rules.h).
//
// The q8 tensor is signed char [n][CB][h][w][16]: the 16 channels of one pixel of one channel block are one 16-byte access.
// One selection function (select()):
// 1. q8_mfma_kernel<WM, WN, IN8, OUT8> (group 1): the implicit GEMM of qconv.hip on v_mfma_i32_16x16x64_i8 -- a block of four waves owns
//    32 * WM output channels x 64 pixel columns and walks the reduction in chunks of 64 rows -- with the reduction laid out tap-major over
//    the channels PADDED to 16 (Cp = 16 * CB), so a run of 16 reduction rows is one (tap, channel block) and, with an int8 input, one 16-byte
//    global load per lane that goes to LDS as it is: the loader has no arithmetic at all.  The packer zeroes the weights of the pad channels,
//    so any C runs and the pad bytes of the input never matter.  With an fp32 input (IN8 = false, C % 16 == 0) the loader is qconv.hip's:
//    16 strided floats, quantised and packed.  The epilogue dequantises as feather_qconv.h says and either stores fp32 NCHW or quantises
//    again (OUT8): the C/D map gives a lane four consecutive output channels of one pixel, which is one dword of the q8 tensor.  Rows from K
//    up to 16 * ceil(K / 16) are stored as 0 (the pad bytes), rows past that are not stored.
// 2. q8_dw_kernel<OUT8>: int8 in, group == C == K, any kernel size and stride.  A lane owns one output pixel of one channel block: per tap
//    one 16-byte load of the input and one (block-uniform) 16-byte load of the weights, 16 int32 sums.
// 3. q8_generic_kernel<DW>: fp32 in, int8 out, everything else (the C = 3 first layer of a net; an fp32-fed depthwise layer): one output
//    pixel and the 16 output channels of one block per lane, quantising in the loader, one 16-byte store.
// And q8_quantize_kernel / q8_dequantize_kernel (fp32 NCHW <-> q8), q8_relu_kernel, q8_max_pool_kernel, and the three packers.
// All stores are plain C++ vector stores.
#include <hip/hip_runtime.h>
#include <cmath>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "feather_hip/feather_q8.h"
#include "direct_conv.h"
#include "int8_rules.h"

namespace fhip
{

typedef int i32x4 __attribute__((ext_vector_type(4)));

// four quantised values (each in [-127, 127]) to a dword, value e in byte e
__device__ __forceinline__ int pack4(int q0, int q1, int q2, int q3)
{
    return (int)((unsigned)(q0 & 0xff) | (unsigned)(q1 & 0xff) << 8 | (unsigned)(q2 & 0xff) << 16 | (unsigned)(q3 & 0xff) << 24);
}

// ---- fp32 NCHW <-> q8, ReLU, max pooling: lane i of [n][CB][pixel], 16 bytes each --------------------------------------------------
__global__ __launch_bounds__(256) void q8_quantize_kernel(i32x4* out, const float* in, int C, int CB, int HW, float s, unsigned total)
{
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= total) return;
    const unsigned pix = i % (unsigned)HW, t = i / (unsigned)HW;
    const int cb = (int)(t % (unsigned)CB), n = (int)(t / (unsigned)CB);
    const int c0 = cb * 16;
    const float* src = in + ((size_t)n * C + c0) * HW + pix;
    i32x4 v;
#pragma unroll
    for (int j = 0; j < 4; ++j)
    {
        int q[4];
#pragma unroll
        for (int e = 0; e < 4; ++e)
        {
            const int c = 4 * j + e;
            q[e] = c0 + c < C ? quantise(src[(size_t)c * HW], s) : 0;
        }
        v[j] = pack4(q[0], q[1], q[2], q[3]);
    }
    out[i] = v;
}

__global__ __launch_bounds__(256) void q8_dequantize_kernel(float* out, const i32x4* in, int C, int CB, int HW, float s, unsigned total)
{
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= total) return;
    const unsigned pix = i % (unsigned)HW, t = i / (unsigned)HW;
    const int cb = (int)(t % (unsigned)CB), n = (int)(t / (unsigned)CB);
    const int c0 = cb * 16;
    float* dst = out + ((size_t)n * C + c0) * HW + pix;
    const i32x4 v = in[i];
#pragma unroll
    for (int c = 0; c < 16; ++c)
        if (c0 + c < C) dst[(size_t)c * HW] = __fdiv_rn((float)byte_of(v[c >> 2], c & 3), s);
}

__global__ __launch_bounds__(256) void q8_relu_kernel(i32x4* out, const i32x4* in, unsigned total)
{
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= total) return;
    const i32x4 v = in[i];
    i32x4 r;
#pragma unroll
    for (int j = 0; j < 4; ++j)
    {
        const unsigned w = (unsigned)v[j];
        r[j] = (int)(w & ~(((w >> 7) & 0x01010101u) * 0xffu)); // a byte whose sign bit is set becomes 0
    }
    out[i] = r;
}

struct Q8PoolArgs
{
    int C, CB, H, W, OH, OW, KH, KW, SH, SW, off_y, off_x;
    unsigned total; // batch * CB * OH * OW
};

__global__ __launch_bounds__(256) void q8_max_pool_kernel(i32x4* out, const i32x4* in, const Q8PoolArgs q)
{
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= q.total) return;
    const int ox = (int)(i % (unsigned)q.OW);
    unsigned t = i / (unsigned)q.OW;
    const int oy = (int)(t % (unsigned)q.OH);
    t /= (unsigned)q.OH; // n * CB + cb
    const int cb = (int)(t % (unsigned)q.CB);
    const i32x4* xp = in + (size_t)t * q.H * q.W;
    const int y0 = oy * q.SH - q.off_y, x0 = ox * q.SW - q.off_x;
    const int ya = max(y0, 0), yb = min(y0 + q.KH, q.H);
    const int xa = max(x0, 0), xb = min(x0 + q.KW, q.W);
    int m[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) m[c] = -127;
    for (int yy = ya; yy < yb; ++yy)
        for (int xx = xa; xx < xb; ++xx)
        {
            const i32x4 v = xp[(size_t)yy * q.W + xx];
#pragma unroll
            for (int c = 0; c < 16; ++c) m[c] = max(m[c], byte_of(v[c >> 2], c & 3));
        }
    i32x4 r;
#pragma unroll
    for (int j = 0; j < 4; ++j)
    {
        int e[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) e[k] = cb * 16 + 4 * j + k < q.C ? m[4 * j + k] : 0; // the pad bytes stay 0, also under an empty window
        r[j] = pack4(e[0], e[1], e[2], e[3]);
    }
    out[i] = r;
}

// ---- the direct routes ---------------------------------------------------------------------------------------------------------------
struct Q8DirectArgs
{
    const void* x;  // dw: q8 tensor; generic: float NCHW
    const i32x4* w; // dw and generic<true>: [CB][taps] x 16 bytes (channel c & 15 of block c >> 4); generic<false>: [KB][C][taps] x 16 bytes (output channel)
    const float* d;
    const float* bias;
    void* y;
    float s_in, s_out;
    int C, K, CB, KB, H, W, Ho, Wo, kh, kw, sh, sw, pt, pl;
    int relu;
    unsigned total; // lanes: batch * Ho * Wo; blockIdx.y = channel block of the output
};

// the epilogue of one lane's 16 sums of block `kb`: one 16-byte store into the q8 tensor [n][KB][Ho][Wo][16]
__device__ __forceinline__ void store_q8_block(const Q8DirectArgs& a, const int* acc, int kb, unsigned pixel_of_image, int n)
{
    i32x4 r;
#pragma unroll
    for (int j = 0; j < 4; ++j)
    {
        int q[4];
#pragma unroll
        for (int e = 0; e < 4; ++e)
        {
            const int k = kb * 16 + 4 * j + e;
            q[e] = k < a.K ? quantise(dequantise(acc[4 * j + e], a.d[min(k, a.K - 1)], a.bias, min(k, a.K - 1), a.relu), a.s_out) : 0;
        }
        r[j] = pack4(q[0], q[1], q[2], q[3]);
    }
    reinterpret_cast<i32x4*>(a.y)[((size_t)n * a.KB + kb) * ((size_t)a.Ho * a.Wo) + pixel_of_image] = r;
}

template <bool OUT8>
__global__ __launch_bounds__(256) void q8_dw_kernel(const Q8DirectArgs a)
{
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= a.total) return;
    const int cb = blockIdx.y;
    const unsigned HoWo = (unsigned)a.Ho * (unsigned)a.Wo;
    const unsigned pix = i % HoWo;
    const int n = (int)(i / HoWo);
    const int oy = (int)(pix / (unsigned)a.Wo), ox = (int)(pix - (unsigned)oy * (unsigned)a.Wo);
    const i32x4* xp = reinterpret_cast<const i32x4*>(a.x) + ((size_t)n * a.CB + cb) * ((size_t)a.H * a.W);
    const i32x4* __restrict__ wp = a.w + (size_t)cb * a.kh * a.kw; // uniform over the block
    const int iy0 = oy * a.sh - a.pt, ix0 = ox * a.sw - a.pl;

    int acc[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) acc[c] = 0;
    for (int r = 0; r < a.kh; ++r)
    {
        const int iy = iy0 + r;
        const bool row_in = iy >= 0 && iy < a.H;
        const i32x4* row = xp + (size_t)min(max(iy, 0), a.H - 1) * a.W; // always a row of the plane
        for (int s = 0; s < a.kw; ++s, ++wp)
        {
            const int ix = ix0 + s;
            i32x4 v = row[min(max(ix, 0), a.W - 1)];
            if (!row_in || ix < 0 || ix >= a.W) v = i32x4{0, 0, 0, 0};
            const i32x4 w = *wp;
#pragma unroll
            for (int c = 0; c < 16; ++c) acc[c] += byte_of(v[c >> 2], c & 3) * byte_of(w[c >> 2], c & 3);
        }
    }
    if constexpr (OUT8)
        store_q8_block(a, acc, cb, pix, n);
    else
    {
        float* yp = reinterpret_cast<float*>(a.y) + ((size_t)n * a.K + (size_t)cb * 16) * HoWo + pix;
#pragma unroll
        for (int c = 0; c < 16; ++c)
        {
            const int k = cb * 16 + c;
            if (k < a.K) yp[(size_t)c * HoWo] = dequantise(acc[c], a.d[k], a.bias, k, a.relu);
        }
    }
}

template <bool DW>
__global__ __launch_bounds__(256) void q8_generic_kernel(const Q8DirectArgs a)
{
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= a.total) return;
    const int kb = blockIdx.y;
    const unsigned HoWo = (unsigned)a.Ho * (unsigned)a.Wo;
    const unsigned pix = i % HoWo;
    const int n = (int)(i / HoWo);
    const int oy = (int)(pix / (unsigned)a.Wo), ox = (int)(pix - (unsigned)oy * (unsigned)a.Wo);
    const size_t plane = (size_t)a.H * a.W;
    const float* xp = reinterpret_cast<const float*>(a.x) + (size_t)n * a.C * plane;
    const int ntaps = a.kh * a.kw;
    const int iy0 = oy * a.sh - a.pt, ix0 = ox * a.sw - a.pl;

    int acc[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) acc[c] = 0;
    if constexpr (DW)
    {
        const i32x4* __restrict__ wp = a.w + (size_t)kb * ntaps; // uniform over the block
        for (int r = 0; r < a.kh; ++r)
        {
            const int iy = iy0 + r;
            const bool row_in = iy >= 0 && iy < a.H;
            const size_t row = (size_t)min(max(iy, 0), a.H - 1) * a.W;
            for (int s = 0; s < a.kw; ++s, ++wp)
            {
                const int ix = ix0 + s;
                const bool in = row_in && ix >= 0 && ix < a.W;
                const size_t at = row + min(max(ix, 0), a.W - 1);
                const i32x4 w = *wp;
#pragma unroll
                for (int c = 0; c < 16; ++c)
                {
                    const int ch = min(kb * 16 + c, a.C - 1); // a pad channel reads the last plane and meets a zero weight
                    const int q = quantise(xp[(size_t)ch * plane + at], a.s_in);
                    acc[c] += (in ? q : 0) * byte_of(w[c >> 2], c & 3);
                }
            }
        }
    }
    else
    {
        const i32x4* __restrict__ wp = a.w + (size_t)kb * a.C * ntaps; // uniform over the block
        for (int c = 0; c < a.C; ++c, xp += plane)
            for (int r = 0; r < a.kh; ++r)
            {
                const int iy = iy0 + r;
                const bool row_in = iy >= 0 && iy < a.H;
                const float* row = xp + (size_t)min(max(iy, 0), a.H - 1) * a.W; // always a row of the plane
                for (int s = 0; s < a.kw; ++s, ++wp)
                {
                    const int ix = ix0 + s;
                    int q = quantise(row[min(max(ix, 0), a.W - 1)], a.s_in);
                    if (!row_in || ix < 0 || ix >= a.W) q = 0;
                    const i32x4 w = *wp;
#pragma unroll
                    for (int k = 0; k < 16; ++k) acc[k] += q * byte_of(w[k >> 2], k & 3);
                }
            }
    }
    store_q8_block(a, acc, kb, pix, n);
}

// kernel [C][taps] int8 -> packed [CB][taps][16]: byte c & 15 = channel c (0 past C); dword i = ((cb * taps + tap) * 4 + j)
__global__ __launch_bounds__(256) void q8_pack_dw_kernel(int* packed, const signed char* kernel, int C, int taps, unsigned total)
{
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= total) return;
    const int j = (int)(i & 3u);
    const unsigned t = i >> 2;
    const int tap = (int)(t % (unsigned)taps), cb = (int)(t / (unsigned)taps);
    int q[4];
#pragma unroll
    for (int e = 0; e < 4; ++e)
    {
        const int c = cb * 16 + 4 * j + e;
        q[e] = c < C ? kernel[(size_t)c * taps + tap] : 0;
    }
    packed[i] = pack4(q[0], q[1], q[2], q[3]);
}

// kernel [K][C][taps] int8 -> packed [KB][C][taps][16]: byte k & 15 = output channel k (0 past K); dword i = (((kb * C + c) * taps + tap) * 4 + j)
__global__ __launch_bounds__(256) void q8_pack_generic_kernel(int* packed, const signed char* kernel, int C, int K, int taps, unsigned total)
{
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= total) return;
    const int j = (int)(i & 3u);
    unsigned t = i >> 2;
    const int tap = (int)(t % (unsigned)taps);
    t /= (unsigned)taps;
    const int c = (int)(t % (unsigned)C), kb = (int)(t / (unsigned)C);
    int q[4];
#pragma unroll
    for (int e = 0; e < 4; ++e)
    {
        const int k = kb * 16 + 4 * j + e;
        q[e] = k < K ? kernel[((size_t)k * C + c) * taps + tap] : 0;
    }
    packed[i] = pack4(q[0], q[1], q[2], q[3]);
}

// ---- the MFMA route ------------------------------------------------------------------------------------------------------------------
constexpr int kQBN = 64;        // pixel columns per block
constexpr int kQBK = 64;        // reduction rows per chunk: the K of v_mfma_i32_16x16x64_i8
constexpr int kQRowPad = 128;   // the packed weights hold a multiple of 128 output-channel rows, whatever the block shape
constexpr int kQLdsStride = 80; // bytes of an LDS row (one pixel's 64 reduction bytes + 16: 16-byte reads of adjacent pixels spread over the banks)

struct Q8GemmArgs
{
    const void* in;
    const i32x4* wq; // [K padded to 128 / 16][chunks][64 lanes] fragments of 16 bytes
    const float* d;
    const float* bias;
    void* out;
    float s_in, s_out;
    int C, CB, K, KB, H, W, Ho, Wo, kh, kw, sh, sw, pt, pl;
    int HW, HoWo, Ntot, runs, chunks, m_tiles, n_tiles, relu;
};

// WM x WN waves; a wave owns 32 output channels (two 16-row tiles) and 64 / WN pixel columns
template <int WM, int WN, bool IN8, bool OUT8>
__global__ __launch_bounds__(256) void q8_mfma_kernel(const Q8GemmArgs p)
{
    static_assert(WM * WN == 4, "four waves");
    static_assert(IN8 || OUT8, "fp32 in and out is libfeather_qconv.so's kernel");
    constexpr int NT = kQBN / WN / 16; // 16-column tiles per wave
    __shared__ __attribute__((aligned(16))) unsigned char lds[kQBN * kQLdsStride];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int vid = xcd_remap((int)blockIdx.x, p.m_tiles * p.n_tiles);
    const int mt = vid % p.m_tiles, nt = vid / p.m_tiles;
    const int wm = wave % WM, wn = wave / WM;

    // loader: lane = pixel column of the block, wave = run of 16 reduction rows of the chunk = one (tap, channel block)
    const int col = nt * kQBN + lane;
    const bool col_ok = col < p.Ntot;
    const int cc = col_ok ? col : 0;
    const int img = cc / p.HoWo, rem = cc - img * p.HoWo;
    const int oy = rem / p.Wo, ox = rem - oy * p.Wo;
    const int y0 = oy * p.sh - p.pt, x0 = ox * p.sw - p.pl;
    const int last_run = p.runs - 1; // runs past the reduction meet zero weights: any address of the tensor will do

    float raw[IN8 ? 1 : 16];
    i32x4 rawq = i32x4{0, 0, 0, 0};
    bool raw_ok;
    auto fetch = [&](int chunk) {
        const int run = min(chunk * 4 + wave, last_run);
        const int tap = run / p.CB, cb = run - tap * p.CB;
        const int i = tap / p.kw, j = tap - i * p.kw;
        const int iy = y0 + i, ix = x0 + j;
        raw_ok = col_ok && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W;
        const int at = min(max(iy, 0), p.H - 1) * p.W + min(max(ix, 0), p.W - 1);
        if constexpr (IN8)
            rawq = reinterpret_cast<const i32x4*>(p.in)[((size_t)img * p.CB + cb) * p.HW + at];
        else
        {
            const float* src = reinterpret_cast<const float*>(p.in) + ((size_t)img * p.C + (size_t)cb * 16) * p.HW + at;
#pragma unroll
            for (int e = 0; e < 16; ++e) raw[e] = src[(size_t)e * p.HW];
        }
    };

    i32x4 acc[2][NT];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < NT; ++b) acc[a][b] = i32x4{0, 0, 0, 0};

    // A fragments of this wave's two row tiles: fragment (tile, chunk, lane)
    const i32x4* wa = p.wq + ((size_t)(mt * (WM * 2) + wm * 2) * p.chunks) * 64 + lane;
    const size_t tile_step = (size_t)p.chunks * 64;

    fetch(0);
    for (int chunk = 0; chunk < p.chunks; ++chunk)
    {
        i32x4 packed4;
        if constexpr (IN8)
            packed4 = raw_ok ? rawq : i32x4{0, 0, 0, 0};
        else
        {
#pragma unroll
            for (int e4 = 0; e4 < 4; ++e4)
            {
                int q[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) q[e] = raw_ok ? quantise(raw[e4 * 4 + e], p.s_in) : 0;
                packed4[e4] = pack4(q[0], q[1], q[2], q[3]);
            }
        }
        *reinterpret_cast<i32x4*>(lds + lane * kQLdsStride + wave * 16) = packed4;
        __syncthreads();
        if (chunk + 1 < p.chunks) fetch(chunk + 1);

        const i32x4 a0 = wa[(size_t)chunk * 64], a1 = wa[tile_step + (size_t)chunk * 64];
#pragma unroll
        for (int b = 0; b < NT; ++b)
        {
            const int n = wn * (kQBN / WN) + b * 16 + (lane & 15);
            const i32x4 bf = *reinterpret_cast<const i32x4*>(lds + n * kQLdsStride + (lane >> 4) * 16);
            acc[0][b] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a0, bf, acc[0][b], 0, 0, 0);
            acc[1][b] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a1, bf, acc[1][b], 0, 0, 0);
        }
        __syncthreads();
    }

    // C/D map of the 16x16 forms: column = lane & 15, row = 4 * (lane >> 4) + register
#pragma unroll
    for (int b = 0; b < NT; ++b)
    {
        const int ocol = nt * kQBN + wn * (kQBN / WN) + b * 16 + (lane & 15);
        if (ocol >= p.Ntot) continue;
        const int oimg = ocol / p.HoWo, orem = ocol - oimg * p.HoWo;
#pragma unroll
        for (int a = 0; a < 2; ++a)
        {
            const int m0 = mt * (32 * WM) + wm * 32 + a * 16 + (lane >> 4) * 4; // four consecutive output channels of one channel block
            if constexpr (OUT8)
            {
                if (m0 >= p.KB * 16) continue;
                int q[4];
#pragma unroll
                for (int e = 0; e < 4; ++e)
                {
                    const int m = min(m0 + e, p.K - 1);
                    q[e] = m0 + e < p.K ? quantise(dequantise(acc[a][b][e], p.d[m], p.bias, m, p.relu), p.s_out) : 0;
                }
                int* obase = reinterpret_cast<int*>(p.out) + (((size_t)oimg * p.KB + (m0 >> 4)) * p.HoWo + orem) * 4 + ((m0 & 15) >> 2);
                *obase = pack4(q[0], q[1], q[2], q[3]);
            }
            else
            {
                float* obase = reinterpret_cast<float*>(p.out) + (size_t)oimg * p.K * p.HoWo + orem;
#pragma unroll
                for (int e = 0; e < 4; ++e)
                {
                    const int m = m0 + e;
                    if (m < p.K) obase[(size_t)m * p.HoWo] = dequantise(acc[a][b][e], p.d[m], p.bias, m, p.relu);
                }
            }
        }
    }
}

// kernel [K][C][taps] int8 -> fragment order: dword i = (tile16, chunk, lane, dword4); byte e of it is reduction row
// chunk * 64 + 16 * (lane >> 4) + dword4 * 4 + e = tap * Cp + c (Cp = C padded to 16) of output channel tile16 * 16 + (lane & 15); zero past
// K, past C inside a tap, and past the reduction
__global__ __launch_bounds__(256) void q8_pack_mfma_kernel(int* packed, const signed char* kernel, int C, int Cp, int K, int taps, int chunks, unsigned total)
{
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= total) return;
    const int d4 = (int)(i & 3u), lane = (int)((i >> 2) & 63u);
    const unsigned t = i >> 8;
    const int chunk = (int)(t % (unsigned)chunks), tile = (int)(t / (unsigned)chunks);
    const int m = tile * 16 + (lane & 15);
    const int R = taps * Cp;
    int q[4];
#pragma unroll
    for (int e = 0; e < 4; ++e)
    {
        const int r = chunk * kQBK + 16 * (lane >> 4) + d4 * 4 + e;
        const int tap = r / Cp, c = r - tap * Cp;
        q[e] = (m < K && r < R && c < C) ? kernel[((size_t)m * C + c) * taps + tap] : 0;
    }
    packed[i] = pack4(q[0], q[1], q[2], q[3]);
}

// ---- host side -------------------------------------------------------------------------------------------------------------------------

static int blocks16(int c) { return (c + 15) / 16; }

// bytes of a q8 tensor, or 0 when that is 2^31 or more
static size_t q8_bytes(long long batch, long long c, long long h, long long w)
{
    const long long cb = (c + 15) / 16;
    if (h > 0x7fffffffLL / w) return 0;
    const long long hw = h * w;
    if (batch * cb > 0x7fffffffLL / 16 / hw) return 0;
    const long long bytes = batch * cb * hw * 16;
    return bytes > 0x7fffffffLL ? 0 : (size_t)bytes;
}

static int check_geometry(const fhip_q8_param* p)
{
    const int rc = check_sizes(p);
    if (rc) return rc;
    if (p->dilation_h != 1 || p->dilation_w != 1) return fail(FHIP_E_BADARG, "dilation must be 1: a dilated int8 convolution is not supported");
    if (p->pad_left < 0 || p->pad_right < 0 || p->pad_top < 0 || p->pad_bottom < 0) return fail(FHIP_E_BADARG, "negative padding");
    if (p->group < 1) return fail(FHIP_E_BADARG, "group must be >= 1");
    if (p->group != 1 && (p->group != p->input_channels || p->group != p->output_channels))
        return fail(FHIP_E_BADARG, "partial group: group must be 1 or equal to both channel counts (depthwise)");
    if (p->int8_scale_term > 200) return fail(FHIP_E_BADARG, "int8_scale_term > 200");
    if (p->int8_scale_term < 0) return fail(FHIP_E_BADARG, "int8_scale_term must not be negative");
    if (p->activation != FHIP_ACT_NONE && p->activation != FHIP_ACT_RELU) return fail(FHIP_E_BADARG, "activation must be None or ReLU");
    if ((p->input_int8 != 0 && p->input_int8 != 1) || (p->output_int8 != 0 && p->output_int8 != 1)) return fail(FHIP_E_BADARG, "input_int8 / output_int8 must be 0 or 1");
    if (!p->input_int8 && !p->output_int8) return fail(FHIP_E_BADARG, "fp32 in and fp32 out: that layer is libfeather_qconv.so's");
    const long long R = (long long)(p->input_channels / p->group) * p->kernel_h * p->kernel_w;
    if (R > 133144) return fail(FHIP_E_BADARG, "reduction too long: more than 133144 products could overflow the int32 sum");
    if (p->kernel_h > (long long)p->input_h + p->pad_top + p->pad_bottom || p->kernel_w > (long long)p->input_w + p->pad_left + p->pad_right)
        return fail(FHIP_E_BADARG, "the kernel is larger than the padded input");
    const long long oh = ((long long)p->input_h + p->pad_top + p->pad_bottom - p->kernel_h) / p->stride_h + 1;
    const long long ow = ((long long)p->input_w + p->pad_left + p->pad_right - p->kernel_w) / p->stride_w + 1;
    const auto too_large = [](long long c, long long h, long long w) { return h > 0x7fffffffLL || w > 0x7fffffffLL || h * w > 0x7fffffffLL || c * (h * w) > 0x7fffffffLL; };
    if (too_large(p->input_channels, p->input_h, p->input_w) || too_large(p->output_channels, oh, ow))
        return fail(FHIP_E_BADARG, "tensor too large: 2^31 elements or more");
    if ((p->input_int8 && !q8_bytes(1, p->input_channels, p->input_h, p->input_w)) || (p->output_int8 && !q8_bytes(1, p->output_channels, oh, ow)))
        return fail(FHIP_E_BADARG, "q8 tensor too large: 2^31 bytes or more");
    return FHIP_OK;
}

static int check_param(const fhip_q8_param* p)
{
    const int rc = check_geometry(p);
    if (rc) return rc;
    if (p->output_h != ((long long)p->input_h + p->pad_top + p->pad_bottom - p->kernel_h) / p->stride_h + 1 ||
        p->output_w != ((long long)p->input_w + p->pad_left + p->pad_right - p->kernel_w) / p->stride_w + 1)
        return fail(FHIP_E_BADARG, "output_h / output_w are not what fhip_q8_assign_output_dim gives");
    return FHIP_OK;
}

// routes: the MFMA kernel as (block shape, input, output), then the direct kernels
enum RouteKind
{
    ROUTE_MFMA_128_II, // 4 x 1 waves, int8 in, int8 out
    ROUTE_MFMA_128_IF, // int8 in, fp32 out
    ROUTE_MFMA_128_FI, // fp32 in, int8 out
    ROUTE_MFMA_64_II,  // 2 x 2 waves
    ROUTE_MFMA_64_IF,
    ROUTE_MFMA_64_FI,
    ROUTE_DW_F, // int8 in, fp32 out
    ROUTE_DW_I, // int8 in, int8 out
    ROUTE_GENERIC,    // fp32 in, int8 out, group 1
    ROUTE_GENERIC_DW, // fp32 in, int8 out, depthwise
    ROUTE_COUNT
};

static bool is_mfma(int r) { return r <= ROUTE_MFMA_64_FI; }
static bool is_dw(int r) { return r == ROUTE_DW_F || r == ROUTE_DW_I; }
static bool route_in8(int r) { return is_mfma(r) ? r % 3 != 2 : is_dw(r); }
static bool route_out8(int r) { return is_mfma(r) ? r % 3 != 1 : r != ROUTE_DW_F; }

static bool accepts(const fhip_q8_param& p, int r)
{
    if ((p.input_int8 != 0) != route_in8(r) || (p.output_int8 != 0) != route_out8(r)) return false;
    if (is_mfma(r)) return p.group == 1 && (p.input_int8 || p.input_channels % 16 == 0);
    if (is_dw(r) || r == ROUTE_GENERIC_DW) return p.group > 1;
    return p.group == 1;
}

// The one selection function: fhip_q8_forward launches what it says, fhip_q8_route reports it, init packs for it.
static int select(const fhip_q8_param& p)
{
    const int io = p.input_int8 ? (p.output_int8 ? 0 : 1) : 2;
    if (p.group > 1) return p.input_int8 ? (p.output_int8 ? ROUTE_DW_I : ROUTE_DW_F) : ROUTE_GENERIC_DW;
    if (p.input_int8 || p.input_channels % 16 == 0) return (p.output_channels > 64 ? ROUTE_MFMA_128_II : ROUTE_MFMA_64_II) + io;
    return ROUTE_GENERIC;
}

static const char* route_name(int r)
{
    switch (r)
    {
    case ROUTE_MFMA_128_II: return "fhip::q8_mfma_kernel<4, 1, true, true>";
    case ROUTE_MFMA_128_IF: return "fhip::q8_mfma_kernel<4, 1, true, false>";
    case ROUTE_MFMA_128_FI: return "fhip::q8_mfma_kernel<4, 1, false, true>";
    case ROUTE_MFMA_64_II: return "fhip::q8_mfma_kernel<2, 2, true, true>";
    case ROUTE_MFMA_64_IF: return "fhip::q8_mfma_kernel<2, 2, true, false>";
    case ROUTE_MFMA_64_FI: return "fhip::q8_mfma_kernel<2, 2, false, true>";
    case ROUTE_DW_F: return "fhip::q8_dw_kernel<false>";
    case ROUTE_DW_I: return "fhip::q8_dw_kernel<true>";
    case ROUTE_GENERIC: return "fhip::q8_generic_kernel<false>";
    default: return "fhip::q8_generic_kernel<true>";
    }
}

static int route_by_name(const char* name)
{
    if (!name) return -1;
    for (int r = 0; r < ROUTE_COUNT; ++r)
        if (!strcmp(name, route_name(r))) return r;
    return -1;
}

static int mfma_chunks(const fhip_q8_param& p) { return (blocks16(p.input_channels) * 16 * p.kernel_h * p.kernel_w + kQBK - 1) / kQBK; }

static size_t packed_bytes_of(const fhip_q8_param& p, int r)
{
    const size_t taps = (size_t)p.kernel_h * p.kernel_w;
    if (is_dw(r) || r == ROUTE_GENERIC_DW) return (size_t)blocks16(p.input_channels) * taps * 16;
    if (r == ROUTE_GENERIC) return (size_t)blocks16(p.output_channels) * p.input_channels * taps * 16;
    return (size_t)((p.output_channels + kQRowPad - 1) / kQRowPad) * kQRowPad * mfma_chunks(p) * kQBK;
}

static int route_checks(const fhip_q8_param* param, const char* route, int& r)
{
    const int rc = check_param(param);
    if (rc) return rc;
    r = route ? route_by_name(route) : select(*param);
    if (r < 0) return fail(FHIP_E_BADARG, "unknown route name");
    if (!accepts(*param, r)) return fail(FHIP_E_UNSUPPORTED, "the named route cannot run this layer");
    return FHIP_OK;
}

static int do_buffer_size(const fhip_q8_param* param, int batch, const char* route, size_t* scratch_bytes, size_t* packed_bytes)
{
    int r;
    const int rc = route_checks(param, route, r);
    if (rc) return rc;
    if (batch < 1 || !scratch_bytes || !packed_bytes) return fail(FHIP_E_BADARG, "batch < 1 or a null size pointer");
    *scratch_bytes = 0;
    *packed_bytes = packed_bytes_of(*param, r);
    return FHIP_OK;
}

static int do_init(const fhip_q8_param* param, void* packed, const signed char* kernel, void* stream, const char* route)
{
    int r;
    const int rc = route_checks(param, route, r);
    if (rc) return rc;
    if (!packed || !kernel) return fail(FHIP_E_BADARG, "null packed / kernel");
    if (!aligned(packed, 16)) return fail(FHIP_E_BADARG, "packed must be 16-byte aligned");
    const fhip_q8_param& p = *param;
    const size_t bytes = packed_bytes_of(p, r);
    if (bytes > 0x7fffffffULL) return fail(FHIP_E_BADARG, "filter tensor too large: 2^31 packed bytes or more");
    const unsigned total = (unsigned)(bytes / 4); // every layout is whole dwords, one lane each
    const dim3 grid((total + 255) / 256);
    const int taps = p.kernel_h * p.kernel_w;
    hipStream_t s = (hipStream_t)stream;
    if (is_dw(r) || r == ROUTE_GENERIC_DW)
        hipLaunchKernelGGL(q8_pack_dw_kernel, grid, dim3(256), 0, s, (int*)packed, kernel, p.input_channels, taps, total);
    else if (r == ROUTE_GENERIC)
        hipLaunchKernelGGL(q8_pack_generic_kernel, grid, dim3(256), 0, s, (int*)packed, kernel, p.input_channels, p.output_channels, taps, total);
    else
        hipLaunchKernelGGL(q8_pack_mfma_kernel, grid, dim3(256), 0, s, (int*)packed, kernel, p.input_channels, blocks16(p.input_channels) * 16, p.output_channels,
                           taps, mfma_chunks(p), total);
    FHIP_CHECK_HIP(hipGetLastError());
    return FHIP_OK;
}

static int do_forward(const fhip_q8_param* param, int batch, void* out, const void* in, const void* packed, const float* d, const float* bias, float s_in,
                      float s_out, void* stream, const char* route)
{
    int r;
    int rc = route_checks(param, route, r);
    if (rc) return rc;
    const fhip_q8_param& p = *param;
    if (batch < 1) return fail(FHIP_E_BADARG, "batch < 1");
    if (!out || !in || !packed || !d) return fail(FHIP_E_BADARG, "null out / in / packed / d");
    if (p.bias_term && !bias) return fail(FHIP_E_BADARG, "bias_term is set and bias is NULL");
    if (!aligned(out, p.output_int8 ? 16 : 4) || !aligned(in, p.input_int8 ? 16 : 4) || !aligned(packed, 16) || !aligned(d, 4) || (p.bias_term && !aligned(bias, 4)))
        return fail(FHIP_E_BADARG, "device pointers must be 4-byte aligned (packed and q8 tensors: 16-byte)");
    if (!p.input_int8 && !good_input_scale(s_in)) return fail(FHIP_E_BADARG, "s_in must be finite and > 0");
    if (p.output_int8 && !good_input_scale(s_out)) return fail(FHIP_E_BADARG, "s_out must be finite and > 0");
    const unsigned long long in_count = (unsigned long long)batch * p.input_channels * p.input_h * p.input_w;
    const unsigned long long out_count = (unsigned long long)batch * p.output_channels * p.output_h * p.output_w;
    if (in_count > 0x7fffffffULL || out_count > 0x7fffffffULL) return fail(FHIP_E_BADARG, "tensor too large: 2^31 elements or more");
    if ((p.input_int8 && !q8_bytes(batch, p.input_channels, p.input_h, p.input_w)) || (p.output_int8 && !q8_bytes(batch, p.output_channels, p.output_h, p.output_w)))
        return fail(FHIP_E_BADARG, "q8 tensor too large: 2^31 bytes or more");
    hipStream_t s = (hipStream_t)stream;
    const float* b = p.bias_term ? bias : nullptr;
    const int relu = p.activation == FHIP_ACT_RELU;
    if (!is_mfma(r))
    {
        Q8DirectArgs a;
        a.x = in, a.w = (const i32x4*)packed, a.d = d, a.bias = b, a.y = out, a.s_in = s_in, a.s_out = s_out;
        a.C = p.input_channels, a.K = p.output_channels, a.CB = blocks16(a.C), a.KB = blocks16(a.K);
        a.H = p.input_h, a.W = p.input_w, a.Ho = p.output_h, a.Wo = p.output_w, a.kh = p.kernel_h, a.kw = p.kernel_w;
        a.sh = p.stride_h, a.sw = p.stride_w, a.pt = p.pad_top, a.pl = p.pad_left, a.relu = relu;
        const size_t total = (size_t)batch * p.output_h * p.output_w;
        if (total > 0x7fffffffULL || a.KB > 65535) return fail(FHIP_E_BADARG, "more than 65535 blocks of 16 output channels");
        a.total = (unsigned)total;
        const dim3 grid((unsigned)((total + 255) / 256), (unsigned)a.KB);
        if (r == ROUTE_DW_F)
            hipLaunchKernelGGL(q8_dw_kernel<false>, grid, dim3(256), 0, s, a);
        else if (r == ROUTE_DW_I)
            hipLaunchKernelGGL(q8_dw_kernel<true>, grid, dim3(256), 0, s, a);
        else if (r == ROUTE_GENERIC)
            hipLaunchKernelGGL(q8_generic_kernel<false>, grid, dim3(256), 0, s, a);
        else
            hipLaunchKernelGGL(q8_generic_kernel<true>, grid, dim3(256), 0, s, a);
    }
    else
    {
        Q8GemmArgs g;
        g.in = in, g.wq = (const i32x4*)packed, g.d = d, g.bias = b, g.out = out, g.s_in = s_in, g.s_out = s_out;
        g.C = p.input_channels, g.CB = blocks16(g.C), g.K = p.output_channels, g.KB = blocks16(g.K);
        g.H = p.input_h, g.W = p.input_w, g.Ho = p.output_h, g.Wo = p.output_w;
        g.kh = p.kernel_h, g.kw = p.kernel_w, g.sh = p.stride_h, g.sw = p.stride_w, g.pt = p.pad_top, g.pl = p.pad_left;
        g.HW = g.H * g.W;
        g.HoWo = g.Ho * g.Wo;
        const unsigned long long ntot = (unsigned long long)batch * g.HoWo;
        if (ntot > 0x3fffffffULL) return fail(FHIP_E_BADARG, "tensor too large: 2^30 GEMM columns or more");
        g.Ntot = (int)ntot;
        g.runs = g.CB * g.kh * g.kw;
        g.chunks = mfma_chunks(p);
        const bool big = r < ROUTE_MFMA_64_II;
        const int bm = big ? 128 : 64;
        g.m_tiles = (g.K + bm - 1) / bm;
        g.n_tiles = (g.Ntot + kQBN - 1) / kQBN;
        g.relu = relu;
        const unsigned long long blocks = (unsigned long long)g.m_tiles * g.n_tiles;
        if (blocks > 0x7fffffffULL) return fail(FHIP_E_BADARG, "tensor too large: 2^31 blocks or more");
        const dim3 grid((unsigned)blocks);
        switch (r)
        {
        case ROUTE_MFMA_128_II: hipLaunchKernelGGL((q8_mfma_kernel<4, 1, true, true>), grid, dim3(256), 0, s, g); break;
        case ROUTE_MFMA_128_IF: hipLaunchKernelGGL((q8_mfma_kernel<4, 1, true, false>), grid, dim3(256), 0, s, g); break;
        case ROUTE_MFMA_128_FI: hipLaunchKernelGGL((q8_mfma_kernel<4, 1, false, true>), grid, dim3(256), 0, s, g); break;
        case ROUTE_MFMA_64_II: hipLaunchKernelGGL((q8_mfma_kernel<2, 2, true, true>), grid, dim3(256), 0, s, g); break;
        case ROUTE_MFMA_64_IF: hipLaunchKernelGGL((q8_mfma_kernel<2, 2, true, false>), grid, dim3(256), 0, s, g); break;
        default: hipLaunchKernelGGL((q8_mfma_kernel<2, 2, false, true>), grid, dim3(256), 0, s, g); break;
        }
    }
    FHIP_CHECK_HIP(hipGetLastError());
    return FHIP_OK;
}

// the checks the four tensor calls share; -> lanes (16 bytes each) in `lanes`
static int check_tensor(const void* out, const void* in, int batch, int channels, int h, int w, bool out_q8, unsigned& lanes)
{
    if (!out || !in) return fail(FHIP_E_BADARG, "null out / in");
    if (batch < 1 || channels < 1 || h < 1 || w < 1) return fail(FHIP_E_BADARG, "batch, channels and sizes must be >= 1");
    if (!aligned(out, out_q8 ? 16 : 4) || !aligned(in, out_q8 ? 4 : 16)) return fail(FHIP_E_BADARG, "the q8 tensor must be 16-byte aligned, the fp32 tensor 4-byte");
    const size_t bytes = q8_bytes(batch, channels, h, w);
    if (!bytes) return fail(FHIP_E_BADARG, "q8 tensor too large: 2^31 bytes or more");
    if ((unsigned long long)batch * channels * h * w > 0x7fffffffULL) return fail(FHIP_E_BADARG, "tensor too large: 2^31 elements or more");
    lanes = (unsigned)(bytes / 16);
    return FHIP_OK;
}

} // namespace fhip

using namespace fhip;

extern "C"
{

int fhip_q8_tensor_bytes(int batch, int channels, int h, int w, size_t* bytes)
{
    if (!bytes) return fail(FHIP_E_BADARG, "null bytes");
    if (batch < 1 || channels < 1 || h < 1 || w < 1) return fail(FHIP_E_BADARG, "batch, channels and sizes must be >= 1");
    const size_t b = q8_bytes(batch, channels, h, w);
    if (!b) return fail(FHIP_E_BADARG, "q8 tensor too large: 2^31 bytes or more");
    *bytes = b;
    return FHIP_OK;
}

int fhip_q8_assign_output_dim(fhip_q8_param* param)
{
    if (!param) return fail(FHIP_E_BADARG, "null param");
    if (param->input_h < 1 || param->input_w < 1 || param->stride_h < 1 || param->stride_w < 1 || param->kernel_h < 1 || param->kernel_w < 1)
        return fail(FHIP_E_BADARG, "input size, kernel size and stride must be >= 1");
    const long long nh = (long long)param->input_h + param->pad_top + param->pad_bottom - param->kernel_h;
    const long long nw = (long long)param->input_w + param->pad_left + param->pad_right - param->kernel_w;
    if (nh < 0 || nw < 0) return fail(FHIP_E_BADARG, "the kernel is larger than the padded input");
    const long long oh = nh / param->stride_h + 1, ow = nw / param->stride_w + 1;
    if (oh > 0x7fffffffLL || ow > 0x7fffffffLL) return fail(FHIP_E_BADARG, "absurdly large output: 2^31 or more per side");
    param->output_h = (int)oh;
    param->output_w = (int)ow;
    return FHIP_OK;
}

int fhip_q8_supported(const fhip_q8_param* param) { return check_param(param) == FHIP_OK ? 1 : 0; }

int fhip_q8_get_buffer_size(const fhip_q8_param* param, int batch, size_t* scratch_bytes, size_t* packed_bytes)
{
    return do_buffer_size(param, batch, nullptr, scratch_bytes, packed_bytes);
}

int fhip_q8_init(const fhip_q8_param* param, void* packed, const signed char* kernel, void* stream) { return do_init(param, packed, kernel, stream, nullptr); }

int fhip_q8_dequant_scales(float* d, const float* s_w, int K, float s_in) { return int8_dequant_scales(d, s_w, K, s_in); }

int fhip_q8_forward(const fhip_q8_param* param, int batch, void* out, const void* in, const void* packed, void* /*scratch*/, const float* d, const float* bias,
                    float s_in, float s_out, void* stream)
{
    return do_forward(param, batch, out, in, packed, d, bias, s_in, s_out, stream, nullptr);
}

int fhip_q8_route(const fhip_q8_param* param, char* name, int len)
{
    const int rc = check_param(param);
    if (rc) return rc;
    if (!name || len < 1) return fail(FHIP_E_BADARG, "null name");
    snprintf(name, (size_t)len, "%s", route_name(select(*param)));
    return FHIP_OK;
}

int fhip_q8_get_buffer_size_route(const fhip_q8_param* param, int batch, const char* route, size_t* scratch_bytes, size_t* packed_bytes)
{
    if (!route) return fail(FHIP_E_BADARG, "null route name");
    return do_buffer_size(param, batch, route, scratch_bytes, packed_bytes);
}

int fhip_q8_init_route(const fhip_q8_param* param, void* packed, const signed char* kernel, void* stream, const char* route)
{
    if (!route) return fail(FHIP_E_BADARG, "null route name");
    return do_init(param, packed, kernel, stream, route);
}

int fhip_q8_forward_route(const fhip_q8_param* param, int batch, void* out, const void* in, const void* packed, void* /*scratch*/, const float* d,
                          const float* bias, float s_in, float s_out, void* stream, const char* route)
{
    if (!route) return fail(FHIP_E_BADARG, "null route name");
    return do_forward(param, batch, out, in, packed, d, bias, s_in, s_out, stream, route);
}

int fhip_q8_quantize_forward(void* out, const float* in, int batch, int channels, int h, int w, float s, void* stream)
{
    unsigned lanes;
    const int rc = check_tensor(out, in, batch, channels, h, w, true, lanes);
    if (rc) return rc;
    if (!good_input_scale(s)) return fail(FHIP_E_BADARG, "the scale must be finite and > 0");
    hipLaunchKernelGGL(q8_quantize_kernel, dim3((lanes + 255) / 256), dim3(256), 0, (hipStream_t)stream, (i32x4*)out, in, channels, blocks16(channels), h * w, s, lanes);
    FHIP_CHECK_HIP(hipGetLastError());
    return FHIP_OK;
}

int fhip_q8_dequantize_forward(float* out, const void* in, int batch, int channels, int h, int w, float s, void* stream)
{
    unsigned lanes;
    const int rc = check_tensor(out, in, batch, channels, h, w, false, lanes);
    if (rc) return rc;
    if (!good_input_scale(s)) return fail(FHIP_E_BADARG, "the scale must be finite and > 0");
    hipLaunchKernelGGL(q8_dequantize_kernel, dim3((lanes + 255) / 256), dim3(256), 0, (hipStream_t)stream, out, (const i32x4*)in, channels, blocks16(channels), h * w, s,
                       lanes);
    FHIP_CHECK_HIP(hipGetLastError());
    return FHIP_OK;
}

int fhip_q8_relu_forward(void* out, const void* in, size_t bytes, void* stream)
{
    if (!out || !in) return fail(FHIP_E_BADARG, "null out / in");
    if (bytes < 16 || bytes % 16 || bytes > 0x7fffffffULL) return fail(FHIP_E_BADARG, "bytes must be a multiple of 16 in [16, 2^31)");
    if (!aligned(out, 16) || !aligned(in, 16)) return fail(FHIP_E_BADARG, "a q8 tensor must be 16-byte aligned");
    const unsigned lanes = (unsigned)(bytes / 16);
    hipLaunchKernelGGL(q8_relu_kernel, dim3((lanes + 255) / 256), dim3(256), 0, (hipStream_t)stream, (i32x4*)out, (const i32x4*)in, lanes);
    FHIP_CHECK_HIP(hipGetLastError());
    return FHIP_OK;
}

int fhip_q8_max_pool_forward(const fhip_pool_param* p, int batch, void* out, const void* in, void* stream)
{
    if (!p || !out || !in) return fail(FHIP_E_BADARG, "null param / out / in");
    if (batch < 1 || p->channels < 1 || p->input_h < 1 || p->input_w < 1) return fail(FHIP_E_BADARG, "batch, channels and input size must be >= 1");
    if (p->pooling_type != 0) return fail(FHIP_E_BADARG, "only max pooling runs on a q8 tensor");
    if (!aligned(out, 16) || !aligned(in, 16)) return fail(FHIP_E_BADARG, "a q8 tensor must be 16-byte aligned");
    Q8PoolArgs q;
    q.C = p->channels, q.CB = blocks16(p->channels), q.H = p->input_h, q.W = p->input_w;
    if (p->global_pooling)
        q.OH = q.OW = 1, q.KH = q.H, q.KW = q.W, q.SH = q.SW = 1;
    else
    {
        if (p->stride_h < 1 || p->stride_w < 1 || p->kernel_h < 1 || p->kernel_w < 1) return fail(FHIP_E_BADARG, "kernel size and stride must be >= 1");
        // ceil, as fhip_pooling_output_dim
        q.OH = (int)ceilf((float)(p->input_h + p->pad_top + p->pad_bottom - p->kernel_h) / p->stride_h) + 1;
        q.OW = (int)ceilf((float)(p->input_w + p->pad_left + p->pad_right - p->kernel_w) / p->stride_w) + 1;
        q.KH = p->kernel_h, q.KW = p->kernel_w, q.SH = p->stride_h, q.SW = p->stride_w;
    }
    if (q.OH < 1 || q.OW < 1) return fail(FHIP_E_BADARG, "empty pooling output");
    q.off_y = p->pad_top + p->pad_bottom;
    q.off_x = p->pad_left + p->pad_right;
    const size_t in_bytes = q8_bytes(batch, p->channels, q.H, q.W), out_bytes = q8_bytes(batch, p->channels, q.OH, q.OW);
    if (!in_bytes || !out_bytes) return fail(FHIP_E_BADARG, "q8 tensor too large: 2^31 bytes or more");
    q.total = (unsigned)(out_bytes / 16);
    hipLaunchKernelGGL(q8_max_pool_kernel, dim3((q.total + 255) / 256), dim3(256), 0, (hipStream_t)stream, (i32x4*)out, (const i32x4*)in, q);
    FHIP_CHECK_HIP(hipGetLastError());
    return FHIP_OK;
}

const char* fhip_q8_last_error(void) { return last_error(); }

} // extern "C"
