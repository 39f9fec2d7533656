// qconv.hip -- libfeather_qconv.so: int8 convolution, fp32 in and out (include/feather_hip/feather_qconv.h is the definition).  A
// library of its own: the main library's kernel set is closed, and the other libraries keep theirs.
//
// Every route quantises the activations in its LOADER (quantise() below: one multiply, roundf, clamp, NaN select) and accumulates exact
// int32 sums; an int8 copy of the activations never exists in memory.  One selection function (select()):
// 1. qconv_mfma_kernel<WM, WN> (group 1, C a multiple of 16): the implicit GEMM
//        acc[K x N * Ho * Wo] = Wq[K x taps * C] * gather(q),   gather(q)[(i, j, c)][(n, oy, ox)] = q[n][c][oy * sh - pt + i][ox * sw - pl + j]
//    on v_mfma_i32_16x16x64_i8.  The reduction is tap-major with the channels innermost, so a run of 16 reduction rows lies inside one tap.
//    A block of four waves owns 32 * WM output channels x 64 pixel columns and walks the reduction in chunks of 64 rows: wave g of the
//    block loads, for each of the 64 pixels (one per lane: adjacent lanes, adjacent addresses), the 16 channels of run g of the chunk,
//    quantises them, packs them four to a dword and writes 16 bytes to LDS; after the barrier every wave reads its B fragments (16 bytes
//    per lane) from LDS and its A fragments (16 bytes per lane, contiguous per wave) straight from the packed weights, which the packer
//    has laid out in fragment order.  The integer sum is order-free, so the only thing the code relies on about the instruction's k map
//    is that byte j of lane group l >> 4 of A meets byte j of lane group l >> 4 of B; both sides use k = 16 * (l >> 4) + j.
//    The next chunk's global loads are issued before the current chunk's MFMAs.  R is padded to 64 with zero weights; rows past K and
//    columns past N * Ho * Wo are masked at the store.
// 2. qconv_dw3x3_kernel<S>: group == C == K, 3x3, stride S in both directions.  A lane produces four adjacent outputs of a row and
//    quantises the 3 + 3 * S input columns of each of its three rows once; the lanes are dealt out over [plane][row][strip] as one flat
//    index, so a 7-pixel plane fills its blocks like a 112-pixel one (a lane reads its channel's nine taps as three cached dwords).
// 3. qconv_generic_kernel<KT>: everything else (few channels, C % 16 != 0, other depthwise kernels): one output pixel and KT output
//    channels per lane, the int8 weights of a tap four to a (scalar) dword.  KT = 16 from 16 output channels per group on: a quantised
//    input value then serves 16 multiply-adds instead of 4 (the C = 3 first layers of VGG-16 and ResNet-50); KT = 4 below.
// All stores are plain C++ vector stores.
#include <hip/hip_runtime.h>
#include <cmath>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "feather_hip/feather_qconv.h"
#include "direct_conv.h"
#include "int8_rules.h"

namespace fhip
{

typedef int i32x4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256) void quantize_kernel(signed char* out, const float* in, unsigned count, float s_in)
{
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i < count) out[i] = (signed char)quantise(in[i], s_in);
}

// What the direct kernels need, by value.
struct QDirectArgs
{
    const float* x;
    const int* w; // generic: [group * chunks][Cg][taps][KT / 4] dwords of 4 int8 (zero past Kg); depthwise: [C][3] dwords = 9 int8 + 3 zero bytes
    const float* d;
    const float* bias;
    float* y;
    float s_in;
    int C, K, Cg, Kg, H, W, Ho, Wo, kh, kw, sh, sw, pt, pl;
    int chunks; // chunks of KT output channels per group
    int strips; // depthwise: lanes per output row, ceil(Wo / 4)
    int relu;
    unsigned total; // lanes: batch * Ho * Wo (depthwise: batch * C * Ho * strips)
};

// ---- the generic route: y[n][g * Kg + chunk * KT .. + KT)[oy][ox]; lane i of [batch][Ho][Wo], blockIdx.y = (group, chunk) ------------
template <int KT>
__global__ __launch_bounds__(256) void qconv_generic_kernel(const QDirectArgs a)
{
    static_assert(KT % 4 == 0, "four int8 weights to a dword");
    constexpr int W4 = KT / 4;
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= a.total) return;
    const int gc = blockIdx.y;
    const int g = gc / a.chunks, chunk = gc - g * a.chunks;
    const int ox = (int)(i % (unsigned)a.Wo);
    const unsigned t = i / (unsigned)a.Wo;
    const int oy = (int)(t % (unsigned)a.Ho), n = (int)(t / (unsigned)a.Ho);
    const int ntaps = a.kh * a.kw;
    const size_t plane = (size_t)a.H * a.W;
    const float* xp = a.x + ((size_t)n * a.C + (size_t)g * a.Cg) * plane;
    const int* __restrict__ wp = a.w + (size_t)gc * a.Cg * ntaps * W4; // uniform over the block
    const int iy0 = oy * a.sh - a.pt, ix0 = ox * a.sw - a.pl;

    int acc[KT];
#pragma unroll
    for (int k = 0; k < KT; ++k) acc[k] = 0;
    for (int c = 0; c < a.Cg; ++c, xp += plane)
        for (int r = 0; r < a.kh; ++r)
        {
            const int iy = iy0 + r;
            const bool row_in = iy >= 0 && iy < a.H;
            const float* row = xp + (size_t)min(max(iy, 0), a.H - 1) * a.W; // always a row of the plane
            for (int s = 0; s < a.kw; ++s, wp += W4)
            {
                const int ix = ix0 + s;
                int q = quantise(row[min(max(ix, 0), a.W - 1)], a.s_in);
                if (!row_in || ix < 0 || ix >= a.W) q = 0;
#pragma unroll
                for (int j = 0; j < W4; ++j)
                {
                    const int w4 = wp[j];
#pragma unroll
                    for (int k = 0; k < 4; ++k) acc[4 * j + k] += q * byte_of(w4, k);
                }
            }
        }

    const int kk0 = chunk * KT;
    const size_t oplane = (size_t)a.Ho * a.Wo;
    float* yp = a.y + (((size_t)n * a.K + (size_t)g * a.Kg + kk0) * a.Ho + oy) * a.Wo + ox;
#pragma unroll
    for (int k = 0; k < KT; ++k)
        if (kk0 + k < a.Kg)
        {
            const int ch = g * a.Kg + kk0 + k;
            yp[k * oplane] = dequantise(acc[k], a.d[ch], a.bias, ch, a.relu);
        }
}

// kernel [K][Cg][taps] int8 -> packed [group][chunk][Cg][taps][kt / 4] dwords, byte k of dword j = output channel chunk * kt + 4 * j + k
// (0 past Kg)
__global__ __launch_bounds__(256) void qconv_pack_generic_kernel(int* packed, const signed char* kernel, int Cg, int Kg, int taps, int kt, int chunks, unsigned total)
{
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= total) return;
    const int w4s = kt / 4;
    const int j = (int)(i % (unsigned)w4s);
    unsigned t = i / (unsigned)w4s;
    const int tap = (int)(t % (unsigned)taps);
    t /= (unsigned)taps;
    const int c = (int)(t % (unsigned)Cg);
    const int gc = (int)(t / (unsigned)Cg);
    const int g = gc / chunks, kk0 = (gc - g * chunks) * kt + 4 * j;
    unsigned w4 = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (kk0 + k < Kg) w4 |= (unsigned)(unsigned char)kernel[(((size_t)g * Kg + kk0 + k) * Cg + c) * taps + tap] << (8 * k);
    packed[i] = (int)w4;
}

// ---- the depthwise route: y[n][c][oy][4 * strip .. + 4) of a 3x3 depthwise layer with stride S; lane i of [batch * C][Ho][strips] ------
template <int S>
__global__ __launch_bounds__(256) void qconv_dw3x3_kernel(const QDirectArgs a)
{
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= a.total) return;
    const int sx = (int)(i % (unsigned)a.strips);
    const unsigned t = i / (unsigned)a.strips;
    const int oy = (int)(t % (unsigned)a.Ho);
    const unsigned pc = t / (unsigned)a.Ho; // plane: image * C + channel
    const int c = (int)(pc % (unsigned)a.C);
    const int ox = sx * 4;
    const float* xp = a.x + (size_t)pc * a.H * a.W;
    const int* __restrict__ wp = a.w + (size_t)c * 3;
    const int w0 = wp[0], w1 = wp[1], w2 = wp[2];
    const int iy0 = oy * S - a.pt, ix0 = ox * S - a.pl;

    int acc[4] = {0, 0, 0, 0};
#pragma unroll
    for (int r = 0; r < 3; ++r)
    {
        const int iy = iy0 + r;
        const bool row_in = iy >= 0 && iy < a.H;
        const float* row = xp + (size_t)min(max(iy, 0), a.H - 1) * a.W; // always a row of the plane
        // the 3 + 3 * S input columns the four outputs see, quantised once
        int q[3 + 3 * S];
#pragma unroll
        for (int e = 0; e < 3 + 3 * S; ++e)
        {
            const int ix = ix0 + e;
            const int v = quantise(row[min(max(ix, 0), a.W - 1)], a.s_in);
            q[e] = (row_in && ix >= 0 && ix < a.W) ? v : 0;
        }
#pragma unroll
        for (int s = 0; s < 3; ++s)
        {
            const int tap = r * 3 + s;
            const int wv = byte_of(tap < 4 ? w0 : tap < 8 ? w1 : w2, tap & 3);
#pragma unroll
            for (int p = 0; p < 4; ++p) acc[p] += wv * q[p * S + s];
        }
    }
    float* yp = a.y + ((size_t)pc * a.Ho + oy) * a.Wo + ox;
    const float dk = a.d[c];
#pragma unroll
    for (int p = 0; p < 4; ++p)
        if (ox + p < a.Wo) yp[p] = dequantise(acc[p], dk, a.bias, c, a.relu);
}

// kernel [C][9] int8 -> packed [C][3] dwords (taps 0..3, 4..7, 8 and three zero bytes)
__global__ __launch_bounds__(256) void qconv_pack_dw_kernel(int* packed, const signed char* kernel, unsigned total)
{
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= total) return;
    const unsigned c = i / 3u, part = i - c * 3u;
    unsigned w4 = 0;
    for (unsigned k = 0; k < 4; ++k)
        if (part * 4 + k < 9) w4 |= (unsigned)(unsigned char)kernel[(size_t)c * 9 + part * 4 + k] << (8 * k);
    packed[i] = (int)w4;
}

// ---- the MFMA route -------------------------------------------------------------------------------------------------
constexpr int kQBN = 64;         // pixel columns per block
constexpr int kQBK = 64;         // reduction rows per chunk: the K of v_mfma_i32_16x16x64_i8
constexpr int kQRowPad = 128;    // the packed weights hold a multiple of 128 output-channel rows, whatever the block shape
constexpr int kQLdsStride = 80;  // bytes of an LDS row (one pixel's 64 reduction bytes + 16: 16-byte reads of adjacent pixels spread over the banks)

struct QGemmArgs
{
    const float* in;
    const i32x4* wq; // [K padded to 128 / 16][chunks][64 lanes] fragments of 16 bytes
    const float* d;
    const float* bias;
    float* out;
    float s_in;
    int C, K, H, W, Ho, Wo, kh, kw, sh, sw, pt, pl;
    int HW, HoWo, Ntot, R, chunks, m_tiles, n_tiles, relu;
};

// WM x WN waves; a wave owns 32 output channels (two 16-row tiles) and 64 / WN pixel columns
template <int WM, int WN>
__global__ __launch_bounds__(256) void qconv_mfma_kernel(const QGemmArgs p)
{
    static_assert(WM * WN == 4, "four waves");
    constexpr int NT = kQBN / WN / 16; // 16-column tiles per wave
    __shared__ __attribute__((aligned(16))) unsigned char lds[kQBN * kQLdsStride];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int vid = xcd_remap((int)blockIdx.x, p.m_tiles * p.n_tiles);
    const int mt = vid % p.m_tiles, nt = vid / p.m_tiles;
    const int wm = wave % WM, wn = wave / WM;

    // loader: lane = pixel column of the block, wave = run of 16 reduction rows of the chunk
    const int col = nt * kQBN + lane;
    const bool col_ok = col < p.Ntot;
    const int cc = col_ok ? col : 0;
    const int img = cc / p.HoWo, rem = cc - img * p.HoWo;
    const int oy = rem / p.Wo, ox = rem - oy * p.Wo;
    const int y0 = oy * p.sh - p.pt, x0 = ox * p.sw - p.pl;
    const float* xin = p.in + (size_t)img * p.C * p.HW;
    const int last_run = p.R / 16 - 1; // runs past R meet zero weights: any address of the tensor will do

    float raw[16];
    bool raw_ok;
    auto fetch = [&](int chunk) {
        const int run = min(chunk * 4 + wave, last_run);
        const int r0 = run * 16;
        const int tap = r0 / p.C, c0 = r0 - tap * p.C;
        const int i = tap / p.kw, j = tap - i * p.kw;
        const int iy = y0 + i, ix = x0 + j;
        raw_ok = col_ok && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W;
        const float* src = xin + (size_t)c0 * p.HW + min(max(iy, 0), p.H - 1) * p.W + min(max(ix, 0), p.W - 1);
#pragma unroll
        for (int e = 0; e < 16; ++e) raw[e] = src[(size_t)e * p.HW];
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
#pragma unroll
        for (int e4 = 0; e4 < 4; ++e4)
        {
            unsigned w = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e)
            {
                const int q = raw_ok ? quantise(raw[e4 * 4 + e], p.s_in) : 0;
                w |= (unsigned)(q & 0xff) << (8 * e);
            }
            packed4[e4] = (int)w;
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
        float* obase = p.out + (size_t)oimg * p.K * p.HoWo + orem;
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int e = 0; e < 4; ++e)
            {
                const int m = mt * (32 * WM) + wm * 32 + a * 16 + (lane >> 4) * 4 + e;
                if (m < p.K) obase[(size_t)m * p.HoWo] = dequantise(acc[a][b][e], p.d[m], p.bias, m, p.relu);
            }
    }
}

// kernel [K][C][taps] int8 -> fragment order: dword i = (tile16, chunk, lane, dword4); byte e of it is reduction row
// chunk * 64 + 16 * (lane >> 4) + dword4 * 4 + e = tap * C + c of output channel tile16 * 16 + (lane & 15); zero past K and past R
__global__ __launch_bounds__(256) void qconv_pack_mfma_kernel(int* packed, const signed char* kernel, int C, int K, int taps, int chunks, unsigned total)
{
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= total) return;
    const int d4 = (int)(i & 3u), lane = (int)((i >> 2) & 63u);
    const unsigned t = i >> 8;
    const int chunk = (int)(t % (unsigned)chunks), tile = (int)(t / (unsigned)chunks);
    const int m = tile * 16 + (lane & 15);
    const int R = taps * C;
    unsigned w4 = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e)
    {
        const int r = chunk * kQBK + 16 * (lane >> 4) + d4 * 4 + e;
        if (m < K && r < R)
        {
            const int tap = r / C, c = r - tap * C;
            w4 |= (unsigned)(unsigned char)kernel[((size_t)m * C + c) * taps + tap] << (8 * e);
        }
    }
    packed[i] = (int)w4;
}

// ---- host side ------------------------------------------------------------------------------------------------------

static int check_geometry(const fhip_qconv_param* p)
{
    const int rc = check_sizes(p);
    if (rc) return rc;
    if (p->dilation_h != 1 || p->dilation_w != 1) return fail(FHIP_E_BADARG, "dilation must be 1: a dilated int8 convolution is not supported");
    if (p->pad_left < 0 || p->pad_right < 0 || p->pad_top < 0 || p->pad_bottom < 0) return fail(FHIP_E_BADARG, "negative padding");
    if (p->group < 1) return fail(FHIP_E_BADARG, "group must be >= 1");
    if (p->group != 1 && (p->group != p->input_channels || p->group != p->output_channels))
        return fail(FHIP_E_BADARG, "partial group: group must be 1 or equal to both channel counts (depthwise)");
    if (p->int8_scale_term > 100) return fail(FHIP_E_BADARG, "int8_scale_term > 100: requantised int8 output is not supported");
    if (p->int8_scale_term < 0) return fail(FHIP_E_BADARG, "int8_scale_term must not be negative");
    if (p->activation != FHIP_ACT_NONE && p->activation != FHIP_ACT_RELU) return fail(FHIP_E_BADARG, "activation must be None or ReLU");
    const long long R = (long long)(p->input_channels / p->group) * p->kernel_h * p->kernel_w;
    if (R > FHIP_QCONV_MAX_REDUCTION) return fail(FHIP_E_BADARG, "reduction too long: more than 133144 products could overflow the int32 sum");
    if (p->kernel_h > (long long)p->input_h + p->pad_top + p->pad_bottom || p->kernel_w > (long long)p->input_w + p->pad_left + p->pad_right)
        return fail(FHIP_E_BADARG, "the kernel is larger than the padded input");
    const long long oh = ((long long)p->input_h + p->pad_top + p->pad_bottom - p->kernel_h) / p->stride_h + 1;
    const long long ow = ((long long)p->input_w + p->pad_left + p->pad_right - p->kernel_w) / p->stride_w + 1;
    const auto too_large = [](long long c, long long h, long long w) { return h > 0x7fffffffLL || w > 0x7fffffffLL || h * w > 0x7fffffffLL || c * (h * w) > 0x7fffffffLL; };
    if (too_large(p->input_channels, p->input_h, p->input_w) || too_large(p->output_channels, oh, ow))
        return fail(FHIP_E_BADARG, "tensor too large: 2^31 elements or more");
    return FHIP_OK;
}

static int check_param(const fhip_qconv_param* p)
{
    const int rc = check_geometry(p);
    if (rc) return rc;
    if (p->output_h != ((long long)p->input_h + p->pad_top + p->pad_bottom - p->kernel_h) / p->stride_h + 1 ||
        p->output_w != ((long long)p->input_w + p->pad_left + p->pad_right - p->kernel_w) / p->stride_w + 1)
        return fail(FHIP_E_BADARG, "output_h / output_w are not what fhip_qconv_assign_output_dim gives");
    return FHIP_OK;
}

enum RouteKind
{
    ROUTE_GENERIC,   // 4 output channels per lane
    ROUTE_GENERIC16, // 16
    ROUTE_DW_S1,
    ROUTE_DW_S2,
    ROUTE_MFMA_128, // 4 x 1 waves
    ROUTE_MFMA_64,  // 2 x 2 waves
    ROUTE_COUNT
};

static bool is_mfma(int r) { return r == ROUTE_MFMA_128 || r == ROUTE_MFMA_64; }
static bool is_dw(int r) { return r == ROUTE_DW_S1 || r == ROUTE_DW_S2; }
static bool is_generic(int r) { return r == ROUTE_GENERIC || r == ROUTE_GENERIC16; }
static int generic_kt(int r) { return r == ROUTE_GENERIC16 ? 16 : 4; }

static bool accepts(const fhip_qconv_param& p, int r)
{
    if (is_generic(r)) return true;
    if (is_dw(r))
        return p.group > 1 && p.kernel_h == 3 && p.kernel_w == 3 && p.stride_h == p.stride_w && p.stride_h == (r == ROUTE_DW_S1 ? 1 : 2);
    return p.group == 1 && p.input_channels % 16 == 0;
}

// The one selection function: fhip_qconv_forward launches what it says, fhip_qconv_route reports it, init packs for it.
static int select(const fhip_qconv_param& p)
{
    if (accepts(p, ROUTE_DW_S1)) return ROUTE_DW_S1;
    if (accepts(p, ROUTE_DW_S2)) return ROUTE_DW_S2;
    if (accepts(p, ROUTE_MFMA_128)) return p.output_channels > 64 ? ROUTE_MFMA_128 : ROUTE_MFMA_64;
    return p.output_channels / p.group >= 16 ? ROUTE_GENERIC16 : ROUTE_GENERIC;
}

static const char* route_name(int r)
{
    switch (r)
    {
    case ROUTE_GENERIC: return "fhip::qconv_generic_kernel<4>";
    case ROUTE_GENERIC16: return "fhip::qconv_generic_kernel<16>";
    case ROUTE_DW_S1: return "fhip::qconv_dw3x3_kernel<1>";
    case ROUTE_DW_S2: return "fhip::qconv_dw3x3_kernel<2>";
    case ROUTE_MFMA_128: return "fhip::qconv_mfma_kernel<4, 1>";
    default: return "fhip::qconv_mfma_kernel<2, 2>";
    }
}

static int route_by_name(const char* name)
{
    if (!name) return -1;
    for (int r = 0; r < ROUTE_COUNT; ++r)
        if (!strcmp(name, route_name(r))) return r;
    return -1;
}

static int mfma_chunks(const fhip_qconv_param& p) { return (p.input_channels * p.kernel_h * p.kernel_w + kQBK - 1) / kQBK; }

static size_t packed_bytes_of(const fhip_qconv_param& p, int r)
{
    if (is_dw(r)) return (size_t)p.input_channels * 12;
    if (is_generic(r)) return generic_packed_floats(p, generic_kt(r)); // one byte per (channel of a chunk, c, tap)
    return (size_t)((p.output_channels + kQRowPad - 1) / kQRowPad) * kQRowPad * mfma_chunks(p) * kQBK;
}

static int route_checks(const fhip_qconv_param* param, const char* route, int& r)
{
    const int rc = check_param(param);
    if (rc) return rc;
    r = route ? route_by_name(route) : select(*param);
    if (r < 0) return fail(FHIP_E_BADARG, "unknown route name");
    if (!accepts(*param, r)) return fail(FHIP_E_UNSUPPORTED, "the named route cannot run this layer");
    return FHIP_OK;
}

static int do_buffer_size(const fhip_qconv_param* param, int batch, const char* route, size_t* scratch_bytes, size_t* packed_bytes)
{
    int r;
    const int rc = route_checks(param, route, r);
    if (rc) return rc;
    if (batch < 1 || !scratch_bytes || !packed_bytes) return fail(FHIP_E_BADARG, "batch < 1 or a null size pointer");
    *scratch_bytes = 0;
    *packed_bytes = packed_bytes_of(*param, r);
    return FHIP_OK;
}

static int do_init(const fhip_qconv_param* param, void* packed, const signed char* kernel, void* stream, const char* route)
{
    int r;
    const int rc = route_checks(param, route, r);
    if (rc) return rc;
    if (!packed || !kernel) return fail(FHIP_E_BADARG, "null packed / kernel");
    if (!aligned(packed, 16)) return fail(FHIP_E_BADARG, "packed must be 16-byte aligned");
    const fhip_qconv_param& p = *param;
    const size_t bytes = packed_bytes_of(p, r);
    if (bytes > 0x7fffffffULL) return fail(FHIP_E_BADARG, "filter tensor too large: 2^31 packed bytes or more");
    const unsigned total = (unsigned)(bytes / 4); // every layout is whole dwords, one lane each
    const dim3 grid((total + 255) / 256);
    const int taps = p.kernel_h * p.kernel_w;
    hipStream_t s = (hipStream_t)stream;
    if (is_dw(r))
        hipLaunchKernelGGL(qconv_pack_dw_kernel, grid, dim3(256), 0, s, (int*)packed, kernel, total);
    else if (is_generic(r))
    {
        const int Cg = p.input_channels / p.group, Kg = p.output_channels / p.group, kt = generic_kt(r);
        hipLaunchKernelGGL(qconv_pack_generic_kernel, grid, dim3(256), 0, s, (int*)packed, kernel, Cg, Kg, taps, kt, (Kg + kt - 1) / kt, total);
    }
    else
        hipLaunchKernelGGL(qconv_pack_mfma_kernel, grid, dim3(256), 0, s, (int*)packed, kernel, p.input_channels, p.output_channels, taps, mfma_chunks(p), total);
    FHIP_CHECK_HIP(hipGetLastError());
    return FHIP_OK;
}

static int do_forward(const fhip_qconv_param* param, int batch, float* out, const float* in, const void* packed, const float* d, const float* bias,
                      float s_in, void* stream, const char* route)
{
    int r;
    int rc = route_checks(param, route, r);
    if (rc) return rc;
    const fhip_qconv_param& p = *param;
    if (batch < 1) return fail(FHIP_E_BADARG, "batch < 1");
    if (!out || !in || !packed || !d) return fail(FHIP_E_BADARG, "null out / in / packed / d");
    if (p.bias_term && !bias) return fail(FHIP_E_BADARG, "bias_term is set and bias is NULL");
    if (!aligned(out, 4) || !aligned(in, 4) || !aligned(packed, 16) || !aligned(d, 4) || (p.bias_term && !aligned(bias, 4)))
        return fail(FHIP_E_BADARG, "device pointers must be 4-byte aligned (packed: 16-byte)");
    if (!good_input_scale(s_in)) return fail(FHIP_E_BADARG, "s_in must be finite and > 0");
    const unsigned long long in_count = (unsigned long long)batch * p.input_channels * p.input_h * p.input_w;
    const unsigned long long out_count = (unsigned long long)batch * p.output_channels * p.output_h * p.output_w;
    if (in_count > 0x7fffffffULL || out_count > 0x7fffffffULL) return fail(FHIP_E_BADARG, "tensor too large: 2^31 elements or more");
    hipStream_t s = (hipStream_t)stream;
    const float* b = p.bias_term ? bias : nullptr;
    if (!is_mfma(r))
    {
        QDirectArgs a;
        a.x = in, a.w = (const int*)packed, a.d = d, a.bias = b, a.y = out, a.s_in = s_in;
        a.C = p.input_channels, a.K = p.output_channels, a.Cg = p.input_channels / p.group, a.Kg = p.output_channels / p.group;
        a.H = p.input_h, a.W = p.input_w, a.Ho = p.output_h, a.Wo = p.output_w, a.kh = p.kernel_h, a.kw = p.kernel_w;
        a.sh = p.stride_h, a.sw = p.stride_w, a.pt = p.pad_top, a.pl = p.pad_left;
        a.chunks = (a.Kg + generic_kt(r) - 1) / generic_kt(r);
        a.strips = (p.output_w + 3) / 4;
        a.relu = p.activation == FHIP_ACT_RELU;
        if (is_generic(r))
        {
            const size_t total = (size_t)batch * p.output_h * p.output_w, gy = (size_t)p.group * a.chunks;
            if (total > 0x7fffffffULL || gy > 65535) return fail(FHIP_E_BADARG, "more than 65535 chunks of 4 (16) output channels");
            a.total = (unsigned)total;
            const dim3 grid((unsigned)((total + 255) / 256), (unsigned)gy);
            if (r == ROUTE_GENERIC)
                hipLaunchKernelGGL(qconv_generic_kernel<4>, grid, dim3(256), 0, s, a);
            else
                hipLaunchKernelGGL(qconv_generic_kernel<16>, grid, dim3(256), 0, s, a);
        }
        else
        {
            const size_t total = (size_t)batch * p.input_channels * p.output_h * a.strips; // <= the output's elements: below 2^31
            a.total = (unsigned)total;
            const dim3 grid((unsigned)((total + 255) / 256));
            if (r == ROUTE_DW_S1)
                hipLaunchKernelGGL(qconv_dw3x3_kernel<1>, grid, dim3(256), 0, s, a);
            else
                hipLaunchKernelGGL(qconv_dw3x3_kernel<2>, grid, dim3(256), 0, s, a);
        }
    }
    else
    {
        QGemmArgs g;
        g.in = in, g.wq = (const i32x4*)packed, g.d = d, g.bias = b, g.out = out, g.s_in = s_in;
        g.C = p.input_channels, g.K = p.output_channels, g.H = p.input_h, g.W = p.input_w, g.Ho = p.output_h, g.Wo = p.output_w;
        g.kh = p.kernel_h, g.kw = p.kernel_w, g.sh = p.stride_h, g.sw = p.stride_w, g.pt = p.pad_top, g.pl = p.pad_left;
        g.HW = g.H * g.W;
        g.HoWo = g.Ho * g.Wo;
        const unsigned long long ntot = (unsigned long long)batch * g.HoWo;
        if (ntot > 0x3fffffffULL) return fail(FHIP_E_BADARG, "tensor too large: 2^30 GEMM columns or more");
        g.Ntot = (int)ntot;
        g.R = g.C * g.kh * g.kw;
        g.chunks = mfma_chunks(p);
        const int bm = r == ROUTE_MFMA_128 ? 128 : 64;
        g.m_tiles = (g.K + bm - 1) / bm;
        g.n_tiles = (g.Ntot + kQBN - 1) / kQBN;
        g.relu = p.activation == FHIP_ACT_RELU;
        const unsigned long long blocks = (unsigned long long)g.m_tiles * g.n_tiles;
        if (blocks > 0x7fffffffULL) return fail(FHIP_E_BADARG, "tensor too large: 2^31 blocks or more");
        if (r == ROUTE_MFMA_128)
            hipLaunchKernelGGL((qconv_mfma_kernel<4, 1>), dim3((unsigned)blocks), dim3(256), 0, s, g);
        else
            hipLaunchKernelGGL((qconv_mfma_kernel<2, 2>), dim3((unsigned)blocks), dim3(256), 0, s, g);
    }
    FHIP_CHECK_HIP(hipGetLastError());
    return FHIP_OK;
}

} // namespace fhip

using namespace fhip;

extern "C"
{

int fhip_qconv_assign_output_dim(fhip_qconv_param* param)
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

int fhip_qconv_supported(const fhip_qconv_param* param) { return check_param(param) == FHIP_OK ? 1 : 0; }

int fhip_qconv_get_buffer_size(const fhip_qconv_param* param, int batch, size_t* scratch_bytes, size_t* packed_bytes)
{
    return do_buffer_size(param, batch, nullptr, scratch_bytes, packed_bytes);
}

int fhip_qconv_init(const fhip_qconv_param* param, void* packed, const signed char* kernel, void* stream) { return do_init(param, packed, kernel, stream, nullptr); }

int fhip_qconv_dequant_scales(float* d, const float* s_w, int K, float s_in) { return int8_dequant_scales(d, s_w, K, s_in); }

int fhip_qconv_forward(const fhip_qconv_param* param, int batch, float* out, const float* in, const void* packed, float* /*scratch*/, const float* d,
                       const float* bias, float s_in, void* stream)
{
    return do_forward(param, batch, out, in, packed, d, bias, s_in, stream, nullptr);
}

int fhip_quantize_forward(signed char* out, const float* in, size_t count, float s_in, void* stream)
{
    if (!out || !in) return fail(FHIP_E_BADARG, "null out / in");
    if (count < 1 || count > 0x7fffffffULL) return fail(FHIP_E_BADARG, "count must be in [1, 2^31)");
    if (!aligned(in, 4)) return fail(FHIP_E_BADARG, "in must be 4-byte aligned");
    if (!good_input_scale(s_in)) return fail(FHIP_E_BADARG, "s_in must be finite and > 0");
    hipLaunchKernelGGL(quantize_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, (hipStream_t)stream, out, in, (unsigned)count, s_in);
    FHIP_CHECK_HIP(hipGetLastError());
    return FHIP_OK;
}

int fhip_qconv_route(const fhip_qconv_param* param, char* name, int len)
{
    const int rc = check_param(param);
    if (rc) return rc;
    if (!name || len < 1) return fail(FHIP_E_BADARG, "null name");
    snprintf(name, (size_t)len, "%s", route_name(select(*param)));
    return FHIP_OK;
}

int fhip_qconv_get_buffer_size_route(const fhip_qconv_param* param, int batch, const char* route, size_t* scratch_bytes, size_t* packed_bytes)
{
    if (!route) return fail(FHIP_E_BADARG, "null route name");
    return do_buffer_size(param, batch, route, scratch_bytes, packed_bytes);
}

int fhip_qconv_init_route(const fhip_qconv_param* param, void* packed, const signed char* kernel, void* stream, const char* route)
{
    if (!route) return fail(FHIP_E_BADARG, "null route name");
    return do_init(param, packed, kernel, stream, route);
}

int fhip_qconv_forward_route(const fhip_qconv_param* param, int batch, float* out, const float* in, const void* packed, float* /*scratch*/, const float* d,
                             const float* bias, float s_in, void* stream, const char* route)
{
    if (!route) return fail(FHIP_E_BADARG, "null route name");
    return do_forward(param, batch, out, in, packed, d, bias, s_in, stream, route);
}

const char* fhip_qconv_last_error(void) { return last_error(); }

} // extern "C"
