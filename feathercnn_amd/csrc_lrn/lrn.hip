// libfeather_lrn.so: local response normalisation, alone and with the Pooling layer behind it, on gfx950 (include/feather_hip/feather_lrn.h is
// the contract; DESIGN.md 3.20 the design and its measurements).
//
// The layer reads a tensor once, writes it once and evaluates one power per element.
//
//   lrn_across_kernel<V, L>   across channels: a lane owns four pixels of an image -- adjacent, read and written as 16 bytes (V = 4), or 256
//                             apart, four coalesced 4-byte accesses (V = 1) -- and marches along the channels with the last L = local_size
//                             values in registers (L = 3, 5), so every element is read once; L = 0 (any other size) re-reads its taps, which
//                             hit the caches.  gridDim.y splits C into chunks of 16 (small grids: 8 or 4) channels that re-read a halo.
//   lrn_within_kernel         within channel: one element per lane, a direct sum over the clipped window
//   lrn_pool_lds_kernel<L>    LRN across channels -> Pooling: a block computes the LRN values of a band of input rows for 16 channels into
//                             LDS once (the same march, lanes along the pixels of the band) and pools from LDS
//   lrn_pool_direct_kernel    LRN -> Pooling for everything else: one pooled output per lane, every LRN value of its window on the spot
//
// Every kernel adds the squares in the order of the header -- ascending channel, or rows then columns, from 0.f -- with contraction off,
// and turns the sum into the output through the one function lrn_finish: they agree with each other bit for bit.  The pooling part restates
// pooling_kernel of csrc/layers.hip operation for operation.  No atomics, no allocation.
#include <float.h>
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <string>

#include "feather_hip/feather_lrn.h"
#include "side_error.h"

namespace fhip
{

// A product and a sum that are each rounded to fp32: hipcc contracts a * b + c into one fma by default, and the pragma takes the
// contraction off these operations wherever they are inlined (as in csrc_gate/gate.hip).
__device__ __forceinline__ float mul_rounded(float a, float b)
{
#pragma clang fp contract(off)
    return a * b;
}
__device__ __forceinline__ float add_rounded(float a, float b)
{
#pragma clang fp contract(off)
    return a + b;
}

enum PowForm
{
    POW_GENERAL = 0,
    POW_B075 = 1,
    POW_B05 = 2
};

// What every kernel needs of the layer.  a = alpha / local_size (across) or alpha / local_size^2 (within), divided on the host.
struct LrnArgs
{
    int local_size;
    float a, bias, beta;
    int form; // PowForm, chosen from beta on the host
};

// pow(d, -beta) for d > 0: the one function of (d, beta) of the whole library (the header names the three forms)
__device__ __forceinline__ float pow_neg(float d, const LrnArgs& g)
{
    if (g.form == POW_B075)
    {
        const float r = sqrtf(d);
        return 1.f / mul_rounded(r, sqrtf(r));
    }
    if (g.form == POW_B05) return 1.f / sqrtf(d);
    return powf(d, -g.beta);
}

// y from x and the sum s of the squares of its window
__device__ __forceinline__ float lrn_finish(float x, float s, const LrnArgs& g) { return mul_rounded(x, pow_neg(add_rounded(g.bias, mul_rounded(g.a, s)), g)); }

// The sum of the window of element (c, y, x) of the image at `img` ([C][H][W]), read from memory in the order of the header.
__device__ __forceinline__ float window_sum(const float* __restrict__ img, int region, int half, int C, int H, int W, int c, int y, int x)
{
    float s = 0.f;
    if (region == FHIP_LRN_ACROSS_CHANNELS)
    {
        const size_t hw = (size_t)H * W, at = (size_t)y * W + x;
        const int ca = c - min(half, c), cb = c + min(half, C - 1 - c); // no sum that could pass INT_MAX: local_size may be anything
        for (int cc = ca; cc <= cb; ++cc)
        {
            const float v = img[cc * hw + at];
            s = add_rounded(s, mul_rounded(v, v));
        }
    }
    else
    {
        const float* p = img + (size_t)c * H * W;
        const int ya = y - min(half, y), yb = y + min(half, H - 1 - y), xa = x - min(half, x), xb = x + min(half, W - 1 - x);
        for (int yy = ya; yy <= yb; ++yy)
            for (int xx = xa; xx <= xb; ++xx)
            {
                const float v = p[(size_t)yy * W + xx];
                s = add_rounded(s, mul_rounded(v, v));
            }
    }
    return s;
}

constexpr int kPixels = 4; // pixels of one lane of lrn_across_kernel

// The kPixels pixels of a lane in one channel.  PACKED: adjacent, one 16-byte access (the caller guarantees the alignment and that all four
// exist).  Otherwise 256 floats apart -- lane t of a block owns pixels t, t + 256, t + 512, t + 768 of the block's 1024, so that every one
// of its 4-byte accesses is coalesced across the wave and four of them are in flight -- and only the first `count` exist.
template <bool PACKED>
struct Quad
{
    float v[kPixels];
    static __device__ __forceinline__ Quad zero()
    {
        Quad r;
#pragma unroll
        for (int k = 0; k < kPixels; ++k) r.v[k] = 0.f;
        return r;
    }
    static __device__ __forceinline__ Quad load(const float* p, int count)
    {
        Quad r;
        if constexpr (PACKED)
        {
            const float4 q = *reinterpret_cast<const float4*>(p);
            r.v[0] = q.x, r.v[1] = q.y, r.v[2] = q.z, r.v[3] = q.w;
        }
        else
        {
#pragma unroll
            for (int k = 0; k < kPixels; ++k) r.v[k] = k < count ? p[k * 256] : 0.f;
        }
        return r;
    }
    __device__ __forceinline__ void store(float* p, int count) const
    {
        if constexpr (PACKED)
            *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
        else
        {
#pragma unroll
            for (int k = 0; k < kPixels; ++k)
                if (k < count) p[k * 256] = v[k];
        }
    }
};

// The march of one lane along the channels c0 .. c1 - 1 of its pixels: `col` points at them in channel 0, channels are `hw` floats apart,
// C is the image's channel count (taps outside [0, C) are zero).  emit(c, y) receives every result.  L = local_size held in registers, or
// 0: any size, the taps re-read.  The value a step takes into its window was loaded one step earlier, so that a load is in flight while a
// step computes.
template <bool PACKED, int L, class Emit>
__device__ __forceinline__ void march(const float* __restrict__ col, size_t hw, int count, int C, int c0, int c1, const LrnArgs& g, Emit emit)
{
    using Q = Quad<PACKED>;
    if constexpr (L > 0)
    {
        constexpr int N = L, HALF = N / 2;
        Q ring[N]; // the values of channels c - HALF .. c + HALF, slot k = channel c - HALF + k
#pragma unroll
        for (int k = 1; k < N; ++k)
        {
            const int cc = c0 - HALF + k - 1;
            ring[k] = cc >= 0 && cc < C ? Q::load(col + cc * hw, count) : Q::zero();
        }
        Q ahead = c0 < C - HALF ? Q::load(col + (c0 + HALF) * hw, count) : Q::zero();
        for (int c = c0; c < c1; ++c)
        {
#pragma unroll
            for (int k = 1; k < N; ++k) ring[k - 1] = ring[k];
            ring[N - 1] = ahead;
            ahead = c + 1 < c1 && c + 1 < C - HALF ? Q::load(col + (c + 1 + HALF) * hw, count) : Q::zero();
            Q y;
#pragma unroll
            for (int e = 0; e < kPixels; ++e)
            {
                float s = 0.f;
#pragma unroll
                for (int k = 0; k < N; ++k) s = add_rounded(s, mul_rounded(ring[k].v[e], ring[k].v[e]));
                y.v[e] = lrn_finish(ring[HALF].v[e], s, g);
            }
            emit(c, y);
        }
    }
    else
    {
        const int half = g.local_size / 2;
        for (int c = c0; c < c1; ++c)
        {
            const int ca = c - min(half, c), cb = c + min(half, C - 1 - c);
            Q s = Q::zero();
            for (int cc = ca; cc <= cb; ++cc)
            {
                const Q t = Q::load(col + cc * hw, count);
#pragma unroll
                for (int e = 0; e < kPixels; ++e) s.v[e] = add_rounded(s.v[e], mul_rounded(t.v[e], t.v[e]));
            }
            const Q x = Q::load(col + c * hw, count);
            Q y;
#pragma unroll
            for (int e = 0; e < kPixels; ++e) y.v[e] = lrn_finish(x.v[e], s.v[e], g);
            emit(c, y);
        }
    }
}

// grid.x = n * blocks_per_image, a block owning 1024 pixels of an image; grid.y = chunks of `chunk` channels.  V = 4: a lane's four pixels
// are adjacent (hw % 4 == 0); V = 1: they are 256 apart.
template <int V, int L>
__global__ __launch_bounds__(256) void lrn_across_kernel(float* __restrict__ out, const float* __restrict__ in, LrnArgs g, int C, unsigned hw,
                                                         unsigned blocks_per_image, int chunk)
{
    const unsigned image = blockIdx.x / blocks_per_image, first = (blockIdx.x % blocks_per_image) * (256u * kPixels);
    const unsigned u = V == 4 ? first + threadIdx.x * kPixels : first + threadIdx.x; // the lane's first pixel
    if (u >= hw) return;
    const int count = V == 4 ? kPixels : (int)min((hw - u + 255u) / 256u, (unsigned)kPixels);
    const int c0 = (int)blockIdx.y * chunk, c1 = c0 + min(chunk, C - c0);
    const size_t base = (size_t)image * C * hw + u;
    float* dst = out + base;
    march<V == 4, L>(in + base, (size_t)hw, count, C, c0, c1, g, [&](int c, const Quad<V == 4>& y) { y.store(dst + (size_t)c * hw, count); });
}

// one element per lane
__global__ __launch_bounds__(256) void lrn_within_kernel(float* __restrict__ out, const float* __restrict__ in, LrnArgs g, int C, int H, int W, unsigned total)
{
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= total) return;
    const unsigned x = i % (unsigned)W, t = i / (unsigned)W;
    const unsigned y = t % (unsigned)H, plane = t / (unsigned)H;
    const unsigned c = plane % (unsigned)C, image = plane / (unsigned)C;
    const float* img = in + (size_t)image * C * H * W;
    const float s = window_sum(img, FHIP_LRN_WITHIN_CHANNEL, g.local_size / 2, C, H, W, (int)c, (int)y, (int)x);
    out[i] = lrn_finish(in[i], s, g);
}

// fhip_pooling's geometry (csrc/layers.hip PoolParams)
struct PoolGeom
{
    int H, W, OH, OW, KH, KW, SH, SW;
    int off_y, off_x; // window origin offset = pad_top + pad_bottom / pad_left + pad_right (reference quirk)
    int average;
};

// pooling_kernel of csrc/layers.hip for one output, its taps supplied by at(yy, xx)
template <class At>
__device__ __forceinline__ float pool_window(const PoolGeom& q, int oy, int ox, At at)
{
    const int y0 = oy * q.SH - q.off_y, x0 = ox * q.SW - q.off_x;
    const int ya = max(y0, 0), yb = min(y0 + q.KH, q.H);
    const int xa = max(x0, 0), xb = min(x0 + q.KW, q.W);
    float total_v = q.average ? 0.f : -FLT_MAX;
    int counter = 0;
    for (int yy = ya; yy < yb; ++yy)
        for (int xx = xa; xx < xb; ++xx)
        {
            const float v = at(yy, xx);
            if (q.average)
            {
                total_v = add_rounded(total_v, v);
                ++counter;
            }
            else
                total_v = total_v > v ? total_v : v;
        }
    return q.average ? total_v / counter : total_v; // empty window: 0/0 = NaN exactly like fhip_pooling
}

// blockIdx.x = (image * chunks + chunk) * bands + band.  A band is `band_rows` pooled rows; LDS holds [channels][npx] LRN values of the
// input rows y_lo .. y_hi - 1 those windows touch: whole rows, so the npx pixels of a band are contiguous in every channel.  The values are
// computed by the march of lrn_across_kernel -- a lane owns the band's pixels t, t + 256, ... -- and the block then pools from LDS.  The host
// chose band_rows so that FHIP_LRN_CHUNK * npx <= FHIP_LRN_POOL_LDS_FLOATS, and `channels` (16, 8 or 4) as select_chunk says.
template <int L>
__global__ __launch_bounds__(256) void lrn_pool_lds_kernel(float* __restrict__ out, const float* __restrict__ in, LrnArgs g, PoolGeom q, int C, int chunks, int bands,
                                                           int band_rows, int channels)
{
    extern __shared__ float lds[];
    const int band = (int)(blockIdx.x % (unsigned)bands);
    const unsigned t = blockIdx.x / (unsigned)bands;
    const int chunk = (int)(t % (unsigned)chunks);
    const unsigned image = t / (unsigned)chunks;
    const int c0 = chunk * channels, c1 = min(c0 + channels, C);
    const int oy0 = band * band_rows, oy1 = min(oy0 + band_rows, q.OH);
    const int y_lo = min(max(oy0 * q.SH - q.off_y, 0), q.H), y_hi = min((oy1 - 1) * q.SH - q.off_y + q.KH, q.H);
    const int npx = max(y_hi - y_lo, 0) * q.W;
    const size_t hw = (size_t)q.H * q.W;
    const float* img = in + (size_t)image * C * hw + (size_t)y_lo * q.W;
    for (int px = (int)threadIdx.x; px < npx; px += 256 * kPixels)
    {
        const int count = min((npx - px + 255) / 256, kPixels);
        float* dst = lds + px;
        march<false, L>(img + px, hw, count, C, c0, c1, g, [&](int c, const Quad<false>& y) { y.store(dst + (c - c0) * npx, count); });
    }
    __syncthreads();
    const int rows = oy1 - oy0, per_channel = rows * q.OW, outputs = (c1 - c0) * per_channel;
    for (int o = (int)threadIdx.x; o < outputs; o += 256)
    {
        const int cl = o / per_channel, r = o % per_channel;
        const int oy = oy0 + r / q.OW, ox = r % q.OW;
        const float* plane = lds + cl * npx; // row yy of the image is row yy - y_lo of the band
        out[(((size_t)image * C + c0 + cl) * q.OH + oy) * q.OW + ox] = pool_window(q, oy, ox, [&](int yy, int xx) { return plane[(yy - y_lo) * q.W + xx]; });
    }
}

// one pooled output per lane
__global__ __launch_bounds__(256) void lrn_pool_direct_kernel(float* __restrict__ out, const float* __restrict__ in, LrnArgs g, PoolGeom q, int region, int C,
                                                              unsigned total)
{
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= total) return;
    const unsigned ox = i % (unsigned)q.OW, t = i / (unsigned)q.OW;
    const unsigned oy = t % (unsigned)q.OH, plane = t / (unsigned)q.OH;
    const int c = (int)(plane % (unsigned)C);
    const float* img = in + (size_t)(plane / (unsigned)C) * C * q.H * q.W;
    const int half = g.local_size / 2;
    out[i] = pool_window(q, (int)oy, (int)ox, [&](int yy, int xx) {
        return lrn_finish(img[((size_t)c * q.H + yy) * q.W + xx], window_sum(img, region, half, C, q.H, q.W, c, yy, xx), g);
    });
}

constexpr long long kMaxBlocks = (1ll << 24) - 1; // of 256 lanes: HIP refuses a launch of 2^32 lanes or more along x

static bool aligned(unsigned mask, const void* a, const void* b = nullptr) { return (((uintptr_t)a | (uintptr_t)b) & mask) == 0; }

// Everything the entries check that is no pointer; fills g.
static int lrn_args(int region, int local_size, float alpha, float beta, float bias, int n, int c, int h, int w, LrnArgs& g)
{
    char buf[160];
    if (region != FHIP_LRN_ACROSS_CHANNELS && region != FHIP_LRN_WITHIN_CHANNEL)
    {
        snprintf(buf, sizeof(buf), "unknown region_type %d (0 across channels and 1 within channel are supported)", region);
        return fail(FHIP_E_BADARG, buf);
    }
    if (local_size < 1 || local_size % 2 == 0)
    {
        snprintf(buf, sizeof(buf), "local_size %d must be odd and at least 1 (an even size has no agreed meaning)", local_size);
        return fail(FHIP_E_BADARG, buf);
    }
    if (!std::isfinite(alpha) || !std::isfinite(beta) || !std::isfinite(bias)) return fail(FHIP_E_BADARG, "alpha, beta and bias must be finite");
    if (!(bias > 0.f) || alpha < 0.f)
    {
        snprintf(buf, sizeof(buf), "bias %g and alpha %g: bias > 0 and alpha >= 0 are required, else bias + alpha * sum could be 0 or negative", (double)bias,
                 (double)alpha);
        return fail(FHIP_E_BADARG, buf);
    }
    if (n < 1 || c < 1 || h < 1 || w < 1) return fail(FHIP_E_BADARG, "every dimension must be at least 1");
    if ((long long)n * c * h * w >= (1ll << 31)) return fail(FHIP_E_BADARG, "tensors of 2^31 elements or more are not supported");
    g.local_size = local_size;
    g.a = region == FHIP_LRN_ACROSS_CHANNELS ? alpha / (float)local_size : alpha / ((float)local_size * (float)local_size);
    g.bias = bias;
    g.beta = beta;
    g.form = beta == 0.75f ? POW_B075 : beta == 0.5f ? POW_B05 : POW_GENERAL;
    return FHIP_OK;
}

static int check_pointers(const float* out, size_t out_count, const float* in, size_t in_count)
{
    if (!out || !in) return fail(FHIP_E_BADARG, "null out / in");
    if (!aligned(3, out, in)) return fail(FHIP_E_BADARG, "pointers must be 4-byte aligned");
    const uintptr_t o0 = (uintptr_t)out, i0 = (uintptr_t)in;
    if (o0 < i0 + in_count * 4 && i0 < o0 + out_count * 4) return fail(FHIP_E_BADARG, "out must not overlap in (the layer is not in place)");
    return FHIP_OK;
}

static int held(int local_size) { return local_size == 3 || local_size == 5 ? local_size : 0; } // the L of the kernels

static bool vec4(int h, int w, const void* out, const void* in) { return (long long)h * w % 4 == 0 && aligned(15, out, in); }

static unsigned across_blocks(int h, int w) { return ((unsigned)h * (unsigned)w + 256u * kPixels - 1) / (256u * kPixels); } // 1024 pixels a block

// The channels of one block: FHIP_LRN_CHUNK, halved (to 8, to 4) while the grid -- `units` blocks per chunk -- stays below 2048 blocks, 8 a CU.
// A block's march is a chain of chunk + local_size - 1 dependent steps, and on a grid that does not fill the chip that chain is the
// kernel's time: measured, 4 channels a block halve it at batch 1 and nothing is lost where the grid is large.
static int select_chunk(long long units, int c)
{
    int chunk = FHIP_LRN_CHUNK;
    while (chunk > 4 && units * ((c + chunk - 1) / chunk) < 2048) chunk /= 2;
    return chunk;
}

template <int V>
static void launch_across(int l, dim3 grid, hipStream_t s, float* out, const float* in, const LrnArgs& g, int c, unsigned hw, unsigned bpi, int chunk)
{
    if (l == 3)
        hipLaunchKernelGGL((lrn_across_kernel<V, 3>), grid, dim3(256), 0, s, out, in, g, c, hw, bpi, chunk);
    else if (l == 5)
        hipLaunchKernelGGL((lrn_across_kernel<V, 5>), grid, dim3(256), 0, s, out, in, g, c, hw, bpi, chunk);
    else
        hipLaunchKernelGGL((lrn_across_kernel<V, 0>), grid, dim3(256), 0, s, out, in, g, c, hw, bpi, chunk);
}

// chunk: the channels of one block, 0 = all; -1 = selected as the header says
static int across_forward(const LrnArgs& g, int n, int c, int h, int w, int chunk, float* out, const float* in, void* stream)
{
    const bool v4 = vec4(h, w, out, in);
    const unsigned bpi = across_blocks(h, w);
    if (chunk < 0) chunk = select_chunk((long long)n * bpi, c);
    if (chunk == 0 || chunk > c) chunk = c;
    const int chunks = (c + chunk - 1) / chunk;
    if (chunks > 65535) return fail(FHIP_E_BADARG, "more than 65535 chunks of channels (c above 1048560 at a chunk of 16)");
    if ((long long)n * bpi > kMaxBlocks) return fail(FHIP_E_BADARG, "more than 2^24 - 1 blocks (n * ceil(h * w / 1024)): a launch takes no more");
    const dim3 grid((unsigned)n * bpi, (unsigned)chunks);
    const unsigned hw = (unsigned)h * (unsigned)w;
    if (v4)
        launch_across<4>(held(g.local_size), grid, (hipStream_t)stream, out, in, g, c, hw, bpi, chunk);
    else
        launch_across<1>(held(g.local_size), grid, (hipStream_t)stream, out, in, g, c, hw, bpi, chunk);
    FHIP_CHECK_HIP(hipGetLastError());
    return FHIP_OK;
}

// fhip_pool_param -> PoolGeom, with fhip_pooling's output size (layers.hip fhip_pooling_output_dim, restated: this library does not link
// libfeather_hip.so)
static int pool_geometry(const fhip_pool_param* p, int n, int c, int h, int w, PoolGeom& q)
{
    if (!p) return fail(FHIP_E_BADARG, "null pool");
    if (p->channels != c || p->input_h != h || p->input_w != w) return fail(FHIP_E_BADARG, "pool->channels / input_h / input_w must equal c / h / w");
    if (p->global_pooling) return fail(FHIP_E_BADARG, "global pooling is not supported behind an LRN (run fhip_lrn_forward and fhip_pooling)");
    if (p->kernel_h < 1 || p->kernel_w < 1 || p->stride_h < 1 || p->stride_w < 1) return fail(FHIP_E_BADARG, "pooling kernel and stride must be at least 1");
    if (p->kernel_h >= (1 << 30) || p->kernel_w >= (1 << 30)) return fail(FHIP_E_BADARG, "pooling kernel too large");
    if (p->pad_left < 0 || p->pad_right < 0 || p->pad_top < 0 || p->pad_bottom < 0) return fail(FHIP_E_BADARG, "negative pooling pad");
    if ((long long)h + p->pad_top + p->pad_bottom >= (1 << 30) || (long long)w + p->pad_left + p->pad_right >= (1 << 30))
        return fail(FHIP_E_BADARG, "pooling pads too large");
    q.H = h, q.W = w;
    q.KH = p->kernel_h, q.KW = p->kernel_w, q.SH = p->stride_h, q.SW = p->stride_w;
    q.off_y = p->pad_top + p->pad_bottom, q.off_x = p->pad_left + p->pad_right;
    q.OH = (int)ceilf((float)(h + q.off_y - q.KH) / q.SH) + 1;
    q.OW = (int)ceilf((float)(w + q.off_x - q.KW) / q.SW) + 1;
    q.average = p->pooling_type != 0;
    if (q.OH < 1 || q.OW < 1) return fail(FHIP_E_BADARG, "empty pooling output");
    // fhip_pooling sends a window that covers the unpadded plane to its plane-reduce kernels (layers.hip), which sum in another order than
    // its generic kernel: this library restates only the generic one, so that geometry is refused like global pooling
    if (q.OH == 1 && q.OW == 1 && q.off_y == 0 && q.off_x == 0 && q.KH >= h && q.KW >= w)
        return fail(FHIP_E_BADARG, "a pooling window that covers the whole unpadded plane is not supported behind an LRN (run fhip_lrn_forward and fhip_pooling)");
    if ((long long)n * c * q.OH * q.OW >= (1ll << 31)) return fail(FHIP_E_BADARG, "tensors of 2^31 elements or more are not supported");
    return FHIP_OK;
}

// pooled rows of one band of lrn_pool_lds_kernel, or 0: the direct kernel runs
static int pool_band_rows(int region, const PoolGeom& q)
{
    if (region != FHIP_LRN_ACROSS_CHANNELS) return 0;
    const long long in_rows = FHIP_LRN_POOL_LDS_FLOATS / FHIP_LRN_CHUNK / (long long)q.W;
    if (in_rows < q.KH) return 0;
    return (int)std::min<long long>((in_rows - q.KH) / q.SH + 1, q.OH);
}

} // namespace fhip

using namespace fhip;

extern "C"
{

int fhip_lrn_forward(int region, int local_size, float alpha, float beta, float bias, int n, int c, int h, int w, float* out, const float* in, void* stream)
{
    LrnArgs g;
    int rc = lrn_args(region, local_size, alpha, beta, bias, n, c, h, w, g);
    if (rc) return rc;
    const size_t total = (size_t)n * c * h * w;
    if ((rc = check_pointers(out, total, in, total))) return rc;
    if (region == FHIP_LRN_ACROSS_CHANNELS) return across_forward(g, n, c, h, w, -1, out, in, stream);
    hipLaunchKernelGGL(lrn_within_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, out, in, g, c, h, w, (unsigned)total);
    FHIP_CHECK_HIP(hipGetLastError());
    return FHIP_OK;
}

int fhip_lrn_forward_chunked(int local_size, float alpha, float beta, float bias, int n, int c, int h, int w, int chunk, float* out, const float* in, void* stream)
{
    LrnArgs g;
    int rc = lrn_args(FHIP_LRN_ACROSS_CHANNELS, local_size, alpha, beta, bias, n, c, h, w, g);
    if (rc) return rc;
    if (chunk < 0) return fail(FHIP_E_BADARG, "chunk must be 0 (no split) or positive");
    const size_t total = (size_t)n * c * h * w;
    if ((rc = check_pointers(out, total, in, total))) return rc;
    return across_forward(g, n, c, h, w, chunk, out, in, stream);
}

int fhip_lrn_route(int region, int local_size, int n, int c, int h, int w, const float* out, const float* in, char* name, int len)
{
    LrnArgs g;
    const int rc = lrn_args(region, local_size, 1.f, 0.75f, 1.f, n, c, h, w, g);
    if (rc) return rc;
    if (!name || len < 1) return fail(FHIP_E_BADARG, "null name");
    if (region == FHIP_LRN_ACROSS_CHANNELS)
        snprintf(name, (size_t)len, "fhip::lrn_across_kernel<%d, %d>", vec4(h, w, out, in) ? 4 : 1, held(local_size));
    else
        snprintf(name, (size_t)len, "fhip::lrn_within_kernel");
    return FHIP_OK;
}

int fhip_lrn_pool_forward(int region, int local_size, float alpha, float beta, float bias, int n, int c, int h, int w, const fhip_pool_param* pool, float* out,
                          const float* in, void* stream)
{
    LrnArgs g;
    PoolGeom q;
    int rc = lrn_args(region, local_size, alpha, beta, bias, n, c, h, w, g);
    if (rc) return rc;
    if ((rc = pool_geometry(pool, n, c, h, w, q))) return rc;
    const size_t total_out = (size_t)n * c * q.OH * q.OW;
    if ((rc = check_pointers(out, total_out, in, (size_t)n * c * h * w))) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int band_rows = pool_band_rows(region, q);
    if (band_rows)
    {
        const int bands = (q.OH + band_rows - 1) / band_rows, channels = select_chunk((long long)n * bands, c), chunks = (c + channels - 1) / channels;
        const long long blocks = (long long)n * chunks * bands;
        if (blocks > kMaxBlocks) return fail(FHIP_E_BADARG, "more than 2^24 - 1 blocks (n * chunks of channels * bands of pooled rows): a launch takes no more");
        const size_t lds = (size_t)channels * (((size_t)band_rows - 1) * q.SH + q.KH) * q.W * sizeof(float);
        const dim3 grid((unsigned)blocks);
        switch (held(local_size))
        {
        case 3: hipLaunchKernelGGL(lrn_pool_lds_kernel<3>, grid, dim3(256), lds, s, out, in, g, q, c, chunks, bands, band_rows, channels); break;
        case 5: hipLaunchKernelGGL(lrn_pool_lds_kernel<5>, grid, dim3(256), lds, s, out, in, g, q, c, chunks, bands, band_rows, channels); break;
        default: hipLaunchKernelGGL(lrn_pool_lds_kernel<0>, grid, dim3(256), lds, s, out, in, g, q, c, chunks, bands, band_rows, channels); break;
        }
    }
    else
        hipLaunchKernelGGL(lrn_pool_direct_kernel, dim3((unsigned)((total_out + 255) / 256)), dim3(256), 0, s, out, in, g, q, region, c, (unsigned)total_out);
    FHIP_CHECK_HIP(hipGetLastError());
    return FHIP_OK;
}

int fhip_lrn_pool_route(int region, int local_size, int n, int c, int h, int w, const fhip_pool_param* pool, const float* out, const float* in, char* name,
                        int len)
{
    (void)out;
    (void)in;
    LrnArgs g;
    PoolGeom q;
    int rc = lrn_args(region, local_size, 1.f, 0.75f, 1.f, n, c, h, w, g);
    if (rc) return rc;
    if ((rc = pool_geometry(pool, n, c, h, w, q))) return rc;
    if (!name || len < 1) return fail(FHIP_E_BADARG, "null name");
    if (pool_band_rows(region, q))
        snprintf(name, (size_t)len, "fhip::lrn_pool_lds_kernel<%d>", held(local_size));
    else
        snprintf(name, (size_t)len, "fhip::lrn_pool_direct_kernel");
    return FHIP_OK;
}

const char* fhip_lrn_last_error(void) { return last_error(); }

} // extern "C"
