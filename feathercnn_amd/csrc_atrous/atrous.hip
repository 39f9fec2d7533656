// atrous.hip -- libfeather_atrous.so: dilated convolution (include/feather_hip/feather_atrous.h).  A library of its own: the main
// library's kernel set is closed, and the other libraries keep theirs.
//
// Three routes, one selection function (select()):
// 1. The MFMA route (group 1, C a multiple of 16, K >= 48): the implicit GEMM
//        out[K x N * Ho * Wo] = Wpack[K x taps * C] * gather(x),   gather(x)[(i, j, c)][(n, oy, ox)] = x[n][c][oy * sh - pt + i * dh][ox * sw - pl + j * dw]
//    on the project's one fp32-MFMA main loop (../csrc/gemm_core.h, included here and instantiated in THIS library only) through the
//    policy AtrousGemmPolicy below.  The reduction is tap-major with the channels innermost, so a k-tile of 16 lies inside one tap: a
//    loader decodes the tap of its request from the k-tile index (a thread issues one or two requests per k-tile) and a dilated tap
//    is nothing but another offset -- the loop never sees the dilation.
//      ROW4   (by name only, see select(); stride_w == 1, Wo % 4 == 0, W >= 4): the four GEMM columns of a lane are four adjacent pixels of one output row, a tap's four
//             inputs four adjacent floats: ONE 4-byte-aligned 16-byte load from the row, its start clamped into [0, W - 4], one row test,
//             and at LDS-write time a shift by (wanted start - clamped start) with per-element masks for the left / right padding.
//      scalar (any stride / width): four clamped 4-byte loads, as MODE 0 of ConvGemmPolicy.
//      SKIP   (at most 16 taps): a block whose column tile lies wholly outside a tap's valid rectangle drops that tap's k-tiles -- the
//             set of live taps is computed once per block (decode()) and both loaders walk it as a compacted list (4 bits per tap).  At dilation 12 .. 24 on a 41-pixel plane
//             most taps of most rows lie in the padding.
// 2. atrous_dw3x3_kernel: group == C == K, 3x3, stride 1 or 2 (DeepLab v3+ / MobileNetV2 at output stride 16, ESPNet).  Direct VALU, a
//    lane produces four adjacent outputs of a row; the block is uniform in (image, channel), so the nine taps are scalar operands.
//    VEC: 16-byte stores (and, stride 1, 16-byte loads with the same clamp-and-shift) at 4-byte alignment; else the 4-byte form.
// 3. atrous_generic_kernel: everything else (other groups, few channels, C % 16 != 0, odd kernels): one output pixel and 4 output
//    channels of one group per lane, clamped addresses.
// Out-of-plane taps are never multiplied by zero weights: their addresses are clamped into the plane and the value is replaced by 0.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>

#include "feather_hip/feather_atrous.h"
#include "direct_conv.h"
#include "gemm_core.h"

namespace fhip
{

// out[e] = r[e + s] for 0 <= e + s < 4 (the other elements are masked by the caller)
__device__ __forceinline__ float4 shift4(const f32x4u r, int s)
{
    float o[4];
#pragma unroll
    for (int e = 0; e < 4; ++e)
    {
        const int idx = e + s;
        o[e] = idx <= 0 ? r.x : idx == 1 ? r.y : idx == 2 ? r.z : r.w;
    }
    return make_float4(o[0], o[1], o[2], o[3]);
}

// ---- the generic route: direct_conv.h's body under this library's kernel names (the names fhip_atrous_route and traces report) ----
template <int KT>
__global__ __launch_bounds__(256) void atrous_generic_kernel(const DirectConvArgs a) { direct_conv_body<KT, DilatedTaps>(a); }

__global__ __launch_bounds__(256) void atrous_pack_generic_kernel(float* packed, const float* kernel, int Cg, int Kg, int taps, int kt, int chunks, unsigned total)
{
    direct_pack_body(packed, kernel, Cg, Kg, taps, kt, chunks, total);
}

// ---- the depthwise route --------------------------------------------------------------------------------------------
// y[n][c][oy][4 * strip .. + 4) of a 3x3 depthwise layer with stride S in both directions, any dilation and pads.  blockIdx.x = n * C + c.
// VEC: Wo % 4 == 0 (every strip is full: one 16-byte store) and, for S == 1, W >= 4 (a tap's four inputs are one 16-byte load from the row).
template <int S, bool VEC>
__global__ __launch_bounds__(256) void atrous_dw3x3_kernel(const DirectConvArgs a)
{
    const unsigned i = blockIdx.y * 256u + threadIdx.x;
    if (i >= a.total) return;
    const unsigned pc = blockIdx.x; // plane: image * C + channel
    const int c = (int)(pc % (unsigned)a.C);
    const int sx = (int)(i % (unsigned)a.strips), oy = (int)(i / (unsigned)a.strips);
    const int ox = sx * 4;
    const float* xp = a.x + (size_t)pc * a.H * a.W;
    const float* __restrict__ wp = a.w + (size_t)c * 9; // uniform over the block
    const int iy0 = oy * S - a.pt, ix0 = ox * S - a.pl;

    float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < 3; ++r)
    {
        const int iy = iy0 + r * a.dh;
        const bool row_in = iy >= 0 && iy < a.H;
        const float* row = xp + (size_t)min(max(iy, 0), a.H - 1) * a.W; // always a row of the plane
#pragma unroll
        for (int s = 0; s < 3; ++s)
        {
            const int xs = ix0 + s * a.dw;
            float v[4];
            if constexpr (VEC && S == 1)
            {
                const int xc = min(max(xs, 0), a.W - 4);
                const float4 f = shift4(*reinterpret_cast<const f32x4u*>(row + xc), xs - xc);
                v[0] = f.x, v[1] = f.y, v[2] = f.z, v[3] = f.w;
            }
            else
            {
#pragma unroll
                for (int p = 0; p < 4; ++p) v[p] = row[min(max(xs + p * S, 0), a.W - 1)];
            }
            const float wv = wp[r * 3 + s];
#pragma unroll
            for (int p = 0; p < 4; ++p)
            {
                const int ix = xs + p * S;
                const float u = (row_in && ix >= 0 && ix < a.W) ? v[p] : 0.f;
                acc[p] = fmaf(wv, u, acc[p]);
            }
        }
    }
    const float b = a.bias ? a.bias[c] : 0.f;
#pragma unroll
    for (int p = 0; p < 4; ++p)
    {
        acc[p] += b;
        if (a.relu) acc[p] = fmaxf(acc[p], 0.f);
    }
    float* yp = a.y + ((size_t)pc * a.Ho + oy) * a.Wo + ox;
    if constexpr (VEC)
    {
        f32x4u o;
        o.x = acc[0], o.y = acc[1], o.z = acc[2], o.w = acc[3];
        *reinterpret_cast<f32x4u*>(yp) = o;
    }
    else
    {
#pragma unroll
        for (int p = 0; p < 4; ++p)
            if (ox + p < a.Wo) yp[p] = acc[p];
    }
}

// the depthwise route reads the filters as they are: its "packed" form is a copy (init writes every packed word)
__global__ __launch_bounds__(256) void atrous_pack_copy_kernel(float* packed, const float* kernel, unsigned total)
{
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i < total) packed[i] = kernel[i];
}

// ---- the MFMA route: a policy of gemm_core.h ------------------------------------------------------------------------
constexpr int kAtrousBK = 16;
constexpr int kSkipMaxTaps = 16; // the compacted tap list holds 4 bits per tap

struct AtrousGemmParams
{
    int batches, m_tiles, n_tiles, k_tiles; // batches = 1; k_tiles = taps * C / 16
    const float* Wt;                        // [m_tiles panels][taps * C][bm], zero padded past K
    const float* in;
    float* out;
    const float* bias;
    int C, K, H, W, Ho, Wo, kh, kw, sh, sw, pt, pl, dh, dw;
    int C16, taps, HW, HoWo, Ntot;
    int bm, bn; // row tile, column tile
    int has_bias, relu;
};

// any o in [a, b] with lo <= o * s <= hi ?
__device__ __forceinline__ bool any_in(int a, int b, int s, int lo, int hi)
{
    const int q = max(a, (max(lo, 0) + s - 1) / s);
    return q <= b && q * s <= hi;
}

template <bool ROW4, bool SKIP>
struct AtrousGemmPolicy
{
    using Params = AtrousGemmParams;
    static constexpr int EXTRA_LDS_FLOATS = 0;
    static __device__ void stage_extra(const Params&, float*, int, int) {}
    static __device__ float bias_at(const Params& p, int m) { return (p.has_bias && m < p.K) ? p.bias[m] : 0.f; }
    // gemm_core's own order: consecutive ids share an XCD and walk row tiles fastest.  The GEMM has one batch entry, so the `batch` value
    // the main loop hands on to k_count and the loaders is free: SKIP computes the block's set of live taps here, ONCE, and passes it there.
    static __device__ void decode(const Params& p, int& mt, int& nt, int& batch)
    {
        const int vid = xcd_remap((int)blockIdx.x, p.m_tiles * p.n_tiles);
        mt = vid % p.m_tiles;
        nt = vid / p.m_tiles;
        batch = SKIP ? tap_mask(p, nt) : 0;
    }
    // SKIP: the taps that reach the plane from at least one column of the block's tile, bit i * kw + j (never empty: a tile that sees no tap
    // at all keeps tap 0, whose values are all masked).  A tile inside one image covers output rows oya .. oyb, inside one row columns
    // oxa .. oxb; tap (i, j) is alive when some such row has 0 <= oy * sh - pt + i * dh < H and some column the same in x.
    static __device__ int tap_mask(const Params& p, int nt)
    {
        const int c0 = nt * p.bn, c1 = min(c0 + p.bn, p.Ntot) - 1;
        const int img0 = c0 / p.HoWo, r0 = c0 - img0 * p.HoWo, img1 = c1 / p.HoWo, r1 = c1 - img1 * p.HoWo;
        int oya = 0, oyb = p.Ho - 1, oxa = 0, oxb = p.Wo - 1;
        if (img0 == img1)
        {
            oya = r0 / p.Wo;
            oyb = r1 / p.Wo;
            if (oya == oyb)
            {
                oxa = r0 - oya * p.Wo;
                oxb = r1 - oyb * p.Wo;
            }
        }
        int mask = 0;
        for (int i = 0; i < p.kh; ++i)
        {
            if (!any_in(oya, oyb, p.sh, p.pt - i * p.dh, p.pt - i * p.dh + p.H - 1)) continue;
            for (int j = 0; j < p.kw; ++j)
                if (any_in(oxa, oxb, p.sw, p.pl - j * p.dw, p.pl - j * p.dw + p.W - 1)) mask |= 1 << (i * p.kw + j);
        }
        return mask ? mask : 1;
    }
    // the live taps compacted, 4 bits each, in tap order
    static __device__ unsigned long long tap_list(int mask, int& count)
    {
        unsigned long long list = 0;
        count = 0;
#pragma unroll
        for (int t = 0; t < kSkipMaxTaps; ++t)
            if (mask & (1 << t))
            {
                list |= (unsigned long long)t << (4 * count);
                ++count;
            }
        return list;
    }
    static __device__ int k_count(const Params& p, int mask) { return SKIP ? __popc((unsigned)mask) * p.C16 : p.k_tiles; }
    // reduction row as the loop counts it -> (tap, channel); the tap of a k-tile is decoded from the k-tile index
    static __device__ void split(const Params& p, unsigned long long list, int krow, int& tap, int& c)
    {
        const int tile = krow >> 4;
        const int ct = tile / p.C16;
        c = ((tile - ct * p.C16) << 4) | (krow & 15);
        tap = SKIP ? (int)((list >> (4 * ct)) & 15ull) : ct;
    }

    struct ALoad
    {
        const float* base;
        unsigned long long list;
        int last; // the last reduction row of this block (address insurance)
        __device__ ALoad(const Params& p, int mask, int m4) : base(p.Wt + (size_t)(m4 / p.bm) * ((size_t)p.k_tiles * kAtrousBK) * p.bm + (m4 % p.bm))
        {
            int count = p.taps;
            list = SKIP ? tap_list(mask, count) : 0ull;
            last = count * p.C - 1;
        }
        __device__ float4 load(const Params& p, int krow) const
        {
            int tap, c;
            split(p, list, min(krow, last), tap, c);
            return *reinterpret_cast<const float4*>(base + (size_t)(tap * p.C + c) * p.bm);
        }
    };

    struct BRaw
    {
        f32x4u v;
        int s; // ROW4: wanted start - clamped start of the 16-byte load
    };

    struct BLoad
    {
        typedef BRaw Raw;
        int ib[ROW4 ? 1 : 4], y0[ROW4 ? 1 : 4], x0[ROW4 ? 1 : 4]; // per column (ROW4: of the first; the others follow in the row)
        unsigned valid;
        unsigned long long list;
        int last;
        __device__ BLoad(const Params& p, int mask, int n4)
        {
            int count = p.taps;
            list = SKIP ? tap_list(mask, count) : 0ull;
            last = count * p.C - 1;
            valid = 0;
#pragma unroll
            for (int e = 0; e < (ROW4 ? 1 : 4); ++e)
            {
                const int col = n4 + e;
                const bool ok = col < p.Ntot;
                const int cc = ok ? col : 0;
                const int img = cc / p.HoWo, rem = cc - img * p.HoWo;
                const int oy = rem / p.Wo, ox = rem - oy * p.Wo;
                ib[e] = img * p.C * p.HW; // < 2^31: the host refuses larger tensors
                y0[e] = oy * p.sh - p.pt;
                x0[e] = ox * p.sw - p.pl;
                valid |= ok ? (ROW4 ? 15u : (1u << e)) : 0u;
            }
        }
        __device__ float4 finish(const Params&, const Raw& raw, int, const float*) const
        {
            if (ROW4) return shift4(raw.v, raw.s);
            return make_float4(raw.v.x, raw.v.y, raw.v.z, raw.v.w);
        }
        // Unconditional loads from clamped addresses; `ok` says which of the 4 values are real (see gemm_core.h).
        __device__ Raw load(const Params& p, int krow, unsigned& ok) const
        {
            int tap, c;
            split(p, list, min(krow, last), tap, c);
            const int i = tap / p.kw, j = tap - i * p.kw;
            const int dy = i * p.dh, dx = j * p.dw;
            const float* plane = p.in + (size_t)c * p.HW;
            Raw r;
            ok = 0u;
            if (ROW4)
            {
                const int iy = y0[0] + dy, xs = x0[0] + dx;
                const bool row_in = (unsigned)iy < (unsigned)p.H;
                const int xc = min(max(xs, 0), p.W - 4);
                r.v = *reinterpret_cast<const f32x4u*>(plane + ib[0] + min(max(iy, 0), p.H - 1) * p.W + xc);
                r.s = xs - xc;
#pragma unroll
                for (int e = 0; e < 4; ++e) ok |= (row_in && (unsigned)(xs + e) < (unsigned)p.W) ? (1u << e) : 0u;
                ok &= valid;
            }
            else
            {
                float v[4];
#pragma unroll
                for (int e = 0; e < 4; ++e)
                {
                    const int iy = y0[e] + dy, ix = x0[e] + dx;
                    const bool in = (valid & (1u << e)) && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W;
                    ok |= in ? (1u << e) : 0u;
                    v[e] = plane[ib[e] + min(max(iy, 0), p.H - 1) * p.W + min(max(ix, 0), p.W - 1)];
                }
                r.v.x = v[0], r.v.y = v[1], r.v.z = v[2], r.v.w = v[3];
                r.s = 0;
            }
            return r;
        }
    };

    struct Store
    {
        float* ptr[ROW4 ? 1 : 4]; // &out[img][0][oy][ox] of each column (ROW4: of the first; the four are one run of a row)
        unsigned valid;
        __device__ Store(const Params& p, int, int n4)
        {
            valid = 0;
#pragma unroll
            for (int e = 0; e < (ROW4 ? 1 : 4); ++e)
            {
                const int col = n4 + e;
                const bool ok = col < p.Ntot;
                const int cc = ok ? col : 0;
                const int img = cc / p.HoWo, rem = cc - img * p.HoWo;
                ptr[e] = p.out + ((size_t)img * p.K) * p.HoWo + rem;
                valid |= ok ? (ROW4 ? 15u : (1u << e)) : 0u;
            }
        }
        __device__ float4 residual4(const Params&, int) const { return make_float4(0.f, 0.f, 0.f, 0.f); }
        __device__ void put4(const Params& p, int m, float4 v) const { put4b(p, m, v, bias_at(p, m), residual4(p, m)); }
        __device__ void put4b(const Params& p, int m, float4 v, float b, float4) const
        {
            if (m >= p.K) return;
            v.x += b;
            v.y += b;
            v.z += b;
            v.w += b;
            if (p.relu)
            {
                v.x = fmaxf(v.x, 0.f);
                v.y = fmaxf(v.y, 0.f);
                v.z = fmaxf(v.z, 0.f);
                v.w = fmaxf(v.w, 0.f);
            }
            const size_t moff = (size_t)m * p.HoWo;
            if constexpr (ROW4)
            {
                if (!valid) return;
                f32x4u o;
                o.x = v.x, o.y = v.y, o.z = v.z, o.w = v.w;
                *reinterpret_cast<f32x4u*>(ptr[0] + moff) = o; // 4-byte aligned: one global_store_dwordx4
            }
            else
            {
                if (valid & 1u) ptr[0][moff] = v.x;
                if (valid & 2u) ptr[1][moff] = v.y;
                if (valid & 4u) ptr[2][moff] = v.z;
                if (valid & 8u) ptr[3][moff] = v.w;
            }
        }
    };
};

using AtrousShapeBig = GemmShape<128, 64, 16, 2, 2>;    // >= 96 output channels
using AtrousShapeSmallM = GemmShape<64, 128, 16, 1, 4>; // 48 .. 95 output channels

// kernel [K][C][taps] -> Wt of AtrousGemmParams (reduction row = tap * C + c); one lane per packed word, every word written
__global__ __launch_bounds__(256) void atrous_pack_mfma_kernel(float* packed, const float* kernel, int C, int K, int taps, int bm, unsigned total)
{
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= total) return;
    const int mrow = (int)(i % (unsigned)bm);
    unsigned r = i / (unsigned)bm;
    const unsigned depth = (unsigned)taps * (unsigned)C;
    const int krow = (int)(r % depth), panel = (int)(r / depth);
    const int m = panel * bm + mrow;
    const int t = krow / C, c = krow - t * C;
    packed[i] = m < K ? kernel[((size_t)m * C + c) * taps + t] : 0.f;
}

// ---- host side ------------------------------------------------------------------------------------------------------

static long long out_dim(int in, int pa, int pb, int k, int d, int s) { return ((long long)in + pa + pb - ((long long)d * (k - 1) + 1)) / s + 1; }

static int check_geometry(const fhip_atrous_param* p)
{
    const int rc = check_sizes(p);
    if (rc) return rc;
    if (p->dilation_h < 1 || p->dilation_w < 1) return fail(FHIP_E_BADARG, "dilation must be >= 1");
    if (p->dilation_h == 1 && p->dilation_w == 1)
        return fail(FHIP_E_BADARG, "dilation 1 x 1 is not this library's: such a layer has tuned routes in libfeather_hip.so / libfeather_gconv.so");
    if (p->pad_left < 0 || p->pad_right < 0 || p->pad_top < 0 || p->pad_bottom < 0) return fail(FHIP_E_BADARG, "negative padding");
    if (p->group < 1 || p->input_channels % p->group) return fail(FHIP_E_BADARG, "input_channels is not divisible by group");
    if (p->output_channels % p->group) return fail(FHIP_E_BADARG, "output_channels (of the whole layer) is not divisible by group");
    if (p->activation != FHIP_ACT_NONE && p->activation != FHIP_ACT_RELU) return fail(FHIP_E_BADARG, "activation must be None or ReLU");
    const long long eh = (long long)p->dilation_h * (p->kernel_h - 1) + 1, ew = (long long)p->dilation_w * (p->kernel_w - 1) + 1;
    if (eh > (long long)p->input_h + p->pad_top + p->pad_bottom || ew > (long long)p->input_w + p->pad_left + p->pad_right)
        return fail(FHIP_E_BADARG, "the dilated kernel extent is larger than the padded input");
    const long long oh = out_dim(p->input_h, p->pad_top, p->pad_bottom, p->kernel_h, p->dilation_h, p->stride_h);
    const long long ow = out_dim(p->input_w, p->pad_left, p->pad_right, p->kernel_w, p->dilation_w, p->stride_w);
    if (oh < 1 || ow < 1) return fail(FHIP_E_BADARG, "empty output");
    // factor by factor: the product of three numbers near 2^31 overflows 64 bits, and the refusal such a param met was the compiler's choice
    const auto too_large = [](long long c, long long h, long long w) { return h > 0x7fffffffLL || w > 0x7fffffffLL || h * w > 0x7fffffffLL || c * (h * w) > 0x7fffffffLL; };
    if (too_large(p->input_channels, p->input_h, p->input_w) || too_large(p->output_channels, oh, ow))
        return fail(FHIP_E_BADARG, "tensor too large: 2^31 elements or more");
    return FHIP_OK;
}

static int check_param(const fhip_atrous_param* p)
{
    const int rc = check_geometry(p);
    if (rc) return rc;
    if (p->output_h != out_dim(p->input_h, p->pad_top, p->pad_bottom, p->kernel_h, p->dilation_h, p->stride_h) ||
        p->output_w != out_dim(p->input_w, p->pad_left, p->pad_right, p->kernel_w, p->dilation_w, p->stride_w))
        return fail(FHIP_E_BADARG, "output_h / output_w are not what fhip_atrous_assign_output_dim gives");
    return FHIP_OK;
}

enum RouteKind
{
    ROUTE_GENERIC,
    ROUTE_DW_S1_VEC,
    ROUTE_DW_S1,
    ROUTE_DW_S2_VEC,
    ROUTE_DW_S2,
    ROUTE_MFMA, // + 4 * small_m + 2 * row4 + skip
    ROUTE_COUNT = ROUTE_MFMA + 8
};

static bool is_mfma(int r) { return r >= ROUTE_MFMA; }
static bool mfma_small(int r) { return ((r - ROUTE_MFMA) & 4) != 0; }
static bool mfma_row4(int r) { return ((r - ROUTE_MFMA) & 2) != 0; }
static bool mfma_skip(int r) { return ((r - ROUTE_MFMA) & 1) != 0; }
static bool is_dw(int r) { return r >= ROUTE_DW_S1_VEC && r <= ROUTE_DW_S2; }

static bool row4_ok(const fhip_atrous_param& p) { return p.stride_w == 1 && p.output_w % 4 == 0 && p.input_w >= 4; }

// Can route `r` run this (supported) layer?
static bool accepts(const fhip_atrous_param& p, int r)
{
    if (r == ROUTE_GENERIC) return true;
    if (is_dw(r))
    {
        if (p.group != p.input_channels || p.output_channels != p.input_channels || p.kernel_h != 3 || p.kernel_w != 3 || p.stride_h != p.stride_w) return false;
        const int s = (r == ROUTE_DW_S1_VEC || r == ROUTE_DW_S1) ? 1 : 2;
        if (p.stride_h != s) return false;
        if (r == ROUTE_DW_S1_VEC) return row4_ok(p);
        if (r == ROUTE_DW_S2_VEC) return p.output_w % 4 == 0;
        return true;
    }
    if (p.group != 1 || p.input_channels % kAtrousBK) return false;
    if (mfma_row4(r) && !row4_ok(p)) return false;
    if (mfma_skip(r) && p.kernel_h * p.kernel_w > kSkipMaxTaps) return false;
    return true;
}

// The one selection function: fhip_atrous_forward launches what it says, fhip_atrous_route reports it, init packs for it.
//   depthwise: group == C == K, 3x3, stride 1 or 2; its 16-byte form where the rows allow it.
//   MFMA: group 1, C % 16 == 0 (a k-tile of 16 stays inside one tap) and at least 48 output channels (a 64-row tile padded by no more than
//   a quarter; the deconvolution route's thresholds); the 128-row tile from 96 channels on.  Tap skipping where the top padding alone
//   hides tap row 0 from at least one whole column tile, (pad_top / stride_h) * Wo >= the tile's columns: measured faster or equal on every
//   DeepLab shape at batch 1 and 8.  The B operand is the SCALAR form: ROW4 measured 1.4 - 3.0 % faster at batch 8 and
//   2 % slower at batch 1 on the 40- and 28-pixel shapes, and this function does not see the batch, so it never chooses ROW4; the form
//   stays reachable by name (fhip_atrous_forward_route) for the A/B.
//   Everything else (grouped, few channels, C % 16 != 0) is the generic kernel's.
static int select(const fhip_atrous_param& p)
{
    if (p.group == p.input_channels && p.group > 1 && accepts(p, ROUTE_DW_S1)) return row4_ok(p) ? ROUTE_DW_S1_VEC : ROUTE_DW_S1;
    if (p.group == p.input_channels && p.group > 1 && accepts(p, ROUTE_DW_S2)) return p.output_w % 4 == 0 ? ROUTE_DW_S2_VEC : ROUTE_DW_S2;
    if (p.group != 1 || p.input_channels % kAtrousBK || p.output_channels < 48) return ROUTE_GENERIC;
    const bool small_m = p.output_channels < 96;
    const int bn = small_m ? AtrousShapeSmallM::BN : AtrousShapeBig::BN;
    const bool skip = p.kernel_h * p.kernel_w <= kSkipMaxTaps && (long long)(p.pad_top / p.stride_h) * p.output_w >= bn;
    return ROUTE_MFMA + (small_m ? 4 : 0) + (skip ? 1 : 0);
}

static const char* route_name(int r)
{
    switch (r)
    {
    case ROUTE_GENERIC: return "fhip::atrous_generic_kernel<4>";
    case ROUTE_DW_S1_VEC: return "fhip::atrous_dw3x3_kernel<1, true>";
    case ROUTE_DW_S1: return "fhip::atrous_dw3x3_kernel<1, false>";
    case ROUTE_DW_S2_VEC: return "fhip::atrous_dw3x3_kernel<2, true>";
    case ROUTE_DW_S2: return "fhip::atrous_dw3x3_kernel<2, false>";
    case ROUTE_MFMA + 0: return "fhip::gemm_mfma_kernel<fhip::GemmShape<128, 64, 16, 2, 2, 4>, fhip::AtrousGemmPolicy<false, false> >";
    case ROUTE_MFMA + 1: return "fhip::gemm_mfma_kernel<fhip::GemmShape<128, 64, 16, 2, 2, 4>, fhip::AtrousGemmPolicy<false, true> >";
    case ROUTE_MFMA + 2: return "fhip::gemm_mfma_kernel<fhip::GemmShape<128, 64, 16, 2, 2, 4>, fhip::AtrousGemmPolicy<true, false> >";
    case ROUTE_MFMA + 3: return "fhip::gemm_mfma_kernel<fhip::GemmShape<128, 64, 16, 2, 2, 4>, fhip::AtrousGemmPolicy<true, true> >";
    case ROUTE_MFMA + 4: return "fhip::gemm_mfma_kernel<fhip::GemmShape<64, 128, 16, 1, 4, 4>, fhip::AtrousGemmPolicy<false, false> >";
    case ROUTE_MFMA + 5: return "fhip::gemm_mfma_kernel<fhip::GemmShape<64, 128, 16, 1, 4, 4>, fhip::AtrousGemmPolicy<false, true> >";
    case ROUTE_MFMA + 6: return "fhip::gemm_mfma_kernel<fhip::GemmShape<64, 128, 16, 1, 4, 4>, fhip::AtrousGemmPolicy<true, false> >";
    default: return "fhip::gemm_mfma_kernel<fhip::GemmShape<64, 128, 16, 1, 4, 4>, fhip::AtrousGemmPolicy<true, true> >";
    }
}

// a route by its name, or -1
static int route_by_name(const char* name)
{
    if (!name) return -1;
    for (int r = 0; r < ROUTE_COUNT; ++r)
        if (!strcmp(name, route_name(r))) return r;
    return -1;
}

static size_t packed_floats(const fhip_atrous_param& p, int r)
{
    const size_t taps = (size_t)p.kernel_h * p.kernel_w;
    if (is_dw(r)) return (size_t)p.input_channels * 9;
    if (r == ROUTE_GENERIC) return generic_packed_floats(p, kGenericKT);
    const int bm = mfma_small(r) ? AtrousShapeSmallM::BM : AtrousShapeBig::BM;
    return (size_t)((p.output_channels + bm - 1) / bm) * bm * taps * p.input_channels;
}

template <class Shape, bool ROW4, bool SKIP>
static void launch_mfma(AtrousGemmParams& g, hipStream_t s)
{
    hipLaunchKernelGGL((gemm_mfma_kernel<Shape, AtrousGemmPolicy<ROW4, SKIP>>), dim3((unsigned)(g.m_tiles * g.n_tiles)), dim3(Shape::THREADS), 0, s, g);
}

static int route_checks(const fhip_atrous_param* param, const char* route, int& r)
{
    const int rc = check_param(param);
    if (rc) return rc;
    r = route ? route_by_name(route) : select(*param);
    if (r < 0) return fail(FHIP_E_BADARG, "unknown route name");
    if (!accepts(*param, r)) return fail(FHIP_E_UNSUPPORTED, "the named route cannot run this layer");
    return FHIP_OK;
}

static int do_buffer_size(const fhip_atrous_param* param, int batch, const char* route, size_t* scratch_bytes, size_t* packed_bytes)
{
    int r;
    const int rc = route_checks(param, route, r);
    if (rc) return rc;
    if (batch < 1 || !scratch_bytes || !packed_bytes) return fail(FHIP_E_BADARG, "batch < 1 or a null size pointer");
    *scratch_bytes = 0;
    *packed_bytes = packed_floats(*param, r) * sizeof(float);
    return FHIP_OK;
}

static int do_init(const fhip_atrous_param* param, float* packed, const float* kernel, void* stream, const char* route)
{
    int r;
    const int rc = route_checks(param, route, r);
    if (rc) return rc;
    if (!packed || !kernel) return fail(FHIP_E_BADARG, "null packed / kernel");
    if (!aligned(packed, 16) || !aligned(kernel, 4)) return fail(FHIP_E_BADARG, "packed must be 16-byte aligned, kernel 4-byte aligned");
    const fhip_atrous_param& p = *param;
    const size_t total = packed_floats(p, r);
    if (total > 0x7fffffffULL) return fail(FHIP_E_BADARG, "filter tensor too large: 2^31 packed floats or more");
    const dim3 grid((unsigned)((total + 255) / 256));
    const int taps = p.kernel_h * p.kernel_w;
    if (is_dw(r))
        hipLaunchKernelGGL(atrous_pack_copy_kernel, grid, dim3(256), 0, (hipStream_t)stream, packed, kernel, (unsigned)total);
    else if (r == ROUTE_GENERIC)
        launch_direct_pack(atrous_pack_generic_kernel, p, kGenericKT, total, packed, kernel, (hipStream_t)stream);
    else
        hipLaunchKernelGGL(atrous_pack_mfma_kernel, grid, dim3(256), 0, (hipStream_t)stream, packed, kernel, p.input_channels, p.output_channels, taps,
                           mfma_small(r) ? AtrousShapeSmallM::BM : AtrousShapeBig::BM, (unsigned)total);
    FHIP_CHECK_HIP(hipGetLastError());
    return FHIP_OK;
}

static int do_forward(const fhip_atrous_param* param, int batch, float* out, const float* in, const float* packed, const float* bias, void* stream,
                      const char* route)
{
    int r;
    int rc = route_checks(param, route, r);
    if (rc) return rc;
    const fhip_atrous_param& p = *param;
    rc = check_forward_pointers(p, batch, out, in, packed, bias, 16, "device pointers must be 4-byte aligned (packed: 16-byte)");
    if (rc) return rc;
    const unsigned long long in_count = (unsigned long long)batch * p.input_channels * p.input_h * p.input_w;
    const unsigned long long out_count = (unsigned long long)batch * p.output_channels * p.output_h * p.output_w;
    if (in_count > 0x7fffffffULL || out_count > 0x7fffffffULL) return fail(FHIP_E_BADARG, "tensor too large: 2^31 elements or more");
    hipStream_t s = (hipStream_t)stream;
    if (!is_mfma(r))
    {
        DirectConvArgs a = direct_conv_args(p, kGenericKT, out, in, packed, bias);
        a.dh = p.dilation_h;
        a.dw = p.dilation_w;
        if (r == ROUTE_GENERIC)
        {
            rc = launch_direct(atrous_generic_kernel<kGenericKT>, a, (size_t)batch * p.output_h * p.output_w, (size_t)p.group * a.chunks, s,
                               "more than 65535 chunks of 4 output channels");
            if (rc) return rc;
        }
        else
        {
            a.strips = (p.output_w + 3) / 4;
            const size_t total = (size_t)p.output_h * a.strips;
            const size_t gy = (total + 255) / 256;
            if (gy > 65535) return fail(FHIP_E_BADARG, "output plane too large for the depthwise route: more than 65535 blocks of 256 lanes");
            a.total = (unsigned)total;
            const dim3 grid((unsigned)((size_t)batch * p.input_channels), (unsigned)gy);
            switch (r)
            {
            case ROUTE_DW_S1_VEC: hipLaunchKernelGGL((atrous_dw3x3_kernel<1, true>), grid, dim3(256), 0, s, a); break;
            case ROUTE_DW_S1: hipLaunchKernelGGL((atrous_dw3x3_kernel<1, false>), grid, dim3(256), 0, s, a); break;
            case ROUTE_DW_S2_VEC: hipLaunchKernelGGL((atrous_dw3x3_kernel<2, true>), grid, dim3(256), 0, s, a); break;
            default: hipLaunchKernelGGL((atrous_dw3x3_kernel<2, false>), grid, dim3(256), 0, s, a); break;
            }
        }
    }
    else
    {
        AtrousGemmParams g;
        memset(&g, 0, sizeof(g));
        const bool small_m = mfma_small(r);
        g.bm = small_m ? AtrousShapeSmallM::BM : AtrousShapeBig::BM;
        g.bn = small_m ? AtrousShapeSmallM::BN : AtrousShapeBig::BN;
        g.C = p.input_channels;
        g.K = p.output_channels;
        g.H = p.input_h;
        g.W = p.input_w;
        g.Ho = p.output_h;
        g.Wo = p.output_w;
        g.kh = p.kernel_h;
        g.kw = p.kernel_w;
        g.sh = p.stride_h;
        g.sw = p.stride_w;
        g.pt = p.pad_top;
        g.pl = p.pad_left;
        g.dh = p.dilation_h;
        g.dw = p.dilation_w;
        g.C16 = g.C / kAtrousBK;
        g.taps = g.kh * g.kw;
        g.HW = g.H * g.W;
        g.HoWo = g.Ho * g.Wo;
        const unsigned long long ntot = (unsigned long long)batch * g.HoWo;
        if (ntot > 0x3fffffffULL) return fail(FHIP_E_BADARG, "tensor too large: 2^30 GEMM columns or more");
        g.Ntot = (int)ntot;
        g.batches = 1;
        g.m_tiles = (g.K + g.bm - 1) / g.bm;
        g.n_tiles = (g.Ntot + g.bn - 1) / g.bn;
        g.k_tiles = g.taps * g.C16;
        g.has_bias = p.bias_term != 0;
        g.relu = p.activation == FHIP_ACT_RELU;
        g.Wt = packed;
        g.in = in;
        g.out = out;
        g.bias = p.bias_term ? bias : nullptr;
        switch (r - ROUTE_MFMA)
        {
        case 0: launch_mfma<AtrousShapeBig, false, false>(g, s); break;
        case 1: launch_mfma<AtrousShapeBig, false, true>(g, s); break;
        case 2: launch_mfma<AtrousShapeBig, true, false>(g, s); break;
        case 3: launch_mfma<AtrousShapeBig, true, true>(g, s); break;
        case 4: launch_mfma<AtrousShapeSmallM, false, false>(g, s); break;
        case 5: launch_mfma<AtrousShapeSmallM, false, true>(g, s); break;
        case 6: launch_mfma<AtrousShapeSmallM, true, false>(g, s); break;
        default: launch_mfma<AtrousShapeSmallM, true, true>(g, s); break;
        }
    }
    FHIP_CHECK_HIP(hipGetLastError());
    return FHIP_OK;
}

} // namespace fhip

using namespace fhip;

extern "C"
{

int fhip_atrous_assign_output_dim(fhip_atrous_param* param)
{
    if (!param) return fail(FHIP_E_BADARG, "null param");
    if (param->input_h < 1 || param->input_w < 1 || param->stride_h < 1 || param->stride_w < 1 || param->kernel_h < 1 || param->kernel_w < 1 ||
        param->dilation_h < 1 || param->dilation_w < 1)
        return fail(FHIP_E_BADARG, "input size, kernel size, stride and dilation must be >= 1");
    const long long nh = (long long)param->input_h + param->pad_top + param->pad_bottom - ((long long)param->dilation_h * (param->kernel_h - 1) + 1);
    const long long nw = (long long)param->input_w + param->pad_left + param->pad_right - ((long long)param->dilation_w * (param->kernel_w - 1) + 1);
    if (nh < 0 || nw < 0) return fail(FHIP_E_BADARG, "the dilated kernel extent is larger than the padded input");
    const long long oh = nh / param->stride_h + 1, ow = nw / param->stride_w + 1;
    if (oh > 0x7fffffffLL || ow > 0x7fffffffLL) return fail(FHIP_E_BADARG, "absurdly large output: 2^31 or more per side");
    param->output_h = (int)oh;
    param->output_w = (int)ow;
    return FHIP_OK;
}

int fhip_atrous_supported(const fhip_atrous_param* param) { return check_param(param) == FHIP_OK ? 1 : 0; }

int fhip_atrous_get_buffer_size(const fhip_atrous_param* param, int batch, size_t* scratch_bytes, size_t* packed_bytes)
{
    return do_buffer_size(param, batch, nullptr, scratch_bytes, packed_bytes);
}

int fhip_atrous_init(const fhip_atrous_param* param, float* packed, const float* kernel, void* stream) { return do_init(param, packed, kernel, stream, nullptr); }

int fhip_atrous_forward(const fhip_atrous_param* param, int batch, float* out, const float* in, const float* packed, float* /*scratch*/, const float* bias,
                        void* stream)
{
    return do_forward(param, batch, out, in, packed, bias, stream, nullptr);
}

int fhip_atrous_route(const fhip_atrous_param* param, char* name, int len)
{
    const int rc = check_param(param);
    if (rc) return rc;
    if (!name || len < 1) return fail(FHIP_E_BADARG, "null name");
    snprintf(name, (size_t)len, "%s", route_name(select(*param)));
    return FHIP_OK;
}

int fhip_atrous_get_buffer_size_route(const fhip_atrous_param* param, int batch, const char* route, size_t* scratch_bytes, size_t* packed_bytes)
{
    if (!route) return fail(FHIP_E_BADARG, "null route name");
    return do_buffer_size(param, batch, route, scratch_bytes, packed_bytes);
}

int fhip_atrous_init_route(const fhip_atrous_param* param, float* packed, const float* kernel, void* stream, const char* route)
{
    if (!route) return fail(FHIP_E_BADARG, "null route name");
    return do_init(param, packed, kernel, stream, route);
}

int fhip_atrous_forward_route(const fhip_atrous_param* param, int batch, float* out, const float* in, const float* packed, float* /*scratch*/,
                              const float* bias, void* stream, const char* route)
{
    if (!route) return fail(FHIP_E_BADARG, "null route name");
    return do_forward(param, batch, out, in, packed, bias, stream, route);
}

const char* fhip_atrous_last_error(void) { return last_error(); }

} // extern "C"
