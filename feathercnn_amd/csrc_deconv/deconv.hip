// deconv.hip -- libfeather_deconv.so: transposed convolution (include/feather_hip/feather_deconv.h).  A library of its own: the main
// library's kernel set is closed.
//
// Both routes are GATHER forms by output phase.  With oy + pad_top = qy * sh + py and ox + pad_left = qx * sw + px (0 <= py < sh,
// 0 <= px < sw) the definition's condition  oy + pad_top - i = iy * sh  reads  i = py + ti * sh, iy = qy - ti: an output of phase
// (py, px) sees the taps i = py (mod sh), j = px (mod sw) only -- ceil((kh - py) / sh) * ceil((kw - px) / sw) of them -- applied at
// stride 1 to the un-stuffed input.  Nothing is multiplied by an inserted zero and no stuffed tensor exists.
//
// 1. The MFMA route (group 1, C a multiple of 16, enough output channels to fill a tile; select()): per phase an implicit GEMM
//        out_phase[K x N * Hq * Wq] = Wpack_phase[K x taps * C] * gather(x),      gather(x)[(ti, tj, c)][(n, qy, qx)] = x[n][c][qy - ti][qx - tj]
//    on the project's one fp32-MFMA main loop (../csrc/gemm_core.h, included here and instantiated in THIS library only) through the
//    policy DeconvGemmPolicy below.  One launch runs every phase: the phase is the GEMM's batch index.
//      (a) the store.  One phase writes every sw-th float of an output row.  The B operand above does not depend on px -- the same
//          (qy, qx) column serves every x-phase -- so for sw == 2 (PAIR) the two x-phases of a row share a block: they are stacked
//          in the M dimension, rows 16 g .. 16 g + 7 are channels 8 g .. 8 g + 7 of px = 0 and rows 16 g + 8 .. 16 g + 15 the same
//          channels of px = 1.  gemm_core's epilogue hands a lane rows r and r + 8 of the same four columns one after the other, so
//          the store keeps the first float4, interleaves it with the second and writes 8 consecutive floats of the output row as two
//          16-byte stores (4-byte aligned addresses: pad_left = 1 makes the run start at an odd pixel).  The x-phase with fewer taps
//          (kw odd) is padded with zero weights: k3 s2 executes 12 tap-products per 2 x 2 outputs where 9 are useful, k4 s2 and k2 s2
//          none in excess.  Other strides keep one phase per block and store dwords sw apart.
//      (b) the schedule.  Phases have different reduction depths (k3 s2 PAIR: 4 and 2 taps).  The host orders the batch entries
//          deepest first and decode() below dispatches phase after phase (the XCD remap of gemm_core is applied inside a phase), so
//          the blocks that run last are the shallowest ones and the tail of the launch is short.
// 2. deconv_generic_kernel: everything else -- any group including depthwise, any kernel / stride / pads, few output channels (an
//    RGB head).  One output pixel and 4 output channels of one group per lane, the phase's taps only, clamped addresses.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>

#include "feather_hip/feather_deconv.h"
#include "direct_conv.h"
#include "gemm_core.h"

namespace fhip
{

// ---- the generic route: direct_conv.h's body under this library's kernel names (the names fhip_deconv_route and traces report) ----
template <int KT>
__global__ __launch_bounds__(256) void deconv_generic_kernel(const DirectConvArgs a) { direct_conv_body<KT, PhaseTaps>(a); }

__global__ __launch_bounds__(256) void deconv_pack_generic_kernel(float* packed, const float* kernel, int Cg, int Kg, int taps, int kt, int chunks, unsigned total)
{
    direct_pack_body(packed, kernel, Cg, Kg, taps, kt, chunks, total);
}

// ---- the MFMA route: a policy of gemm_core.h ------------------------------------------------------------------------
constexpr int kDeconvBK = 16;
constexpr int kMaxPhases = 16;

struct DeconvGemmParams
{
    int batches, m_tiles, n_tiles, k_tiles; // batches = phases of this launch; k_tiles = the deepest phase's
    const float* Wt;                        // per phase [m_tiles panels][k_tiles of the phase * 16][bm], zero padded
    const float* in;
    float* out;
    const float* bias;
    int C, K, H, W, Ho, Wo, kh, kw, sh, sw, pt, pl;
    int qy0, qx0, Hq, Wq; // columns are (n, qy - qy0, qx - qx0): qy0 = pt / sh ... qy0 + Hq - 1 = (Ho - 1 + pt) / sh
    int HqWq, Ntot, HW, HoWo;
    int bm, rows; // row tile; rows of the GEMM (PAIR: 2 * round_up(K, 8))
    int has_bias, relu;
    // per batch entry, deepest first
    int ph_py[kMaxPhases], ph_px[kMaxPhases], ph_ntw[kMaxPhases], ph_ktiles[kMaxPhases];
    unsigned ph_woff[kMaxPhases]; // first float of the phase in Wt
};

// PAIR: stride_w == 2 and both x-phases stacked in the rows (see the header comment); else one (py, px) per batch entry, rows = channels
template <bool PAIR>
struct DeconvGemmPolicy
{
    using Params = DeconvGemmParams;
    static constexpr int EXTRA_LDS_FLOATS = 0;
    static __device__ void stage_extra(const Params&, float*, int, int) {}
    static __device__ int row_channel(int m) { return PAIR ? ((m >> 4) << 3) + (m & 7) : m; }
    static __device__ float bias_at(const Params& p, int m)
    {
        const int k = row_channel(m);
        return (p.has_bias && m < p.rows && k < p.K) ? p.bias[k] : 0.f;
    }
    static __device__ int k_count(const Params& p, int batch) { return p.ph_ktiles[batch]; }
    // phase after phase in dispatch order (deepest first); inside a phase consecutive ids share an XCD and walk row tiles fastest
    static __device__ void decode(const Params& p, int& mt, int& nt, int& batch)
    {
        const int per = p.m_tiles * p.n_tiles;
        batch = (int)blockIdx.x / per;
        const int vid = xcd_remap((int)blockIdx.x - batch * per, per);
        mt = vid % p.m_tiles;
        nt = vid / p.m_tiles;
    }

    struct ALoad
    {
        const float* base;
        __device__ ALoad(const Params& p, int batch, int m4)
            : base(p.Wt + p.ph_woff[batch] + (size_t)(m4 / p.bm) * ((size_t)p.ph_ktiles[batch] * kDeconvBK) * p.bm + (m4 % p.bm))
        {
        }
        __device__ float4 load(const Params& p, int krow) const { return *reinterpret_cast<const float4*>(base + (size_t)krow * p.bm); }
    };

    struct BLoad
    {
        typedef float4 Raw;
        const float* ptr[4]; // &in[n][0][qy][qx] of each of the 4 columns (dereferenced only where the tap lands inside the plane)
        int y0[4], x0[4];
        unsigned valid;
        int ntw, rows_k; // x-taps of this phase; reduction rows that hold data
        __device__ BLoad(const Params& p, int batch, int n4)
        {
            valid = 0;
            ntw = p.ph_ntw[batch];
            rows_k = p.ph_ktiles[batch] * kDeconvBK;
#pragma unroll
            for (int e = 0; e < 4; ++e)
            {
                const int col = n4 + e;
                const bool ok = col < p.Ntot;
                const int cc = ok ? col : 0;
                const int img = cc / p.HqWq, rem = cc - img * p.HqWq;
                const int ry = rem / p.Wq;
                y0[e] = ry + p.qy0;
                x0[e] = rem - ry * p.Wq + p.qx0;
                ptr[e] = p.in + ((size_t)img * p.C) * p.HW + (ptrdiff_t)y0[e] * p.W + x0[e];
                valid |= ok ? (1u << e) : 0u;
            }
        }
        __device__ float4 finish(const Params&, const Raw& raw, int, const float*) const { return raw; }
        // Unconditional loads from clamped addresses; `ok` says which of the 4 values are real (see gemm_core.h).
        __device__ Raw load(const Params& p, int krow, unsigned& ok) const
        {
            const int kr = min(krow, rows_k - 1); // (the loop never asks past the phase's own depth; cheap insurance for the address)
            const int t = kr / p.C, c = kr - t * p.C;
            const int ti = t / ntw, tj = t - ti * ntw;
            const ptrdiff_t koff = (ptrdiff_t)c * p.HW - (ptrdiff_t)ti * p.W - tj;
            float v[4];
            ok = 0u;
#pragma unroll
            for (int e = 0; e < 4; ++e)
            {
                const bool in = (valid & (1u << e)) && ((unsigned)(y0[e] - ti) < (unsigned)p.H) && ((unsigned)(x0[e] - tj) < (unsigned)p.W);
                ok |= in ? (1u << e) : 0u;
                v[e] = *(in ? ptr[e] + koff : p.in); // a tap outside the plane reads in[0] and is zeroed at LDS-write time
            }
            return make_float4(v[0], v[1], v[2], v[3]);
        }
    };

    struct Store
    {
        float* ptr[4];   // &out[img][0][oy][ox] of each column (PAIR: of its x-phase 0; x-phase 1 is the next float)
        unsigned valid;  // bit e: column e lands inside the output; PAIR: bit 4 + e the same for x-phase 1
        bool wide;       // PAIR: the 8 floats are one run inside one output row
        mutable float4 held; // PAIR: the x-phase 0 row of this lane's channel, waiting for its x-phase 1 row
        __device__ Store(const Params& p, int batch, int n4)
        {
            const int py = p.ph_py[batch], px = PAIR ? 0 : p.ph_px[batch];
            valid = 0;
            held = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int e = 0; e < 4; ++e)
            {
                const int col = n4 + e;
                const bool ok = col < p.Ntot;
                const int cc = ok ? col : 0;
                const int img = cc / p.HqWq, rem = cc - img * p.HqWq;
                const int ry = rem / p.Wq, rx = rem - ry * p.Wq;
                const int oy = (ry + p.qy0) * p.sh + py - p.pt, ox = (rx + p.qx0) * p.sw + px - p.pl;
                const bool row_ok = ok && oy >= 0 && oy < p.Ho;
                ptr[e] = p.out + ((size_t)img * p.K) * p.HoWo + (ptrdiff_t)oy * p.Wo + ox;
                valid |= (row_ok && ox >= 0 && ox < p.Wo) ? (1u << e) : 0u;
                if (PAIR) valid |= (row_ok && ox + 1 >= 0 && ox + 1 < p.Wo) ? (16u << e) : 0u;
            }
            wide = PAIR && valid == 0xffu && ptr[1] == ptr[0] + 2 && ptr[2] == ptr[0] + 4 && ptr[3] == ptr[0] + 6;
        }
        __device__ float4 residual4(const Params&, int) const { return make_float4(0.f, 0.f, 0.f, 0.f); }
        __device__ void put4(const Params& p, int m, float4 v) const { put4b(p, m, v, bias_at(p, m), residual4(p, m)); }
        __device__ void put4b(const Params& p, int m, float4 v, float b, float4) const
        {
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
            const int k = row_channel(m);
            if (PAIR)
            {
                if (((m >> 3) & 1) == 0)
                {
                    held = v; // rows m and m + 8 reach this lane back to back (gemm_core.h's epilogue: q, q + 1)
                    return;
                }
                if (k >= p.K || m >= p.rows) return;
                const size_t moff = (size_t)k * p.HoWo;
                if (wide)
                {
                    f32x4u lo, hi;
                    lo.x = held.x, lo.y = v.x, lo.z = held.y, lo.w = v.y;
                    hi.x = held.z, hi.y = v.z, hi.z = held.w, hi.w = v.w;
                    *reinterpret_cast<f32x4u*>(ptr[0] + moff) = lo; // 4-byte aligned: one global_store_dwordx4 each
                    *reinterpret_cast<f32x4u*>(ptr[0] + moff + 4) = hi;
                    return;
                }
                if (valid & 1u) ptr[0][moff] = held.x;
                if (valid & 2u) ptr[1][moff] = held.y;
                if (valid & 4u) ptr[2][moff] = held.z;
                if (valid & 8u) ptr[3][moff] = held.w;
                if (valid & 16u) ptr[0][moff + 1] = v.x;
                if (valid & 32u) ptr[1][moff + 1] = v.y;
                if (valid & 64u) ptr[2][moff + 1] = v.z;
                if (valid & 128u) ptr[3][moff + 1] = v.w;
                return;
            }
            if (k >= p.K) return;
            const size_t moff = (size_t)k * p.HoWo;
            if (valid & 1u) ptr[0][moff] = v.x;
            if (valid & 2u) ptr[1][moff] = v.y;
            if (valid & 4u) ptr[2][moff] = v.z;
            if (valid & 8u) ptr[3][moff] = v.w;
        }
    };
};

using DeconvShapeBig = GemmShape<128, 64, 16, 2, 2>;    // >= 128 GEMM rows
using DeconvShapeSmallM = GemmShape<64, 128, 16, 1, 4>; // 64 .. 127 GEMM rows

// kernel [K][C][kh][kw] -> Wt of DeconvGemmParams; one lane per packed word, every word written
template <bool PAIR>
__global__ __launch_bounds__(256) void deconv_pack_mfma_kernel(float* packed, const float* kernel, const DeconvGemmParams p, unsigned total)
{
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= total) return;
    int b = 0;
    while (b + 1 < p.batches && i >= p.ph_woff[b + 1]) ++b;
    unsigned r = i - p.ph_woff[b];
    const int mrow = (int)(r % (unsigned)p.bm);
    r /= (unsigned)p.bm;
    const int depth = p.ph_ktiles[b] * kDeconvBK;
    const int krow = (int)(r % (unsigned)depth), panel = (int)(r / (unsigned)depth);
    const int m = panel * p.bm + mrow;
    const int k = DeconvGemmPolicy<PAIR>::row_channel(m);
    const int px = PAIR ? ((m >> 3) & 1) : p.ph_px[b];
    const int t = krow / p.C, c = krow - t * p.C;
    const int ti = t / p.ph_ntw[b], tj = t - ti * p.ph_ntw[b];
    const int ki = p.ph_py[b] + ti * p.sh, kj = px + tj * p.sw;
    float v = 0.f;
    if (m < p.rows && k < p.K && ki < p.kh && kj < p.kw) v = kernel[(((size_t)k * p.C + c) * p.kh + ki) * p.kw + kj];
    packed[i] = v;
}

// ---- host side ------------------------------------------------------------------------------------------------------

static int out_h(const fhip_deconv_param& p) { return (p.input_h - 1) * p.stride_h + p.kernel_h - p.pad_top - p.pad_bottom + p.output_pad_bottom; }
static int out_w(const fhip_deconv_param& p) { return (p.input_w - 1) * p.stride_w + p.kernel_w - p.pad_left - p.pad_right + p.output_pad_right; }

// Every refusal of a param except the output dims; 0 when the layer is one of this library's.
static int check_geometry(const fhip_deconv_param* p)
{
    const int rc = check_sizes(p);
    if (rc) return rc;
    if (p->pad_left < 0 || p->pad_right < 0 || p->pad_top < 0 || p->pad_bottom < 0) return fail(FHIP_E_BADARG, "negative padding");
    if (p->output_pad_right < 0 || p->output_pad_bottom < 0) return fail(FHIP_E_BADARG, "negative output padding");
    if (p->group < 1 || p->input_channels % p->group) return fail(FHIP_E_BADARG, "input_channels is not divisible by group");
    if (p->output_channels % p->group) return fail(FHIP_E_BADARG, "output_channels (of the whole layer) is not divisible by group");
    if (p->output_pad_bottom >= p->stride_h || p->output_pad_right >= p->stride_w) return fail(FHIP_E_BADARG, "output padding must be smaller than the stride");
    if (p->output_pad_bottom > p->pad_bottom || p->output_pad_right > p->pad_right)
        return fail(FHIP_E_BADARG, "output padding larger than the padding of that side: outputs outside the scatter range are not defined here");
    if (p->activation != FHIP_ACT_NONE && p->activation != FHIP_ACT_RELU) return fail(FHIP_E_BADARG, "activation must be None or ReLU");
    const long long oh = (long long)(p->input_h - 1) * p->stride_h + p->kernel_h - p->pad_top - p->pad_bottom + p->output_pad_bottom;
    const long long ow = (long long)(p->input_w - 1) * p->stride_w + p->kernel_w - p->pad_left - p->pad_right + p->output_pad_right;
    if (oh < 1 || ow < 1 || oh > 0x7fffffffLL || ow > 0x7fffffffLL) return fail(FHIP_E_BADARG, "empty (or absurdly large: 2^31 or more per side) output");
    return FHIP_OK;
}

static int check_param(const fhip_deconv_param* p)
{
    const int rc = check_geometry(p);
    if (rc) return rc;
    if (p->output_h != out_h(*p) || p->output_w != out_w(*p)) return fail(FHIP_E_BADARG, "output_h / output_w are not what fhip_deconv_assign_output_dim gives");
    return FHIP_OK;
}

enum RouteKind
{
    ROUTE_GENERIC,
    ROUTE_MFMA_BIG,
    ROUTE_MFMA_SMALLM,
    ROUTE_MFMA_PAIR_BIG,
    ROUTE_MFMA_PAIR_SMALLM
};

// The one selection function: fhip_deconv_forward launches what it says, fhip_deconv_route reports it, init packs for it.
//   MFMA: group 1, C % 16 == 0 (a k-tile of 16 stays inside one tap), at most 16 phases, and enough GEMM rows for a 64-row tile without
//   padding more than a third of it away: K >= 48 per phase, or K >= 24 with the two x-phases of stride_w == 2 stacked (rows = 2 K).
//   128-row tiles from 96 rows on.  Everything else (grouped, depthwise, C = 3, an RGB head) is the generic kernel's.
static RouteKind select(const fhip_deconv_param& p)
{
    if (p.group != 1 || p.input_channels % kDeconvBK || p.stride_h * p.stride_w > kMaxPhases) return ROUTE_GENERIC;
    const bool pair = p.stride_w == 2;
    const int rows = pair ? 2 * ((p.output_channels + 7) / 8 * 8) : p.output_channels;
    if (rows < 48) return ROUTE_GENERIC;
    if (pair) return rows >= 96 ? ROUTE_MFMA_PAIR_BIG : ROUTE_MFMA_PAIR_SMALLM;
    return rows >= 96 ? ROUTE_MFMA_BIG : ROUTE_MFMA_SMALLM;
}

static const char* route_name(RouteKind r)
{
    switch (r)
    {
    case ROUTE_MFMA_BIG: return "fhip::gemm_mfma_kernel<fhip::GemmShape<128, 64, 16, 2, 2, 4>, fhip::DeconvGemmPolicy<false> >";
    case ROUTE_MFMA_SMALLM: return "fhip::gemm_mfma_kernel<fhip::GemmShape<64, 128, 16, 1, 4, 4>, fhip::DeconvGemmPolicy<false> >";
    case ROUTE_MFMA_PAIR_BIG: return "fhip::gemm_mfma_kernel<fhip::GemmShape<128, 64, 16, 2, 2, 4>, fhip::DeconvGemmPolicy<true> >";
    case ROUTE_MFMA_PAIR_SMALLM: return "fhip::gemm_mfma_kernel<fhip::GemmShape<64, 128, 16, 1, 4, 4>, fhip::DeconvGemmPolicy<true> >";
    default: return "fhip::deconv_generic_kernel<4>";
    }
}

// Everything of DeconvGemmParams that does not depend on the batch or the pointers; returns the packed floats.
static size_t mfma_plan(const fhip_deconv_param& p, RouteKind r, DeconvGemmParams& g)
{
    memset(&g, 0, sizeof(g));
    const bool pair = r == ROUTE_MFMA_PAIR_BIG || r == ROUTE_MFMA_PAIR_SMALLM;
    g.bm = (r == ROUTE_MFMA_BIG || r == ROUTE_MFMA_PAIR_BIG) ? DeconvShapeBig::BM : DeconvShapeSmallM::BM;
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
    g.qy0 = p.pad_top / p.stride_h;
    g.qx0 = p.pad_left / p.stride_w;
    g.Hq = (p.output_h - 1 + p.pad_top) / p.stride_h - g.qy0 + 1;
    g.Wq = (p.output_w - 1 + p.pad_left) / p.stride_w - g.qx0 + 1;
    g.HqWq = g.Hq * g.Wq;
    g.HW = p.input_h * p.input_w;
    g.HoWo = p.output_h * p.output_w;
    g.rows = pair ? 2 * ((g.K + 7) / 8 * 8) : g.K;
    g.m_tiles = (g.rows + g.bm - 1) / g.bm;
    g.has_bias = p.bias_term != 0;
    g.relu = p.activation == FHIP_ACT_RELU;
    // phases, deepest first (a stable order: equal depths keep (py, px) order, so the packing is a function of the param alone)
    struct Ph
    {
        int py, px, ntw, taps;
    } ph[kMaxPhases];
    int n = 0;
    for (int py = 0; py < p.stride_h; ++py)
        for (int px = 0; px < (pair ? 1 : p.stride_w); ++px)
        {
            const int nth = std::max((p.kernel_h - py + p.stride_h - 1) / p.stride_h, 1);
            const int ntw = std::max((p.kernel_w - px + p.stride_w - 1) / p.stride_w, 1); // PAIR: px = 0 has the most x-taps
            ph[n++] = Ph{py, px, ntw, nth * ntw};
        }
    std::stable_sort(ph, ph + n, [](const Ph& a, const Ph& b) { return a.taps > b.taps; });
    g.batches = n;
    size_t off = 0;
    for (int i = 0; i < n; ++i)
    {
        g.ph_py[i] = ph[i].py;
        g.ph_px[i] = ph[i].px;
        g.ph_ntw[i] = ph[i].ntw;
        g.ph_ktiles[i] = ph[i].taps * g.C / kDeconvBK; // C % 16 == 0
        g.ph_woff[i] = (unsigned)off;
        off += (size_t)g.m_tiles * g.bm * g.ph_ktiles[i] * kDeconvBK;
    }
    g.k_tiles = g.ph_ktiles[0];
    return off;
}

static size_t packed_floats(const fhip_deconv_param& p)
{
    const RouteKind r = select(p);
    if (r == ROUTE_GENERIC) return generic_packed_floats(p, kGenericKT);
    DeconvGemmParams g;
    return mfma_plan(p, r, g);
}

template <class Shape, bool PAIR>
static void launch_mfma(DeconvGemmParams& g, hipStream_t s)
{
    g.n_tiles = (g.Ntot + Shape::BN - 1) / Shape::BN;
    const unsigned grid = (unsigned)(g.batches * g.m_tiles * g.n_tiles);
    hipLaunchKernelGGL((gemm_mfma_kernel<Shape, DeconvGemmPolicy<PAIR>>), dim3(grid), dim3(Shape::THREADS), 0, s, g);
}

} // namespace fhip

using namespace fhip;

extern "C"
{

int fhip_deconv_assign_output_dim(fhip_deconv_param* param)
{
    if (!param) return fail(FHIP_E_BADARG, "null param");
    if (param->input_h < 1 || param->input_w < 1 || param->stride_h < 1 || param->stride_w < 1 || param->kernel_h < 1 || param->kernel_w < 1)
        return fail(FHIP_E_BADARG, "input size, kernel size and stride must be >= 1");
    const long long oh = (long long)(param->input_h - 1) * param->stride_h + param->kernel_h - param->pad_top - param->pad_bottom + param->output_pad_bottom;
    const long long ow = (long long)(param->input_w - 1) * param->stride_w + param->kernel_w - param->pad_left - param->pad_right + param->output_pad_right;
    if (oh < 1 || ow < 1 || oh > 0x7fffffffLL || ow > 0x7fffffffLL) return fail(FHIP_E_BADARG, "empty (or absurdly large: 2^31 or more per side) output");
    param->output_h = (int)oh;
    param->output_w = (int)ow;
    return FHIP_OK;
}

int fhip_deconv_supported(const fhip_deconv_param* param) { return check_param(param) == FHIP_OK ? 1 : 0; }

int fhip_deconv_get_buffer_size(const fhip_deconv_param* param, int batch, size_t* scratch_bytes, size_t* packed_bytes)
{
    const int rc = check_param(param);
    if (rc) return rc;
    if (batch < 1 || !scratch_bytes || !packed_bytes) return fail(FHIP_E_BADARG, "batch < 1 or a null size pointer");
    *scratch_bytes = 0;
    *packed_bytes = packed_floats(*param) * sizeof(float);
    return FHIP_OK;
}

int fhip_deconv_init(const fhip_deconv_param* param, float* packed, const float* kernel, void* stream)
{
    const int rc = check_param(param);
    if (rc) return rc;
    if (!packed || !kernel) return fail(FHIP_E_BADARG, "null packed / kernel");
    if (!aligned(packed, 16) || !aligned(kernel, 4)) return fail(FHIP_E_BADARG, "packed must be 16-byte aligned, kernel 4-byte aligned");
    const fhip_deconv_param& p = *param;
    const RouteKind r = select(p);
    const size_t total = packed_floats(p);
    if (total > 0x7fffffffULL) return fail(FHIP_E_BADARG, "filter tensor too large: 2^31 packed floats or more");
    const dim3 grid((unsigned)((total + 255) / 256));
    if (r == ROUTE_GENERIC)
        launch_direct_pack(deconv_pack_generic_kernel, p, kGenericKT, total, packed, kernel, (hipStream_t)stream);
    else
    {
        DeconvGemmParams g;
        mfma_plan(p, r, g);
        if (r == ROUTE_MFMA_PAIR_BIG || r == ROUTE_MFMA_PAIR_SMALLM)
            hipLaunchKernelGGL(deconv_pack_mfma_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, packed, kernel, g, (unsigned)total);
        else
            hipLaunchKernelGGL(deconv_pack_mfma_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, packed, kernel, g, (unsigned)total);
    }
    FHIP_CHECK_HIP(hipGetLastError());
    return FHIP_OK;
}

int fhip_deconv_forward(const fhip_deconv_param* param, int batch, float* out, const float* in, const float* packed, float* /*scratch*/,
                        const float* bias, void* stream)
{
    int rc = check_param(param);
    if (rc) return rc;
    const fhip_deconv_param& p = *param;
    rc = check_forward_pointers(p, batch, out, in, packed, bias, 16, "device pointers must be 4-byte aligned (packed: 16-byte)");
    if (rc) return rc;
    const unsigned long long in_count = (unsigned long long)batch * p.input_channels * p.input_h * p.input_w;
    const unsigned long long out_count = (unsigned long long)batch * p.output_channels * p.output_h * p.output_w;
    if (in_count > 0x7fffffffULL || out_count > 0x7fffffffULL) return fail(FHIP_E_BADARG, "tensor too large: 2^31 elements or more");
    const RouteKind r = select(p);
    if (r == ROUTE_GENERIC)
    {
        DirectConvArgs a = direct_conv_args(p, kGenericKT, out, in, packed, bias);
        rc = launch_direct(deconv_generic_kernel<kGenericKT>, a, (size_t)batch * p.output_h * p.output_w, (size_t)p.group * a.chunks, (hipStream_t)stream,
                           "more than 65535 chunks of 4 output channels");
        if (rc) return rc;
    }
    else
    {
        DeconvGemmParams g;
        mfma_plan(p, r, g);
        g.Wt = packed;
        g.in = in;
        g.out = out;
        g.bias = p.bias_term ? bias : nullptr;
        const unsigned long long ntot = (unsigned long long)batch * g.HqWq;
        if (ntot > 0x3fffffffULL) return fail(FHIP_E_BADARG, "tensor too large: 2^30 GEMM columns or more");
        g.Ntot = (int)ntot;
        switch (r)
        {
        case ROUTE_MFMA_BIG: launch_mfma<DeconvShapeBig, false>(g, (hipStream_t)stream); break;
        case ROUTE_MFMA_SMALLM: launch_mfma<DeconvShapeSmallM, false>(g, (hipStream_t)stream); break;
        case ROUTE_MFMA_PAIR_BIG: launch_mfma<DeconvShapeBig, true>(g, (hipStream_t)stream); break;
        default: launch_mfma<DeconvShapeSmallM, true>(g, (hipStream_t)stream); break;
        }
    }
    FHIP_CHECK_HIP(hipGetLastError());
    return FHIP_OK;
}

int fhip_deconv_route(const fhip_deconv_param* param, char* name, int len)
{
    const int rc = check_param(param);
    if (rc) return rc;
    if (!name || len < 1) return fail(FHIP_E_BADARG, "null name");
    snprintf(name, (size_t)len, "%s", route_name(select(*param)));
    return FHIP_OK;
}

const char* fhip_deconv_last_error(void) { return last_error(); }

} // extern "C"
