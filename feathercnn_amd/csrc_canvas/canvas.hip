// libfeather_canvas.so: the chained Winograd F(6x6,3x3) transforms of layers that run on 2x2 image canvases
// (include/feather_hip/feather_canvas.h is the contract; DESIGN.md 3.16 the design and its measurements).
//
// canvas_chain_kernel is csrc/winograd_f63.hip's wino_chain_kernel -- persistent blocks that walk units of ppb planes, phase 1 = A^T m A
// (+ bias, ReLU, pooling) of the producer's tiles into a zero-bordered LDS plane, the next unit's 64 M values per lane requested behind the
// barrier, phase 2 = B^T d B of the consumer's 8 x 8 windows out of the LDS -- with a "plane" that is a canvas: four images of one channel.
// Only the index arithmetic between the two phases differs per form; the butterflies are csrc/wino_butterfly.h's, so every value equals
// the plain kernels'.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <string>

#include "feather_hip/feather_canvas.h"
#include "side_error.h"
#include "wino_butterfly.h"
#include "wino_layout.h"

namespace fhip
{

struct CanvasChain
{
    int K, NC;        // channels of the plane set (the producer's output channels), canvases (batch / 4)
    int TX, T, Tq;    // producer: tiles per row (ENTRY: of an image, else of a canvas), tiles per canvas (ENTRY: 4 * Tq), ENTRY: tiles per image
    int IH;           // side of one image as the consumer sees it (behind the pooling of ENTRY and EXIT)
    int QP;           // distance of two quadrants in those pixels: IH + 2 (EXIT: IH + 1, the pooled seam is one pixel)
    int TX2, T2, T2q; // consumer: tiles per row (EXIT: of an image, else of a canvas), tiles per canvas (EXIT: 4 * T2q), EXIT: tiles per image
    int planes, ppb;  // K * NC canvases, canvas index fastest; canvases per block
    int LDW, LDH;     // LDS plane the consumer's windows are read from: a canvas (EXIT: ONE image) + border, as wino_chain_kernel's
    int sub, pf;      // floats of that plane; floats per canvas (EXIT: four of them, one per quadrant; else pf == sub)
    WinoLayout Lm, Lv2;
};

// FORM (fhip_canvas_form): ENTRY and EXIT pool, INSIDE does not.  MULTI: a canvas with more producer tiles than the block has lanes (ENTRY
// from 112-pixel images: 4 * 361), the lane's tiles are tid, tid + blockDim, ...
template <bool HAS_BIAS, bool RELU, int FORM, bool MULTI>
__global__ __launch_bounds__(512, 3) void canvas_chain_kernel(float* __restrict__ Vn, const float* __restrict__ M, const float* __restrict__ bias,
                                                              const CanvasChain g, const int units)
{
    extern __shared__ __attribute__((aligned(16))) float smem[]; // [ppb][pf]
    const int tid = threadIdx.x, nthreads = blockDim.x;
    // phase 1 writes the images' pixels (ENTRY, INSIDE: and zeros on the seam and beyond the images where its tiles reach) and nothing else:
    // the consumer's padding, the seam of an ENTRY canvas and the borders of the EXIT images are zeroed once per block
    for (int i = tid; i < g.ppb * g.pf; i += nthreads) smem[i] = 0.f;
    const int n1 = MULTI ? (g.T + nthreads - 1) / nthreads : 1;
    int pl = MULTI ? 0 : tid / g.T, t = tid - pl * g.T; // phase 1: the producer's tile t of canvas pl of the unit
    bool lane_on = MULTI ? t < g.T : pl < g.ppb;
    const int pl2 = tid / g.T2, t2 = tid - pl2 * g.T2; // phase 2: the consumer's tile
    const bool lane_on2 = pl2 < g.ppb;
    const int q2 = FORM == FHIP_CANVAS_EXIT ? t2 / g.T2q : 0, tt2 = t2 - q2 * g.T2q;
    const int ty2 = tt2 / g.TX2, tx2 = tt2 - ty2 * g.TX2;
    // unit order: as wino_chain_kernel (the XCD blockIdx % 8 owns a contiguous eighth of the units)
    const int xcd = blockIdx.x & 7, j = blockIdx.x >> 3, xcd_blocks = (gridDim.x + 7 - xcd) >> 3;
    const int u_lo = (int)((long long)units * xcd / 8), u_hi = (int)((long long)units * (xcd + 1) / 8);
    const size_t xi_stride = g.Lm.xis, xi_stride2 = g.Lv2.xis;
    float* const lp1 = smem + pl * g.pf;

    float m[8][8];
    auto fetch = [&](int unit, int tile) {
        // clamped and unconditional (a load under a branch is waited for on the spot).  The tiles of a canvas are consecutive columns in
        // every form: ENTRY's four images are n = 4c .. 4c + 3, whose columns n * Tq + t are c * T + (q * Tq + t)
        const int plane = min(unit * g.ppb + (lane_on ? pl : 0), g.planes - 1);
        const int k = plane / g.NC, c = plane - k * g.NC;
        const float* mp = M + (size_t)k * g.Lm.bp + g.Lm.col(c * g.T + min(tile, g.T - 1));
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) m[i][jj] = mp[(size_t)(i * 8 + jj) * xi_stride];
    };
    int unit = u_lo + j;
    if (unit < u_hi) fetch(unit, t);
    __syncthreads();
    for (; unit < u_hi; unit += xcd_blocks)
    {
        const int plane = unit * g.ppb + pl;
        const int k = min(plane, g.planes - 1) / g.NC;
        // ---- phase 1: the producer's tiles -> activation canvas(es) in LDS
        for (int it = 0; it < n1; ++it)
        {
            if (MULTI)
            {
                t = tid + it * nthreads;
                lane_on = t < g.T;
            }
            if (lane_on && plane < g.planes)
            {
                const int q = FORM == FHIP_CANVAS_ENTRY ? t / g.Tq : 0, tt = t - q * g.Tq; // ENTRY: the image (quadrant) this tile belongs to
                const int ty = tt / g.TX, tx = tt - ty * g.TX;
                float tmp[6][8];
#pragma unroll
                for (int jj = 0; jj < 8; ++jj)
                    at6(m[0][jj], m[1][jj], m[2][jj], m[3][jj], m[4][jj], m[5][jj], m[6][jj], m[7][jj], tmp[0][jj], tmp[1][jj], tmp[2][jj], tmp[3][jj],
                        tmp[4][jj], tmp[5][jj]);
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
                    if (FORM != FHIP_CANVAS_INSIDE)
                    {
                        // images and the seam are even: a 2x2 cell never straddles an image edge
                        const float h0 = fmaxf(y[0], y[1]), h1 = fmaxf(y[2], y[3]), h2 = fmaxf(y[4], y[5]);
                        if ((a & 1) == 0)
                        {
                            prev0 = h0;
                            prev1 = h1;
                            prev2 = h2;
                            continue;
                        }
                        const float pv[3] = {fmaxf(prev0, h0), fmaxf(prev1, h1), fmaxf(prev2, h2)};
                        const int py = 3 * ty + (a >> 1);
                        if (FORM == FHIP_CANVAS_ENTRY)
                        {
                            // the image's pooled pixel (py, 3tx + c) -> canvas pixel (py + (q / 2) QP, 3tx + c + (q % 2) QP); what the image's
                            // last tiles compute beyond it lands on the seam or the border and is written as zero
                            if (py < g.IH)
                            {
                                float* row = lp1 + (size_t)(py + 1 + (q >> 1) * g.QP) * g.LDW + 2 + 3 * tx + (q & 1) * g.QP;
#pragma unroll
                                for (int c = 0; c < 3; ++c) row[c] = (3 * tx + c < g.IH) ? pv[c] : 0.f;
                            }
                        }
                        else
                        {
                            // EXIT: the canvas's pooled pixel (py, px) is pixel (py - qy QP, px - qx QP) of quadrant (qy, qx), or seam
                            const int qy = py >= g.QP ? 1 : 0, yy = py - qy * g.QP;
                            if (yy < g.IH)
                            {
#pragma unroll
                                for (int c = 0; c < 3; ++c)
                                {
                                    const int px = 3 * tx + c, qx = px >= g.QP ? 1 : 0, xx = px - qx * g.QP;
                                    if (xx < g.IH) lp1[(size_t)(2 * qy + qx) * g.sub + (size_t)(yy + 1) * g.LDW + 2 + xx] = pv[c];
                                }
                            }
                        }
                        continue;
                    }
                    // INSIDE: the canvas is whole tiles (2 IH + 2 = 6 TX); rows and columns IH, IH + 1 are the seam
                    const int ay = 6 * ty + a;
                    const bool row_seam = (unsigned)(ay - g.IH) < 2u;
                    float* row = lp1 + (size_t)(ay + 1) * g.LDW + 2 + 6 * tx; // even offset: 8-byte aligned pairs
#pragma unroll
                    for (int bb = 0; bb < 6; bb += 2)
                    {
                        const bool seam = row_seam || (unsigned)(6 * tx + bb - g.IH) < 2u; // IH even: a pair is inside or outside as a whole
                        *reinterpret_cast<float2*>(row + bb) = seam ? make_float2(0.f, 0.f) : make_float2(y[bb], y[bb + 1]);
                    }
                }
            }
            if (MULTI && it + 1 < n1) fetch(unit, tid + (it + 1) * nthreads);
        }
        __syncthreads();
        // ---- the next unit's tiles: in flight through phase 2
        if (unit + xcd_blocks < u_hi) fetch(unit + xcd_blocks, MULTI ? tid : t);
        __builtin_amdgcn_sched_barrier(0); // hipcc would sink the loads to their uses
        // ---- phase 2: the consumer's tiles (EXIT: tile tt2 of image q2, read from that quadrant's own plane), as wino_chain_kernel
        const int plane2 = unit * g.ppb + pl2;
        if (lane_on2 && plane2 < g.planes)
        {
            const int k2 = plane2 / g.NC, c2 = plane2 - k2 * g.NC;
            const float* lp = smem + (size_t)pl2 * g.pf + (size_t)q2 * g.sub + (size_t)(6 * ty2) * g.LDW + 6 * tx2 + 1;
            float d[8][8];
#pragma unroll
            for (int i = 0; i < 8; ++i)
#pragma unroll
                for (int jj = 0; jj < 8; ++jj) d[i][jj] = lp[(size_t)i * g.LDW + jj];
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) bt8(d[0][jj], d[1][jj], d[2][jj], d[3][jj], d[4][jj], d[5][jj], d[6][jj], d[7][jj]);
#pragma unroll
            for (int i = 0; i < 8; ++i) bt8(d[i][0], d[i][1], d[i][2], d[i][3], d[i][4], d[i][5], d[i][6], d[i][7]);
            float* vp = Vn + (size_t)k2 * g.Lv2.bp + g.Lv2.col(c2 * g.T2 + t2);
#pragma unroll
            for (int i = 0; i < 8; ++i)
#pragma unroll
                for (int jj = 0; jj < 8; ++jj) vp[(size_t)(i * 8 + jj) * xi_stride2] = d[i][jj];
        }
        __syncthreads(); // the windows are read: the next phase 1 may overwrite the planes
    }
}

// The last layer of a canvas run: Y = A^T m A, + bias, ReLU [, 2x2 max pooling], one tile per lane with lanes along the column index (the 64
// M loads of a wave are coalesced rows), every value stored to its image: canvas pixel (y, x) is pixel (y - qy QP, x - qx QP) of image
// 4 c + 2 qy + qx, or seam.  (VGG-16: conv5_3's pooled 7 x 7 planes, 3.2 MB of output behind 26 MB of M.)
struct CanvasOut
{
    int K, T, TX, P; // channels, tiles per canvas, tiles per row, columns = canvases * T
    int IH, QP;      // image side and quadrant distance in OUTPUT pixels (pooled: H / 2 and H / 2 + 1, else H and H + 2)
    WinoLayout Lm;
};

template <bool HAS_BIAS, bool RELU, bool POOL>
__global__ __launch_bounds__(256) void canvas_output_kernel(float* __restrict__ out, const float* __restrict__ M, const float* __restrict__ bias,
                                                            const CanvasOut g)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    const int k = blockIdx.y;
    if (p >= g.P) return;
    const int c = p / g.T, t = p - c * g.T;
    const int ty = t / g.TX, tx = t - ty * g.TX;
    const size_t xi_stride = g.Lm.xis;
    const float* mp = M + (size_t)k * g.Lm.bp + g.Lm.col(p);
    float m[8][8];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) m[i][jj] = mp[(size_t)(i * 8 + jj) * xi_stride];
    float tmp[6][8];
#pragma unroll
    for (int jj = 0; jj < 8; ++jj)
        at6(m[0][jj], m[1][jj], m[2][jj], m[3][jj], m[4][jj], m[5][jj], m[6][jj], m[7][jj], tmp[0][jj], tmp[1][jj], tmp[2][jj], tmp[3][jj], tmp[4][jj],
            tmp[5][jj]);
    const float b = HAS_BIAS ? bias[k] : 0.f;
    const size_t plane = (size_t)g.IH * g.IH;
    float* const op = out + ((size_t)(4 * c) * g.K + k) * plane; // image 4c; image 4c + q is q * K planes further
    auto put = [&](int y, int x, float v) {
        const int qy = y >= g.QP ? 1 : 0, yy = y - qy * g.QP, qx = x >= g.QP ? 1 : 0, xx = x - qx * g.QP;
        if (yy < g.IH && xx < g.IH) op[(size_t)(2 * qy + qx) * g.K * plane + (size_t)yy * g.IH + xx] = v;
    };
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
            const float h0 = fmaxf(y[0], y[1]), h1 = fmaxf(y[2], y[3]), h2 = fmaxf(y[4], y[5]);
            if ((a & 1) == 0)
            {
                prev0 = h0;
                prev1 = h1;
                prev2 = h2;
            }
            else
            {
                const int py = 3 * ty + (a >> 1);
                put(py, 3 * tx, fmaxf(prev0, h0));
                put(py, 3 * tx + 1, fmaxf(prev1, h1));
                put(py, 3 * tx + 2, fmaxf(prev2, h2));
            }
            continue;
        }
#pragma unroll
        for (int bb = 0; bb < 6; ++bb) put(6 * ty + a, 6 * tx + bb, y[bb]);
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

static bool k3s1p1(const fhip_conv_param& c)
{
    return c.kernel_h == 3 && c.kernel_w == 3 && c.stride_h <= 1 && c.stride_w <= 1 && c.group <= 1 && c.pad_left == 1 && c.pad_right == 1 &&
           c.pad_top == 1 && c.pad_bottom == 1 && c.input_h == c.input_w && c.output_h == c.input_h && c.output_w == c.input_w;
}

// is `pl` the F(6,3) plan of a pad-1 image of `side` pixels at `images` images?
static bool plan_is(const fhip_winograd_plan& pl, int side, int images)
{
    const int tiles = (side + 2 + 3) / 6;
    return pl.frequency_points == 64 && pl.tiles_x == tiles && pl.tiles_y == tiles && pl.tiles_per_image == tiles * tiles &&
           (long long)pl.columns == (long long)tiles * tiles * images && pl.columns_padded >= pl.columns && pl.column_block > 0;
}

static int canvas_chain(int form, const fhip_conv_param& p, const fhip_conv_param& next, int batch, const fhip_winograd_plan& pp,
                        const fhip_winograd_plan& pn, float* vn, const float* m, const float* bias, hipStream_t s)
{
    if (batch < 4 || (batch & 3)) return fail(FHIP_E_UNSUPPORTED, "canvases hold four images: the batch must be a multiple of 4");
    if (!k3s1p1(p) || !k3s1p1(next) || next.input_channels != p.output_channels)
        return fail(FHIP_E_UNSUPPORTED, "canvas layers are square 3x3 / stride-1 / pad-1 convolutions that follow each other");
    if (p.activation != FHIP_ACT_NONE && p.activation != FHIP_ACT_RELU) return fail(FHIP_E_UNSUPPORTED, "activation other than none / ReLU");
    const bool has_bias = p.bias_term != 0, relu = p.activation == FHIP_ACT_RELU;
    if (has_bias && !bias) return fail(FHIP_E_BADARG, "bias_term set but bias is NULL");
    const int H = p.output_h, IH = next.input_h, nc = batch / 4;
    if (IH < 2 || (IH & 1)) return fail(FHIP_E_UNSUPPORTED, "canvas images have an even side");
    CanvasChain g;
    g.K = p.output_channels;
    g.NC = nc;
    g.IH = IH;
    g.QP = IH + 2;
    bool ok;
    switch (form)
    {
        case FHIP_CANVAS_ENTRY: // plain H = 2 IH -> pool -> canvas of IH
            ok = H == 2 * IH && (2 * IH + 2) % 6 == 0 && plan_is(pp, H, batch) && plan_is(pn, 2 * IH + 2, nc);
            g.Tq = pp.tiles_per_image;
            g.T = 4 * g.Tq;
            g.T2q = g.T2 = pn.tiles_per_image;
            break;
        case FHIP_CANVAS_INSIDE: // canvas of IH -> canvas of IH
            ok = H == IH && (2 * IH + 2) % 6 == 0 && plan_is(pp, 2 * IH + 2, nc) && plan_is(pn, 2 * IH + 2, nc);
            g.Tq = g.T = pp.tiles_per_image;
            g.T2q = g.T2 = pn.tiles_per_image;
            break;
        case FHIP_CANVAS_EXIT: // canvas of H = 2 IH -> pool -> plain IH
            ok = H == 2 * IH && (2 * H + 2) % 6 == 0 && plan_is(pp, 2 * H + 2, nc) && plan_is(pn, IH, batch);
            g.QP = IH + 1;
            g.Tq = g.T = pp.tiles_per_image;
            g.T2q = pn.tiles_per_image;
            g.T2 = 4 * g.T2q;
            break;
        default: return fail(FHIP_E_BADARG, "unknown canvas form");
    }
    if (!ok) return fail(FHIP_E_BADARG, "the geometries or plans do not belong to this canvas form (fhip_winograd_f63_plan_canvas)");
    g.TX = pp.tiles_x;
    g.TX2 = pn.tiles_x;
    g.Lm = wino_layout(g.K, pp.columns_padded, pp.column_block);
    g.Lv2 = wino_layout(g.K, pn.columns_padded, pn.column_block);
    const long long planes = (long long)nc * g.K;
    if (planes > 0x7fffffffLL) return fail(FHIP_E_BADARG, "N*K too large: 2^31 canvas planes or more");
    g.planes = (int)planes;
    g.LDH = 6 * pn.tiles_y + 2;
    g.LDW = 6 * pn.tiles_x + 4;
    g.sub = g.LDH * g.LDW;
    g.pf = form == FHIP_CANVAS_EXIT ? 4 * g.sub : g.sub;
    const size_t plane_bytes = (size_t)g.pf * sizeof(float);
    if (plane_bytes > 64 * 1024) return fail(FHIP_E_UNSUPPORTED, "the canvas does not fit a block's LDS");
    // one tile per lane, as many canvases per block as 256 lanes and 48 KB of LDS take (wino_chain_kernel's rule)
    const int work = std::max(g.T, g.T2);
    int ppb = std::max(1, 256 / work);
    ppb = (int)std::min<size_t>(ppb, std::max<size_t>(1, (48 * 1024) / plane_bytes));
    g.ppb = (int)std::min<long long>(ppb, planes);
    const bool multi = work > 512;
    if (multi && form != FHIP_CANVAS_ENTRY) return fail(FHIP_E_UNSUPPORTED, "a canvas of more than 512 tiles");
    const unsigned threads = std::max(256u, (unsigned)((multi ? g.T2 : work) + 63) / 64 * 64);
    if (threads > 512u) return fail(FHIP_E_UNSUPPORTED, "the consumer's canvas has more than 512 tiles");
    const size_t lds = plane_bytes * g.ppb;
    const long long units = (planes + g.ppb - 1) / g.ppb;
    int cus;
    size_t dev_lds;
    if (const int rc = device_limits(&cus, &dev_lds)) return rc;
    const int bpc = std::max(1, std::min((int)(dev_lds / lds), 12 / (int)(threads / 64)));
    const unsigned grid = ((unsigned)std::min<long long>(units, (long long)cus * bpc) + 7u) & ~7u;
#define FHIP_CANVAS_LAUNCH(F_, M_)                                                                                                             \
    do                                                                                                                                         \
    {                                                                                                                                          \
        if (has_bias && relu) hipLaunchKernelGGL((canvas_chain_kernel<true, true, F_, M_>), dim3(grid), dim3(threads), lds, s, vn, m, bias, g, (int)units); \
        else if (has_bias) hipLaunchKernelGGL((canvas_chain_kernel<true, false, F_, M_>), dim3(grid), dim3(threads), lds, s, vn, m, bias, g, (int)units);   \
        else if (relu) hipLaunchKernelGGL((canvas_chain_kernel<false, true, F_, M_>), dim3(grid), dim3(threads), lds, s, vn, m, bias, g, (int)units);       \
        else hipLaunchKernelGGL((canvas_chain_kernel<false, false, F_, M_>), dim3(grid), dim3(threads), lds, s, vn, m, bias, g, (int)units);                \
    } while (0)
    if (form == FHIP_CANVAS_ENTRY && multi) FHIP_CANVAS_LAUNCH(FHIP_CANVAS_ENTRY, true);
    else if (form == FHIP_CANVAS_ENTRY) FHIP_CANVAS_LAUNCH(FHIP_CANVAS_ENTRY, false);
    else if (form == FHIP_CANVAS_INSIDE) FHIP_CANVAS_LAUNCH(FHIP_CANVAS_INSIDE, false);
    else FHIP_CANVAS_LAUNCH(FHIP_CANVAS_EXIT, false);
#undef FHIP_CANVAS_LAUNCH
    FHIP_CHECK_HIP(hipGetLastError());
    return FHIP_OK;
}

static int canvas_output(const fhip_conv_param& p, int batch, const fhip_winograd_plan& pl, float* out, const float* m, const float* bias, int pool,
                         hipStream_t s)
{
    if (batch < 4 || (batch & 3)) return fail(FHIP_E_UNSUPPORTED, "canvases hold four images: the batch must be a multiple of 4");
    if (!k3s1p1(p)) return fail(FHIP_E_UNSUPPORTED, "canvas layers are square 3x3 / stride-1 / pad-1 convolutions");
    if (p.activation != FHIP_ACT_NONE && p.activation != FHIP_ACT_RELU) return fail(FHIP_E_UNSUPPORTED, "activation other than none / ReLU");
    const bool has_bias = p.bias_term != 0, relu = p.activation == FHIP_ACT_RELU;
    if (has_bias && !bias) return fail(FHIP_E_BADARG, "bias_term set but bias is NULL");
    const int H = p.output_h, nc = batch / 4;
    if (H < 2 || (H & 1) || (2 * H + 2) % 6 != 0 || !plan_is(pl, 2 * H + 2, nc))
        return fail(FHIP_E_BADARG, "the geometry or plan is not a canvas layer's (fhip_winograd_f63_plan_canvas)");
    if (p.output_channels > 65535) return fail(FHIP_E_UNSUPPORTED, "more than 65535 output channels");
    CanvasOut g;
    g.K = p.output_channels;
    g.T = pl.tiles_per_image;
    g.TX = pl.tiles_x;
    g.P = pl.columns;
    g.IH = pool ? H / 2 : H;
    g.QP = pool ? H / 2 + 1 : H + 2;
    g.Lm = wino_layout(g.K, pl.columns_padded, pl.column_block);
    const dim3 grid((unsigned)((g.P + 255) / 256), (unsigned)g.K);
#define FHIP_CANVAS_OUT(P_)                                                                                                     \
    do                                                                                                                          \
    {                                                                                                                           \
        if (has_bias && relu) hipLaunchKernelGGL((canvas_output_kernel<true, true, P_>), grid, dim3(256), 0, s, out, m, bias, g); \
        else if (has_bias) hipLaunchKernelGGL((canvas_output_kernel<true, false, P_>), grid, dim3(256), 0, s, out, m, bias, g);   \
        else if (relu) hipLaunchKernelGGL((canvas_output_kernel<false, true, P_>), grid, dim3(256), 0, s, out, m, bias, g);       \
        else hipLaunchKernelGGL((canvas_output_kernel<false, false, P_>), grid, dim3(256), 0, s, out, m, bias, g);                \
    } while (0)
    if (pool) FHIP_CANVAS_OUT(true);
    else FHIP_CANVAS_OUT(false);
#undef FHIP_CANVAS_OUT
    FHIP_CHECK_HIP(hipGetLastError());
    return FHIP_OK;
}

} // namespace fhip

extern "C"
{

int fhip_canvas_output_to_next_input(int form, const fhip_conv_param* param, const fhip_conv_param* next, int batch, const fhip_winograd_plan* plan,
                                     const fhip_winograd_plan* plan_next, float* v_next, const float* m, const float* bias, void* stream)
{
    if (!param || !next || !plan || !plan_next || !v_next || !m) return fhip::fail(FHIP_E_BADARG, "bad argument");
    return fhip::canvas_chain(form, *param, *next, batch, *plan, *plan_next, v_next, m, bias, (hipStream_t)stream);
}

int fhip_canvas_output_transform(const fhip_conv_param* param, int batch, const fhip_winograd_plan* plan, float* output, const float* m,
                                 const float* bias, int pool, void* stream)
{
    if (!param || !plan || !output || !m) return fhip::fail(FHIP_E_BADARG, "bad argument");
    return fhip::canvas_output(*param, batch, *plan, output, m, bias, pool, (hipStream_t)stream);
}

const char* fhip_canvas_last_error(void) { return fhip::last_error(); }

} // extern "C"
