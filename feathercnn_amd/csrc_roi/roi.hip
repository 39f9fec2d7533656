// libfeather_roi.so: the layers of a two-stage detector on gfx950 (include/feather_hip/feather_roi.h is the contract and the definition;
// DESIGN.md 3.26 the design and its measurements).
//
//   proposal_key_kernel       one lane per (image, anchor, cell), plane reads coalesced across the cells: decodes the anchor's box, clips it,
//                             tests the minimum size and writes the anchor's 64-bit key (score bits, inverted index), 0 when it is no
//                             candidate: no compaction, no atomic, nothing to clear
//   proposal_select_kernel    a block per image, in rounds: the FHIP_ROI_CHUNK best keys below the previous round's last are gathered chunk by
//                             chunk into an LDS buffer of 2 * FHIP_ROI_CHUNK keys (an LDS counter gives the slots, the bitonic sort the order),
//                             their boxes alone are decoded again into LDS (the same device function: the same bits), tested against the boxes
//                             kept in earlier rounds and then greedily among themselves (a barrier per kept box); kept boxes stay in LDS (32 KiB
//                             at FHIP_ROI_MAX_ROIS); the block is 1024 lanes wide: one image is one block; ends when after_nms_topN are kept,
//                             pre_nms_topN candidates were taken or a round saw no more keys than it took; writes every row, the sentinel
//                             rows included
//   roi_pool_kernel, roi_align_kernel<V>, psroi_pool_kernel    one output element per lane, pooled_w fastest: coalesced stores, the ROI's four
//                             values broadcast from cache
//
// Contraction is off for the whole file: every product and sum is rounded on its own, as the header defines.
#include <float.h>
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <string>

#include "feather_hip/feather_roi.h"
#include "side_error.h"

#pragma clang fp contract(off)

namespace fhip
{

typedef unsigned long long u64;

constexpr int kChunk = FHIP_ROI_CHUNK;
constexpr int kKeys = 2 * kChunk; // keys of the selection buffer: the kept ones and a chunk's candidates
constexpr unsigned kIndexMask = FHIP_ROI_MAX_CELLS - 1;
constexpr int kThreads = 1024;    // lanes of the selection block: one image is one block, so the block is as wide as a block gets
static_assert(kChunk % kThreads == 0 && (kKeys & (kKeys - 1)) == 0, "a chunk is whole passes of the block, the buffer a power of two");

struct ProposalArgs
{
    const float *score, *bbox, *im_info;
    float anchors[FHIP_ROI_MAX_ANCHORS][4];
    int A, h, w, feat_stride, pre, rows;
    float nms_thresh, min_size;
};

// a float as an unsigned that orders the same way (NaN never gets here)
__device__ __forceinline__ unsigned ordered(float f)
{
    const unsigned b = f == 0.f ? 0u : __float_as_uint(f); // -0.f is 0.f
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ __forceinline__ float clip(float v, float hi) { return v < 0.f ? 0.f : (v > hi ? hi : v); }

// the box and the score of anchor index r = (q * h + i) * w + j of image img; -> whether it is a candidate
__device__ __forceinline__ bool decode(const ProposalArgs& g, unsigned img, unsigned r, float* box, float* score)
{
    const unsigned hw = (unsigned)g.h * (unsigned)g.w, q = r / hw, cell = r - q * hw, i = cell / (unsigned)g.w, j = cell - i * (unsigned)g.w;
    const float s = g.score[((size_t)img * 2 * g.A + g.A + q) * hw + cell];
    const float* d = g.bbox + ((size_t)img * 4 * g.A + 4 * q) * hw + cell;
    const float dx = d[0], dy = d[hw], dw = d[(size_t)2 * hw], dh = d[(size_t)3 * hw];
    const float* info = g.im_info + (size_t)img * 3;
    const float im_h = info[0], im_w = info[1], min_box = g.min_size * info[2];
    const float* a = g.anchors[q];
    const float ax = a[0] + (float)((int)j * g.feat_stride), ay = a[1] + (float)((int)i * g.feat_stride), aw = a[2] - a[0], ah = a[3] - a[1];
    const float cx = ax + aw * 0.5f, cy = ay + ah * 0.5f;
    const float pcx = cx + aw * dx, pcy = cy + ah * dy, pw = aw * expf(dw), ph = ah * expf(dh);
    const float x1 = clip(pcx - pw * 0.5f, im_w - 1.f), y1 = clip(pcy - ph * 0.5f, im_h - 1.f);
    const float x2 = clip(pcx + pw * 0.5f, im_w - 1.f), y2 = clip(pcy + ph * 0.5f, im_h - 1.f);
    box[0] = x1;
    box[1] = y1;
    box[2] = x2;
    box[3] = y2;
    *score = s;
    return x2 - x1 + 1.f >= min_box && y2 - y1 + 1.f >= min_box && s == s;
}

__global__ __launch_bounds__(256) void proposal_key_kernel(u64* __restrict__ keys, ProposalArgs g, unsigned total /* n * anchors per image */)
{
    const unsigned at = blockIdx.x * 256u + threadIdx.x;
    if (at >= total) return;
    const unsigned per = (unsigned)g.A * (unsigned)g.h * (unsigned)g.w, img = at / per, r = at - img * per;
    float box[4], s;
    keys[at] = decode(g, img, r, box, &s) ? (((u64)ordered(s) << 32) | (u64)(kIndexMask - r)) : 0;
}

// keys[0, size) sorted descending; size is a power of two <= kKeys.  Every lane of the block calls it; ends on a barrier.
__device__ void sort_descending(u64* keys, int size)
{
    for (int len = 2; len <= size; len <<= 1)
        for (int stride = len >> 1; stride > 0; stride >>= 1)
        {
            for (int t = threadIdx.x; t < size / 2; t += kThreads)
            {
                const int i = ((t & ~(stride - 1)) << 1) | (t & (stride - 1)), j = i + stride;
                const u64 a = keys[i], b = keys[j];
                if ((a < b) == ((i & len) == 0))
                {
                    keys[i] = b;
                    keys[j] = a;
                }
            }
            __syncthreads();
        }
}

// ncnn's test: the intersection without + 1, the areas with it
__device__ __forceinline__ bool suppresses(const float* a, const float* b, float thr)
{
    const float aa = (a[2] - a[0] + 1.f) * (a[3] - a[1] + 1.f), ab = (b[2] - b[0] + 1.f) * (b[3] - b[1] + 1.f);
    float inter = 0.f;
    if (!(a[0] > b[2] || a[2] < b[0] || a[1] > b[3] || a[3] < b[1])) inter = (fminf(a[2], b[2]) - fmaxf(a[0], b[0])) * (fminf(a[3], b[3]) - fmaxf(a[1], b[1]));
    return inter / (aa + ab - inter) > thr;
}

__global__ __launch_bounds__(kThreads) void proposal_select_kernel(float* __restrict__ rois, float* __restrict__ scores, const u64* __restrict__ all_keys, ProposalArgs g)
{
    __shared__ u64 keys[kKeys];
    __shared__ float kept[FHIP_ROI_MAX_ROIS][4];
    __shared__ float box[kChunk][4];
    __shared__ float sc[kChunk];
    __shared__ unsigned char alive[kChunk];
    __shared__ int s_all, s_mine, s_at;
    const int tid = threadIdx.x, img = blockIdx.x, per = g.A * g.h * g.w, pre = g.pre > 0 ? g.pre : INT_MAX;
    const u64* src = all_keys + (size_t)img * per;
    float* rows = rois + (size_t)img * g.rows * 4;
    float* srow = scores ? scores + (size_t)img * g.rows : nullptr;
    int kept_n = 0, consumed = 0;
    u64 bound = ~0ull; // this round takes the keys below it
    for (;;)
    {
        for (int i = tid; i < kKeys; i += kThreads) keys[i] = 0;
        if (tid == 0) s_all = s_mine = 0;
        __syncthreads();
        int filled = 0, taken = 0, seen = 0; // keys in the buffer; keys put into it and keys below the bound seen so far in this round
        u64 cutoff = 0; // once the buffer was cut: the smallest key it kept -- kChunk better ones are held, so a key at or below it is not taken
        for (int base = 0; base < per; base += kChunk)
        {
            u64 v[kChunk / kThreads];
            int mine = 0, all = 0;
#pragma unroll
            for (int k = 0; k < kChunk / kThreads; ++k)
            {
                const int p = base + k * kThreads + tid;
                v[k] = p < per ? src[p] : 0;
                if (v[k] >= bound) v[k] = 0; // taken by an earlier round
                all += v[k] != 0 ? 1 : 0;
                if (v[k] <= cutoff) v[k] = 0;
                mine += v[k] != 0 ? 1 : 0;
            }
            if (all) atomicAdd(&s_all, all);
            if (mine) atomicAdd(&s_mine, mine);
            __syncthreads();
            const int total = s_mine - taken; // the counters run on through a round; sums: the same whatever the order of the atomics
            seen = s_all;
            __syncthreads(); // every lane has read them before the next chunk adds
            taken += total;
            if (total == 0) continue;
            if (filled + total > kKeys) // sort and keep the best kChunk: filled <= kChunk afterwards, and a chunk fits behind them
            {
                sort_descending(keys, kKeys);
                cutoff = keys[kChunk - 1]; // (the tail cleared next lies behind it)
                for (int i = kChunk + tid; i < kKeys; i += kThreads) keys[i] = 0;
                filled = min(filled, kChunk);
            }
            if (tid == 0) s_at = filled;
            __syncthreads();
#pragma unroll
            for (int k = 0; k < kChunk / kThreads; ++k)
                if (v[k] != 0) keys[atomicAdd(&s_at, 1)] = v[k]; // the slot is arbitrary, the sort is not
            filled += total;
            __syncthreads();
        }
        int size = 2;
        while (size < filled) size <<= 1;
        sort_descending(keys, size);
        const int m = min(min(filled, kChunk), pre - consumed);
        if (m <= 0) break;
        // the boxes of this round's candidates, tested against the boxes earlier rounds kept (kept[] was last written before this round's barriers)
        for (int i = tid; i < m; i += kThreads)
        {
            const unsigned r = kIndexMask - (unsigned)(keys[i] & kIndexMask);
            decode(g, (unsigned)img, r, box[i], &sc[i]);
            unsigned char live = 1;
            for (int k = 0; k < kept_n && live; ++k)
                if (suppresses(kept[k], box[i], g.nms_thresh)) live = 0;
            alive[i] = live;
        }
        // greedy NMS in key order; every lane follows the same steps, lanes 0 .. 4 write a kept candidate out.  alive[] changes only in a
        // suppression pass, and a barrier follows each: a dropped candidate is passed over without one
        __syncthreads();
        for (int i = 0; i < m && kept_n < g.rows; ++i)
        {
            if (!alive[i]) continue;
            if (tid < 4)
            {
                kept[kept_n][tid] = box[i][tid];
                rows[(size_t)kept_n * 4 + tid] = box[i][tid];
            }
            if (tid == 4 && srow) srow[kept_n] = sc[i];
            ++kept_n;
            for (int j = i + 1 + tid; j < m; j += kThreads)
                if (alive[j] && suppresses(box[i], box[j], g.nms_thresh)) alive[j] = 0;
            __syncthreads();
        }
        consumed += m;
        if (kept_n >= g.rows || consumed >= pre || seen <= kChunk) break; // full, the candidates' share taken, or this round took every key there was
        bound = keys[m - 1];
        __syncthreads(); // every lane has read the bound (and the boxes) before the buffer is cleared
    }
    for (int i = kept_n * 4 + tid; i < g.rows * 4; i += kThreads) rows[i] = (i & 2) ? -1.f : 0.f; // the sentinel (0, 0, -1, -1)
    if (srow)
        for (int i = kept_n + tid; i < g.rows; i += kThreads) srow[i] = 0.f;
}

// ---- the ROI layers --------------------------------------------------------------------------------------------------------------------
struct RoiArgs
{
    const float *in, *rois;
    int R, c, h, w, ph, pw, out_c;
    float scale;
    int sampling, aligned;
};

// the output element `idx` of [n * R][out_c][ph][pw]: its row, channel and bin
__device__ __forceinline__ void element(const RoiArgs& g, unsigned idx, unsigned* row, unsigned* ch, int* p, int* q)
{
    *q = (int)(idx % (unsigned)g.pw);
    unsigned t = idx / (unsigned)g.pw;
    *p = (int)(t % (unsigned)g.ph);
    t /= (unsigned)g.ph;
    *ch = t % (unsigned)g.out_c;
    *row = t / (unsigned)g.out_c;
}

__device__ __forceinline__ int clampi(int v, int hi) { return min(max(v, 0), hi); }

__global__ __launch_bounds__(256) void roi_pool_kernel(float* __restrict__ out, RoiArgs g, unsigned total)
{
    const unsigned idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= total) return;
    unsigned row, ch;
    int p, q;
    element(g, idx, &row, &ch, &p, &q);
    const float* r = g.rois + (size_t)row * 4;
    const int x1 = (int)roundf(r[0] * g.scale), y1 = (int)roundf(r[1] * g.scale), x2 = (int)roundf(r[2] * g.scale), y2 = (int)roundf(r[3] * g.scale);
    const int rw = max(x2 - x1 + 1, 1), rh = max(y2 - y1 + 1, 1);
    const float bw = (float)rw / (float)g.pw, bh = (float)rh / (float)g.ph;
    const int hs = clampi(y1 + (int)floorf((float)p * bh), g.h), he = clampi(y1 + (int)ceilf((float)(p + 1) * bh), g.h);
    const int ws = clampi(x1 + (int)floorf((float)q * bw), g.w), we = clampi(x1 + (int)ceilf((float)(q + 1) * bw), g.w);
    float m = 0.f;
    if (he > hs && we > ws)
    {
        const float* src = g.in + ((size_t)(row / (unsigned)g.R) * g.c + ch) * g.h * g.w;
        m = src[(size_t)hs * g.w + ws];
        for (int y = hs; y < he; ++y)
            for (int x = ws; x < we; ++x)
            {
                const float v = src[(size_t)y * g.w + x];
                m = m < v ? v : m;
            }
    }
    out[idx] = m;
}

__global__ __launch_bounds__(256) void psroi_pool_kernel(float* __restrict__ out, RoiArgs g, unsigned total)
{
    const unsigned idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= total) return;
    unsigned row, d;
    int p, q;
    element(g, idx, &row, &d, &p, &q);
    const float* r = g.rois + (size_t)row * 4;
    const float x1 = roundf(r[0]) * g.scale, y1 = roundf(r[1]) * g.scale, x2 = roundf(r[2] + 1.f) * g.scale, y2 = roundf(r[3] + 1.f) * g.scale;
    const float rw = fmaxf(x2 - x1, 0.1f), rh = fmaxf(y2 - y1, 0.1f);
    const float bw = rw / (float)g.pw, bh = rh / (float)g.ph;
    const int hs = clampi((int)floorf(y1 + (float)p * bh), g.h), he = clampi((int)ceilf(y1 + (float)(p + 1) * bh), g.h);
    const int ws = clampi((int)floorf(x1 + (float)q * bw), g.w), we = clampi((int)ceilf(x1 + (float)(q + 1) * bw), g.w);
    float v = 0.f;
    if (he > hs && we > ws)
    {
        const unsigned ch = (d * (unsigned)g.ph + (unsigned)p) * (unsigned)g.pw + (unsigned)q;
        const float* src = g.in + ((size_t)(row / (unsigned)g.R) * g.c + ch) * g.h * g.w;
        float sum = 0.f;
        for (int y = hs; y < he; ++y)
            for (int x = ws; x < we; ++x) sum = sum + src[(size_t)y * g.w + x];
        v = sum / (float)((he - hs) * (we - ws));
    }
    out[idx] = v;
}

__device__ __forceinline__ int grid_of(int sampling, float extent)
{
    const int g = sampling > 0 ? sampling : (int)ceilf(extent);
    return min(g, FHIP_ROI_MAX_GRID);
}

template <int V>
__global__ __launch_bounds__(256) void roi_align_kernel(float* __restrict__ out, RoiArgs g, unsigned total)
{
    const unsigned idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= total) return;
    unsigned row, ch;
    int p, q;
    element(g, idx, &row, &ch, &p, &q);
    const float* r = g.rois + (size_t)row * 4;
    const int h = g.h, w = g.w;
    const float* src = g.in + ((size_t)(row / (unsigned)g.R) * g.c + ch) * h * w;
    float x1 = r[0] * g.scale, y1 = r[1] * g.scale, x2 = r[2] * g.scale, y2 = r[3] * g.scale;
    if (g.aligned)
    {
        x1 = x1 - 0.5f;
        y1 = y1 - 0.5f;
        x2 = x2 - 0.5f;
        y2 = y2 - 0.5f;
    }
    float rw = x2 - x1, rh = y2 - y1;
    if (!g.aligned)
    {
        rw = fmaxf(rw, 1.f);
        rh = fmaxf(rh, 1.f);
    }
    const float bw = rw / (float)g.pw, bh = rh / (float)g.ph;
    float result = 0.f;
    if constexpr (V == 0)
    {
        const float hs = clip(y1 + (float)p * bh, (float)h), he = clip(y1 + (float)(p + 1) * bh, (float)h);
        const float ws = clip(x1 + (float)q * bw, (float)w), we = clip(x1 + (float)(q + 1) * bw, (float)w);
        if (!(he <= hs || we <= ws))
        {
            const int gh = grid_of(g.sampling, he - hs), gw = grid_of(g.sampling, we - ws);
            float sum = 0.f;
            for (int by = 0; by < gh; ++by)
            {
                const float y = hs + (((float)by + 0.5f) * bh) / (float)gh;
                int y0 = max((int)y, 0), yn;
                float b0, b1;
                if (y0 >= h - 1)
                {
                    y0 = yn = h - 1;
                    b0 = 1.f;
                    b1 = 0.f;
                }
                else
                {
                    yn = y0 + 1;
                    b0 = (float)yn - y;
                    b1 = y - (float)y0;
                }
                for (int bx = 0; bx < gw; ++bx)
                {
                    const float x = ws + (((float)bx + 0.5f) * bw) / (float)gw;
                    int x0 = max((int)x, 0), xn;
                    float a0, a1;
                    if (x0 >= w - 1)
                    {
                        x0 = xn = w - 1;
                        a0 = 1.f;
                        a1 = 0.f;
                    }
                    else
                    {
                        xn = x0 + 1;
                        a0 = (float)xn - x;
                        a1 = x - (float)x0;
                    }
                    const float r0 = src[(size_t)y0 * w + x0] * a0 + src[(size_t)y0 * w + xn] * a1;
                    const float r1 = src[(size_t)yn * w + x0] * a0 + src[(size_t)yn * w + xn] * a1;
                    sum = sum + (r0 * b0 + r1 * b1);
                }
            }
            result = sum / (float)(gh * gw);
        }
    }
    else
    {
        const int gh = grid_of(g.sampling, rh / (float)g.ph), gw = grid_of(g.sampling, rw / (float)g.pw);
        const float count = (float)max(gh * gw, 1);
        const float ybase = y1 + (float)p * bh, xbase = x1 + (float)q * bw;
        float sum = 0.f;
        for (int iy = 0; iy < gh; ++iy)
        {
            float y = ybase + (((float)iy + 0.5f) * bh) / (float)gh;
            const bool y_out = y < -1.f || y > (float)h;
            y = y <= 0.f ? 0.f : y;
            int yl = max((int)y, 0), yh;
            if (yl >= h - 1)
            {
                yh = yl = h - 1;
                y = (float)yl;
            }
            else
                yh = yl + 1;
            const float ly = y - (float)yl, hy = 1.f - ly;
            for (int ix = 0; ix < gw; ++ix)
            {
                float x = xbase + (((float)ix + 0.5f) * bw) / (float)gw;
                if (y_out || x < -1.f || x > (float)w) continue; // the sample is 0.f: sum + 0.f is sum (a -0.f sum cannot occur: it starts at 0.f)
                x = x <= 0.f ? 0.f : x;
                int xl = max((int)x, 0), xh;
                if (xl >= w - 1)
                {
                    xh = xl = w - 1;
                    x = (float)xl;
                }
                else
                    xh = xl + 1;
                const float lx = x - (float)xl, hx = 1.f - lx;
                const float v = (((hy * hx) * src[(size_t)yl * w + xl] + (hy * lx) * src[(size_t)yl * w + xh]) + (ly * hx) * src[(size_t)yh * w + xl]) +
                                (ly * lx) * src[(size_t)yh * w + xh];
                sum = sum + v;
            }
        }
        result = sum / count;
    }
    out[idx] = result;
}

// ---- host checks -----------------------------------------------------------------------------------------------------------------------
constexpr long long kMaxElements = 1ll << 31;

static bool overlap(const void* a, size_t na, const void* b, size_t nb)
{
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}

// the counts and extents of a Proposal; -> anchors per image in *per
static int proposal_shape(int n, int A, int h, int w, long long* per)
{
    if (n < 1 || n > 65535) return fail(FHIP_E_BADARG, "1 .. 65535 images");
    if (A < 1 || A > FHIP_ROI_MAX_ANCHORS) return fail(FHIP_E_BADARG, "num_anchors must be 1 .. FHIP_ROI_MAX_ANCHORS (32)");
    if (h < 1 || w < 1) return fail(FHIP_E_BADARG, "a dimension < 1");
    const long long cells = (long long)h * w;
    if (cells > FHIP_ROI_MAX_CELLS || cells * A > FHIP_ROI_MAX_CELLS) return fail(FHIP_E_BADARG, "more than FHIP_ROI_MAX_CELLS (2^24) anchors per image");
    if ((long long)n * 4 * A * cells >= kMaxElements) return fail(FHIP_E_BADARG, "tensors of 2^31 elements or more are not supported");
    *per = cells * A;
    return FHIP_OK;
}

// the checks the three ROI layers share; -> elements of the output in *total
static int roi_shape(int n, int c, int h, int w, int R, int pw, int ph, float scale, int out_c, const float* out, const float* in, const float* rois,
                     long long* total)
{
    if (n < 1 || c < 1 || h < 1 || w < 1 || R < 1 || out_c < 1) return fail(FHIP_E_BADARG, "a dimension < 1");
    if (pw < 1 || ph < 1 || pw > FHIP_ROI_MAX_POOLED || ph > FHIP_ROI_MAX_POOLED) return fail(FHIP_E_BADARG, "pooled extents must be 1 .. FHIP_ROI_MAX_POOLED (64)");
    if (!std::isfinite(scale)) return fail(FHIP_E_BADARG, "spatial_scale must be finite");
    const long long total_in = (long long)n * c * h * w, rows = (long long)n * R;
    if (total_in >= kMaxElements || rows * 4 >= kMaxElements) return fail(FHIP_E_BADARG, "tensors of 2^31 elements or more are not supported");
    if (rows * out_c >= kMaxElements || rows * out_c * ph * pw >= kMaxElements) return fail(FHIP_E_BADARG, "tensors of 2^31 elements or more are not supported");
    *total = rows * out_c * ph * pw;
    if (!out || !in || !rois) return fail(FHIP_E_BADARG, "null pointer");
    if (!aligned(out, 4) || !aligned(in, 4) || !aligned(rois, 4)) return fail(FHIP_E_BADARG, "pointers must be 4-byte aligned");
    if (overlap(out, (size_t)*total * 4, in, (size_t)total_in * 4) || overlap(out, (size_t)*total * 4, rois, (size_t)rows * 16))
        return fail(FHIP_E_BADARG, "out must not overlap in or rois");
    return FHIP_OK;
}

static RoiArgs roi_args(int c, int h, int w, int R, int pw, int ph, float scale, int out_c, const float* in, const float* rois)
{
    RoiArgs g;
    memset(&g, 0, sizeof(g));
    g.in = in;
    g.rois = rois;
    g.R = R;
    g.c = c;
    g.h = h;
    g.w = w;
    g.ph = ph;
    g.pw = pw;
    g.out_c = out_c;
    g.scale = scale;
    return g;
}

} // namespace fhip

using namespace fhip;

extern "C"
{

int fhip_roi_generate_anchors(int base_size, const float* ratios, int num_ratios, const float* scales, int num_scales, float* anchors)
{
    if (base_size < 1) return fail(FHIP_E_BADARG, "base_size < 1");
    if (num_ratios < 1 || num_scales < 1 || (long long)num_ratios * num_scales > FHIP_ROI_MAX_ANCHORS)
        return fail(FHIP_E_BADARG, "1 .. FHIP_ROI_MAX_ANCHORS (32) anchors: ratios x scales");
    if (!ratios || !scales || !anchors) return fail(FHIP_E_BADARG, "null argument");
    for (int i = 0; i < num_ratios; ++i)
        if (!std::isfinite(ratios[i]) || !(ratios[i] > 0.f)) return fail(FHIP_E_BADARG, "ratios must be finite and > 0");
    for (int j = 0; j < num_scales; ++j)
        if (!std::isfinite(scales[j]) || !(scales[j] > 0.f)) return fail(FHIP_E_BADARG, "scales must be finite and > 0");
    const float c = (float)base_size * 0.5f;
    for (int i = 0; i < num_ratios; ++i)
    {
        const double r_w = round((double)base_size / sqrt((double)ratios[i])), r_h = round(r_w * (double)ratios[i]);
        for (int j = 0; j < num_scales; ++j)
        {
            const float rs_w = (float)r_w * scales[j], rs_h = (float)r_h * scales[j];
            float* a = anchors + ((size_t)i * num_scales + j) * 4;
            a[0] = c - rs_w * 0.5f;
            a[1] = c - rs_h * 0.5f;
            a[2] = c + rs_w * 0.5f;
            a[3] = c + rs_h * 0.5f;
        }
    }
    return FHIP_OK;
}

int fhip_proposal_get_buffer_size(int n, int num_anchors, int h, int w, size_t* bytes)
{
    long long per;
    const int rc = proposal_shape(n, num_anchors, h, w, &per);
    if (rc) return rc;
    if (!bytes) return fail(FHIP_E_BADARG, "null argument");
    *bytes = (size_t)n * (size_t)per * sizeof(u64);
    return FHIP_OK;
}

int fhip_proposal_forward(int n, int num_anchors, int h, int w, int feat_stride, int pre_nms_topN, int after_nms_topN, float nms_thresh, float min_size,
                          const float* anchors, float* rois, float* scores, const float* score, const float* bbox, const float* im_info, void* scratch,
                          void* stream)
{
    long long per;
    const int rc = proposal_shape(n, num_anchors, h, w, &per);
    if (rc) return rc;
    if (feat_stride < 1 || (long long)feat_stride * std::max(h, w) >= kMaxElements) return fail(FHIP_E_BADARG, "feat_stride must be >= 1 and feat_stride * extent below 2^31");
    if (after_nms_topN < 1 || after_nms_topN > FHIP_ROI_MAX_ROIS) return fail(FHIP_E_BADARG, "after_nms_topN must be 1 .. FHIP_ROI_MAX_ROIS (2048)");
    if (!std::isfinite(nms_thresh) || !std::isfinite(min_size)) return fail(FHIP_E_BADARG, "nms_thresh and min_size must be finite");
    if (!anchors) return fail(FHIP_E_BADARG, "null anchors");
    for (int k = 0; k < 4 * num_anchors; ++k)
        if (!std::isfinite(anchors[k])) return fail(FHIP_E_BADARG, "anchors must be finite");
    if (!rois || !score || !bbox || !im_info || !scratch) return fail(FHIP_E_BADARG, "null pointer");
    if (!aligned(rois, 4) || !aligned(score, 4) || !aligned(bbox, 4) || !aligned(im_info, 4) || !aligned(scratch, 8) || (scores && !aligned(scores, 4)))
        return fail(FHIP_E_BADARG, "pointers must be 4-byte aligned (scratch: 8)");
    const size_t rois_bytes = (size_t)n * after_nms_topN * 16, scores_bytes = (size_t)n * after_nms_topN * 4, scratch_bytes = (size_t)n * (size_t)per * sizeof(u64);
    const size_t score_bytes = (size_t)n * 2 * per * 4, bbox_bytes = (size_t)n * 4 * per * 4, info_bytes = (size_t)n * 12;
    const void* written[3] = {rois, scratch, scores};
    const size_t written_bytes[3] = {rois_bytes, scratch_bytes, scores_bytes};
    const void* read[3] = {score, bbox, im_info};
    const size_t read_bytes[3] = {score_bytes, bbox_bytes, info_bytes};
    for (int a = 0; a < 3; ++a)
    {
        if (!written[a]) continue;
        for (int b = 0; b < 3; ++b)
            if (overlap(written[a], written_bytes[a], read[b], read_bytes[b])) return fail(FHIP_E_BADARG, "rois, scores and scratch must not overlap a bottom");
        for (int b = a + 1; b < 3; ++b)
            if (written[b] && overlap(written[a], written_bytes[a], written[b], written_bytes[b]))
                return fail(FHIP_E_BADARG, "rois, scores and scratch must not overlap each other");
    }
    ProposalArgs g;
    memset(&g, 0, sizeof(g));
    g.score = score;
    g.bbox = bbox;
    g.im_info = im_info;
    memcpy(g.anchors, anchors, (size_t)num_anchors * 16);
    g.A = num_anchors;
    g.h = h;
    g.w = w;
    g.feat_stride = feat_stride;
    g.pre = pre_nms_topN;
    g.rows = after_nms_topN;
    g.nms_thresh = nms_thresh;
    g.min_size = min_size;
    hipStream_t s = (hipStream_t)stream;
    const unsigned total = (unsigned)((long long)n * per); // < 2^31: n * 4 * per is
    hipLaunchKernelGGL(proposal_key_kernel, dim3((total + 255) / 256), dim3(256), 0, s, (u64*)scratch, g, total);
    FHIP_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(proposal_select_kernel, dim3((unsigned)n), dim3(kThreads), 0, s, rois, scores, (const u64*)scratch, g);
    FHIP_CHECK_HIP(hipGetLastError());
    return FHIP_OK;
}

int fhip_roi_pool_forward(int n, int c, int h, int w, int num_rois, int pooled_w, int pooled_h, float spatial_scale, float* out, const float* in,
                          const float* rois, void* stream)
{
    long long total;
    const int rc = roi_shape(n, c, h, w, num_rois, pooled_w, pooled_h, spatial_scale, c, out, in, rois, &total);
    if (rc) return rc;
    const RoiArgs g = roi_args(c, h, w, num_rois, pooled_w, pooled_h, spatial_scale, c, in, rois);
    hipLaunchKernelGGL(roi_pool_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, out, g, (unsigned)total);
    FHIP_CHECK_HIP(hipGetLastError());
    return FHIP_OK;
}

int fhip_roi_align_forward(int n, int c, int h, int w, int num_rois, int pooled_w, int pooled_h, float spatial_scale, int sampling_ratio, int aligned_,
                           int version, float* out, const float* in, const float* rois, void* stream)
{
    if (version != 0 && version != 1) return fail(FHIP_E_BADARG, "ROIAlign version must be 0 or 1");
    if (aligned_ != 0 && aligned_ != 1) return fail(FHIP_E_BADARG, "ROIAlign aligned must be 0 or 1");
    if (sampling_ratio < 0 || sampling_ratio > FHIP_ROI_MAX_GRID) return fail(FHIP_E_BADARG, "ROIAlign sampling_ratio must be 0 .. FHIP_ROI_MAX_GRID (4096)");
    long long total;
    const int rc = roi_shape(n, c, h, w, num_rois, pooled_w, pooled_h, spatial_scale, c, out, in, rois, &total);
    if (rc) return rc;
    RoiArgs g = roi_args(c, h, w, num_rois, pooled_w, pooled_h, spatial_scale, c, in, rois);
    g.sampling = sampling_ratio;
    g.aligned = aligned_;
    const dim3 blocks((unsigned)((total + 255) / 256));
    if (version == 0)
        hipLaunchKernelGGL(roi_align_kernel<0>, blocks, dim3(256), 0, (hipStream_t)stream, out, g, (unsigned)total);
    else
        hipLaunchKernelGGL(roi_align_kernel<1>, blocks, dim3(256), 0, (hipStream_t)stream, out, g, (unsigned)total);
    FHIP_CHECK_HIP(hipGetLastError());
    return FHIP_OK;
}

int fhip_psroi_pool_forward(int n, int c, int h, int w, int num_rois, int pooled_w, int pooled_h, float spatial_scale, int output_dim, float* out,
                            const float* in, const float* rois, void* stream)
{
    if (output_dim < 1) return fail(FHIP_E_BADARG, "output_dim < 1");
    if (pooled_w >= 1 && pooled_h >= 1 && pooled_w <= FHIP_ROI_MAX_POOLED && pooled_h <= FHIP_ROI_MAX_POOLED && (long long)output_dim * pooled_h * pooled_w != c)
        return fail(FHIP_E_BADARG, "PSROIPooling needs c == output_dim * pooled_h * pooled_w");
    long long total;
    const int rc = roi_shape(n, c, h, w, num_rois, pooled_w, pooled_h, spatial_scale, output_dim, out, in, rois, &total);
    if (rc) return rc;
    const RoiArgs g = roi_args(c, h, w, num_rois, pooled_w, pooled_h, spatial_scale, output_dim, in, rois);
    hipLaunchKernelGGL(psroi_pool_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, out, g, (unsigned)total);
    FHIP_CHECK_HIP(hipGetLastError());
    return FHIP_OK;
}

int fhip_roi_route(int what, int a, int b, char* name, int len)
{
    (void)b;
    if (!name || len < 1) return fail(FHIP_E_BADARG, "null name");
    switch (what)
    {
    case FHIP_ROI_KEYS: snprintf(name, (size_t)len, "fhip::proposal_key_kernel"); return FHIP_OK;
    case FHIP_ROI_SELECT: snprintf(name, (size_t)len, "fhip::proposal_select_kernel"); return FHIP_OK;
    case FHIP_ROI_POOL: snprintf(name, (size_t)len, "fhip::roi_pool_kernel"); return FHIP_OK;
    case FHIP_ROI_ALIGN:
        if (a != 0 && a != 1) return fail(FHIP_E_BADARG, "version must be 0 or 1");
        snprintf(name, (size_t)len, "fhip::roi_align_kernel<%d>", a);
        return FHIP_OK;
    case FHIP_ROI_PSROI: snprintf(name, (size_t)len, "fhip::psroi_pool_kernel"); return FHIP_OK;
    default: return fail(FHIP_E_BADARG, "unknown operation");
    }
}

const char* fhip_roi_last_error(void) { return last_error(); }

} // extern "C"
