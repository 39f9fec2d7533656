// libfeather_yolo.so: the layers of a YOLO detection head on gfx950 (include/feather_hip/feather_yolo.h is the contract and the definition;
// DESIGN.md 3.25 the design and its measurements).
//
//   reorg_tile_kernel         a block owns a group of output rows of one input plane: the input rows behind them are one contiguous span, loaded
//                             into LDS with coalesced loads; each of the stride x stride output channels then receives one contiguous run
//                             (its rows of the group), read from LDS at stride `stride` -- so both sides of the copy are coalesced
//   reorg_direct_kernel       one output element per lane, coalesced stores: stride 1 (a copy) and planes whose stride rows pass the tile
//   yolo_score_kernel<V>      one lane per (image, bottom, box, cell), plane reads coalesced across the cells; V = 3: one pass over the class
//                             planes, the first maximum of the raw scores; V = 2: three passes that each read the planes again -- max, sum of
//                             exp, first maximum of the quotients (the quotient needs the finished sum: the header's rounding); every
//                             box writes its 64-bit key (confidence bits, inverted global index, label), 0 when it is no candidate: no
//                             compaction, no atomic
//   yolo_select_kernel        a block per image, in rounds: the FHIP_YOLO_CHUNK best keys below the previous round's last are gathered chunk by
//                             chunk into an LDS buffer of 2048 keys (an LDS counter gives the slots, the bitonic sort the order), their boxes
//                             alone are decoded into LDS, tested against the boxes kept in earlier rounds and then greedily among themselves
//                             (a barrier per kept box); once the buffer was cut, keys at or below its last key are passed over;
//                             kept boxes stay in LDS; ends when `rows` are kept or a round saw no more keys than it took; writes every row
//
// Contraction is off for the whole file: every product and sum is rounded on its own, as the header defines.
#include <float.h>
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <string>

#include "feather_hip/feather_yolo.h"
#include "side_error.h"

#pragma clang fp contract(off)

namespace fhip
{

typedef unsigned long long u64;

constexpr int kKeys = 2 * FHIP_YOLO_CHUNK; // keys of the selection buffer: the kept ones and a chunk's candidates
constexpr unsigned kIndexMask = FHIP_YOLO_MAX_CELLS - 1;
static_assert(FHIP_YOLO_MAX_ROWS <= FHIP_YOLO_CHUNK, "a round's survivors fit the kept boxes");
static_assert(FHIP_YOLO_MAX_CLASSES <= 256 && FHIP_YOLO_MAX_CELLS <= (1 << 24), "a key's low word holds the inverted index above the label's 8 bits");

// ---- Reorg -----------------------------------------------------------------------------------------------------------------------------
// blockIdx.x runs over (image, input plane, group of `group` output rows)
__global__ __launch_bounds__(256) void reorg_tile_kernel(float* __restrict__ out, const float* __restrict__ in, int s, int mode, int c, int h, int w, int oh, int ow,
                                                         int group, int groups)
{
    __shared__ float tile[FHIP_REORG_TILE];
    const unsigned plane = blockIdx.x / (unsigned)groups, i0 = (blockIdx.x - plane * (unsigned)groups) * (unsigned)group;
    const unsigned img = plane / (unsigned)c, q = plane - img * (unsigned)c;
    const int here = min(group, oh - (int)i0);
    const int span = here * s * w; // <= FHIP_REORG_TILE, and inside the plane: (i0 + here) * s <= oh * s <= h
    const float* src = in + ((size_t)plane * h + (size_t)i0 * s) * w;
    for (int t = threadIdx.x; t < span; t += 256) tile[t] = src[t];
    __syncthreads();
    const int run = here * ow, total = s * s * run;
    for (int e = threadIdx.x; e < total; e += 256)
    {
        const int k = e / run, r = e - k * run; // k = sh * s + sw
        const int ii = r / ow, j = r - ii * ow, sh = k / s, sw = k - sh * s;
        const unsigned ch = mode ? (unsigned)k * c + q : q * (unsigned)(s * s) + k;
        out[(((size_t)img * c * s * s + ch) * oh + i0 + ii) * ow + j] = tile[(ii * s + sh) * w + j * s + sw];
    }
}

__global__ __launch_bounds__(256) void reorg_direct_kernel(float* __restrict__ out, const float* __restrict__ in, unsigned total, int s, int mode, int c, int h,
                                                           int w, int oh, int ow)
{
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= total) return;
    const unsigned j = i % (unsigned)ow, r = i / (unsigned)ow;
    const unsigned ii = r % (unsigned)oh, p = r / (unsigned)oh;
    const unsigned oc = (unsigned)c * s * s, ch = p % oc, img = p / oc;
    const unsigned q = mode ? ch % (unsigned)c : ch / (unsigned)(s * s), k = mode ? ch / (unsigned)c : ch % (unsigned)(s * s);
    const unsigned sh = k / (unsigned)s, sw = k - sh * s;
    out[i] = in[(((size_t)img * c + q) * h + ii * s + sh) * w + j * s + sw];
}

// ---- the detection ---------------------------------------------------------------------------------------------------------------------
// bottom b is [n][num_box * (5 + num_class)][h[b]][w[b]] and owns the global box indices [first[b], first[b + 1]); bias_w / bias_h: the anchor
// of (bottom, box), resolved on the host (version 2: biases[2 * pp], version 3: biases[2 * mask[b * num_box + pp]])
struct YoloArgs
{
    const float* in[FHIP_YOLO_MAX_SCALES];
    int h[FHIP_YOLO_MAX_SCALES], w[FHIP_YOLO_MAX_SCALES], first[FHIP_YOLO_MAX_SCALES + 1];
    float anchors_scale[FHIP_YOLO_MAX_SCALES];
    float bias_w[FHIP_YOLO_MAX_SCALES][FHIP_YOLO_MAX_BOXES], bias_h[FHIP_YOLO_MAX_SCALES][FHIP_YOLO_MAX_BOXES];
    int scales, num_box, num_class, version, rows;
    float confidence_threshold, nms_threshold;
};

// a float as an unsigned that orders the same way (NaN never gets here), and back
__device__ __forceinline__ unsigned ordered(float f)
{
    const unsigned b = f == 0.f ? 0u : __float_as_uint(f); // -0.f is 0.f
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float unordered(unsigned u) { return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u); }

__device__ __forceinline__ float sigmoid(float v) { return 1.f / (1.f + expf(-v)); }

// the bottom that owns global box index r
__device__ __forceinline__ int bottom_of(const YoloArgs& g, unsigned r)
{
    int b = 0;
    while (b + 1 < g.scales && r >= (unsigned)g.first[b + 1]) ++b;
    return b;
}

template <int V>
__global__ __launch_bounds__(256) void yolo_score_kernel(u64* __restrict__ keys, YoloArgs g, unsigned total /* n * boxes per image */)
{
    const unsigned at = blockIdx.x * 256u + threadIdx.x;
    if (at >= total) return;
    const unsigned per = (unsigned)g.first[g.scales], img = at / per, r = at - img * per;
    const int b = bottom_of(g, r), C = g.num_class;
    const unsigned hw = (unsigned)g.h[b] * (unsigned)g.w[b], local = r - (unsigned)g.first[b], pp = local / hw, cell = local - pp * hw;
    const float* p = g.in[b] + ((size_t)img * g.num_box + pp) * (5 + C) * hw + cell;
    const float objectness = p[(size_t)4 * hw];
    const float* s = p + (size_t)5 * hw;
    int label = 0;
    float confidence;
    if constexpr (V == 2)
    {
        float m = -FLT_MAX;
#pragma unroll 4
        for (int c = 0; c < C; ++c) m = fmaxf(m, s[(size_t)c * hw]);
        float sum = 0.f;
#pragma unroll 4
        for (int c = 0; c < C; ++c) sum = sum + expf(s[(size_t)c * hw] - m);
        float best = expf(s[0] - m) / sum;
#pragma unroll 4
        for (int c = 1; c < C; ++c)
        {
            const float q = expf(s[(size_t)c * hw] - m) / sum;
            if (q > best)
            {
                best = q;
                label = c;
            }
        }
        confidence = sigmoid(objectness) * best;
    }
    else
    {
        float best = s[0];
#pragma unroll 4
        for (int c = 1; c < C; ++c)
        {
            const float v = s[(size_t)c * hw];
            if (v > best)
            {
                best = v;
                label = c;
            }
        }
        confidence = 1.f / ((1.f + expf(-objectness)) * (1.f + expf(-best)));
    }
    u64 key = 0;
    if (confidence >= g.confidence_threshold) key = ((u64)ordered(confidence) << 32) | ((u64)(kIndexMask - r) << 8) | (unsigned)label;
    keys[at] = key;
}

// keys[0, size) sorted descending; size is a power of two <= kKeys.  Every lane of the block calls it; ends on a barrier.
__device__ void sort_descending(u64* keys, int size)
{
    for (int len = 2; len <= size; len <<= 1)
        for (int stride = len >> 1; stride > 0; stride >>= 1)
        {
            for (int t = threadIdx.x; t < size / 2; t += 256)
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

__device__ __forceinline__ float iou(const float* a, const float* b)
{
    const float iw = fminf(a[2], b[2]) - fmaxf(a[0], b[0]), ih = fminf(a[3], b[3]) - fmaxf(a[1], b[1]);
    const float inter = (iw <= 0.f || ih <= 0.f) ? 0.f : iw * ih;
    const float aa = (a[2] - a[0]) * (a[3] - a[1]), ab = (b[2] - b[0]) * (b[3] - b[1]);
    return inter / (aa + ab - inter);
}

__global__ __launch_bounds__(256) void yolo_select_kernel(float* __restrict__ out, const u64* __restrict__ all_keys, YoloArgs g)
{
    __shared__ u64 keys[kKeys];
    __shared__ float kept[FHIP_YOLO_MAX_ROWS][4];
    __shared__ float box[FHIP_YOLO_CHUNK][4];
    __shared__ unsigned char alive[FHIP_YOLO_CHUNK];
    __shared__ int s_all, s_mine, s_at;
    const int tid = threadIdx.x, img = blockIdx.x, per = g.first[g.scales];
    const u64* src = all_keys + (size_t)img * per;
    float* rows = out + (size_t)img * g.rows * 6;
    int kept_n = 0;
    u64 bound = ~0ull; // this round takes the keys below it
    for (;;)
    {
        for (int i = tid; i < kKeys; i += 256) keys[i] = 0;
        if (tid == 0) s_all = s_mine = 0;
        __syncthreads();
        int filled = 0, taken = 0, seen = 0; // keys in the buffer; keys put into it and keys below the bound seen so far in this round
        u64 cutoff = 0; // once the buffer was cut: the smallest key it kept -- 1024 better ones are held, so a key at or below it is not taken
        for (int base = 0; base < per; base += FHIP_YOLO_CHUNK)
        {
            u64 v[FHIP_YOLO_CHUNK / 256];
            int mine = 0, all = 0;
#pragma unroll
            for (int k = 0; k < FHIP_YOLO_CHUNK / 256; ++k)
            {
                const int p = base + k * 256 + tid;
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
            if (filled + total > kKeys) // sort and keep the best FHIP_YOLO_CHUNK: filled <= FHIP_YOLO_CHUNK afterwards, and a chunk fits behind them
            {
                sort_descending(keys, kKeys);
                cutoff = keys[FHIP_YOLO_CHUNK - 1];
                for (int i = FHIP_YOLO_CHUNK + tid; i < kKeys; i += 256) keys[i] = 0;
                filled = min(filled, FHIP_YOLO_CHUNK);
            }
            if (tid == 0) s_at = filled;
            __syncthreads();
#pragma unroll
            for (int k = 0; k < FHIP_YOLO_CHUNK / 256; ++k)
                if (v[k] != 0) keys[atomicAdd(&s_at, 1)] = v[k]; // the slot is arbitrary, the sort is not
            filled += total;
            __syncthreads();
        }
        int size = 2;
        while (size < filled) size <<= 1;
        sort_descending(keys, size);
        const int m = min(filled, FHIP_YOLO_CHUNK);
        if (m == 0) break;
        // the boxes of this round's candidates
        for (int i = tid; i < m; i += 256)
        {
            const unsigned r = kIndexMask - (unsigned)((keys[i] >> 8) & kIndexMask);
            const int b = bottom_of(g, r), h = g.h[b], w = g.w[b];
            const unsigned hw = (unsigned)h * (unsigned)w, local = r - (unsigned)g.first[b], pp = local / hw, cell = local - pp * hw;
            const unsigned ci = cell / (unsigned)w, cj = cell - ci * (unsigned)w;
            const float* p = g.in[b] + ((size_t)img * g.num_box + pp) * (5 + g.num_class) * hw + cell;
            const float cx = ((float)cj + sigmoid(p[0])) / (float)w, cy = ((float)ci + sigmoid(p[hw])) / (float)h;
            float bw, bh;
            if (g.version == 2)
            {
                bw = (expf(p[(size_t)2 * hw]) * g.bias_w[b][pp]) / (float)w;
                bh = (expf(p[(size_t)3 * hw]) * g.bias_h[b][pp]) / (float)h;
            }
            else
            {
                bw = (expf(p[(size_t)2 * hw]) * g.bias_w[b][pp]) / (g.anchors_scale[b] * (float)w);
                bh = (expf(p[(size_t)3 * hw]) * g.bias_h[b][pp]) / (g.anchors_scale[b] * (float)h);
            }
            box[i][0] = cx - bw * 0.5f;
            box[i][1] = cy - bh * 0.5f;
            box[i][2] = cx + bw * 0.5f;
            box[i][3] = cy + bh * 0.5f;
            // against the boxes earlier rounds kept (kept[] was last written before this round's barriers)
            unsigned char live = 1;
            for (int k = 0; k < kept_n && live; ++k)
                if (iou(kept[k], box[i]) > g.nms_threshold) live = 0;
            alive[i] = live;
        }
        // greedy NMS in key order; every lane follows the same steps, lanes 0 .. 5 write a kept candidate out.  alive[] changes only in a
        // suppression pass, and a barrier follows each: a dropped candidate is passed over without one
        __syncthreads();
        for (int i = 0; i < m && kept_n < g.rows; ++i)
        {
            if (!alive[i]) continue;
            if (tid < 4) kept[kept_n][tid] = box[i][tid];
            if (tid < 6)
            {
                const u64 key = keys[i];
                const float v = tid == 0 ? (float)((unsigned)(key & 0xffu) + 1u) : (tid == 1 ? unordered((unsigned)(key >> 32)) : box[i][tid - 2]);
                rows[(size_t)kept_n * 6 + tid] = v;
            }
            ++kept_n;
            for (int j = i + 1 + tid; j < m; j += 256)
                if (alive[j] && iou(box[i], box[j]) > g.nms_threshold) alive[j] = 0;
            __syncthreads();
        }
        if (kept_n >= g.rows || seen <= FHIP_YOLO_CHUNK) break; // full, or this round took every key there was
        bound = keys[m - 1];
        __syncthreads(); // every lane has read the bound (and the boxes) before the buffer is cleared
    }
    for (int i = kept_n * 6 + tid; i < g.rows * 6; i += 256) rows[i] = 0.f;
}

// ---- host checks -----------------------------------------------------------------------------------------------------------------------
constexpr long long kMaxElements = 1ll << 31;

static bool overlap(const void* a, size_t na, const void* b, size_t nb)
{
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}

static int reorg_dims(int stride, int c, int h, int w, int* oc, int* oh, int* ow)
{
    if (stride < 1) return fail(FHIP_E_BADARG, "Reorg stride < 1");
    if (c < 1 || h < 1 || w < 1) return fail(FHIP_E_BADARG, "a dimension < 1");
    if (h < stride || w < stride) return fail(FHIP_E_BADARG, "a plane smaller than the stride has no output");
    if ((long long)c * stride * stride >= kMaxElements) return fail(FHIP_E_BADARG, "c * stride * stride must stay below 2^31");
    *oc = c * stride * stride;
    *oh = h / stride;
    *ow = w / stride;
    return FHIP_OK;
}

static bool reorg_tiled(int stride, int w) { return stride > 1 && (long long)stride * w <= FHIP_REORG_TILE; }

// the counts and extents of a detection; -> boxes per image in *per
static int yolo_shape(int n, int scales, int num_box, int num_class, const int* h, const int* w, long long* per)
{
    if (n < 1 || n > 65535) return fail(FHIP_E_BADARG, "1 .. 65535 images");
    if (scales < 1 || scales > FHIP_YOLO_MAX_SCALES) return fail(FHIP_E_BADARG, "1 .. FHIP_YOLO_MAX_SCALES (4) bottoms");
    if (num_box < 1 || num_box > FHIP_YOLO_MAX_BOXES) return fail(FHIP_E_BADARG, "num_box must be 1 .. FHIP_YOLO_MAX_BOXES (16)");
    if (num_class < 1 || num_class > FHIP_YOLO_MAX_CLASSES) return fail(FHIP_E_BADARG, "num_class must be 1 .. FHIP_YOLO_MAX_CLASSES (256)");
    if (!h || !w) return fail(FHIP_E_BADARG, "null argument");
    long long total = 0;
    for (int b = 0; b < scales; ++b)
    {
        if (h[b] < 1 || w[b] < 1) return fail(FHIP_E_BADARG, "a dimension < 1");
        const long long cells = (long long)h[b] * w[b];
        if (cells > FHIP_YOLO_MAX_CELLS) return fail(FHIP_E_BADARG, "more than FHIP_YOLO_MAX_CELLS (2^22) boxes per image");
        total += cells * num_box;
        if (total > FHIP_YOLO_MAX_CELLS) return fail(FHIP_E_BADARG, "more than FHIP_YOLO_MAX_CELLS (2^22) boxes per image");
        if ((long long)n * num_box * (5 + num_class) * cells >= kMaxElements) return fail(FHIP_E_BADARG, "tensors of 2^31 elements or more are not supported");
    }
    if ((long long)n * total >= kMaxElements) return fail(FHIP_E_BADARG, "n * boxes per image must stay below 2^31");
    *per = total;
    return FHIP_OK;
}

} // namespace fhip

using namespace fhip;

extern "C"
{

int fhip_reorg_output_dim(int stride, int c, int h, int w, int* out_c, int* out_h, int* out_w)
{
    if (!out_c || !out_h || !out_w) return fail(FHIP_E_BADARG, "null argument");
    return reorg_dims(stride, c, h, w, out_c, out_h, out_w);
}

int fhip_reorg_forward(int stride, int mode, int n, int c, int h, int w, float* out, const float* in, void* stream)
{
    int oc, oh, ow;
    const int rc = reorg_dims(stride, c, h, w, &oc, &oh, &ow);
    if (rc) return rc;
    if (mode != 0 && mode != 1) return fail(FHIP_E_BADARG, "Reorg mode must be 0 or 1");
    if (n < 1) return fail(FHIP_E_BADARG, "n < 1");
    const long long total_in = (long long)n * c * h * w, total = (long long)n * oc * oh * ow;
    if (total_in >= kMaxElements) return fail(FHIP_E_BADARG, "tensors of 2^31 elements or more are not supported");
    if (!out || !in) return fail(FHIP_E_BADARG, "null pointer");
    if (!aligned(out, 4) || !aligned(in, 4)) return fail(FHIP_E_BADARG, "pointers must be 4-byte aligned");
    if (overlap(out, (size_t)total * 4, in, (size_t)total_in * 4)) return fail(FHIP_E_BADARG, "out must not overlap in");
    hipStream_t s = (hipStream_t)stream;
    if (reorg_tiled(stride, w))
    {
        const int group = std::max(1, std::min(oh, FHIP_REORG_TILE / (stride * w))), groups = (oh + group - 1) / group;
        const long long blocks = (long long)n * c * groups; // <= n * c * h < 2^31
        hipLaunchKernelGGL(reorg_tile_kernel, dim3((unsigned)blocks), dim3(256), 0, s, out, in, stride, mode, c, h, w, oh, ow, group, groups);
    }
    else
        hipLaunchKernelGGL(reorg_direct_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, out, in, (unsigned)total, stride, mode, c, h, w, oh, ow);
    FHIP_CHECK_HIP(hipGetLastError());
    return FHIP_OK;
}

int fhip_yolo_get_buffer_size(int n, int scales, int num_box, int num_class, const int* h, const int* w, size_t* bytes)
{
    long long per;
    const int rc = yolo_shape(n, scales, num_box, num_class, h, w, &per);
    if (rc) return rc;
    if (!bytes) return fail(FHIP_E_BADARG, "null argument");
    *bytes = (size_t)n * (size_t)per * sizeof(u64);
    return FHIP_OK;
}

int fhip_yolo_detection_forward(int version, int n, int scales, int num_box, int num_class, const int* h, const int* w, float confidence_threshold,
                                float nms_threshold, const float* biases, int num_biases, const int* mask, const float* anchors_scale, int rows, float* out,
                                const float* const* bottoms, void* scratch, void* stream)
{
    if (version != 2 && version != 3) return fail(FHIP_E_BADARG, "version must be 2 (YoloDetectionOutput) or 3 (Yolov3DetectionOutput)");
    long long per;
    const int rc = yolo_shape(n, scales, num_box, num_class, h, w, &per);
    if (rc) return rc;
    if (rows < 1 || rows > FHIP_YOLO_MAX_ROWS) return fail(FHIP_E_BADARG, "rows must be 1 .. FHIP_YOLO_MAX_ROWS (1024)");
    if (!std::isfinite(confidence_threshold) || !std::isfinite(nms_threshold)) return fail(FHIP_E_BADARG, "thresholds must be finite");
    if (!biases || num_biases < 2 || num_biases % 2 || num_biases > 2 * FHIP_YOLO_MAX_SCALES * FHIP_YOLO_MAX_BOXES)
        return fail(FHIP_E_BADARG, "biases: an even count of 2 .. 128 floats");
    for (int k = 0; k < num_biases; ++k)
        if (!std::isfinite(biases[k])) return fail(FHIP_E_BADARG, "biases must be finite");
    if (version == 2 && num_biases < 2 * num_box) return fail(FHIP_E_BADARG, "fewer than 2 * num_box biases");
    if (version == 3 && (!mask || !anchors_scale)) return fail(FHIP_E_BADARG, "version 3 needs mask and anchors_scale");
    if (!out || !bottoms || !scratch) return fail(FHIP_E_BADARG, "null pointer");
    if (!aligned(out, 4) || !aligned(scratch, 8)) return fail(FHIP_E_BADARG, "pointers must be 4-byte aligned (scratch: 8)");
    const size_t out_bytes = (size_t)n * rows * 6 * 4, scratch_bytes = (size_t)n * (size_t)per * sizeof(u64);
    if (overlap(out, out_bytes, scratch, scratch_bytes)) return fail(FHIP_E_BADARG, "out must not overlap scratch");
    YoloArgs g;
    memset(&g, 0, sizeof(g));
    int first = 0;
    for (int b = 0; b < scales; ++b)
    {
        if (!bottoms[b] || !aligned(bottoms[b], 4)) return fail(FHIP_E_BADARG, "null or unaligned bottom");
        const size_t bytes = (size_t)n * num_box * (5 + num_class) * h[b] * w[b] * 4;
        if (overlap(out, out_bytes, bottoms[b], bytes) || overlap(scratch, scratch_bytes, bottoms[b], bytes))
            return fail(FHIP_E_BADARG, "out and scratch must not overlap a bottom");
        g.in[b] = bottoms[b];
        g.h[b] = h[b];
        g.w[b] = w[b];
        g.first[b] = first;
        first += num_box * h[b] * w[b];
        g.anchors_scale[b] = 1.f;
        if (version == 3)
        {
            if (!std::isfinite(anchors_scale[b]) || !(anchors_scale[b] > 0.f)) return fail(FHIP_E_BADARG, "anchors_scale must be finite and > 0");
            g.anchors_scale[b] = anchors_scale[b];
        }
        for (int pp = 0; pp < num_box; ++pp)
        {
            int a = pp;
            if (version == 3)
            {
                a = mask[b * num_box + pp];
                if (a < 0 || a >= num_biases / 2) return fail(FHIP_E_BADARG, "a mask entry outside the anchors");
            }
            g.bias_w[b][pp] = biases[2 * a];
            g.bias_h[b][pp] = biases[2 * a + 1];
        }
    }
    for (int b = scales; b <= FHIP_YOLO_MAX_SCALES; ++b) g.first[b] = first;
    g.scales = scales;
    g.num_box = num_box;
    g.num_class = num_class;
    g.version = version;
    g.rows = rows;
    g.confidence_threshold = confidence_threshold;
    g.nms_threshold = nms_threshold;
    hipStream_t s = (hipStream_t)stream;
    const unsigned total = (unsigned)((long long)n * per);
    if (version == 2)
        hipLaunchKernelGGL(yolo_score_kernel<2>, dim3((total + 255) / 256), dim3(256), 0, s, (u64*)scratch, g, total);
    else
        hipLaunchKernelGGL(yolo_score_kernel<3>, dim3((total + 255) / 256), dim3(256), 0, s, (u64*)scratch, g, total);
    FHIP_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(yolo_select_kernel, dim3((unsigned)n), dim3(256), 0, s, out, (const u64*)scratch, g);
    FHIP_CHECK_HIP(hipGetLastError());
    return FHIP_OK;
}

int fhip_yolo_route(int what, int a, int b, char* name, int len)
{
    if (!name || len < 1) return fail(FHIP_E_BADARG, "null name");
    switch (what)
    {
    case FHIP_YOLO_REORG:
        if (a < 1 || b < 1) return fail(FHIP_E_BADARG, "stride or w < 1");
        snprintf(name, (size_t)len, reorg_tiled(a, b) ? "fhip::reorg_tile_kernel" : "fhip::reorg_direct_kernel");
        return FHIP_OK;
    case FHIP_YOLO_SCORE:
        if (a != 2 && a != 3) return fail(FHIP_E_BADARG, "version must be 2 or 3");
        snprintf(name, (size_t)len, "fhip::yolo_score_kernel<%d>", a);
        return FHIP_OK;
    case FHIP_YOLO_SELECT: snprintf(name, (size_t)len, "fhip::yolo_select_kernel"); return FHIP_OK;
    default: return fail(FHIP_E_BADARG, "unknown operation");
    }
}

const char* fhip_yolo_last_error(void) { return last_error(); }

} // extern "C"
