// libfeather_detect.so: the layers of an SSD detection head on gfx950 (include/feather_hip/feather_detect.h is the contract and the
// definition; DESIGN.md 3.23 the design and its measurements).
//
//   permute_tile_kernel       batched transposes of [rows][cols] matrices through a 32 x 33 LDS tile: loads run along the input's rows, stores
//                             along the output's, both coalesced; ragged tiles are guarded, so 19 x 19 or 1 x 1 planes and 12 or 63 channels
//                             take the same path (Permute order 3: NCHW -> NHWC, and order 1: the transpose of every plane)
//   permute_concat_kernel     the same transpose for up to FHIP_PERMUTE_CONCAT_MAX sources at once, each written into its slice of one concatenated
//                             row per image (Concat of Flatten of Permute order 3): the sources' pointers and extents travel as kernel arguments
//   permute_generic_kernel    every other order: one output element per lane, coalesced stores, strided loads
//   normalize_kernel<V>       lanes along the pixels of an image, V = 4 adjacent pixels per lane as one 16-byte access or V = 1; two passes
//                             over the channels: the sum of squares in ascending c, then the scaled values (the second pass hits the caches)
//   axis_softmax_kernel       one lane per (outer, inner) pair walks the axis three times: max, sum of exp, quotient
//   detect_select_kernel      DetectionOutput, a block per (class, image): the candidates above the threshold are compacted chunk by chunk
//                             (FHIP_DETECT_CHUNK priors) into an LDS buffer of 2048 keys (score, prior) with an LDS counter, and the buffer is
//                             sorted (bitonic, descending) and cut to nms_top_k whenever the next chunk would not fit -- so the order never
//                             depends on which lane's atomic came first and no candidate count is capped; then the boxes of the selected priors
//                             alone are decoded into LDS and the greedy NMS runs there, one step per candidate, lanes along the later candidates
//   detect_merge_kernel       a block per image: the survivors of all classes through the same buffer and sort, keyed (score, class, rank in
//                             the class), cut to keep_top_k; writes every row of the output, zeros past the count
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

#include "feather_hip/feather_detect.h"
#include "side_error.h"

#pragma clang fp contract(off)

namespace fhip
{

typedef unsigned long long u64;

constexpr int kTile = 32;
constexpr int kKeys = 2 * FHIP_DETECT_MAX_TOP_K; // keys of the selection buffer: the kept ones and a chunk's candidates
static_assert(FHIP_DETECT_CHUNK + FHIP_DETECT_MAX_TOP_K <= kKeys, "a chunk's candidates fit behind the kept keys");

// ---- Permute ---------------------------------------------------------------------------------------------------------------------------
// out[b][col][row] = in[b][row][col] for `batch` matrices; blockIdx.x runs over batch x row tiles x column tiles
__global__ __launch_bounds__(256) void permute_tile_kernel(float* __restrict__ out, const float* __restrict__ in, int rows, int cols, int tiles_r, int tiles_c)
{
    __shared__ float tile[kTile][kTile + 1];
    const unsigned per = (unsigned)tiles_r * tiles_c;
    const unsigned b = blockIdx.x / per, t = blockIdx.x - b * per;
    const int r0 = (int)(t / tiles_c) * kTile, c0 = (int)(t % tiles_c) * kTile;
    const int tx = threadIdx.x & (kTile - 1), ty = threadIdx.x / kTile; // 32 x 8
    const float* src = in + (size_t)b * rows * cols;
    float* dst = out + (size_t)b * rows * cols;
    for (int k = ty; k < kTile; k += 8)
        if (r0 + k < rows && c0 + tx < cols) tile[k][tx] = src[(size_t)(r0 + k) * cols + c0 + tx];
    __syncthreads();
    for (int k = ty; k < kTile; k += 8)
        if (c0 + k < cols && r0 + tx < rows) dst[(size_t)(c0 + k) * rows + r0 + tx] = tile[tx][k];
}

// The sources of permute_concat_kernel: source i is [n][c][hw], starts `offset` floats into every image's row of `total` floats and owns the
// blocks [first[i], first[i + 1]) of an image, its tiles row-major.
struct ConcatSources
{
    const float* in[FHIP_PERMUTE_CONCAT_MAX];
    int c[FHIP_PERMUTE_CONCAT_MAX], hw[FHIP_PERMUTE_CONCAT_MAX], offset[FHIP_PERMUTE_CONCAT_MAX], first[FHIP_PERMUTE_CONCAT_MAX + 1];
    int count, total;
};

// out[img][offset_i + p * c_i + ch] = in_i[img][ch][p]
__global__ __launch_bounds__(256) void permute_concat_kernel(float* __restrict__ out, ConcatSources g)
{
    __shared__ float tile[kTile][kTile + 1];
    const unsigned per = (unsigned)g.first[g.count];
    const unsigned img = blockIdx.x / per, t0 = blockIdx.x - img * per;
    int i = 0;
    while (i + 1 < g.count && t0 >= (unsigned)g.first[i + 1]) ++i;
    const int rows = g.c[i], cols = g.hw[i], tiles_c = (cols + kTile - 1) / kTile;
    const unsigned t = t0 - (unsigned)g.first[i];
    const int r0 = (int)(t / tiles_c) * kTile, c0 = (int)(t % tiles_c) * kTile;
    const int tx = threadIdx.x & (kTile - 1), ty = threadIdx.x / kTile;
    const float* src = g.in[i] + (size_t)img * rows * cols;
    float* dst = out + (size_t)img * g.total + g.offset[i];
    for (int k = ty; k < kTile; k += 8)
        if (r0 + k < rows && c0 + tx < cols) tile[k][tx] = src[(size_t)(r0 + k) * cols + c0 + tx];
    __syncthreads();
    for (int k = ty; k < kTile; k += 8)
        if (c0 + k < cols && r0 + tx < rows) dst[(size_t)(c0 + k) * rows + r0 + tx] = tile[tx][k];
}

// out[b][oc][oh][ow] = in[b][...]: (sw, sh, sc) are the input strides of the dimensions that became the output's w, h and c
__global__ __launch_bounds__(256) void permute_generic_kernel(float* __restrict__ out, const float* __restrict__ in, unsigned total, int ow, int oh, int oc, int sw,
                                                              int sh, int sc)
{
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= total) return;
    const unsigned x = i % (unsigned)ow, r = i / (unsigned)ow;
    const unsigned y = r % (unsigned)oh, q = r / (unsigned)oh;
    const unsigned ch = q % (unsigned)oc, b = q / (unsigned)oc;
    out[i] = in[(size_t)b * oc * oh * ow + (size_t)x * sw + (size_t)y * sh + (size_t)ch * sc];
}

// ---- Normalize -------------------------------------------------------------------------------------------------------------------------
template <int V>
__global__ __launch_bounds__(256) void normalize_kernel(float* __restrict__ out, const float* __restrict__ in, const float* __restrict__ scale, int shared_scale,
                                                        float eps, int c, unsigned hw, unsigned groups /* n * hw / V */)
{
    const unsigned g = blockIdx.x * 256u + threadIdx.x;
    if (g >= groups) return;
    const unsigned per = hw / V, img = g / per, at = (g - img * per) * V;
    const float* x = in + (size_t)img * c * hw + at;
    float* y = out + (size_t)img * c * hw + at;
    float s[V];
#pragma unroll
    for (int k = 0; k < V; ++k) s[k] = 0.f;
    // eight channels' loads in flight per lane: at batch 1 a plane has a few hundred lanes and the loop is bound by load latency; the adds stay
    // in ascending c
#pragma unroll 8
    for (int ch = 0; ch < c; ++ch)
    {
        float v[V];
        if constexpr (V == 4)
        {
            const float4 q = *reinterpret_cast<const float4*>(x + (size_t)ch * hw);
            v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
        }
        else
            v[0] = x[(size_t)ch * hw];
#pragma unroll
        for (int k = 0; k < V; ++k) s[k] = s[k] + v[k] * v[k];
    }
    float a[V];
#pragma unroll
    for (int k = 0; k < V; ++k) a[k] = 1.f / sqrtf(s[k] + eps);
#pragma unroll 8
    for (int ch = 0; ch < c; ++ch)
    {
        const float m = scale[shared_scale ? 0 : ch];
        if constexpr (V == 4)
        {
            const float4 q = *reinterpret_cast<const float4*>(x + (size_t)ch * hw);
            float4 r;
            r.x = (q.x * a[0]) * m, r.y = (q.y * a[1]) * m, r.z = (q.z * a[2]) * m, r.w = (q.w * a[3]) * m;
            *reinterpret_cast<float4*>(y + (size_t)ch * hw) = r;
        }
        else
            y[(size_t)ch * hw] = (x[(size_t)ch * hw] * a[0]) * m;
    }
}

// ---- softmax along the middle axis of [outer][len][inner] --------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void axis_softmax_kernel(float* __restrict__ out, const float* __restrict__ in, unsigned pairs, int len, unsigned inner)
{
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= pairs) return;
    const unsigned o = i / inner, r = i - o * inner;
    const float* x = in + (size_t)o * len * inner + r;
    float* y = out + (size_t)o * len * inner + r;
    float m = -FLT_MAX;
    for (int k = 0; k < len; ++k) m = fmaxf(m, x[(size_t)k * inner]);
    float sum = 0.f;
    for (int k = 0; k < len; ++k) sum = sum + expf(x[(size_t)k * inner] - m);
    for (int k = 0; k < len; ++k) y[(size_t)k * inner] = expf(x[(size_t)k * inner] - m) / sum;
}

// ---- DetectionOutput -------------------------------------------------------------------------------------------------------------------
// a float as an unsigned that orders the same way (NaN never gets here), and back
__device__ __forceinline__ unsigned ordered(float f)
{
    const unsigned b = f == 0.f ? 0u : __float_as_uint(f); // -0.f is 0.f
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float unordered(unsigned u) { return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u); }

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

// The buffer holds `filled` keys (zeros behind them) and `more` are about to come: if they would not fit, sort and keep the first `keep`.
// Uniform over the block; -> the new `filled`.
__device__ int make_room(u64* keys, int filled, int more, int keep)
{
    if (filled + more <= kKeys) return filled;
    __syncthreads();
    sort_descending(keys, kKeys);
    for (int i = keep + threadIdx.x; i < kKeys; i += 256) keys[i] = 0;
    __syncthreads();
    return min(filled, keep);
}

// keys[0, filled) (zeros behind) sorted descending; -> min(filled, keep)
__device__ int finish_keys(u64* keys, int filled, int keep)
{
    int size = 2;
    while (size < filled) size <<= 1;
    __syncthreads();
    sort_descending(keys, size);
    return min(filled, keep);
}

struct DetectArgs
{
    int num_priors, num_class, nms_top_k, keep_top_k, per_class; // per_class = min(nms_top_k, keep_top_k): survivors a class hands on
    float nms_threshold, confidence_threshold;
    int prior_per_image; // 0: one set of priors for the batch
};

__device__ __forceinline__ float iou(const float* a, const float* b)
{
    const float iw = fminf(a[2], b[2]) - fmaxf(a[0], b[0]), ih = fminf(a[3], b[3]) - fmaxf(a[1], b[1]);
    const float inter = (iw <= 0.f || ih <= 0.f) ? 0.f : iw * ih;
    const float aa = (a[2] - a[0]) * (a[3] - a[1]), ab = (b[2] - b[0]) * (b[3] - b[1]);
    return inter / (aa + ab - inter);
}

// scratch: int count[n][num_class], then (8-byte aligned) float box[n][num_class][per_class][4], then unsigned score[n][num_class][per_class]
__device__ __forceinline__ size_t scratch_boxes_at(int n, int num_class) { return ((size_t)n * num_class * sizeof(int) + 15) / 16 * 16; }

__global__ __launch_bounds__(256) void detect_select_kernel(unsigned char* __restrict__ scratch, const float* __restrict__ location,
                                                            const float* __restrict__ confidence, const float* __restrict__ priorbox, DetectArgs g, int n)
{
    __shared__ u64 keys[kKeys];
    __shared__ float box[FHIP_DETECT_MAX_TOP_K][4];
    __shared__ unsigned char alive[FHIP_DETECT_MAX_TOP_K];
    __shared__ int s_total, s_at;
    const int tid = threadIdx.x, cls = blockIdx.x + 1, img = blockIdx.y, P = g.num_priors;
    const float* conf = confidence + (size_t)img * P * g.num_class + cls;
    for (int i = tid; i < kKeys; i += 256) keys[i] = 0;
    if (tid == 0) s_total = 0;
    __syncthreads();
    int filled = 0;
    for (int base = 0; base < P; base += FHIP_DETECT_CHUNK)
    {
        float v[FHIP_DETECT_CHUNK / 256];
        int mine = 0;
#pragma unroll
        for (int k = 0; k < FHIP_DETECT_CHUNK / 256; ++k)
        {
            const int p = base + k * 256 + tid;
            v[k] = p < P ? conf[(size_t)p * g.num_class] : __uint_as_float(0x7fc00000u);
            mine += v[k] > g.confidence_threshold ? 1 : 0;
        }
        if (mine) atomicAdd(&s_total, mine);
        __syncthreads();
        const int total = s_total; // a sum: the same whatever the order of the atomics
        __syncthreads();
        if (total == 0) continue;
        filled = make_room(keys, filled, total, g.nms_top_k);
        if (tid == 0)
        {
            s_at = filled;
            s_total = 0;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < FHIP_DETECT_CHUNK / 256; ++k)
            if (v[k] > g.confidence_threshold)
            {
                const int p = base + k * 256 + tid;
                keys[atomicAdd(&s_at, 1)] = ((u64)ordered(v[k]) << 32) | (0xffffffffu - (unsigned)p); // the slot is arbitrary, the sort is not
            }
        filled += total;
        __syncthreads();
    }
    const int m = finish_keys(keys, filled, g.nms_top_k);
    // the boxes of the selected priors
    const float* prior = priorbox + (g.prior_per_image ? (size_t)img * 8 * P : 0);
    const float* loc = location + (size_t)img * 4 * P;
    for (int i = tid; i < m; i += 256)
    {
        const size_t p = 0xffffffffu - (unsigned)(keys[i] & 0xffffffffu);
        const float x0 = prior[4 * p], y0 = prior[4 * p + 1], x1 = prior[4 * p + 2], y1 = prior[4 * p + 3];
        const float* var = prior + (size_t)4 * P + 4 * p;
        const float pw = x1 - x0, ph = y1 - y0, pcx = (x0 + x1) * 0.5f, pcy = (y0 + y1) * 0.5f;
        const float cx = (var[0] * loc[4 * p]) * pw + pcx, cy = (var[1] * loc[4 * p + 1]) * ph + pcy;
        const float bw = expf(var[2] * loc[4 * p + 2]) * pw, bh = expf(var[3] * loc[4 * p + 3]) * ph;
        box[i][0] = cx - bw * 0.5f;
        box[i][1] = cy - bh * 0.5f;
        box[i][2] = cx + bw * 0.5f;
        box[i][3] = cy + bh * 0.5f;
        alive[i] = 1;
    }
    // greedy NMS in key order; every lane follows the same steps, lanes 0 .. 4 write a kept candidate out
    const size_t slot0 = ((size_t)img * g.num_class + cls) * g.per_class;
    float* out_box = reinterpret_cast<float*>(scratch + scratch_boxes_at(n, g.num_class)) + slot0 * 4;
    unsigned* out_score = reinterpret_cast<unsigned*>(scratch + scratch_boxes_at(n, g.num_class) + (size_t)n * g.num_class * g.per_class * 16) + slot0;
    int kept = 0;
    for (int i = 0; i < m && kept < g.per_class; ++i)
    {
        __syncthreads();
        if (!alive[i]) continue;
        if (tid < 4) out_box[(size_t)kept * 4 + tid] = box[i][tid];
        if (tid == 4) out_score[kept] = (unsigned)(keys[i] >> 32);
        ++kept;
        for (int j = i + 1 + tid; j < m; j += 256)
            if (alive[j] && iou(box[i], box[j]) > g.nms_threshold) alive[j] = 0;
    }
    if (tid == 0) reinterpret_cast<int*>(scratch)[(size_t)img * g.num_class + cls] = kept;
}

__global__ __launch_bounds__(256) void detect_merge_kernel(float* __restrict__ out, const unsigned char* __restrict__ scratch, DetectArgs g, int n)
{
    __shared__ u64 keys[kKeys];
    const int tid = threadIdx.x, img = blockIdx.x;
    const int* count = reinterpret_cast<const int*>(scratch) + (size_t)img * g.num_class;
    const float* boxes = reinterpret_cast<const float*>(scratch + scratch_boxes_at(n, g.num_class)) + (size_t)img * g.num_class * g.per_class * 4;
    const unsigned* scores = reinterpret_cast<const unsigned*>(scratch + scratch_boxes_at(n, g.num_class) + (size_t)n * g.num_class * g.per_class * 16) +
                             (size_t)img * g.num_class * g.per_class;
    for (int i = tid; i < kKeys; i += 256) keys[i] = 0;
    __syncthreads();
    int filled = 0;
    for (int cls = 1; cls < g.num_class; ++cls)
    {
        const int cnt = count[cls]; // <= per_class <= 1024
        if (cnt == 0) continue;
        filled = make_room(keys, filled, cnt, g.keep_top_k);
        // rank within the class stands for the prior: a class's survivors are in (score descending, prior ascending) order
        for (int i = tid; i < cnt; i += 256)
            keys[filled + i] = ((u64)scores[(size_t)cls * g.per_class + i] << 32) | ((u64)(0xffu - (unsigned)cls) << 16) | (0xffffu - (unsigned)i);
        filled += cnt;
    }
    const int m = finish_keys(keys, filled, g.keep_top_k);
    float* rows = out + (size_t)img * g.keep_top_k * 6;
    for (int r = tid; r < g.keep_top_k; r += 256)
    {
        float v[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (r < m)
        {
            const u64 k = keys[r];
            const int cls = 0xff - (int)((k >> 16) & 0xff), i = 0xffff - (int)(k & 0xffff);
            const float* b = boxes + ((size_t)cls * g.per_class + i) * 4;
            v[0] = (float)cls, v[1] = unordered((unsigned)(k >> 32)), v[2] = b[0], v[3] = b[1], v[4] = b[2], v[5] = b[3];
        }
#pragma unroll
        for (int k = 0; k < 6; ++k) rows[(size_t)r * 6 + k] = v[k];
    }
}

// ---- host checks -----------------------------------------------------------------------------------------------------------------------
constexpr long long kMaxElements = 1ll << 31;

static bool overlap(const void* a, size_t na, const void* b, size_t nb)
{
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}

static int check_pair(const float* out, const float* in, size_t count)
{
    if (!out || !in) return fail(FHIP_E_BADARG, "null pointer");
    if (!aligned(out, 4) || !aligned(in, 4)) return fail(FHIP_E_BADARG, "pointers must be 4-byte aligned");
    if (overlap(out, count * 4, in, count * 4)) return fail(FHIP_E_BADARG, "out must not overlap in");
    return FHIP_OK;
}

static int permute_dims(int order, int dims, int c, int h, int w, int* oc, int* oh, int* ow)
{
    if (dims != 2 && dims != 3) return fail(FHIP_E_BADARG, "Permute takes a blob of rank 2 or 3");
    if (order < 0 || order > 5 || (dims == 2 && order > 1)) return fail(FHIP_E_BADARG, "order_type must be 0 .. 5 (0 .. 1 at rank 2)");
    if (c < 1 || h < 1 || w < 1 || (dims == 2 && c != 1)) return fail(FHIP_E_BADARG, "a dimension < 1 (or c != 1 at rank 2)");
    const int src[6][3] = {{0, 1, 2}, {1, 0, 2}, {0, 2, 1}, {2, 0, 1}, {1, 2, 0}, {2, 1, 0}}; // the old dimension (w, h, c = 0, 1, 2) behind the new w, h, c
    const int old[3] = {w, h, c};
    *ow = old[src[order][0]];
    *oh = old[src[order][1]];
    *oc = old[src[order][2]];
    return FHIP_OK;
}

static bool permute_tiled(int order, int dims) { return order == 1 || (order == 3 && dims == 3); }

static bool normalize_v4(int h, int w, const float* out, const float* in) { return ((size_t)h * w) % 4 == 0 && aligned(out, 16) && aligned(in, 16); }

static int normalize_args(int n, int c, int h, int w, float eps)
{
    if (n < 1 || c < 1 || h < 1 || w < 1) return fail(FHIP_E_BADARG, "a dimension < 1");
    if ((long long)n * c * h * w >= kMaxElements) return fail(FHIP_E_BADARG, "tensors of 2^31 elements or more are not supported");
    if (!std::isfinite(eps) || !(eps > 0.f)) return fail(FHIP_E_BADARG, "eps must be finite and > 0");
    return FHIP_OK;
}

static int detect_args(int n, int P, int num_class, int nms_top_k, int keep_top_k, DetectArgs& g)
{
    if (n < 1 || n > 65535) return fail(FHIP_E_BADARG, "1 .. 65535 images");
    if (P < 1 || P > FHIP_DETECT_MAX_PRIORS) return fail(FHIP_E_BADARG, "1 .. FHIP_DETECT_MAX_PRIORS (2^22) priors");
    if (num_class < 2 || num_class > FHIP_DETECT_MAX_CLASSES) return fail(FHIP_E_BADARG, "2 .. FHIP_DETECT_MAX_CLASSES (256) classes, the background included");
    if (nms_top_k < 1 || nms_top_k > FHIP_DETECT_MAX_TOP_K) return fail(FHIP_E_BADARG, "nms_top_k must be 1 .. FHIP_DETECT_MAX_TOP_K (1024)");
    if (keep_top_k < 1 || keep_top_k > FHIP_DETECT_MAX_TOP_K) return fail(FHIP_E_BADARG, "keep_top_k must be 1 .. FHIP_DETECT_MAX_TOP_K (1024)");
    if ((long long)n * P * num_class >= kMaxElements) return fail(FHIP_E_BADARG, "n * priors * classes must stay below 2^31");
    g.num_priors = P;
    g.num_class = num_class;
    g.nms_top_k = nms_top_k;
    g.keep_top_k = keep_top_k;
    g.per_class = std::min(nms_top_k, keep_top_k);
    return FHIP_OK;
}

static size_t detect_scratch_bytes(int n, const DetectArgs& g)
{
    return ((size_t)n * g.num_class * sizeof(int) + 15) / 16 * 16 + (size_t)n * g.num_class * g.per_class * (16 + 4);
}

} // namespace fhip

using namespace fhip;

extern "C"
{

int fhip_permute_output_dim(int order_type, int dims, int c, int h, int w, int* out_c, int* out_h, int* out_w)
{
    if (!out_c || !out_h || !out_w) return fail(FHIP_E_BADARG, "null argument");
    return permute_dims(order_type, dims, c, h, w, out_c, out_h, out_w);
}

int fhip_permute_forward(int order_type, int dims, int n, int c, int h, int w, float* out, const float* in, void* stream)
{
    int oc, oh, ow;
    int rc = permute_dims(order_type, dims, c, h, w, &oc, &oh, &ow);
    if (rc) return rc;
    if (n < 1) return fail(FHIP_E_BADARG, "n < 1");
    const long long total = (long long)n * c * h * w;
    if (total >= kMaxElements) return fail(FHIP_E_BADARG, "tensors of 2^31 elements or more are not supported");
    if ((rc = check_pair(out, in, (size_t)total))) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (permute_tiled(order_type, dims))
    {
        // order 3: [c][h * w] -> [h * w][c] per image; order 1: [h][w] -> [w][h] per plane
        const int rows = order_type == 3 ? c : h, cols = order_type == 3 ? h * w : w;
        const long long batch = order_type == 3 ? n : (long long)n * c;
        const int tr = (rows + kTile - 1) / kTile, tc = (cols + kTile - 1) / kTile;
        const long long blocks = batch * tr * tc;
        if (blocks >= kMaxElements) return fail(FHIP_E_BADARG, "more than 2^31 - 1 blocks");
        hipLaunchKernelGGL(permute_tile_kernel, dim3((unsigned)blocks), dim3(256), 0, s, out, in, rows, cols, tr, tc);
    }
    else
    {
        const int src[6][3] = {{0, 1, 2}, {1, 0, 2}, {0, 2, 1}, {2, 0, 1}, {1, 2, 0}, {2, 1, 0}};
        const int stride[3] = {1, w, h * w};
        hipLaunchKernelGGL(permute_generic_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, out, in, (unsigned)total, ow, oh, oc,
                           stride[src[order_type][0]], stride[src[order_type][1]], stride[src[order_type][2]]);
    }
    FHIP_CHECK_HIP(hipGetLastError());
    return FHIP_OK;
}

int fhip_permute_concat_forward(int sources, const int* c, const int* hw, int n, float* out, const float* const* in, void* stream)
{
    if (sources < 1 || sources > FHIP_PERMUTE_CONCAT_MAX) return fail(FHIP_E_BADARG, "1 .. FHIP_PERMUTE_CONCAT_MAX (8) sources");
    if (!c || !hw || !in || !out || n < 1) return fail(FHIP_E_BADARG, "null argument or n < 1");
    if (!aligned(out, 4)) return fail(FHIP_E_BADARG, "pointers must be 4-byte aligned");
    ConcatSources g;
    memset(&g, 0, sizeof(g));
    long long total = 0, blocks = 0;
    for (int i = 0; i < sources; ++i)
    {
        if (c[i] < 1 || hw[i] < 1) return fail(FHIP_E_BADARG, "a dimension < 1");
        if (!in[i] || !aligned(in[i], 4)) return fail(FHIP_E_BADARG, "null or unaligned source");
        g.in[i] = in[i];
        g.c[i] = c[i];
        g.hw[i] = hw[i];
        g.offset[i] = (int)total;
        g.first[i] = (int)blocks;
        total += (long long)c[i] * hw[i];
        blocks += (long long)((c[i] + kTile - 1) / kTile) * ((hw[i] + kTile - 1) / kTile);
        if (total * n >= kMaxElements || blocks * n >= kMaxElements) return fail(FHIP_E_BADARG, "tensors of 2^31 elements or more are not supported");
    }
    for (int i = 0; i < sources; ++i)
        if (overlap(out, (size_t)total * n * 4, in[i], (size_t)c[i] * hw[i] * n * 4)) return fail(FHIP_E_BADARG, "out must not overlap a source");
    g.first[sources] = (int)blocks;
    g.count = sources;
    g.total = (int)total;
    hipLaunchKernelGGL(permute_concat_kernel, dim3((unsigned)(blocks * n)), dim3(256), 0, (hipStream_t)stream, out, g);
    FHIP_CHECK_HIP(hipGetLastError());
    return FHIP_OK;
}

int fhip_normalize_forward(int n, int c, int h, int w, int channel_shared, float eps, float* out, const float* in, const float* scale, void* stream)
{
    int rc = normalize_args(n, c, h, w, eps);
    if (rc) return rc;
    const size_t total = (size_t)n * c * h * w;
    if ((rc = check_pair(out, in, total))) return rc;
    if (!scale || !aligned(scale, 4)) return fail(FHIP_E_BADARG, "null or unaligned scale");
    const unsigned hw = (unsigned)h * (unsigned)w;
    if (normalize_v4(h, w, out, in))
    {
        const unsigned groups = (unsigned)((size_t)n * hw / 4);
        hipLaunchKernelGGL(normalize_kernel<4>, dim3((groups + 255) / 256), dim3(256), 0, (hipStream_t)stream, out, in, scale, channel_shared != 0, eps, c, hw, groups);
    }
    else
    {
        const unsigned groups = (unsigned)((size_t)n * hw);
        hipLaunchKernelGGL(normalize_kernel<1>, dim3((groups + 255) / 256), dim3(256), 0, (hipStream_t)stream, out, in, scale, channel_shared != 0, eps, c, hw, groups);
    }
    FHIP_CHECK_HIP(hipGetLastError());
    return FHIP_OK;
}

int fhip_axis_softmax_forward(int outer, int len, int inner, float* out, const float* in, void* stream)
{
    if (outer < 1 || len < 1 || inner < 1) return fail(FHIP_E_BADARG, "an extent < 1");
    const long long total = (long long)outer * len * inner;
    if (total >= kMaxElements) return fail(FHIP_E_BADARG, "tensors of 2^31 elements or more are not supported");
    const int rc = check_pair(out, in, (size_t)total);
    if (rc) return rc;
    const unsigned pairs = (unsigned)((long long)outer * inner);
    hipLaunchKernelGGL(axis_softmax_kernel, dim3((pairs + 255) / 256), dim3(256), 0, (hipStream_t)stream, out, in, pairs, len, (unsigned)inner);
    FHIP_CHECK_HIP(hipGetLastError());
    return FHIP_OK;
}

int fhip_priorbox_fill(int h, int w, int image_w, int image_h, const float* min_sizes, int num_min, const float* max_sizes, int num_max,
                       const float* aspect_ratios, int num_ratios, const float* variances, int flip, int clip, float step_w, float step_h, float offset,
                       int* num_prior, float* out, size_t capacity)
{
    if (h < 1 || w < 1 || image_w < 1 || image_h < 1) return fail(FHIP_E_BADARG, "feature map and image extents must be at least 1");
    if (num_min < 1 || !min_sizes) return fail(FHIP_E_BADARG, "PriorBox needs at least one min_size");
    if (num_max != 0 && num_max != num_min) return fail(FHIP_E_BADARG, "max_sizes must be absent or as many as min_sizes");
    if (num_ratios < 0 || (num_max && !max_sizes) || (num_ratios && !aspect_ratios) || !variances) return fail(FHIP_E_BADARG, "null array or negative count");
    if (num_min > 4096 || num_ratios > 4096) return fail(FHIP_E_BADARG, "more than 4096 sizes or aspect ratios");
    const auto positive = [](float v) { return std::isfinite(v) && v > 0.f; };
    for (int k = 0; k < num_min; ++k)
        if (!positive(min_sizes[k]) || (num_max && !positive(max_sizes[k]))) return fail(FHIP_E_BADARG, "min_sizes and max_sizes must be finite and > 0");
    for (int k = 0; k < num_ratios; ++k)
        if (!positive(aspect_ratios[k])) return fail(FHIP_E_BADARG, "aspect_ratios must be finite and > 0");
    for (int k = 0; k < 4; ++k)
        if (!std::isfinite(variances[k])) return fail(FHIP_E_BADARG, "variances must be finite");
    if (!std::isfinite(offset) || !std::isfinite(step_w) || !std::isfinite(step_h)) return fail(FHIP_E_BADARG, "offset and steps must be finite");
    const long long per = (long long)num_min * (1 + (long long)num_ratios * (flip ? 2 : 1)) + num_max;
    const long long floats = 2ll * 4 * h * w * per;
    if (floats >= kMaxElements) return fail(FHIP_E_BADARG, "2 * 4 * h * w * num_prior must stay below 2^31");
    if (num_prior) *num_prior = (int)per;
    if (!out) return FHIP_OK;
    if (capacity < (size_t)floats) return fail(FHIP_E_BADARG, "output buffer too small");
    const float sw = step_w > 0.f ? step_w : (float)image_w / w, sh = step_h > 0.f ? step_h : (float)image_h / h;
    const float iw = (float)image_w, ih = (float)image_h;
    float* b = out;
    const auto put = [&](float cx, float cy, float bw, float bh) {
        b[0] = (cx - bw * 0.5f) / iw;
        b[1] = (cy - bh * 0.5f) / ih;
        b[2] = (cx + bw * 0.5f) / iw;
        b[3] = (cy + bh * 0.5f) / ih;
        b += 4;
    };
    for (int i = 0; i < h; ++i)
        for (int j = 0; j < w; ++j)
        {
            const float cx = ((float)j + offset) * sw, cy = ((float)i + offset) * sh;
            for (int k = 0; k < num_min; ++k)
            {
                const float mn = min_sizes[k];
                put(cx, cy, mn, mn);
                if (num_max)
                {
                    const float e = sqrtf(mn * max_sizes[k]);
                    put(cx, cy, e, e);
                }
                for (int r = 0; r < num_ratios; ++r)
                {
                    const float root = sqrtf(aspect_ratios[r]);
                    const float bw = mn * root, bh = mn / root;
                    put(cx, cy, bw, bh);
                    if (flip) put(cx, cy, bh, bw);
                }
            }
        }
    const size_t row = (size_t)floats / 2;
    if (clip)
        for (size_t i = 0; i < row; ++i) out[i] = std::min(std::max(out[i], 0.f), 1.f);
    for (size_t i = 0; i < row; ++i) out[row + i] = variances[i & 3];
    return FHIP_OK;
}

int fhip_detection_output_get_buffer_size(int n, int num_priors, int num_class, int nms_top_k, int keep_top_k, size_t* bytes)
{
    DetectArgs g;
    const int rc = detect_args(n, num_priors, num_class, nms_top_k, keep_top_k, g);
    if (rc) return rc;
    if (!bytes) return fail(FHIP_E_BADARG, "null argument");
    *bytes = detect_scratch_bytes(n, g);
    return FHIP_OK;
}

int fhip_detection_output_forward(int n, int num_priors, int num_class, float nms_threshold, int nms_top_k, int keep_top_k, float confidence_threshold,
                                  int prior_n, float* out, const float* location, const float* confidence, const float* priorbox, void* scratch, void* stream)
{
    DetectArgs g;
    const int rc = detect_args(n, num_priors, num_class, nms_top_k, keep_top_k, g);
    if (rc) return rc;
    if (!std::isfinite(nms_threshold) || !std::isfinite(confidence_threshold)) return fail(FHIP_E_BADARG, "thresholds must be finite");
    if (prior_n != 1 && prior_n != n) return fail(FHIP_E_BADARG, "prior_n must be 1 or n");
    if (!out || !location || !confidence || !priorbox || !scratch) return fail(FHIP_E_BADARG, "null pointer");
    if (!aligned(out, 4) || !aligned(location, 4) || !aligned(confidence, 4) || !aligned(priorbox, 4) || !aligned(scratch, 8))
        return fail(FHIP_E_BADARG, "pointers must be 4-byte aligned (scratch: 8)");
    g.nms_threshold = nms_threshold;
    g.confidence_threshold = confidence_threshold;
    g.prior_per_image = prior_n == n && n > 1 ? 1 : 0;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(detect_select_kernel, dim3((unsigned)(num_class - 1), (unsigned)n), dim3(256), 0, s, (unsigned char*)scratch, location, confidence, priorbox, g, n);
    FHIP_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(detect_merge_kernel, dim3((unsigned)n), dim3(256), 0, s, out, (const unsigned char*)scratch, g, n);
    FHIP_CHECK_HIP(hipGetLastError());
    return FHIP_OK;
}

int fhip_detect_route(int what, int a, int b, int c, int h, int w, const float* out, const float* in, char* name, int len)
{
    if (!name || len < 1) return fail(FHIP_E_BADARG, "null name");
    switch (what)
    {
    case FHIP_DETECT_PERMUTE:
    {
        int oc, oh, ow;
        const int rc = permute_dims(a, b, c, h, w, &oc, &oh, &ow);
        if (rc) return rc;
        snprintf(name, (size_t)len, permute_tiled(a, b) ? "fhip::permute_tile_kernel" : "fhip::permute_generic_kernel");
        return FHIP_OK;
    }
    case FHIP_DETECT_NORMALIZE:
    {
        const int rc = normalize_args(1, c, h, w, 1.f);
        if (rc) return rc;
        snprintf(name, (size_t)len, "fhip::normalize_kernel<%d>", normalize_v4(h, w, out, in) ? 4 : 1);
        return FHIP_OK;
    }
    case FHIP_DETECT_PERMUTE_CONCAT: snprintf(name, (size_t)len, "fhip::permute_concat_kernel"); return FHIP_OK;
    case FHIP_DETECT_SOFTMAX: snprintf(name, (size_t)len, "fhip::axis_softmax_kernel"); return FHIP_OK;
    case FHIP_DETECT_SELECT: snprintf(name, (size_t)len, "fhip::detect_select_kernel"); return FHIP_OK;
    case FHIP_DETECT_MERGE: snprintf(name, (size_t)len, "fhip::detect_merge_kernel"); return FHIP_OK;
    default: return fail(FHIP_E_BADARG, "unknown operation");
    }
}

const char* fhip_detect_last_error(void) { return last_error(); }

} // extern "C"
