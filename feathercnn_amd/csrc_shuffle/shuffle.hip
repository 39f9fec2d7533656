// libfeather_shuffle.so: ncnn's ShuffleChannel and Slice, and every chain of them with Concat, on gfx950
// (include/feather_hip/feather_shuffle.h is the contract; DESIGN.md 3.15 the design and its measurements).
//
// One kernel family, the channel map: every output channel (a "row") of every output blob names one channel of one source blob, and a
// launch copies rows * n planes.  The work is pure data movement, one read and one write per element, so the kernel is a flat grid-stride
// copy over (image, row, position in the plane):
//
//   channel_map_kernel<KIND, VEC>   KIND 0: the row's (output, output channel, source, source channel) comes from a device table (int4 per
//                                           row, built and checked on the host by fhip_channel_map_create);
//                                   KIND 1: ShuffleChannel, the source channel is arithmetic (one source, one output, no table);
//                                   KIND 2: Slice, the output is found by comparing the row with up to four prefix sums (no table).
//                                   VEC true: the plane moves as float4 (h * w a multiple of 4, every tensor 16-byte aligned, so every
//                                   channel run of source and destination starts on a 16-byte boundary); VEC false: as floats, correct
//                                   for any 4-byte aligned pointer and any plane (7 x 7: runs of 49 floats whose source and destination
//                                   misalignment differ).  Both forms are coalesced: consecutive threads take consecutive elements of a
//                                   run and cross into the next row's run where one ends.
//
// Grid: one thread per element while that needs at most kMaxBlocks blocks of 256, then kMaxBlocks blocks striding with four independent
// loads in flight per thread before the first store.  Blob pointers travel in the kernel arguments and are selected with a compare chain
// (a run-time index into a by-value argument array would go through scratch memory).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <string>
#include <type_traits>
#include <vector>

#include "feather_hip/feather_shuffle.h"
#include "side_error.h"

struct fhip_channel_map
{
    int n_src = 0, n_out = 0, rows = 0;
    int src_c[FHIP_CHANNEL_MAP_MAX_BLOBS] = {0, 0, 0, 0};
    int out_c[FHIP_CHANNEL_MAP_MAX_BLOBS] = {0, 0, 0, 0};
    int4* table = nullptr; // [rows] on the device: x output, y output channel, z source, w source channel
};

namespace fhip
{

constexpr int MAXB = FHIP_CHANNEL_MAP_MAX_BLOBS;
constexpr int kBlock = 256;
constexpr int kMaxBlocks = 2048; // 256 CUs x 8 blocks: beyond it the blocks stride
constexpr int kInFlight = 4;     // independent loads per thread before the first store (the kernel's rounds are written out for 4)

struct MapArgs
{
    const float* src[MAXB];
    float* dst[MAXB];
    int src_c[MAXB];
    int dst_c[MAXB];
    int dst_row0[MAXB]; // KIND 2: the first row of each output
    const int4* table;  // KIND 0
    unsigned rows;      // output channels of all outputs together
    unsigned plane;     // elements (floats or float4s) of one h x w plane
    unsigned total;     // n * rows * plane
    int group, per_group; // KIND 1: out channel i * group + k  <-  in channel k * per_group + i
    int n_dst;
};

// where element idx of the launch comes from and goes to
template <int KIND, typename T>
__device__ __forceinline__ void locate(const MapArgs& a, unsigned idx, const T*& from, T*& to)
{
    const unsigned q = idx / a.plane, p = idx - q * a.plane;
    const unsigned n = q / a.rows, r = q - n * a.rows;
    int di = 0, dc = (int)r, si = 0, sc = (int)r;
    if (KIND == 0)
    {
        const int4 e = a.table[r];
        di = e.x;
        dc = e.y;
        si = e.z;
        sc = e.w;
    }
    else if (KIND == 1)
        sc = (int)(r % (unsigned)a.group) * a.per_group + (int)(r / (unsigned)a.group);
    else
    {
#pragma unroll
        for (int k = 1; k < MAXB; ++k)
            if (k < a.n_dst && (int)r >= a.dst_row0[k]) di = k;
    }
    const float* s = a.src[0];
    float* d = a.dst[0];
    int s_c = a.src_c[0], d_c = a.dst_c[0], row0 = a.dst_row0[0];
#pragma unroll
    for (int k = 1; k < MAXB; ++k)
    {
        if (si == k)
        {
            s = a.src[k];
            s_c = a.src_c[k];
        }
        if (di == k)
        {
            d = a.dst[k];
            d_c = a.dst_c[k];
            row0 = a.dst_row0[k];
        }
    }
    if (KIND == 2) dc = (int)r - row0;
    from = reinterpret_cast<const T*>(s) + ((size_t)n * s_c + sc) * a.plane + p;
    to = reinterpret_cast<T*>(d) + ((size_t)n * d_c + dc) * a.plane + p;
}

template <int KIND, bool VEC>
__global__ __launch_bounds__(kBlock) void channel_map_kernel(const MapArgs a)
{
    using T = typename std::conditional<VEC, float4, float>::type;
    const unsigned stride = gridDim.x * kBlock;
    unsigned base = blockIdx.x * kBlock + threadIdx.x;
    // whole rounds: kInFlight loads before the first store (base + 3 * stride < 2^31 + 2^21: no wrap)
    for (; base + (kInFlight - 1) * stride < a.total; base += stride * kInFlight)
    {
        // named values, not arrays: an array of float4 is placed in LDS by the compiler
        const T *f0, *f1, *f2, *f3;
        T *t0, *t1, *t2, *t3;
        locate<KIND, T>(a, base, f0, t0);
        locate<KIND, T>(a, base + stride, f1, t1);
        locate<KIND, T>(a, base + 2 * stride, f2, t2);
        locate<KIND, T>(a, base + 3 * stride, f3, t3);
        const T v0 = *f0, v1 = *f1, v2 = *f2, v3 = *f3;
        *t0 = v0;
        *t1 = v1;
        *t2 = v2;
        *t3 = v3;
    }
    for (; base < a.total; base += stride)
    {
        const T* from;
        T* to;
        locate<KIND, T>(a, base, from, to);
        *to = *from;
    }
}

static int check_shape(int n, int c, int h, int w)
{
    if (n < 1 || c < 1 || h < 1 || w < 1) return fail(FHIP_E_BADARG, "every dimension must be at least 1");
    if ((double)n * c * h * w >= 2147483648.0) return fail(FHIP_E_BADARG, "tensors of 2^31 elements or more are not supported");
    return 0;
}

static int resolve_slice(int c, const int* sizes, int count, int* resolved)
{
    if (!sizes || !resolved) return fail(FHIP_E_BADARG, "null sizes");
    if (count < 1) return fail(FHIP_E_BADARG, "a slice needs at least one output (count >= 1)");
    if (c < 1) return fail(FHIP_E_BADARG, "every dimension must be at least 1");
    long used = 0;
    for (int j = 0; j < count; ++j)
    {
        long s = sizes[j];
        if (s == FHIP_SLICE_SHARE)
            s = ((long)c - used) / (count - j);
        else if (s < 1)
            return fail(FHIP_E_BADARG, "a slice size must be positive or -233 (an equal share of what is left)");
        if (s < 1) return fail(FHIP_E_BADARG, "the slice sizes leave an output without a channel (sum larger than the channel count)");
        used += s;
        if (used > c) return fail(FHIP_E_BADARG, "the slice sizes sum to more than the channel count");
        resolved[j] = (int)s;
    }
    return 0;
}

// pointers: n_dst outputs then n_src sources
static bool can_vectorise(int h, int w, const void* const* pointers, int count)
{
    if (((size_t)h * w) % 4) return false;
    for (int i = 0; i < count; ++i)
        if (!aligned(pointers[i], 16)) return false;
    return true;
}

template <int KIND>
static int launch(MapArgs& a, int n, int h, int w, bool vec, hipStream_t stream)
{
    a.plane = (unsigned)((size_t)h * w / (vec ? 4 : 1));
    a.total = (unsigned)((size_t)n * a.rows * a.plane);
    const unsigned blocks = std::min<unsigned>((a.total + kBlock - 1) / kBlock, kMaxBlocks);
    if (vec)
        hipLaunchKernelGGL((channel_map_kernel<KIND, true>), dim3(blocks), dim3(kBlock), 0, stream, a);
    else
        hipLaunchKernelGGL((channel_map_kernel<KIND, false>), dim3(blocks), dim3(kBlock), 0, stream, a);
    FHIP_CHECK_HIP(hipGetLastError());
    return 0;
}

static int map_forward(int route, const fhip_channel_map* m, float* const* outs, const float* const* srcs, int n, int h, int w, void* stream)
{
    if (!m || !outs || !srcs) return fail(FHIP_E_BADARG, "null map or pointer array");
    if (route < -1 || route > FHIP_CHANNEL_MAP_ROUTE_16B) return fail(FHIP_E_BADARG, "unknown route");
    MapArgs a = {};
    const void* pointers[2 * MAXB];
    int np = 0;
    for (int j = 0; j < m->n_out; ++j)
    {
        if (int rc = check_shape(n, m->out_c[j], h, w)) return rc;
        if (!outs[j]) return fail(FHIP_E_BADARG, "null output pointer");
        if (!aligned(outs[j], 4)) return fail(FHIP_E_BADARG, "output pointer is not 4-byte aligned");
        a.dst[j] = outs[j];
        a.dst_c[j] = m->out_c[j];
        pointers[np++] = outs[j];
    }
    for (int s = 0; s < m->n_src; ++s)
    {
        if (int rc = check_shape(n, m->src_c[s], h, w)) return rc;
        if (!srcs[s]) return fail(FHIP_E_BADARG, "null source pointer");
        if (!aligned(srcs[s], 4)) return fail(FHIP_E_BADARG, "source pointer is not 4-byte aligned");
        a.src[s] = srcs[s];
        a.src_c[s] = m->src_c[s];
        pointers[np++] = srcs[s];
    }
    if (int rc = check_shape(n, m->rows, h, w)) return rc;
    const bool can = can_vectorise(h, w, pointers, np);
    if (route == FHIP_CHANNEL_MAP_ROUTE_16B && !can)
        return fail(FHIP_E_BADARG, "16-byte accesses need h * w to be a multiple of 4 and every pointer 16-byte aligned");
    a.table = m->table;
    a.rows = (unsigned)m->rows;
    a.n_dst = m->n_out;
    return launch<FHIP_CHANNEL_MAP_TABLE>(a, n, h, w, route == -1 ? can : route == FHIP_CHANNEL_MAP_ROUTE_16B, (hipStream_t)stream);
}

} // namespace fhip

using namespace fhip;

extern "C"
{

int fhip_channel_map_supported(int n, int c, int h, int w) { return check_shape(n, c, h, w); }

int fhip_channel_slice_resolve(int c, const int* sizes, int count, int* resolved) { return resolve_slice(c, sizes, count, resolved); }

int fhip_channel_shuffle_forward(float* out, const float* in, int n, int c, int h, int w, int group, int reverse, void* stream)
{
    if (int rc = check_shape(n, c, h, w)) return rc;
    if (group < 1) return fail(FHIP_E_BADARG, "group must be at least 1");
    if (c % group) return fail(FHIP_E_BADARG, "group does not divide the channel count");
    if (!out || !in) return fail(FHIP_E_BADARG, "null pointer");
    if (!aligned(out, 4) || !aligned(in, 4)) return fail(FHIP_E_BADARG, "pointers must be 4-byte aligned");
    MapArgs a = {};
    a.src[0] = in;
    a.dst[0] = out;
    a.src_c[0] = a.dst_c[0] = c;
    a.rows = (unsigned)c;
    a.n_dst = 1;
    a.group = reverse ? c / group : group; // the inverse of a shuffle by g is the shuffle by C / g
    a.per_group = c / a.group;
    const void* pointers[2] = {out, in};
    return launch<FHIP_CHANNEL_MAP_SHUFFLE>(a, n, h, w, can_vectorise(h, w, pointers, 2), (hipStream_t)stream);
}

int fhip_channel_slice_forward(float* const* outs, const float* in, int n, int c, int h, int w, const int* sizes, int count, void* stream)
{
    if (int rc = check_shape(n, c, h, w)) return rc;
    if (!outs || !in) return fail(FHIP_E_BADARG, "null pointer");
    if (count > MAXB) return fail(FHIP_E_BADARG, "too many outputs for one slice (FHIP_CHANNEL_MAP_MAX_BLOBS)");
    int resolved[MAXB];
    if (int rc = resolve_slice(c, sizes, count, resolved)) return rc;
    if (!aligned(in, 4)) return fail(FHIP_E_BADARG, "pointers must be 4-byte aligned");
    MapArgs a = {};
    const void* pointers[MAXB + 1];
    int row = 0;
    for (int j = 0; j < count; ++j)
    {
        if (!outs[j]) return fail(FHIP_E_BADARG, "null output pointer");
        if (!aligned(outs[j], 4)) return fail(FHIP_E_BADARG, "pointers must be 4-byte aligned");
        a.dst[j] = outs[j];
        a.dst_c[j] = resolved[j];
        a.dst_row0[j] = row;
        row += resolved[j];
        pointers[j] = outs[j];
    }
    pointers[count] = in;
    a.src[0] = in;
    a.src_c[0] = c;
    a.rows = (unsigned)row;
    a.n_dst = count;
    return launch<FHIP_CHANNEL_MAP_SLICE>(a, n, h, w, can_vectorise(h, w, pointers, count + 1), (hipStream_t)stream);
}

int fhip_channel_map_create(fhip_channel_map** map, const int* src_channels, int n_src, const int* out_channels, int n_out, const int* entries)
{
    if (!map || !src_channels || !out_channels || !entries) return fail(FHIP_E_BADARG, "null argument");
    *map = nullptr;
    if (n_src < 1 || n_src > MAXB || n_out < 1 || n_out > MAXB)
        return fail(FHIP_E_BADARG, "a channel map has 1 .. FHIP_CHANNEL_MAP_MAX_BLOBS sources and as many outputs");
    long rows = 0;
    for (int s = 0; s < n_src; ++s)
        if (src_channels[s] < 1) return fail(FHIP_E_BADARG, "every source needs at least one channel");
    for (int j = 0; j < n_out; ++j)
    {
        if (out_channels[j] < 1) return fail(FHIP_E_BADARG, "every output needs at least one channel");
        rows += out_channels[j];
    }
    if (rows >= (1L << 24)) return fail(FHIP_E_BADARG, "too many output channels: 2^24 or more");
    std::vector<int4> table((size_t)rows);
    size_t r = 0;
    for (int j = 0; j < n_out; ++j)
        for (int ch = 0; ch < out_channels[j]; ++ch, ++r)
        {
            const int si = entries[2 * r], sc = entries[2 * r + 1];
            if (si < 0 || si >= n_src || sc < 0 || sc >= src_channels[si]) return fail(FHIP_E_BADARG, "a table entry names no channel of any source");
            table[r] = make_int4(j, ch, si, sc);
        }
    fhip_channel_map* m = new fhip_channel_map;
    m->n_src = n_src;
    m->n_out = n_out;
    m->rows = (int)rows;
    for (int s = 0; s < n_src; ++s) m->src_c[s] = src_channels[s];
    for (int j = 0; j < n_out; ++j) m->out_c[j] = out_channels[j];
    hipError_t e = hipMalloc((void**)&m->table, table.size() * sizeof(int4));
    if (e == hipSuccess) e = hipMemcpy(m->table, table.data(), table.size() * sizeof(int4), hipMemcpyHostToDevice);
    if (e != hipSuccess)
    {
        if (m->table) (void)hipFree(m->table);
        delete m;
        return fail(FHIP_E_HIP, (std::string("channel map table: ") + hipGetErrorString(e)).c_str());
    }
    *map = m;
    return 0;
}

int fhip_channel_map_destroy(fhip_channel_map* map)
{
    if (!map) return 0;
    if (map->table) (void)hipFree(map->table);
    delete map;
    return 0;
}

int fhip_channel_map_forward(const fhip_channel_map* map, float* const* outs, const float* const* srcs, int n, int h, int w, void* stream)
{
    return map_forward(-1, map, outs, srcs, n, h, w, stream);
}

int fhip_channel_map_forward_route(int route, const fhip_channel_map* map, float* const* outs, const float* const* srcs, int n, int h, int w,
                                   void* stream)
{
    if (route != FHIP_CHANNEL_MAP_ROUTE_4B && route != FHIP_CHANNEL_MAP_ROUTE_16B) return fail(FHIP_E_BADARG, "unknown route");
    return map_forward(route, map, outs, srcs, n, h, w, stream);
}

int fhip_channel_map_route(int kind, int h, int w, const void* const* pointers, int count, char* name, int len)
{
    if (!name || len < 1 || (count > 0 && !pointers)) return fail(FHIP_E_BADARG, "null argument");
    if (kind < FHIP_CHANNEL_MAP_TABLE || kind > FHIP_CHANNEL_MAP_SLICE) return fail(FHIP_E_BADARG, "unknown kind");
    if (h < 1 || w < 1 || count < 0) return fail(FHIP_E_BADARG, "every dimension must be at least 1");
    snprintf(name, (size_t)len, "fhip::channel_map_kernel<%d, %s>", kind, can_vectorise(h, w, pointers, count) ? "true" : "false");
    return 0;
}

const char* fhip_shuffle_last_error(void) { return last_error(); }

} // extern "C"
