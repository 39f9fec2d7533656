// libfeather_frame.so: ncnn's Padding, Crop and PixelShuffle on gfx950 (include/feather_hip/feather_frame.h is the contract and the definition;
// DESIGN.md 3.27 the design and its measurements).  Pure data movement: the work is to keep both sides of every copy wide and coalesced.
//
//   window_kernel<T, V>              Padding and Crop: a lane owns 4 consecutive output pixels of one row (1-D grid, 64-bit indices, grid-strided).
//                                    A lane whose 4 pixels come from 4 consecutive source pixels -- every lane of a crop, the interior lanes
//                                    of a padded row -- loads them as one 16-byte vector where that run is 16-byte aligned, else as 4 scalars;
//                                    only the other lanes go through the border map.  T: the border type (0 constant, 1 replicate, 2 reflect),
//                                    or 3 for a window without a positive margin, which carries no border code at all.  V = 1: the row
//                                    length is a multiple of 4 and `out` 16-byte aligned, one 16-byte store; V = 0: scalar stores
//   pixel_shuffle_tile_kernel        a block owns a group of output rows of one output plane: behind each lie r input rows (one per sw) of w
//                                    contiguous floats, loaded with coalesced loads and written into LDS interleaved (j * r + sw), so the
//                                    group leaves as one contiguous run, 16 bytes a lane where it is aligned
//   pixel_shuffle_direct_kernel      one output element per lane, coalesced stores: r = 1 (a copy), rows whose r * w pass the tile, and planes so
//                                    small that a tile block would move fewer than FHIP_FRAME_TILE_MIN elements
//
// Values travel as 32-bit words, so a NaN's payload and the sign of a zero survive; PixelShuffle's optional ReLU is the one operation.
// Contraction is off for the whole file.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>

#include "feather_hip/feather_frame.h"
#include "side_error.h"

#pragma clang fp contract(off)

namespace fhip
{

typedef unsigned int u32;
typedef long long i64;
typedef u32 u32x4 __attribute__((ext_vector_type(4)));

constexpr int kCropOnly = 3; // T of a window without a positive margin
constexpr unsigned kMaxBlocks = 16384;

struct WindowArgs
{
    int c, h, w, oc, oh, ow; // one image: in (c, h, w), out (oc, oh, ow)
    int front, top, left;
    u32 value;
    i64 lanes; // n * oc * oh * ceil(ow / 4)
};

// the source index of output index i - margin along an axis of d elements, or -1 where a type-0 window has none
template <int T>
__device__ __forceinline__ int border_map(int i, int d)
{
    if constexpr (T == FHIP_FRAME_REPLICATE) return min(max(i, 0), d - 1);
    if constexpr (T == FHIP_FRAME_REFLECT) return i < 0 ? -i : (i >= d ? 2 * (d - 1) - i : i);
    if constexpr (T == FHIP_FRAME_CONSTANT) return (i < 0 || i >= d) ? -1 : i;
    return i; // a crop: always inside
}

template <int T, int V>
__global__ __launch_bounds__(256) void window_kernel(u32* __restrict__ out, const u32* __restrict__ in, const u32* __restrict__ per_channel, WindowArgs g)
{
    const u32 quads = (u32)(g.ow + 3) >> 2;
    for (i64 lane = (i64)blockIdx.x * 256 + threadIdx.x; lane < g.lanes; lane += (i64)gridDim.x * 256)
    {
        const u32 at = (u32)lane; // lanes <= the output's elements < 2^31 (host): the split is 32-bit, every offset into memory 64-bit
        const u32 row = at / quads;
        const int x0 = (int)(at - row * quads) * 4;
        const u32 plane = row / (u32)g.oh;
        const int y = (int)(row - plane * (u32)g.oh);
        const i64 img = plane / (u32)g.oc;
        const int q = (int)(plane - (u32)img * (u32)g.oc);
        u32* dst = out + (i64)row * g.ow + x0;
        const int left_in_row = g.ow - x0; // >= 1; V: >= 4
        u32 v[4];
        const int sq = q - g.front;
        u32 fill = g.value;
        bool have_row = true;
        int sy = y - g.top;
        if constexpr (T == FHIP_FRAME_CONSTANT)
        {
            have_row = sq >= 0 && sq < g.c; // a padded channel (type 0 only: the host refuses the others)
            if (have_row && per_channel) fill = per_channel[sq];
        }
        sy = border_map<T>(sy, g.h);
        if (T == FHIP_FRAME_CONSTANT && sy < 0) have_row = false;
        if (!have_row)
        {
            v[0] = v[1] = v[2] = v[3] = fill;
        }
        else
        {
            const u32* src_row = in + ((img * g.c + sq) * g.h + sy) * (i64)g.w;
            const int sx0 = x0 - g.left;
            if (left_in_row >= 4 && sx0 >= 0 && sx0 + 3 < g.w) // 4 consecutive source pixels
            {
                const u32* p = src_row + sx0;
                if (((uintptr_t)p & 15) == 0)
                {
                    const u32x4 t = *reinterpret_cast<const u32x4*>(p);
                    v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
                }
                else
                {
#pragma unroll
                    for (int k = 0; k < 4; ++k) v[k] = p[k];
                }
            }
            else
            {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                {
                    v[k] = fill;
                    if (k < left_in_row) // (a pixel past the row's end is neither read nor stored)
                    {
                        const int sx = border_map<T>(sx0 + k, g.w);
                        if (T != FHIP_FRAME_CONSTANT || sx >= 0) v[k] = src_row[sx];
                    }
                }
            }
        }
        if constexpr (V)
        {
            u32x4 t;
            t.x = v[0], t.y = v[1], t.z = v[2], t.w = v[3];
            *reinterpret_cast<u32x4*>(dst) = t;
        }
        else
        {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < left_in_row) dst[k] = v[k];
        }
    }
}

// ---- PixelShuffle ------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float shuffle_act(float x, int relu, float slope)
{
    if (relu == FHIP_FRAME_RELU_SLOPE) return x > 0.f ? x : x * slope;
    if (relu == FHIP_FRAME_RELU_PLAIN) return fmaxf(x, 0.f);
    return x;
}

__device__ __forceinline__ u32 shuffle_word(u32 x, int relu, float slope) { return relu ? __float_as_uint(shuffle_act(__uint_as_float(x), relu, slope)) : x; }

// blockIdx.x runs over (image, output plane, group of `group` output rows); C = output planes, (h, w) the input plane, r * w <= FHIP_FRAME_TILE
__global__ __launch_bounds__(256) void pixel_shuffle_tile_kernel(u32* __restrict__ out, const u32* __restrict__ in, int r, int mode, int relu, float slope, int C,
                                                                 int h, int w, int group, int groups)
{
    __shared__ __attribute__((aligned(16))) u32 tile[FHIP_FRAME_TILE];
    const int oh = h * r, ow = w * r;
    const unsigned plane = blockIdx.x / (unsigned)groups, oy0 = (blockIdx.x - plane * (unsigned)groups) * (unsigned)group;
    const unsigned img = plane / (unsigned)C, q = plane - img * (unsigned)C;
    const int here = min(group, oh - (int)oy0);
    const int total = here * ow; // <= FHIP_FRAME_TILE
    // a wave takes one input row (output row gr, column phase sw) at a time: the split of the index is per row, not per element
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int row = wave; row < here * r; row += 4)
    {
        const int gr = row / r, sw = row - gr * r;
        const unsigned oy = oy0 + gr, i = oy / (unsigned)r, sh = oy - i * r, k = sh * r + sw;
        const unsigned ch = mode ? k * (unsigned)C + q : q * (unsigned)(r * r) + k;
        const u32* src = in + (((size_t)img * C * r * r + ch) * h + i) * w;
        u32* dst_row = tile + gr * ow + sw;
        for (int j = lane; j < w; j += 64) dst_row[j * r] = src[j];
    }
    __syncthreads();
    u32* dst = out + ((size_t)plane * oh + oy0) * ow;
    if ((((uintptr_t)dst | (uintptr_t)total * 4) & 15) == 0) // the same for the whole block
    {
        for (int e = threadIdx.x; e < total / 4; e += 256)
        {
            u32x4 t = reinterpret_cast<const u32x4*>(tile)[e];
            t.x = shuffle_word(t.x, relu, slope), t.y = shuffle_word(t.y, relu, slope), t.z = shuffle_word(t.z, relu, slope), t.w = shuffle_word(t.w, relu, slope);
            reinterpret_cast<u32x4*>(dst)[e] = t;
        }
    }
    else
        for (int e = threadIdx.x; e < total; e += 256) dst[e] = shuffle_word(tile[e], relu, slope);
}

__global__ __launch_bounds__(256) void pixel_shuffle_direct_kernel(u32* __restrict__ out, const u32* __restrict__ in, unsigned total, int r, int mode, int relu,
                                                                   float slope, int C, int h, int w)
{
    const unsigned at = blockIdx.x * 256u + threadIdx.x;
    if (at >= total) return;
    const unsigned ow = (unsigned)w * r, oh = (unsigned)h * r;
    const unsigned x = at % ow, t = at / ow, y = t % oh, plane = t / oh;
    const unsigned q = plane % (unsigned)C, img = plane / (unsigned)C;
    const unsigned i = y / (unsigned)r, sh = y - i * r, j = x / (unsigned)r, sw = x - j * r, k = sh * r + sw;
    const unsigned ch = mode ? k * (unsigned)C + q : q * (unsigned)(r * r) + k;
    out[at] = shuffle_word(in[(((size_t)img * C * r * r + ch) * h + i) * w + j], relu, slope);
}

// ---- host checks -----------------------------------------------------------------------------------------------------------------------
constexpr i64 kMaxElements = 1ll << 31;

static bool overlap(const void* a, size_t na, const void* b, size_t nb)
{
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}

static int window_dims(int c, int h, int w, int front, int behind, int top, int bottom, int left, int right, int* oc, int* oh, int* ow)
{
    if (c < 1 || h < 1 || w < 1) return fail(FHIP_E_BADARG, "a dimension < 1");
    const i64 qc = (i64)c + front + behind, qh = (i64)h + top + bottom, qw = (i64)w + left + right;
    if (qc < 1 || qh < 1 || qw < 1) return fail(FHIP_E_BADARG, "an output dimension < 1: the window leaves nothing");
    if (qc >= kMaxElements || qh >= kMaxElements || qw >= kMaxElements) return fail(FHIP_E_BADARG, "an output dimension of 2^31 or more");
    *oc = (int)qc, *oh = (int)qh, *ow = (int)qw;
    return FHIP_OK;
}

static bool window_pads(int front, int behind, int top, int bottom, int left, int right)
{
    return front > 0 || behind > 0 || top > 0 || bottom > 0 || left > 0 || right > 0;
}

static int shuffle_dims(int r, int c, int h, int w, int* oc, int* oh, int* ow)
{
    if (r < 1) return fail(FHIP_E_BADARG, "PixelShuffle upscale_factor < 1");
    if (c < 1 || h < 1 || w < 1) return fail(FHIP_E_BADARG, "a dimension < 1");
    const i64 rr = (i64)r * r;
    if (rr > c || c % rr) return fail(FHIP_E_BADARG, "PixelShuffle needs a multiple of upscale_factor^2 channels");
    if ((i64)h * r >= kMaxElements || (i64)w * r >= kMaxElements) return fail(FHIP_E_BADARG, "an output dimension of 2^31 or more");
    *oc = (int)(c / rr), *oh = h * r, *ow = w * r;
    return FHIP_OK;
}

// the tile kernel where an output row fits the tile AND a block then moves FHIP_FRAME_TILE_MIN elements or more: one block per tiny plane
// would be a grid of up to 2^29 blocks of a few lanes' work each; the direct kernel's grid is elements / 256
static bool shuffle_tiled(int r, int h, int w)
{
    if (r <= 1 || (i64)r * w > FHIP_FRAME_TILE) return false;
    const i64 oh = (i64)h * r, ow = (i64)w * r;
    return std::min<i64>(oh, FHIP_FRAME_TILE / ow) * ow >= FHIP_FRAME_TILE_MIN;
}

static int check_buffers(float* out, i64 total_out, const float* in, i64 total_in)
{
    if (total_in >= kMaxElements || total_out >= kMaxElements) return fail(FHIP_E_BADARG, "tensors of 2^31 elements or more are not supported");
    if (!out || !in) return fail(FHIP_E_BADARG, "null pointer");
    if (!aligned(out, 4) || !aligned(in, 4)) return fail(FHIP_E_BADARG, "pointers must be 4-byte aligned");
    if (overlap(out, (size_t)total_out * 4, in, (size_t)total_in * 4)) return fail(FHIP_E_BADARG, "out must not overlap in");
    return FHIP_OK;
}

template <int V>
static void launch_window(int t, unsigned blocks, hipStream_t s, u32* out, const u32* in, const u32* pc, const WindowArgs& g)
{
    switch (t)
    {
    case FHIP_FRAME_CONSTANT: hipLaunchKernelGGL((window_kernel<FHIP_FRAME_CONSTANT, V>), dim3(blocks), dim3(256), 0, s, out, in, pc, g); break;
    case FHIP_FRAME_REPLICATE: hipLaunchKernelGGL((window_kernel<FHIP_FRAME_REPLICATE, V>), dim3(blocks), dim3(256), 0, s, out, in, pc, g); break;
    case FHIP_FRAME_REFLECT: hipLaunchKernelGGL((window_kernel<FHIP_FRAME_REFLECT, V>), dim3(blocks), dim3(256), 0, s, out, in, pc, g); break;
    default: hipLaunchKernelGGL((window_kernel<kCropOnly, V>), dim3(blocks), dim3(256), 0, s, out, in, pc, g); break;
    }
}

} // namespace fhip

using namespace fhip;

extern "C"
{

int fhip_frame_window_output_dim(int c, int h, int w, int front, int behind, int top, int bottom, int left, int right, int* out_c, int* out_h, int* out_w)
{
    if (!out_c || !out_h || !out_w) return fail(FHIP_E_BADARG, "null argument");
    return window_dims(c, h, w, front, behind, top, bottom, left, right, out_c, out_h, out_w);
}

int fhip_frame_window_forward(int type, float value, const float* per_channel, int n, int c, int h, int w, int front, int behind, int top, int bottom,
                              int left, int right, float* out, const float* in, void* stream)
{
    int oc, oh, ow;
    const int rc = window_dims(c, h, w, front, behind, top, bottom, left, right, &oc, &oh, &ow);
    if (rc) return rc;
    if (n < 1) return fail(FHIP_E_BADARG, "n < 1");
    if (type < FHIP_FRAME_CONSTANT || type > FHIP_FRAME_REFLECT) return fail(FHIP_E_BADARG, "the window type must be 0 (constant), 1 (replicate) or 2 (reflect)");
    if (type != FHIP_FRAME_CONSTANT && (front > 0 || behind > 0)) return fail(FHIP_E_BADARG, "channel pads (front, behind) are defined for type 0 only");
    if (type != FHIP_FRAME_CONSTANT && per_channel) return fail(FHIP_E_BADARG, "per_channel values are defined for type 0 only");
    if (type == FHIP_FRAME_REFLECT && (top >= h || bottom >= h || left >= w || right >= w))
        return fail(FHIP_E_BADARG, "a reflect pad must be smaller than the dimension it pads");
    if (per_channel && !aligned(per_channel, 4)) return fail(FHIP_E_BADARG, "pointers must be 4-byte aligned");
    const i64 total_in = (i64)n * c * h * w;
    // n * oc * oh * ow without overflow: each factor is below 2^31, the running product is checked
    i64 total = (i64)n * oc;
    if (total < kMaxElements) total *= oh;
    if (total < kMaxElements) total *= ow;
    const int ck = check_buffers(out, std::min(total, kMaxElements), in, total_in);
    if (ck) return ck;
    WindowArgs g;
    g.c = c, g.h = h, g.w = w, g.oc = oc, g.oh = oh, g.ow = ow;
    g.front = front, g.top = top, g.left = left;
    memcpy(&g.value, &value, 4);
    g.lanes = (i64)n * oc * oh * ((ow + 3) / 4);
    const unsigned blocks = (unsigned)std::min<i64>((g.lanes + 255) / 256, kMaxBlocks);
    const int t = window_pads(front, behind, top, bottom, left, right) ? type : kCropOnly;
    hipStream_t s = (hipStream_t)stream;
    if (ow % 4 == 0 && aligned(out, 16))
        launch_window<1>(t, blocks, s, (u32*)out, (const u32*)in, (const u32*)per_channel, g);
    else
        launch_window<0>(t, blocks, s, (u32*)out, (const u32*)in, (const u32*)per_channel, g);
    FHIP_CHECK_HIP(hipGetLastError());
    return FHIP_OK;
}

int fhip_pixel_shuffle_output_dim(int r, int c, int h, int w, int* out_c, int* out_h, int* out_w)
{
    if (!out_c || !out_h || !out_w) return fail(FHIP_E_BADARG, "null argument");
    return shuffle_dims(r, c, h, w, out_c, out_h, out_w);
}

int fhip_pixel_shuffle_forward(int r, int mode, int relu, float slope, int n, int c, int h, int w, float* out, const float* in, void* stream)
{
    int C, oh, ow;
    const int rc = shuffle_dims(r, c, h, w, &C, &oh, &ow);
    if (rc) return rc;
    if (mode != 0 && mode != 1) return fail(FHIP_E_BADARG, "PixelShuffle mode must be 0 or 1");
    if (relu < FHIP_FRAME_RELU_NONE || relu > FHIP_FRAME_RELU_PLAIN) return fail(FHIP_E_BADARG, "relu must be 0 (none), 1 (with a slope) or 2 (plain)");
    if (n < 1) return fail(FHIP_E_BADARG, "n < 1");
    const i64 total = (i64)n * c * h * w; // the same on both sides
    const int ck = check_buffers(out, total, in, total);
    if (ck) return ck;
    hipStream_t s = (hipStream_t)stream;
    if (shuffle_tiled(r, h, w))
    {
        const int group = std::max(1, std::min(oh, FHIP_FRAME_TILE / ow)), groups = (oh + group - 1) / group;
        const i64 blocks = (i64)n * C * groups; // <= n * C * oh < 2^31
        hipLaunchKernelGGL(pixel_shuffle_tile_kernel, dim3((unsigned)blocks), dim3(256), 0, s, (u32*)out, (const u32*)in, r, mode, relu, slope, C, h, w, group, groups);
    }
    else
        hipLaunchKernelGGL(pixel_shuffle_direct_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, (u32*)out, (const u32*)in, (unsigned)total, r, mode,
                           relu, slope, C, h, w);
    FHIP_CHECK_HIP(hipGetLastError());
    return FHIP_OK;
}

int fhip_frame_route(int what, int a, int w, int b, int out_w, int aligned16, char* name, int len)
{
    if (!name || len < 1) return fail(FHIP_E_BADARG, "null name");
    switch (what)
    {
    case FHIP_FRAME_WINDOW:
        if (a < FHIP_FRAME_CONSTANT || a > FHIP_FRAME_REFLECT) return fail(FHIP_E_BADARG, "the window type must be 0, 1 or 2");
        if (out_w < 1) return fail(FHIP_E_BADARG, "out_w < 1");
        snprintf(name, (size_t)len, "fhip::window_kernel<%d, %d>", b ? a : kCropOnly, out_w % 4 == 0 && aligned16 ? 1 : 0);
        return FHIP_OK;
    case FHIP_FRAME_SHUFFLE:
        if (a < 1 || w < 1 || b < 1) return fail(FHIP_E_BADARG, "upscale_factor, h or w < 1");
        snprintf(name, (size_t)len, shuffle_tiled(a, b, w) ? "fhip::pixel_shuffle_tile_kernel" : "fhip::pixel_shuffle_direct_kernel");
        return FHIP_OK;
    default: return fail(FHIP_E_BADARG, "unknown operation");
    }
}

const char* fhip_frame_last_error(void) { return last_error(); }

} // extern "C"
