// libfeather_gate.so: squeeze-and-excitation channel gating on gfx950 (include/feather_hip/feather_gate.h is the contract; DESIGN.md 3.18
// the design and its measurements).
//
// An SE block is two HBM-bound streams over x[n][c][h][w] and one small matrix-vector pair per image between them:
//
//   squeeze   mean[n][c] = sum(x[n][c][:]) / HW          squeeze_group_kernel<V>   HW <= 4096: a group of 1 .. 64 lanes per plane (the smallest
//                                                                                  power of two that leaves a lane at most four accesses), so a
//                                                                                  wave takes 64 / G planes: a 7 x 7 plane costs 16 lanes, not 64
//                                                        squeeze_block_kernel<V>   HW <= 16384: one 256-thread block per plane
//                                                        squeeze_block_kernel<V> + squeeze_merge_kernel   larger planes: chunks of 16384 floats,
//                                                                                  one block each, partial sums to scratch, merged in chunk order
//   excite    gate = gact(W2 . mact(W1 . mean + b1) + b2)   excite_kernel          one 512-thread block per image (and slice of the output channels):
//                                                                                  a wave per hidden row, then a group of lanes per output channel;
//                                                                                  both weight matrices are read from L2
//   apply     out = act(fl(x * gate[n][c]) [+ residual])   gate_apply_kernel<V>    grid-strided over the tensor, one gate scalar per plane, no LDS
//
// V = true: 16-byte accesses (HW a multiple of 4, tensors 16-byte aligned); V = false: 4-byte accesses.  Every sum has a fixed order (a
// lane's own elements in index order, xor-shuffles inside the group, the waves' LDS slots in wave order, chunks in chunk order): no atomics,
// bit-identical run to run.  The product and the sum of the apply kernel are rounded separately (mul_rounded, add_rounded: contraction off), so the fused form
// equals a multiply followed by fhip_add bit for bit.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <string>

#include "feather_hip/feather_gate.h"
#include "side_error.h"

namespace fhip
{

constexpr int kGroupMaxHW = 4096;   // planes up to here: a group of lanes of one wave per plane
constexpr int kChunk = 16384;       // floats one 256-thread block sums: a whole plane up to here, a chunk of a larger one
constexpr unsigned kMaxGrid = 2048; // blocks of the grid-strided kernels (256 CUs x 8)
constexpr int kExciteThreads = 512;
constexpr int kExciteTile = 1024; // hidden values held in LDS at a time; a larger R is processed in tiles of this many

// sum of `cnt` floats at src, taken by GROUP lanes (lane t of the group): a lane adds its own accesses in index order
template <bool VEC>
__device__ __forceinline__ float lane_sum(const float* __restrict__ src, int cnt, int t, int group)
{
    if (VEC)
    {
        const float4* s4 = reinterpret_cast<const float4*>(src);
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 4
        for (int i = t; i < (cnt >> 2); i += group)
        {
            const float4 q = s4[i];
            a.x += q.x;
            a.y += q.y;
            a.z += q.z;
            a.w += q.w;
        }
        return (a.x + a.y) + (a.z + a.w);
    }
    float a = 0.f;
#pragma unroll 4
    for (int i = t; i < cnt; i += group) a += src[i];
    return a;
}

// group = lanes per plane, a power of two in 1 .. 64; a 256-thread block takes 256 / group planes and strides over the rest
template <bool VEC>
__global__ __launch_bounds__(256) void squeeze_group_kernel(float* __restrict__ mean, const float* __restrict__ in, int planes, int hw, int group)
{
    const int t = threadIdx.x & (group - 1), per_block = 256 / group;
    // `plane` is the same in every lane of a group, and a group never straddles a wave: the shuffles below stay inside lanes that are
    // active together
    for (long long plane = (long long)blockIdx.x * per_block + threadIdx.x / group; plane < planes; plane += (long long)gridDim.x * per_block)
    {
        float s = lane_sum<VEC>(in + (size_t)plane * hw, hw, t, group);
        for (int o = group >> 1; o; o >>= 1) s += __shfl_xor(s, o);
        if (t == 0) mean[plane] = s / (float)hw;
    }
}

// block b sums chunk b % nchunks of plane b / nchunks.  nchunks == 1: dst[plane] = the mean; else dst[b] = the chunk's sum
template <bool VEC>
__global__ __launch_bounds__(256) void squeeze_block_kernel(float* __restrict__ dst, const float* __restrict__ in, int nchunks, int hw)
{
    __shared__ float red[4];
    const int plane = blockIdx.x / nchunks, chunk = blockIdx.x % nchunks;
    const int start = chunk * kChunk, cnt = min(kChunk, hw - start);
    float s = lane_sum<VEC>(in + (size_t)plane * hw + start, cnt, threadIdx.x, 256);
#pragma unroll
    for (int o = 32; o; o >>= 1) s += __shfl_xor(s, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0)
    {
        s = ((red[0] + red[1]) + red[2]) + red[3];
        dst[blockIdx.x] = nchunks == 1 ? s / (float)hw : s;
    }
}

// split route, second launch: thread p adds the chunk sums of plane p in chunk order
__global__ __launch_bounds__(256) void squeeze_merge_kernel(float* __restrict__ mean, const float* __restrict__ partial, int planes, int nchunks, int hw)
{
    const int plane = blockIdx.x * 256 + threadIdx.x;
    if (plane >= planes) return;
    float s = 0.f;
    for (int k = 0; k < nchunks; ++k) s += partial[(size_t)plane * nchunks + k];
    mean[plane] = s / (float)hw;
}

__device__ __forceinline__ float swish(float x) { return x / (1.f + expf(-x)); }
// A product and a sum that are each rounded to fp32.  hipcc contracts a * b + c into one fma by default, and this toolchain's __fmul_rn and
// __fadd_rn are the plain operators, which it contracts as well; the pragma takes the contraction off these two operations wherever they
// are inlined.
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
// rounded after the product and after the sum, as numpy's fp32 expression is
__device__ __forceinline__ float hard_sigmoid(float x, float alpha, float beta) { return fminf(fmaxf(add_rounded(mul_rounded(alpha, x), beta), 0.f), 1.f); }

// grid (slices, n): block (s, i) computes the gates of image i for the s-th share of the output channels; every block of an image
// recomputes the hidden vector.  hid holds kExciteTile hidden values; a larger R runs in tiles, the running sums kept in gate[] by the
// thread that owns the channel (the same thread in every tile).
__global__ __launch_bounds__(kExciteThreads) void excite_kernel(float* __restrict__ gate, const float* __restrict__ mean, const float* __restrict__ w1,
                                                                const float* __restrict__ b1, const float* __restrict__ w2, const float* __restrict__ b2,
                                                                int C, int R, int mact, int gact, float alpha, float beta)
{
    __shared__ float hid[kExciteTile];
    const int per = (C + (int)gridDim.x - 1) / (int)gridDim.x;
    const int c0 = (int)blockIdx.x * per, c1 = min(C, c0 + per);
    const float* m = mean + (size_t)blockIdx.y * C;
    float* g = gate + (size_t)blockIdx.y * C;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int r0 = 0; r0 < R; r0 += kExciteTile)
    {
        const int rt = min(kExciteTile, R - r0);
        if (r0) __syncthreads(); // the previous tile's readers are done with hid
        for (int r = wave; r < rt; r += kExciteThreads / 64)
        {
            const float* row = w1 + (size_t)(r0 + r) * C;
            float s = 0.f;
#pragma unroll 4
            for (int k = lane; k < C; k += 64) s = fmaf(row[k], m[k], s);
#pragma unroll
            for (int o = 32; o; o >>= 1) s += __shfl_xor(s, o);
            if (lane == 0)
            {
                if (b1) s += b1[r0 + r];
                hid[r] = mact == FHIP_EXCITE_MACT_RELU ? fmaxf(s, 0.f) : mact == FHIP_EXCITE_MACT_SWISH ? swish(s) : s;
            }
        }
        __syncthreads();
        // lanes per output channel: the smallest power of two that covers a full tile, at most a wave.  It does not depend on the tile, so
        // a channel belongs to the same thread in every tile and that thread alone reads and writes its running sum in g[]
        int group = 1;
        while (group < min(kExciteTile, R) && group < 64) group <<= 1;
        const int t = threadIdx.x & (group - 1);
        for (int c = c0 + threadIdx.x / group; c < c1; c += kExciteThreads / group)
        {
            const float* row = w2 + (size_t)c * R + r0;
            float s = 0.f;
            for (int k = t; k < rt; k += group) s = fmaf(row[k], hid[k], s);
            for (int o = group >> 1; o; o >>= 1) s += __shfl_xor(s, o);
            if (t == 0)
            {
                s += r0 ? g[c] : (b2 ? b2[c] : 0.f);
                if (r0 + rt == R) s = gact == FHIP_EXCITE_GACT_SIGMOID ? 1.f / (1.f + expf(-s)) : hard_sigmoid(s, alpha, beta);
                g[c] = s;
            }
        }
    }
}

// units = floats (VEC: float4s) of the whole tensor, grid-strided; a float4 never straddles two planes (hw is a multiple of 4).
// out may be in or residual: every unit is read before it is written, by the thread that writes it.
template <bool VEC>
__global__ __launch_bounds__(256) void gate_apply_kernel(float* out, const float* in, const float* __restrict__ gate, const float* residual, unsigned units,
                                                         unsigned hw, int relu)
{
    for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < units; i += gridDim.x * 256u)
    {
        const float g = gate[(VEC ? i * 4u : i) / hw];
        if (VEC)
        {
            const float4 x = reinterpret_cast<const float4*>(in)[i];
            float4 y = make_float4(mul_rounded(x.x, g), mul_rounded(x.y, g), mul_rounded(x.z, g), mul_rounded(x.w, g));
            if (residual)
            {
                const float4 r = reinterpret_cast<const float4*>(residual)[i];
                y = make_float4(add_rounded(y.x, r.x), add_rounded(y.y, r.y), add_rounded(y.z, r.z), add_rounded(y.w, r.w));
            }
            if (relu) y = make_float4(fmaxf(y.x, 0.f), fmaxf(y.y, 0.f), fmaxf(y.z, 0.f), fmaxf(y.w, 0.f));
            reinterpret_cast<float4*>(out)[i] = y;
        }
        else
        {
            float y = mul_rounded(in[i], g);
            if (residual) y = add_rounded(y, residual[i]);
            out[i] = relu ? fmaxf(y, 0.f) : y;
        }
    }
}

template <bool VEC>
__global__ __launch_bounds__(256) void gate_activation_kernel(float* out, const float* in, int kind, unsigned units, float alpha, float beta)
{
    for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < units; i += gridDim.x * 256u)
    {
        if (VEC)
        {
            const float4 q = reinterpret_cast<const float4*>(in)[i];
            reinterpret_cast<float4*>(out)[i] =
                kind == FHIP_GATE_SWISH ? make_float4(swish(q.x), swish(q.y), swish(q.z), swish(q.w))
                                        : make_float4(hard_sigmoid(q.x, alpha, beta), hard_sigmoid(q.y, alpha, beta), hard_sigmoid(q.z, alpha, beta),
                                                      hard_sigmoid(q.w, alpha, beta));
        }
        else
            out[i] = kind == FHIP_GATE_SWISH ? swish(in[i]) : hard_sigmoid(in[i], alpha, beta);
    }
}

enum SqueezeRoute
{
    SQ_GROUP,
    SQ_BLOCK,
    SQ_SPLIT
};

static SqueezeRoute squeeze_route(int hw) { return hw <= kGroupMaxHW ? SQ_GROUP : hw <= kChunk ? SQ_BLOCK : SQ_SPLIT; }

static int nchunks_of(int hw) { return (hw + kChunk - 1) / kChunk; }

static bool aligned16(const void* a, const void* b = nullptr, const void* c = nullptr) { return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15) == 0; }
static bool aligned4(const void* a, const void* b = nullptr, const void* c = nullptr, const void* d = nullptr, const void* e = nullptr, const void* f = nullptr)
{
    return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d | (uintptr_t)e | (uintptr_t)f) & 3) == 0;
}

static int check_shape(int n, int c, int h, int w)
{
    if (n < 1 || c < 1 || h < 1 || w < 1) return fail(FHIP_E_BADARG, "every dimension must be at least 1");
    if ((long long)n * c * h * w >= (1ll << 31)) return fail(FHIP_E_BADARG, "tensors of 2^31 elements or more are not supported");
    return FHIP_OK;
}

// lanes per plane of squeeze_group_kernel: the smallest power of two that leaves a lane at most four accesses
static int group_of(int hw, bool vec)
{
    const int units = vec ? hw / 4 : hw;
    int g = 1;
    while (g < 64 && g * 4 < units) g <<= 1;
    return g;
}

static unsigned grid_for(unsigned units) { return std::min(kMaxGrid, (units + 255u) / 256u); }

static int excite_launch(int slices, int n, int c, int r, float* gate, const float* mean, const float* w1, const float* b1, const float* w2, const float* b2,
                         int mact, int gact, float alpha, float beta, void* stream)
{
    if (n < 1 || c < 1 || r < 1) return fail(FHIP_E_BADARG, "every dimension must be at least 1");
    if ((long long)n * c >= (1ll << 31) || (long long)c * r >= (1ll << 31)) return fail(FHIP_E_BADARG, "tensors of 2^31 elements or more are not supported");
    if (n > 65535) return fail(FHIP_E_BADARG, "a batch dimension above 65535 is not supported");
    if (!gate || !mean || !w1 || !w2) return fail(FHIP_E_BADARG, "null gate / mean / w1 / w2");
    if (!aligned4(gate, mean, w1, b1, w2, b2)) return fail(FHIP_E_BADARG, "pointers must be 4-byte aligned");
    if (mact != FHIP_EXCITE_MACT_NONE && mact != FHIP_EXCITE_MACT_RELU && mact != FHIP_EXCITE_MACT_SWISH) return fail(FHIP_E_BADARG, "unknown mact");
    if (gact != FHIP_EXCITE_GACT_SIGMOID && gact != FHIP_EXCITE_GACT_HARDSIGMOID) return fail(FHIP_E_BADARG, "unknown gact");
    if (gact == FHIP_EXCITE_GACT_HARDSIGMOID && (!std::isfinite(alpha) || !std::isfinite(beta))) return fail(FHIP_E_BADARG, "alpha and beta must be finite");
    if (slices < 1 || slices > 1024) return fail(FHIP_E_BADARG, "slices must be in 1 .. 1024");
    hipLaunchKernelGGL(excite_kernel, dim3(std::min(slices, c), n), dim3(kExciteThreads), 0, (hipStream_t)stream, gate, mean, w1, b1, w2, b2, c, r, mact, gact, alpha,
                       beta);
    FHIP_CHECK_HIP(hipGetLastError());
    return FHIP_OK;
}

} // namespace fhip

using namespace fhip;

extern "C"
{

int fhip_channel_gate_forward(int n, int c, int h, int w, float* out, const float* in, const float* gate, const float* residual, int act, void* stream)
{
    const int rc = check_shape(n, c, h, w);
    if (rc) return rc;
    if (!out || !in || !gate) return fail(FHIP_E_BADARG, "null out / in / gate");
    if (!aligned4(out, in, gate, residual)) return fail(FHIP_E_BADARG, "pointers must be 4-byte aligned");
    if (act != FHIP_GATE_ACT_NONE && act != FHIP_GATE_ACT_RELU) return fail(FHIP_E_BADARG, "unknown act");
    const unsigned hw = (unsigned)h * w, total = (unsigned)n * c * hw;
    hipStream_t s = (hipStream_t)stream;
    if (hw % 4 == 0 && aligned16(out, in, residual))
        hipLaunchKernelGGL(gate_apply_kernel<true>, dim3(grid_for(total / 4)), dim3(256), 0, s, out, in, gate, residual, total / 4, hw, act);
    else
        hipLaunchKernelGGL(gate_apply_kernel<false>, dim3(grid_for(total)), dim3(256), 0, s, out, in, gate, residual, total, hw, act);
    FHIP_CHECK_HIP(hipGetLastError());
    return FHIP_OK;
}

int fhip_squeeze_get_buffer_size(int n, int c, int h, int w, size_t* scratch_bytes)
{
    const int rc = check_shape(n, c, h, w);
    if (rc) return rc;
    if (!scratch_bytes) return fail(FHIP_E_BADARG, "null scratch_bytes");
    *scratch_bytes = squeeze_route(h * w) == SQ_SPLIT ? (size_t)n * c * nchunks_of(h * w) * sizeof(float) : 0;
    return FHIP_OK;
}

int fhip_squeeze_forward(int n, int c, int h, int w, float* mean, const float* in, float* scratch, void* stream)
{
    const int rc = check_shape(n, c, h, w);
    if (rc) return rc;
    if (!mean || !in) return fail(FHIP_E_BADARG, "null mean / in");
    if (!aligned4(mean, in, scratch)) return fail(FHIP_E_BADARG, "pointers must be 4-byte aligned");
    const int hw = h * w, planes = n * c;
    const bool vec = hw % 4 == 0 && aligned16(in);
    hipStream_t s = (hipStream_t)stream;
    switch (squeeze_route(hw))
    {
    case SQ_GROUP:
    {
        const int group = group_of(hw, vec);
        const dim3 grid(std::min<long long>(((long long)planes * group + 255) / 256, 1 << 20));
        if (vec)
            hipLaunchKernelGGL(squeeze_group_kernel<true>, grid, dim3(256), 0, s, mean, in, planes, hw, group);
        else
            hipLaunchKernelGGL(squeeze_group_kernel<false>, grid, dim3(256), 0, s, mean, in, planes, hw, group);
        break;
    }
    case SQ_BLOCK:
        if (vec)
            hipLaunchKernelGGL(squeeze_block_kernel<true>, dim3(planes), dim3(256), 0, s, mean, in, 1, hw);
        else
            hipLaunchKernelGGL(squeeze_block_kernel<false>, dim3(planes), dim3(256), 0, s, mean, in, 1, hw);
        break;
    default:
    {
        if (!scratch) return fail(FHIP_E_BADARG, "null scratch: this shape takes the split route (fhip_squeeze_get_buffer_size)");
        const int nchunks = nchunks_of(hw); // every chunk holds at least one float: fewer blocks than elements, < 2^31
        if (vec)
            hipLaunchKernelGGL(squeeze_block_kernel<true>, dim3((unsigned)planes * nchunks), dim3(256), 0, s, scratch, in, nchunks, hw);
        else
            hipLaunchKernelGGL(squeeze_block_kernel<false>, dim3((unsigned)planes * nchunks), dim3(256), 0, s, scratch, in, nchunks, hw);
        hipLaunchKernelGGL(squeeze_merge_kernel, dim3((planes + 255) / 256), dim3(256), 0, s, mean, scratch, planes, nchunks, hw);
        break;
    }
    }
    FHIP_CHECK_HIP(hipGetLastError());
    return FHIP_OK;
}

int fhip_excite_forward(int n, int c, int r, float* gate, const float* mean, const float* w1, const float* b1, const float* w2, const float* b2, int mact,
                        int gact, float alpha, float beta, void* stream)
{
    // blocks for about four per CU, at most 8 slices: every slice recomputes the hidden vector, and beyond 8 that costs more than the
    // idle CUs did.  Any slice count gives the same bits.
    int slices = 1;
    while (slices < 8 && (long long)n * slices < 1024) slices <<= 1;
    return excite_launch(slices, n, c, r, gate, mean, w1, b1, w2, b2, mact, gact, alpha, beta, stream);
}

int fhip_excite_forward_slices(int slices, int n, int c, int r, float* gate, const float* mean, const float* w1, const float* b1, const float* w2,
                               const float* b2, int mact, int gact, float alpha, float beta, void* stream)
{
    return excite_launch(slices, n, c, r, gate, mean, w1, b1, w2, b2, mact, gact, alpha, beta, stream);
}

int fhip_gate_activation_forward(int kind, float* out, const float* in, int n, int c, int hw, float alpha, float beta, void* stream)
{
    const int rc = check_shape(n, c, hw, 1);
    if (rc) return rc;
    if (!out || !in) return fail(FHIP_E_BADARG, "null out / in");
    if (!aligned4(out, in)) return fail(FHIP_E_BADARG, "pointers must be 4-byte aligned");
    if (kind != FHIP_GATE_SWISH && kind != FHIP_GATE_HARDSIGMOID) return fail(FHIP_E_BADARG, "unknown kind");
    if (kind == FHIP_GATE_HARDSIGMOID && (!std::isfinite(alpha) || !std::isfinite(beta))) return fail(FHIP_E_BADARG, "alpha and beta must be finite");
    const unsigned total = (unsigned)n * c * hw;
    hipStream_t s = (hipStream_t)stream;
    if (total % 4 == 0 && aligned16(out, in))
        hipLaunchKernelGGL(gate_activation_kernel<true>, dim3(grid_for(total / 4)), dim3(256), 0, s, out, in, kind, total / 4, alpha, beta);
    else
        hipLaunchKernelGGL(gate_activation_kernel<false>, dim3(grid_for(total)), dim3(256), 0, s, out, in, kind, total, alpha, beta);
    FHIP_CHECK_HIP(hipGetLastError());
    return FHIP_OK;
}

int fhip_gate_route(int op, int n, int c, int h, int w, const float* out, const float* in, const float* residual, char* name, int len)
{
    const int rc = check_shape(n, c, h, w);
    if (rc) return rc;
    if (!name || len < 1) return fail(FHIP_E_BADARG, "null name");
    const int hw = h * w;
    char buf[96];
    switch (op)
    {
    case FHIP_GATE_OP_APPLY: snprintf(buf, sizeof(buf), "fhip::gate_apply_kernel<%s>", hw % 4 == 0 && aligned16(out, in, residual) ? "true" : "false"); break;
    case FHIP_GATE_OP_SQUEEZE:
        snprintf(buf, sizeof(buf), "fhip::squeeze_%s_kernel<%s>", squeeze_route(hw) == SQ_GROUP ? "group" : "block", hw % 4 == 0 && aligned16(in) ? "true" : "false");
        break;
    case FHIP_GATE_OP_EXCITE: snprintf(buf, sizeof(buf), "fhip::excite_kernel"); break;
    case FHIP_GATE_OP_ACTIVATION:
        snprintf(buf, sizeof(buf), "fhip::gate_activation_kernel<%s>", (long long)n * c * hw % 4 == 0 && aligned16(out, in) ? "true" : "false");
        break;
    default: return fail(FHIP_E_BADARG, "unknown op");
    }
    snprintf(name, (size_t)len, "%s", buf);
    return FHIP_OK;
}

const char* fhip_gate_last_error(void) { return last_error(); }

} // extern "C"
