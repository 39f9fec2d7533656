// libfeather_inorm.so: ncnn's InstanceNorm and the element-wise activations of generative nets on gfx950
// (include/feather_hip/feather_inorm.h is the contract; DESIGN.md 3.14 the design and its measurements).
//
// InstanceNorm is a per-plane reduction followed by an affine map: HBM-bound, 8 bytes per element when the plane is read once.  A thread
// holds PER = 16 floats of its plane in registers, so a wave holds 1024, a 256-thread block 4096 and a 1024-thread block 16384:
//
//   inorm_plane_kernel<256, 64, V>      HW <= 1024: one wave per plane, four planes per block, no barrier, no LDS
//   inorm_plane_kernel<256, 256, V>     HW <= 4096: one block per plane
//   inorm_plane_kernel<1024, 1024, V>   HW <= 16384 and at least kSplitMinPlanes planes: one 1024-thread block per plane
//   inorm_partial_kernel<V> + inorm_apply_kernel<V>   everything else (large planes, or too few 64 KB planes to fill 256 CUs): the plane
//       is cut into chunks of 4096 floats, one block per chunk writes (mean, M2) of its chunk to scratch, and every block of the second
//       launch merges its plane's partials in chunk order (Chan) before it re-reads its own chunk -- the same block index handles the
//       same chunk in both launches, so the second read comes from L2 / Infinity Cache where the tensor fits.
//
// V = true: 16-byte accesses (HW a multiple of 4, tensors 16-byte aligned); V = false: 4-byte accesses.  Statistics are the corrected
// two-pass form on the register copy: mean0 = sum(x) / n, then s1 = sum(x - mean0), s2 = sum((x - mean0)^2), mean = mean0 + s1 / n,
// M2 = s2 - s1^2 / n.  The s1 step makes the mean of a constant plane exact, so such a plane gives act(beta) exactly for eps > 0.
// Reductions are xor-shuffles inside a wave and a fixed-order sum over the waves' LDS slots: no atomics, bit-identical run to run.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <string>

#include "feather_hip/feather_inorm.h"
#include "side_error.h"

namespace fhip
{

constexpr int PER = 16;            // floats of a plane (or chunk) one thread holds
constexpr int CHUNK = 256 * PER;   // floats per block of the split-plane route
constexpr int kMaxGrid = 1 << 20;  // blocks of the plane kernels; they stride over what is left
constexpr int kSplitMinPlanes = 256; // fewer 1024-thread blocks than CUs: split the planes instead

// thread t of GROUP threads takes float4 (or float) t + j * GROUP of a run of cnt floats; what lies beyond the run reads as 0
template <int GROUP, bool VEC>
__device__ __forceinline__ bool holds(int j, int t, int cnt)
{
    return VEC ? (t + (j >> 2) * GROUP) < (cnt >> 2) : (t + j * GROUP) < cnt;
}

template <int GROUP, bool VEC>
__device__ __forceinline__ void load_run(float (&v)[PER], const float* __restrict__ src, int cnt, int t)
{
    if (VEC)
    {
        const float4* s4 = reinterpret_cast<const float4*>(src);
#pragma unroll
        for (int j = 0; j < PER / 4; ++j)
        {
            const int i = t + j * GROUP;
            const float4 q = i < (cnt >> 2) ? s4[i] : make_float4(0.f, 0.f, 0.f, 0.f);
            v[4 * j] = q.x;
            v[4 * j + 1] = q.y;
            v[4 * j + 2] = q.z;
            v[4 * j + 3] = q.w;
        }
    }
    else
    {
#pragma unroll
        for (int j = 0; j < PER; ++j)
        {
            const int i = t + j * GROUP;
            v[j] = i < cnt ? src[i] : 0.f;
        }
    }
}

// sums of a and b over the GROUP threads that share a plane, the same value in every thread.  GROUP 64: inside the wave.  Larger: GROUP is
// the whole block, the waves' sums go through `red` ([2][GROUP / 64]) and are added in wave order.
template <int GROUP>
__device__ __forceinline__ void group_sum2(float& a, float& b, float* red)
{
#pragma unroll
    for (int o = 32; o; o >>= 1)
    {
        a += __shfl_xor(a, o);
        b += __shfl_xor(b, o);
    }
    if (GROUP > 64)
    {
        constexpr int W = GROUP / 64;
        const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
        __syncthreads(); // the previous round's readers are done with `red`
        if (lane == 0)
        {
            red[wave] = a;
            red[W + wave] = b;
        }
        __syncthreads();
        a = 0.f;
        b = 0.f;
#pragma unroll
        for (int i = 0; i < W; ++i)
        {
            a += red[i];
            b += red[W + i];
        }
    }
}

template <int GROUP>
__device__ __forceinline__ float group_sum(float a, float* red)
{
#pragma unroll
    for (int o = 32; o; o >>= 1) a += __shfl_xor(a, o);
    if (GROUP > 64)
    {
        constexpr int W = GROUP / 64;
        __syncthreads();
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
        __syncthreads();
        a = 0.f;
#pragma unroll
        for (int i = 0; i < W; ++i) a += red[i];
    }
    return a;
}

// mean and M2 = sum((x - mean)^2) of the cnt floats the group holds
template <int GROUP, bool VEC>
__device__ __forceinline__ void run_stats(const float (&v)[PER], int cnt, int t, float* red, float& mean, float& m2)
{
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < PER; ++j) s += v[j];
    s = group_sum<GROUP>(s, red);
    const float inv = 1.f / (float)cnt;
    const float mean0 = s * inv;
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int j = 0; j < PER; ++j)
        if (holds<GROUP, VEC>(j, t, cnt))
        {
            const float d = v[j] - mean0;
            s1 += d;
            s2 = fmaf(d, d, s2);
        }
    group_sum2<GROUP>(s1, s2, red);
    const float dm = s1 * inv;
    mean = mean0 + dm;
    m2 = fmaxf(s2 - s1 * dm, 0.f);
}

__device__ __forceinline__ float epilogue(float y, int act, float slope)
{
    if (act == FHIP_INORM_ACT_NONE) return y;
    return y > 0.f ? y : (act == FHIP_INORM_ACT_RELU ? 0.f : y * slope);
}

template <int GROUP, bool VEC>
__device__ __forceinline__ void store_run(float* __restrict__ dst, const float (&v)[PER], int cnt, int t, float mean, float a, float b, int act,
                                          float slope)
{
    if (VEC)
    {
        float4* d4 = reinterpret_cast<float4*>(dst);
#pragma unroll
        for (int j = 0; j < PER / 4; ++j)
        {
            const int i = t + j * GROUP;
            if (i < (cnt >> 2))
                d4[i] = make_float4(epilogue(fmaf(v[4 * j] - mean, a, b), act, slope), epilogue(fmaf(v[4 * j + 1] - mean, a, b), act, slope),
                                    epilogue(fmaf(v[4 * j + 2] - mean, a, b), act, slope), epilogue(fmaf(v[4 * j + 3] - mean, a, b), act, slope));
        }
    }
    else
    {
#pragma unroll
        for (int j = 0; j < PER; ++j)
        {
            const int i = t + j * GROUP;
            if (i < cnt) dst[i] = epilogue(fmaf(v[j] - mean, a, b), act, slope);
        }
    }
}

// a plane of at most GROUP * PER floats per GROUP threads, THREADS / GROUP planes per block: read once, held in registers
template <int THREADS, int GROUP, bool VEC>
__global__ __launch_bounds__(THREADS) void inorm_plane_kernel(float* __restrict__ out, const float* __restrict__ in, const float* __restrict__ gamma,
                                                              const float* __restrict__ beta, int planes, int c, int hw, float eps, int act, float slope)
{
    static_assert(GROUP == 64 || GROUP == THREADS, "a group is a wave or the block");
    __shared__ float red[2 * (THREADS / 64)];
    const int t = threadIdx.x % GROUP;
    // grid-strided over the planes (the launch caps the grid): `plane` is the same in a whole wave of a GROUP 64 block, which has no
    // barrier, and in the whole of a GROUP == THREADS block, so every barrier is reached by all of its threads
    for (long long plane = (long long)blockIdx.x * (THREADS / GROUP) + threadIdx.x / GROUP; plane < planes; plane += (long long)gridDim.x * (THREADS / GROUP))
    {
        const size_t base = (size_t)plane * hw;
        float v[PER];
        load_run<GROUP, VEC>(v, in + base, hw, t);
        float mean, m2;
        run_stats<GROUP, VEC>(v, hw, t, red, mean, m2);
        const int ch = (int)(plane % c);
        const float a = (gamma ? gamma[ch] : 1.f) / sqrtf(m2 / (float)hw + eps);
        store_run<GROUP, VEC>(out + base, v, hw, t, mean, a, beta ? beta[ch] : 0.f, act, slope);
    }
}

// split-plane route, first launch: block plane * nchunks + chunk writes (mean, M2) of its chunk
template <bool VEC>
__global__ __launch_bounds__(256) void inorm_partial_kernel(float2* __restrict__ partial, const float* __restrict__ in, int nchunks, int hw)
{
    __shared__ float red[8];
    const int plane = blockIdx.x / nchunks, chunk = blockIdx.x % nchunks;
    const int start = chunk * CHUNK, cnt = min(CHUNK, hw - start);
    float v[PER];
    load_run<256, VEC>(v, in + (size_t)plane * hw + start, cnt, threadIdx.x);
    float mean, m2;
    run_stats<256, VEC>(v, cnt, threadIdx.x, red, mean, m2);
    if (threadIdx.x == 0) partial[blockIdx.x] = make_float2(mean, m2);
}

// split-plane route, second launch: every block merges the partials of its plane in chunk order (the same arithmetic in every block and
// every run), then normalises its own chunk.  The merge is serial and every block of a plane repeats it: nchunks dependent steps on
// L2-resident partials, 4 - 16 for the planes of the zoo's nets (under the latency of the chunk's own loads, which are issued first) and 256
// for a 1024 x 1024 plane, where it is no longer hidden (DESIGN.md 3.14 states the limit).
template <bool VEC>
__global__ __launch_bounds__(256) void inorm_apply_kernel(float* __restrict__ out, const float* __restrict__ in, const float2* __restrict__ partial,
                                                          const float* __restrict__ gamma, const float* __restrict__ beta, int nchunks, int c, int hw,
                                                          float eps, int act, float slope)
{
    const int plane = blockIdx.x / nchunks, chunk = blockIdx.x % nchunks;
    const int start = chunk * CHUNK, cnt = min(CHUNK, hw - start);
    const size_t base = (size_t)plane * hw + start;
    float v[PER];
    load_run<256, VEC>(v, in + base, cnt, threadIdx.x); // issued before the merge
    float na = 0.f, mean = 0.f, m2 = 0.f;
    for (int k = 0; k < nchunks; ++k)
    {
        const float2 p = partial[plane * nchunks + k];
        const float nb = (float)min(CHUNK, hw - k * CHUNK);
        const float n = na + nb, delta = p.x - mean, r = nb / n;
        mean = fmaf(delta, r, mean);
        m2 += p.y + delta * delta * na * r;
        na = n;
    }
    const int ch = plane % c;
    const float a = (gamma ? gamma[ch] : 1.f) / sqrtf(m2 / (float)hw + eps);
    store_run<256, VEC>(out + base, v, cnt, threadIdx.x, mean, a, beta ? beta[ch] : 0.f, act, slope);
}

__device__ __forceinline__ float act_apply(int kind, float x, float p0, float p1)
{
    switch (kind)
    {
    case FHIP_ACTIVATION_SIGMOID: return 1.f / (1.f + expf(-x));
    case FHIP_ACTIVATION_TANH: return tanhf(x);
    case FHIP_ACTIVATION_CLIP: return fminf(fmaxf(x, p0), p1);
    default: return x > 0.f ? x : x * p0; // leaky ReLU, PReLU
    }
}

// units = floats (VEC: float4s) of the whole tensor, grid-strided; slopes (PReLU per channel) replaces p0 by slopes[channel]
template <bool VEC>
__global__ __launch_bounds__(256) void activation_kernel(float* out, const float* in, const float* __restrict__ slopes, int kind, unsigned units, int c,
                                                         int hw, float p0, float p1)
{
    for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < units; i += gridDim.x * 256u)
    {
        if (slopes) p0 = slopes[((VEC ? i * 4u : i) / (unsigned)hw) % (unsigned)c];
        if (VEC)
        {
            const float4 q = reinterpret_cast<const float4*>(in)[i];
            reinterpret_cast<float4*>(out)[i] =
                make_float4(act_apply(kind, q.x, p0, p1), act_apply(kind, q.y, p0, p1), act_apply(kind, q.z, p0, p1), act_apply(kind, q.w, p0, p1));
        }
        else
            out[i] = act_apply(kind, in[i], p0, p1);
    }
}

enum Route
{
    ROUTE_WAVE,
    ROUTE_BLOCK256,
    ROUTE_BLOCK1024,
    ROUTE_SPLIT
};

static Route select_route(long long planes, int hw)
{
    if (hw <= 64 * PER) return ROUTE_WAVE;
    if (hw <= 256 * PER) return ROUTE_BLOCK256;
    if (hw <= 1024 * PER && planes >= kSplitMinPlanes) return ROUTE_BLOCK1024;
    return ROUTE_SPLIT;
}

static bool vectorised(int hw, const void* out, const void* in) { return hw % 4 == 0 && (((uintptr_t)out | (uintptr_t)in) & 15) == 0; }

static int check_shape(int n, int c, int h, int w)
{
    if (n < 1 || c < 1 || h < 1 || w < 1) return fail(FHIP_E_BADARG, "every dimension must be at least 1");
    if ((long long)n * c * h * w >= (1ll << 31)) return fail(FHIP_E_BADARG, "tensors of 2^31 elements or more are not supported");
    return FHIP_OK;
}

static int nchunks_of(int hw) { return (hw + CHUNK - 1) / CHUNK; }

} // namespace fhip

using namespace fhip;

extern "C"
{

int fhip_instance_norm_get_buffer_size(int n, int c, int h, int w, size_t* scratch_bytes)
{
    const int rc = check_shape(n, c, h, w);
    if (rc) return rc;
    if (!scratch_bytes) return fail(FHIP_E_BADARG, "null scratch_bytes");
    const long long planes = (long long)n * c;
    *scratch_bytes = select_route(planes, h * w) == ROUTE_SPLIT ? (size_t)planes * nchunks_of(h * w) * sizeof(float2) : 0;
    return FHIP_OK;
}

int fhip_instance_norm_route(int n, int c, int h, int w, const float* out, const float* in, char* name, int len)
{
    const int rc = check_shape(n, c, h, w);
    if (rc) return rc;
    if (!name || len < 1) return fail(FHIP_E_BADARG, "null name");
    const char* v = vectorised(h * w, out, in) ? "true" : "false";
    char buf[96];
    switch (select_route((long long)n * c, h * w))
    {
    case ROUTE_WAVE: snprintf(buf, sizeof(buf), "fhip::inorm_plane_kernel<256, 64, %s>", v); break;
    case ROUTE_BLOCK256: snprintf(buf, sizeof(buf), "fhip::inorm_plane_kernel<256, 256, %s>", v); break;
    case ROUTE_BLOCK1024: snprintf(buf, sizeof(buf), "fhip::inorm_plane_kernel<1024, 1024, %s>", v); break;
    default: snprintf(buf, sizeof(buf), "fhip::inorm_partial_kernel<%s>", v); break;
    }
    snprintf(name, (size_t)len, "%s", buf);
    return FHIP_OK;
}

static int launch(Route route, int n, int c, int h, int w, float* out, const float* in, const float* gamma, const float* beta, float eps, int act,
                  float slope, float* scratch, void* stream)
{
    if (!out || !in) return fail(FHIP_E_BADARG, "null out / in");
    if ((((uintptr_t)out | (uintptr_t)in | (uintptr_t)gamma | (uintptr_t)beta) & 3) != 0) return fail(FHIP_E_BADARG, "pointers must be 4-byte aligned");
    if (!(eps >= 0.f) || !std::isfinite(eps)) return fail(FHIP_E_BADARG, "eps must be finite and not negative");
    if (act != FHIP_INORM_ACT_NONE && act != FHIP_INORM_ACT_RELU && act != FHIP_INORM_ACT_LEAKY) return fail(FHIP_E_BADARG, "unknown activation");
    const int hw = h * w, planes = n * c;
    const bool vec = vectorised(hw, out, in);
    hipStream_t s = (hipStream_t)stream;
    if (route == ROUTE_SPLIT)
    {
        if (!scratch) return fail(FHIP_E_BADARG, "null scratch: this shape takes the split-plane route (fhip_instance_norm_get_buffer_size)");
        if (((uintptr_t)scratch & 7) != 0) return fail(FHIP_E_BADARG, "scratch must be 8-byte aligned");
        const int nchunks = nchunks_of(hw);
        const unsigned blocks = (unsigned)planes * nchunks; // every chunk holds at least one float: fewer blocks than elements, < 2^31
        float2* partial = reinterpret_cast<float2*>(scratch);
        if (vec)
        {
            hipLaunchKernelGGL(inorm_partial_kernel<true>, dim3(blocks), dim3(256), 0, s, partial, in, nchunks, hw);
            hipLaunchKernelGGL(inorm_apply_kernel<true>, dim3(blocks), dim3(256), 0, s, out, in, partial, gamma, beta, nchunks, c, hw, eps, act, slope);
        }
        else
        {
            hipLaunchKernelGGL(inorm_partial_kernel<false>, dim3(blocks), dim3(256), 0, s, partial, in, nchunks, hw);
            hipLaunchKernelGGL(inorm_apply_kernel<false>, dim3(blocks), dim3(256), 0, s, out, in, partial, gamma, beta, nchunks, c, hw, eps, act, slope);
        }
    }
    else if (route == ROUTE_WAVE)
    {
        const dim3 grid(std::min((planes + 3) / 4, kMaxGrid)); // the kernel strides over the rest: 2^31 one-pixel planes stay a legal launch
        if (vec)
            hipLaunchKernelGGL((inorm_plane_kernel<256, 64, true>), grid, dim3(256), 0, s, out, in, gamma, beta, planes, c, hw, eps, act, slope);
        else
            hipLaunchKernelGGL((inorm_plane_kernel<256, 64, false>), grid, dim3(256), 0, s, out, in, gamma, beta, planes, c, hw, eps, act, slope);
    }
    else if (route == ROUTE_BLOCK256)
    {
        const dim3 grid(std::min(planes, kMaxGrid));
        if (vec)
            hipLaunchKernelGGL((inorm_plane_kernel<256, 256, true>), grid, dim3(256), 0, s, out, in, gamma, beta, planes, c, hw, eps, act, slope);
        else
            hipLaunchKernelGGL((inorm_plane_kernel<256, 256, false>), grid, dim3(256), 0, s, out, in, gamma, beta, planes, c, hw, eps, act, slope);
    }
    else
    {
        const dim3 grid(std::min(planes, kMaxGrid));
        if (vec)
            hipLaunchKernelGGL((inorm_plane_kernel<1024, 1024, true>), grid, dim3(1024), 0, s, out, in, gamma, beta, planes, c, hw, eps, act, slope);
        else
            hipLaunchKernelGGL((inorm_plane_kernel<1024, 1024, false>), grid, dim3(1024), 0, s, out, in, gamma, beta, planes, c, hw, eps, act, slope);
    }
    FHIP_CHECK_HIP(hipGetLastError());
    return FHIP_OK;
}

int fhip_instance_norm_forward(int n, int c, int h, int w, float* out, const float* in, const float* gamma, const float* beta, float eps, int act,
                               float slope, float* scratch, void* stream)
{
    const int rc = check_shape(n, c, h, w);
    if (rc) return rc;
    return launch(select_route((long long)n * c, h * w), n, c, h, w, out, in, gamma, beta, eps, act, slope, scratch, stream);
}

int fhip_instance_norm_forward_route(int route, int n, int c, int h, int w, float* out, const float* in, const float* gamma, const float* beta, float eps,
                                     int act, float slope, float* scratch, void* stream)
{
    const int rc = check_shape(n, c, h, w);
    if (rc) return rc;
    if (route < ROUTE_WAVE || route > ROUTE_SPLIT) return fail(FHIP_E_BADARG, "unknown route");
    const int capacity[3] = {64 * PER, 256 * PER, 1024 * PER};
    if (route != ROUTE_SPLIT && h * w > capacity[route]) return fail(FHIP_E_BADARG, "the plane does not fit this route");
    return launch((Route)route, n, c, h, w, out, in, gamma, beta, eps, act, slope, scratch, stream);
}

int fhip_activation_forward(int kind, float* out, const float* in, int n, int c, int hw, float slope_or_min, float max, const float* slope_vector,
                            void* stream)
{
    const int rc = check_shape(n, c, hw, 1);
    if (rc) return rc;
    if (!out || !in) return fail(FHIP_E_BADARG, "null out / in");
    if ((((uintptr_t)out | (uintptr_t)in | (uintptr_t)slope_vector) & 3) != 0) return fail(FHIP_E_BADARG, "pointers must be 4-byte aligned");
    if (kind < FHIP_ACTIVATION_LEAKY_RELU || kind > FHIP_ACTIVATION_CLIP) return fail(FHIP_E_BADARG, "unknown activation kind");
    if (kind == FHIP_ACTIVATION_CLIP && !(slope_or_min <= max)) return fail(FHIP_E_BADARG, "clip needs min <= max");
    const float* slopes = kind == FHIP_ACTIVATION_PRELU ? slope_vector : nullptr;
    const unsigned total = (unsigned)n * c * hw;
    const bool vec = vectorised(hw, out, in);
    const unsigned units = vec ? total / 4 : total;
    const unsigned blocks = std::min(2048u, (units + 255u) / 256u);
    hipStream_t s = (hipStream_t)stream;
    if (vec)
        hipLaunchKernelGGL(activation_kernel<true>, dim3(blocks), dim3(256), 0, s, out, in, slopes, kind, units, c, hw, slope_or_min, max);
    else
        hipLaunchKernelGGL(activation_kernel<false>, dim3(blocks), dim3(256), 0, s, out, in, slopes, kind, units, c, hw, slope_or_min, max);
    FHIP_CHECK_HIP(hipGetLastError());
    return FHIP_OK;
}

const char* fhip_inorm_last_error(void) { return last_error(); }

} // extern "C"
