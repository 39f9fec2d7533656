// libfeather_resample.so: Interp (nearest / bilinear resize) and HardSwish on gfx950 (include/feather_hip/feather_resample.h is the
// contract; DESIGN.md 3.19 the design and its measurements).
//
// Both layers are bound by writing their output; the input of an up-sampling is read several times and those reads hit L2.
//
//   interp_nearest2x_kernel     nearest x2 on both axes (FPN's top-down path, YOLOv3's routes): a lane reads two adjacent input pixels (8 bytes)
//                               and writes one 16-byte store on each of the two output rows they cover
//   interp_vec4_kernel<MODE>    out_w a multiple of 4, out (and residual) 16-byte aligned, no axis scaled down: a lane produces four adjacent
//                               outputs of a row for one 16-byte store, on four rows one after the other; its taps are 4-byte gathers of
//                               neighbouring addresses
//   interp_gather_kernel<MODE>  everything else (odd widths, misaligned pointers, down-scaling): one output column per lane, four rows,
//                               4-byte accesses
// The general kernels are bound by their index and coefficient arithmetic, not by memory, when a lane pays it per output (measured: DESIGN.md
// 3.19); a lane therefore computes its column taps once and reuses them down kRows rows.
//   hardswish_kernel<V>         grid-strided, 16-byte (V) or 4-byte accesses
//
// Indices and coefficients are computed in the kernel from the expressions of the header -- the bilinear source position in double,
// rounded once to fp32 -- with contraction off, so that no product is fused into a sum: the bits are the definition's.  The optional
// residual is added after the resize and the optional ReLU follows, each rounded on its own: the fused form equals the layers one by
// one bit for bit.  No atomics, no LDS, no allocation.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <string>

#include "feather_hip/feather_resample.h"
#include "side_error.h"

namespace fhip
{

constexpr unsigned kMaxGrid = 4096; // blocks of the grid-strided kernels (256 CUs x 16)

// A product, a sum and a difference that are each rounded to fp32: hipcc contracts a * b + c into one fma by default, and the pragma takes
// the contraction off these operations wherever they are inlined (as in csrc_gate/gate.hip).
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

// One axis of the geometry: what a kernel needs to turn an output coordinate into its taps.
struct Axis
{
    int in, out;   // extents
    float step;    // NEAREST: the fp32 step hs / ws of the header
    double scale;  // BILINEAR: (double)in / out, or (double)(in - 1) / (out - 1) with align_corner (0 when out = 1)
    int align;
};

__device__ __forceinline__ int nearest_index(int d, const Axis& a) { return min((int)mul_rounded((float)d, a.step), a.in - 1); }

// mat_pixel_resize.cpp:53-66 for one output coordinate: the two taps (clamped into the plane) and the weight of the second
__device__ __forceinline__ void bilinear_taps(int d, const Axis& a, int& i0, int& i1, float& f)
{
#pragma clang fp contract(off)
    {
        f = a.align ? (float)((double)d * a.scale) : (float)(((double)d + 0.5) * a.scale - 0.5);
        int s = (int)floorf(f);
        f = f - (float)s;
        if (s < 0)
        {
            s = 0;
            f = 0.f;
        }
        if (s >= a.in - 1)
        {
            s = a.in - 2;
            f = 1.f;
        }
        i0 = max(s, 0);
        i1 = min(s + 1, a.in - 1);
    }
}

__device__ __forceinline__ float lerp_rounded(float p, float q, float f)
{
#pragma clang fp contract(off)
    {
        const float g = 1.f - f;
        return add_rounded(mul_rounded(p, g), mul_rounded(q, f));
    }
}

__device__ __forceinline__ float finish(float v, const float* residual, size_t at, int relu)
{
    if (residual) v = add_rounded(v, residual[at]);
    return relu ? fmaxf(v, 0.f) : v;
}

// units = pairs of input pixels of the whole tensor: planes x in_h x in_w / 2.  out = [planes][2 in_h][2 in_w].
__global__ __launch_bounds__(256) void interp_nearest2x_kernel(float* out, const float* __restrict__ in, const float* residual, unsigned units, int in_h,
                                                               int in_w, int relu)
{
    const unsigned half = (unsigned)in_w >> 1;
    const size_t out_w = (size_t)in_w * 2;
    for (unsigned u = blockIdx.x * 256u + threadIdx.x; u < units; u += gridDim.x * 256u)
    {
        const unsigned x2 = u % half, row = u / half; // row = plane * in_h + y
        const float2 p = *reinterpret_cast<const float2*>(in + (size_t)row * in_w + 2 * x2);
        const size_t o = (size_t)row * 2 * out_w + 4 * x2; // (plane * 2 in_h + 2 y) * out_w
#pragma unroll
        for (int r = 0; r < 2; ++r)
        {
            float4 v = make_float4(p.x, p.x, p.y, p.y);
            const size_t at = o + r * out_w;
            if (residual)
            {
                const float4 q = *reinterpret_cast<const float4*>(residual + at);
                v = make_float4(add_rounded(v.x, q.x), add_rounded(v.y, q.y), add_rounded(v.z, q.z), add_rounded(v.w, q.w));
            }
            if (relu) v = make_float4(fmaxf(v.x, 0.f), fmaxf(v.y, 0.f), fmaxf(v.z, 0.f), fmaxf(v.w, 0.f));
            *reinterpret_cast<float4*>(out + at) = v;
        }
    }
}

constexpr int kRows = 4; // output rows one lane produces: the column taps and the index arithmetic are paid once for all of them

// units = groups of four adjacent outputs on kRows consecutive rows of a plane: planes x ceil(out_h / kRows) x out_w / 4.  A lane computes
// the taps of its four columns once and walks down its rows, one 16-byte store each; the taps of a row are the same in every lane of it.
template <int MODE>
__global__ __launch_bounds__(256) void interp_vec4_kernel(float* out, const float* __restrict__ in, const float* residual, unsigned units, Axis ay, Axis ax,
                                                          int relu)
{
    const unsigned w4 = (unsigned)ax.out >> 2, groups = ((unsigned)ay.out + kRows - 1) / kRows;
    for (unsigned u = blockIdx.x * 256u + threadIdx.x; u < units; u += gridDim.x * 256u)
    {
        const unsigned x4 = u % w4, t = u / w4;
        const unsigned dy0 = (t % groups) * kRows, plane = t / groups;
        const float* src = in + (size_t)plane * ay.in * ax.in;
        int x0[4], x1[4];
        float fx[4];
#pragma unroll
        for (int k = 0; k < 4; ++k)
        {
            if (MODE == FHIP_INTERP_NEAREST)
                x0[k] = nearest_index((int)(4 * x4) + k, ax);
            else
                bilinear_taps((int)(4 * x4) + k, ax, x0[k], x1[k], fx[k]);
        }
        const unsigned rows = min((unsigned)kRows, (unsigned)ay.out - dy0);
        for (unsigned r = 0; r < rows; ++r)
        {
            const unsigned dy = dy0 + r;
            const size_t at = ((size_t)plane * ay.out + dy) * ax.out + 4 * x4;
            float v[4];
            if (MODE == FHIP_INTERP_NEAREST)
            {
                const float* s0 = src + (size_t)nearest_index((int)dy, ay) * ax.in;
#pragma unroll
                for (int k = 0; k < 4; ++k) v[k] = s0[x0[k]];
            }
            else
            {
                int y0, y1;
                float fy;
                bilinear_taps((int)dy, ay, y0, y1, fy);
                const float* s0 = src + (size_t)y0 * ax.in;
                const float* s1 = src + (size_t)y1 * ax.in;
#pragma unroll
                for (int k = 0; k < 4; ++k) v[k] = lerp_rounded(lerp_rounded(s0[x0[k]], s0[x1[k]], fx[k]), lerp_rounded(s1[x0[k]], s1[x1[k]], fx[k]), fy);
            }
            float4 y = make_float4(v[0], v[1], v[2], v[3]);
            if (residual)
            {
                const float4 q = *reinterpret_cast<const float4*>(residual + at);
                y = make_float4(add_rounded(y.x, q.x), add_rounded(y.y, q.y), add_rounded(y.z, q.z), add_rounded(y.w, q.w));
            }
            if (relu) y = make_float4(fmaxf(y.x, 0.f), fmaxf(y.y, 0.f), fmaxf(y.z, 0.f), fmaxf(y.w, 0.f));
            *reinterpret_cast<float4*>(out + at) = y;
        }
    }
}

// units = one output column on kRows consecutive rows of a plane: planes x ceil(out_h / kRows) x out_w
template <int MODE>
__global__ __launch_bounds__(256) void interp_gather_kernel(float* out, const float* __restrict__ in, const float* residual, unsigned units, Axis ay, Axis ax,
                                                            int relu)
{
    const unsigned groups = ((unsigned)ay.out + kRows - 1) / kRows;
    for (unsigned u = blockIdx.x * 256u + threadIdx.x; u < units; u += gridDim.x * 256u)
    {
        const unsigned dx = u % (unsigned)ax.out, t = u / (unsigned)ax.out;
        const unsigned dy0 = (t % groups) * kRows, plane = t / groups;
        const float* src = in + (size_t)plane * ay.in * ax.in;
        int x0 = 0, x1 = 0;
        float fx = 0.f;
        if (MODE == FHIP_INTERP_NEAREST)
            x0 = nearest_index((int)dx, ax);
        else
            bilinear_taps((int)dx, ax, x0, x1, fx);
        const unsigned rows = min((unsigned)kRows, (unsigned)ay.out - dy0);
        for (unsigned r = 0; r < rows; ++r)
        {
            const unsigned dy = dy0 + r;
            const size_t at = ((size_t)plane * ay.out + dy) * ax.out + dx;
            float v;
            if (MODE == FHIP_INTERP_NEAREST)
                v = src[(size_t)nearest_index((int)dy, ay) * ax.in + x0];
            else
            {
                int y0, y1;
                float fy;
                bilinear_taps((int)dy, ay, y0, y1, fy);
                const float* s0 = src + (size_t)y0 * ax.in;
                const float* s1 = src + (size_t)y1 * ax.in;
                v = lerp_rounded(lerp_rounded(s0[x0], s0[x1], fx), lerp_rounded(s1[x0], s1[x1], fx), fy);
            }
            out[at] = finish(v, residual, at, relu);
        }
    }
}

// units = floats (VEC: float4s) of the tensor; out may be in: every unit is read before it is written, by the thread that writes it
__device__ __forceinline__ float hard_swish(float x, float alpha, float beta, float lower, float upper)
{
    return x < lower ? 0.f : x > upper ? x : mul_rounded(x, add_rounded(mul_rounded(x, alpha), beta));
}

template <bool VEC>
__global__ __launch_bounds__(256) void hardswish_kernel(float* out, const float* in, unsigned units, float alpha, float beta, float lower, float upper)
{
    for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < units; i += gridDim.x * 256u)
    {
        if (VEC)
        {
            const float4 q = reinterpret_cast<const float4*>(in)[i];
            reinterpret_cast<float4*>(out)[i] = make_float4(hard_swish(q.x, alpha, beta, lower, upper), hard_swish(q.y, alpha, beta, lower, upper),
                                                            hard_swish(q.z, alpha, beta, lower, upper), hard_swish(q.w, alpha, beta, lower, upper));
        }
        else
            out[i] = hard_swish(in[i], alpha, beta, lower, upper);
    }
}

static bool aligned(unsigned mask, const void* a, const void* b = nullptr, const void* c = nullptr) { return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & mask) == 0; }

static unsigned grid_for(unsigned units) { return std::max(1u, std::min(kMaxGrid, (units + 255u) / 256u)); }

static bool good_scale(float s) { return s == 0.f || (std::isfinite(s) && s > 0.f); }

enum InterpRoute
{
    R_NEAREST2X,
    R_VEC4,
    R_GATHER
};

// Everything fhip_interp_forward and fhip_interp_route check that is no pointer, and the two axes.
static int interp_geometry(int mode, int align_corner, int n, int c, int in_h, int in_w, int out_h, int out_w, float height_scale, float width_scale, Axis& ay,
                           Axis& ax)
{
    if (mode != FHIP_INTERP_NEAREST && mode != FHIP_INTERP_BILINEAR)
    {
        char buf[96];
        snprintf(buf, sizeof(buf), "unknown resize_type %d (1 nearest and 2 bilinear are supported)", mode);
        return fail(FHIP_E_BADARG, buf);
    }
    if (n < 1 || c < 1 || in_h < 1 || in_w < 1 || out_h < 1 || out_w < 1) return fail(FHIP_E_BADARG, "every dimension must be at least 1");
    if ((long long)n * c * in_h * in_w >= (1ll << 31) || (long long)n * c * out_h * out_w >= (1ll << 31))
        return fail(FHIP_E_BADARG, "tensors of 2^31 elements or more are not supported");
    if (!good_scale(height_scale) || !good_scale(width_scale)) return fail(FHIP_E_BADARG, "a scale must be finite and positive (or 0: the size was given)");
    ay.in = in_h, ay.out = out_h, ay.align = align_corner != 0;
    ax.in = in_w, ax.out = out_w, ax.align = align_corner != 0;
    ay.step = height_scale > 0.f ? 1.f / height_scale : in_h / (float)out_h;
    ax.step = width_scale > 0.f ? 1.f / width_scale : in_w / (float)out_w;
    ay.scale = align_corner ? (out_h > 1 ? (double)(in_h - 1) / (out_h - 1) : 0.0) : (double)in_h / out_h;
    ax.scale = align_corner ? (out_w > 1 ? (double)(in_w - 1) / (out_w - 1) : 0.0) : (double)in_w / out_w;
    return FHIP_OK;
}

static InterpRoute interp_route(int mode, const Axis& ay, const Axis& ax, const void* out, const void* in, const void* residual)
{
    if (ax.out % 4 != 0 || !aligned(15, out, residual)) return R_GATHER;
    if (mode == FHIP_INTERP_NEAREST && ay.out == 2 * ay.in && ax.out == 2 * ax.in && ay.step == 0.5f && ax.step == 0.5f && aligned(7, in)) return R_NEAREST2X;
    return ay.out >= ay.in && ax.out >= ax.in ? R_VEC4 : R_GATHER;
}

static int check_flat(int n, int c, int hw)
{
    if (n < 1 || c < 1 || hw < 1) return fail(FHIP_E_BADARG, "every dimension must be at least 1");
    if ((long long)n * c * hw >= (1ll << 31)) return fail(FHIP_E_BADARG, "tensors of 2^31 elements or more are not supported");
    return FHIP_OK;
}

} // namespace fhip

using namespace fhip;

extern "C"
{

int fhip_interp_output_dim(int in_h, int in_w, float height_scale, float width_scale, int output_height, int output_width, int* out_h, int* out_w)
{
    if (!out_h || !out_w) return fail(FHIP_E_BADARG, "null out_h / out_w");
    if (in_h < 1 || in_w < 1) return fail(FHIP_E_BADARG, "every dimension must be at least 1");
    const int in[2] = {in_h, in_w}, given[2] = {output_height, output_width};
    const float scale[2] = {height_scale, width_scale};
    int got[2];
    for (int a = 0; a < 2; ++a)
    {
        char buf[128];
        if (given[a])
        {
            if (given[a] < 1)
            {
                snprintf(buf, sizeof(buf), "output %s %d: every dimension must be at least 1", a ? "width" : "height", given[a]);
                return fail(FHIP_E_BADARG, buf);
            }
            got[a] = given[a];
            continue;
        }
        if (!std::isfinite(scale[a]) || !(scale[a] > 0.f))
        {
            snprintf(buf, sizeof(buf), "%s scale %g must be finite and positive", a ? "width" : "height", (double)scale[a]);
            return fail(FHIP_E_BADARG, buf);
        }
        const float prod = (float)in[a] * scale[a];
        if (!(prod < 2147483648.f))
        {
            snprintf(buf, sizeof(buf), "%s scale %g gives an output dimension of 2^31 or more", a ? "width" : "height", (double)scale[a]);
            return fail(FHIP_E_BADARG, buf);
        }
        got[a] = (int)prod;
        if (got[a] < 1)
        {
            snprintf(buf, sizeof(buf), "%s scale %g gives an output dimension below 1", a ? "width" : "height", (double)scale[a]);
            return fail(FHIP_E_BADARG, buf);
        }
    }
    *out_h = got[0];
    *out_w = got[1];
    return FHIP_OK;
}

int fhip_interp_forward(int mode, int align_corner, int n, int c, int in_h, int in_w, int out_h, int out_w, float height_scale, float width_scale, float* out,
                        const float* in, const float* residual, int relu, void* stream)
{
    Axis ay, ax;
    const int rc = interp_geometry(mode, align_corner, n, c, in_h, in_w, out_h, out_w, height_scale, width_scale, ay, ax);
    if (rc) return rc;
    if (!out || !in) return fail(FHIP_E_BADARG, "null out / in");
    if (!aligned(3, out, in, residual)) return fail(FHIP_E_BADARG, "pointers must be 4-byte aligned");
    if (relu != 0 && relu != 1) return fail(FHIP_E_BADARG, "unknown relu (0 or 1)");
    const unsigned planes = (unsigned)n * c, total_in = planes * in_h * in_w, total_out = planes * out_h * out_w;
    const unsigned groups = ((unsigned)out_h + kRows - 1) / kRows; // a lane of the general kernels walks kRows rows
    const unsigned vec_units = planes * groups * ((unsigned)out_w / 4), gather_units = planes * groups * (unsigned)out_w;
    const uintptr_t o0 = (uintptr_t)out, i0 = (uintptr_t)in;
    if (o0 < i0 + (uintptr_t)total_in * 4 && i0 < o0 + (uintptr_t)total_out * 4) return fail(FHIP_E_BADARG, "out must not overlap in");
    hipStream_t s = (hipStream_t)stream;
    switch (interp_route(mode, ay, ax, out, in, residual))
    {
    case R_NEAREST2X:
        hipLaunchKernelGGL(interp_nearest2x_kernel, dim3(grid_for(total_in / 2)), dim3(256), 0, s, out, in, residual, total_in / 2, in_h, in_w, relu);
        break;
    case R_VEC4:
        if (mode == FHIP_INTERP_NEAREST)
            hipLaunchKernelGGL(interp_vec4_kernel<FHIP_INTERP_NEAREST>, dim3(grid_for(vec_units)), dim3(256), 0, s, out, in, residual, vec_units, ay, ax, relu);
        else
            hipLaunchKernelGGL(interp_vec4_kernel<FHIP_INTERP_BILINEAR>, dim3(grid_for(vec_units)), dim3(256), 0, s, out, in, residual, vec_units, ay, ax, relu);
        break;
    default:
        if (mode == FHIP_INTERP_NEAREST)
            hipLaunchKernelGGL(interp_gather_kernel<FHIP_INTERP_NEAREST>, dim3(grid_for(gather_units)), dim3(256), 0, s, out, in, residual, gather_units, ay, ax, relu);
        else
            hipLaunchKernelGGL(interp_gather_kernel<FHIP_INTERP_BILINEAR>, dim3(grid_for(gather_units)), dim3(256), 0, s, out, in, residual, gather_units, ay, ax, relu);
        break;
    }
    FHIP_CHECK_HIP(hipGetLastError());
    return FHIP_OK;
}

int fhip_interp_route(int mode, int n, int c, int in_h, int in_w, int out_h, int out_w, float height_scale, float width_scale, const float* out, const float* in,
                      const float* residual, char* name, int len)
{
    Axis ay, ax;
    const int rc = interp_geometry(mode, 0, n, c, in_h, in_w, out_h, out_w, height_scale, width_scale, ay, ax);
    if (rc) return rc;
    if (!name || len < 1) return fail(FHIP_E_BADARG, "null name");
    char buf[96];
    switch (interp_route(mode, ay, ax, out, in, residual))
    {
    case R_NEAREST2X: snprintf(buf, sizeof(buf), "fhip::interp_nearest2x_kernel"); break;
    case R_VEC4: snprintf(buf, sizeof(buf), "fhip::interp_vec4_kernel<%d>", mode); break;
    default: snprintf(buf, sizeof(buf), "fhip::interp_gather_kernel<%d>", mode); break;
    }
    snprintf(name, (size_t)len, "%s", buf);
    return FHIP_OK;
}

int fhip_hardswish_forward(float* out, const float* in, int n, int c, int hw, float alpha, float beta, void* stream)
{
    const int rc = check_flat(n, c, hw);
    if (rc) return rc;
    if (!out || !in) return fail(FHIP_E_BADARG, "null out / in");
    if (!aligned(3, out, in)) return fail(FHIP_E_BADARG, "pointers must be 4-byte aligned");
    if (!std::isfinite(alpha) || !std::isfinite(beta)) return fail(FHIP_E_BADARG, "alpha and beta must be finite");
    if (alpha == 0.f) return fail(FHIP_E_BADARG, "alpha must not be zero");
    const float lower = -beta / alpha, upper = 1.f / alpha + lower;
    const unsigned total = (unsigned)n * c * hw;
    hipStream_t s = (hipStream_t)stream;
    if (total % 4 == 0 && aligned(15, out, in))
        hipLaunchKernelGGL(hardswish_kernel<true>, dim3(grid_for(total / 4)), dim3(256), 0, s, out, in, total / 4, alpha, beta, lower, upper);
    else
        hipLaunchKernelGGL(hardswish_kernel<false>, dim3(grid_for(total)), dim3(256), 0, s, out, in, total, alpha, beta, lower, upper);
    FHIP_CHECK_HIP(hipGetLastError());
    return FHIP_OK;
}

int fhip_hardswish_route(const float* out, const float* in, int n, int c, int hw, char* name, int len)
{
    const int rc = check_flat(n, c, hw);
    if (rc) return rc;
    if (!name || len < 1) return fail(FHIP_E_BADARG, "null name");
    snprintf(name, (size_t)len, "fhip::hardswish_kernel<%s>", (long long)n * c * hw % 4 == 0 && aligned(15, out, in) ? "true" : "false");
    return FHIP_OK;
}

const char* fhip_resample_last_error(void) { return last_error(); }

} // extern "C"
