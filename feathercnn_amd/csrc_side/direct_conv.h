// direct_conv.h -- the direct ("generic") convolution route of libfeather_gconv.so, libfeather_deconv.so and libfeather_atrous.so: one
// output pixel and KT output channels of one group per lane, bounds-checked dword loads, any kernel size, stride, padding and group.
// A wave is uniform in (group, chunk of KT output channels) = blockIdx.y, so the filter taps are scalar operands wherever every lane walks
// the same taps (the convolutions; a transposed convolution's taps depend on the lane's output phase).  Out-of-plane taps are
// never multiplied by zero weights: their addresses are clamped into the plane and the value is replaced by 0.
// The three libraries differ in ONE thing, the order in which a lane walks the filter taps and the input pixel under each of them: a tap
// walk (UnitTaps, DilatedTaps, PhaseTaps below) is the only per-library code of the kernel.  The host helpers report through side_error.h.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "side_error.h"

namespace fhip
{

typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4))); // a float4 that is only 4-byte aligned

constexpr int kGenericKT = 4; // output channels per lane of the generic kernels

// What a kernel needs, by value (nothing to upload, so the call is stream-capturable).  The tuned direct kernels of the libraries
// (gconv3x3_kernel, atrous_dw3x3_kernel) take the same struct.
struct DirectConvArgs
{
    const float* x;
    const float* w; // packed [group][chunk][C/group][kh * kw][KT], zero-padded past K/group (atrous depthwise: [C][9])
    const float* bias;
    float* y;
    int C, K, Cg, Kg, H, W, Ho, Wo, kh, kw, sh, sw, pt, pl;
    int dh, dw; // dilation: read by the atrous kernels only
    int chunks; // chunks of KT output channels per group
    int strips; // lanes per output row: Wo (generic) or ceil(Wo / 4) (the tuned kernels)
    int relu;
    unsigned total; // lanes: batch * Ho * strips (atrous depthwise: Ho * strips of one plane)
};

// ---- tap walks ----------------------------------------------------------------------------------------------------------
// A walk names, per axis, the first filter tap of the output pixel (oy, ox), the input pixel under it, and the step of both to the next
// tap: the body runs  for (r = r0, iy = iy0; r < kh; r += rstep, iy += ystep)  and the same in x.  Steps that are the same for every
// layer are compile-time constants, so an instance carries no multiply or add it does not need.  `every_tap`: the walk visits every tap, in
// the order of the packed weights, so the body reads them as one stream; else it looks tap (r, s) up.

// convolution: tap r lies over input row oy * sh - pt + r
struct UnitTaps
{
    static constexpr bool every_tap = true;
    static constexpr int r0 = 0, s0 = 0, rstep = 1, sstep = 1, ystep = 1, xstep = 1;
    int iy0, ix0;
    __device__ UnitTaps(const DirectConvArgs& a, int oy, int ox) : iy0(oy * a.sh - a.pt), ix0(ox * a.sw - a.pl) {}
};

// dilated convolution: tap r lies over input row oy * sh - pt + r * dh
struct DilatedTaps
{
    static constexpr bool every_tap = true;
    static constexpr int r0 = 0, s0 = 0, rstep = 1, sstep = 1;
    int iy0, ix0, ystep, xstep;
    __device__ DilatedTaps(const DirectConvArgs& a, int oy, int ox) : iy0(oy * a.sh - a.pt), ix0(ox * a.sw - a.pl), ystep(a.dh), xstep(a.dw) {}
};

// transposed convolution, gathered by output phase: with oy + pt = qy * sh + py (0 <= py < sh) the output sees the taps r = py, py + sh,
// ... only, over the input rows qy, qy - 1, ... of the un-stuffed input (csrc_deconv/deconv.hip derives it)
struct PhaseTaps
{
    static constexpr bool every_tap = false;
    static constexpr int ystep = -1, xstep = -1;
    int r0, s0, iy0, ix0, rstep, sstep;
    __device__ PhaseTaps(const DirectConvArgs& a, int oy, int ox) : rstep(a.sh), sstep(a.sw)
    {
        const int ty = oy + a.pt, tx = ox + a.pl;
        iy0 = ty / a.sh, r0 = ty - iy0 * a.sh;
        ix0 = tx / a.sw, s0 = tx - ix0 * a.sw;
    }
};

// y[n][g * Kg + chunk * KT .. + KT)[oy][ox]; lane i of [batch][Ho][Wo].  Each library wraps this in a one-line __global__ kernel of its
// own name (gconv_generic_kernel, deconv_generic_kernel, atrous_generic_kernel): the names are what fhip_*_route reports and what traces,
// profiles and DESIGN.md's tables show.
template <int KT, class Taps>
__device__ __forceinline__ void direct_conv_body(const DirectConvArgs& a)
{
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= a.total) return;
    const int gc = blockIdx.y;
    const int g = gc / a.chunks, chunk = gc - g * a.chunks;
    const int ox = (int)(i % (unsigned)a.Wo);
    const unsigned t = i / (unsigned)a.Wo;
    const int oy = (int)(t % (unsigned)a.Ho), n = (int)(t / (unsigned)a.Ho);
    const int ntaps = a.kh * a.kw;
    const size_t plane = (size_t)a.H * a.W;
    const float* xp = a.x + ((size_t)n * a.C + (size_t)g * a.Cg) * plane;
    const float* __restrict__ wp = a.w + (size_t)gc * a.Cg * ntaps * KT; // every_tap: the next tap's weights; else the channel's first
    const Taps taps(a, oy, ox);

    float acc[KT];
#pragma unroll
    for (int k = 0; k < KT; ++k) acc[k] = 0.f;
    for (int c = 0; c < a.Cg; ++c, xp += plane, wp += Taps::every_tap ? 0 : ntaps * KT)
        for (int r = taps.r0, iy = taps.iy0; r < a.kh; r += taps.rstep, iy += taps.ystep)
        {
            const bool row_in = iy >= 0 && iy < a.H;
            const float* row = xp + (size_t)min(max(iy, 0), a.H - 1) * a.W; // always a row of the plane
            for (int s = taps.s0, ix = taps.ix0; s < a.kw; s += taps.sstep, ix += taps.xstep, wp += Taps::every_tap ? KT : 0)
            {
                float v = row[min(max(ix, 0), a.W - 1)];
                if (!row_in || ix < 0 || ix >= a.W) v = 0.f;
                const float* wq = Taps::every_tap ? wp : wp + (r * a.kw + s) * KT; // uniform over the wave unless the taps depend on the lane
#pragma unroll
                for (int k = 0; k < KT; ++k) acc[k] = fmaf(wq[k], v, acc[k]);
            }
        }

    const int kk0 = chunk * KT;
    const size_t oplane = (size_t)a.Ho * a.Wo;
    float* yp = a.y + (((size_t)n * a.K + (size_t)g * a.Kg + kk0) * a.Ho + oy) * a.Wo + ox;
#pragma unroll
    for (int k = 0; k < KT; ++k)
        if (kk0 + k < a.Kg)
        {
            float o = acc[k] + (a.bias ? a.bias[g * a.Kg + kk0 + k] : 0.f);
            if (a.relu) o = fmaxf(o, 0.f);
            yp[k * oplane] = o;
        }
}

// kernel [K][Cg][taps] -> packed [group][chunk][Cg][taps][kt], zeros past Kg; one lane per packed word
__device__ __forceinline__ void direct_pack_body(float* packed, const float* kernel, int Cg, int Kg, int taps, int kt, int chunks, unsigned total)
{
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= total) return;
    const int k = (int)(i % (unsigned)kt);
    unsigned t = i / (unsigned)kt;
    const int tap = (int)(t % (unsigned)taps);
    t /= (unsigned)taps;
    const int c = (int)(t % (unsigned)Cg);
    const int gc = (int)(t / (unsigned)Cg);
    const int g = gc / chunks, kk = (gc - g * chunks) * kt + k;
    packed[i] = kk < Kg ? kernel[(((size_t)g * Kg + kk) * Cg + c) * taps + tap] : 0.f;
}

// ---- host side ------------------------------------------------------------------------------------------------------
// `Param` is fhip_conv_param, fhip_deconv_param or fhip_atrous_param: they share the names of their first 17 fields.

// The refusals every library states first, in this order.
template <class Param>
static int check_sizes(const Param* p)
{
    if (!p) return fail(FHIP_E_BADARG, "null param");
    if (p->input_channels < 1 || p->output_channels < 1 || p->input_h < 1 || p->input_w < 1) return fail(FHIP_E_BADARG, "channels and input size must be >= 1");
    if (p->kernel_h < 1 || p->kernel_w < 1 || p->stride_h < 1 || p->stride_w < 1) return fail(FHIP_E_BADARG, "kernel size and stride must be >= 1");
    return FHIP_OK;
}

// The refusals of a forward call's batch and pointers; `packed_to` and `align_msg` are the library's.
template <class Param>
static int check_forward_pointers(const Param& p, int batch, const float* out, const float* in, const float* packed, const float* bias, uintptr_t packed_to,
                                  const char* align_msg)
{
    if (batch < 1) return fail(FHIP_E_BADARG, "batch < 1");
    if (!out || !in || !packed) return fail(FHIP_E_BADARG, "null out / in / packed");
    if (p.bias_term && !bias) return fail(FHIP_E_BADARG, "bias_term is set and bias is NULL");
    if (!aligned(out, 4) || !aligned(in, 4) || !aligned(packed, packed_to) || (p.bias_term && !aligned(bias, 4))) return fail(FHIP_E_BADARG, align_msg);
    return FHIP_OK;
}

// floats of the packed layout above for chunks of `kt` output channels
template <class Param>
static size_t generic_packed_floats(const Param& p, int kt)
{
    const int Cg = p.input_channels / p.group, Kg = p.output_channels / p.group;
    return (size_t)p.group * ((Kg + kt - 1) / kt) * Cg * p.kernel_h * p.kernel_w * kt;
}

// launch a packer kernel (a __global__ around direct_pack_body) over `total` = generic_packed_floats(p, kt) words
template <class Param>
static void launch_direct_pack(void (*kernel)(float*, const float*, int, int, int, int, int, unsigned), const Param& p, int kt, size_t total, float* packed,
                               const float* weights, hipStream_t s)
{
    const int Cg = p.input_channels / p.group, Kg = p.output_channels / p.group;
    hipLaunchKernelGGL(kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, packed, weights, Cg, Kg, p.kernel_h * p.kernel_w, kt, (Kg + kt - 1) / kt,
                       (unsigned)total);
}

// Everything of the args but `total`: one lane per output pixel, no dilation (a caller with strips or dilation sets them after).
template <class Param>
static DirectConvArgs direct_conv_args(const Param& p, int kt, float* out, const float* in, const float* packed, const float* bias)
{
    DirectConvArgs a;
    a.x = in;
    a.w = packed;
    a.bias = p.bias_term ? bias : nullptr;
    a.y = out;
    a.C = p.input_channels;
    a.K = p.output_channels;
    a.Cg = p.input_channels / p.group;
    a.Kg = p.output_channels / p.group;
    a.H = p.input_h;
    a.W = p.input_w;
    a.Ho = p.output_h;
    a.Wo = p.output_w;
    a.kh = p.kernel_h;
    a.kw = p.kernel_w;
    a.sh = p.stride_h;
    a.sw = p.stride_w;
    a.pt = p.pad_top;
    a.pl = p.pad_left;
    a.dh = a.dw = 1;
    a.chunks = (a.Kg + kt - 1) / kt;
    a.strips = p.output_w;
    a.relu = p.activation == FHIP_ACT_RELU;
    a.total = 0;
    return a;
}

// Launch `kernel` with `total` lanes in x and `gy` (group, chunk) pairs in y; `too_large` is the library's refusal of a grid past the limits.
static int launch_direct(void (*kernel)(const DirectConvArgs), DirectConvArgs& a, size_t total, size_t gy, hipStream_t s, const char* too_large)
{
    if (total > 0x7fffffffULL || gy > 65535) return fail(FHIP_E_BADARG, too_large);
    a.total = (unsigned)total;
    hipLaunchKernelGGL(kernel, dim3((unsigned)((total + 255) / 256), (unsigned)gy), dim3(256), 0, s, a);
    return FHIP_OK;
}

} // namespace fhip
