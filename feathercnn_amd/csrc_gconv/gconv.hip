// gconv.hip -- libfeather_gconv.so: grouped convolution, 1 < group < C (include/feather_hip/feather_gconv.h).  A library of its own: the
// main library's kernel set is closed, and its selection (fhip_conv_select_algo) keeps refusing a partial group as the reference does.
//
// Shape of the kernels: register-tiled direct convolution on the VALU.  A group is a small GEMM (C/group = K/group = 4 .. 32, a reduction
// of 36 .. 288 terms): too small to fill a 16x16 MFMA tile without padding, and fp32 MFMA and fp32 VALU have the same peak on gfx950, so
// the VALU loses nothing and needs no operand shuffling.  What makes it cheap:
//   * a wave is uniform in (group, chunk of KT output channels): blockIdx.y.  The filter taps it multiplies with are therefore the same
//     for all 64 lanes, sit at addresses that depend on blockIdx and loop counters only, and reach the FMAs as scalar-register operands
//     (one read-only scalar load per 4 .. 16 taps) -- no LDS, no barrier, no bank conflicts;
//   * lanes run over (image, output row, strip of 4 output pixels) flattened, so small planes (7 x 7) still fill waves with the batch;
//   * a lane keeps KT x 4 accumulators and loads 3 x (4 * stride + 2) inputs per input channel: 9 * 4 * KT FMAs per 18 (27) loads, the
//     loads of neighbouring lanes overlap and hit the L1;
//   * rows that are a multiple of 4 wide and 16-byte aligned move as float4 (VEC); any other plane takes the dword form of the same kernel.
// Everything else (any kernel size, stride, asymmetric padding, channel counts that are not 4 / 8 / 16 / 32 per group, grouped 1x1) runs
// on gconv_generic_kernel: one output pixel and 4 output channels per lane, bounds-checked dword loads.
// Out-of-plane taps are never multiplied by zero weights: their addresses are clamped into the plane and the value is replaced by 0.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "feather_hip/feather_gconv.h"
#include "direct_conv.h"

namespace fhip
{

// y[n][g * Kg + chunk * KT .. + KT)[oy][ox .. ox + 4) for a 3x3 kernel with pad 1 and stride S in both directions.
// VEC: W % (4 * S) == 0 (so Wo % 4 == 0, every strip is full and every 4 * S input columns behind ox * S are inside the row) and x, y
// 16-byte aligned; else dword accesses, columns past the row neither loaded out of the plane nor stored.
template <int KT, int S, bool VEC>
__global__ __launch_bounds__(256) void gconv3x3_kernel(const DirectConvArgs a)
{
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= a.total) return;
    const int gc = blockIdx.y;
    const int g = gc / a.chunks, chunk = gc - g * a.chunks;
    const int sx = (int)(i % (unsigned)a.strips);
    const unsigned t = i / (unsigned)a.strips;
    const int oy = (int)(t % (unsigned)a.Ho), n = (int)(t / (unsigned)a.Ho);
    const int ox = sx * 4;
    constexpr int NIN = 3 * S + 3; // input columns under 4 outputs
    const size_t plane = (size_t)a.H * a.W;
    const float* xp = a.x + ((size_t)n * a.C + (size_t)g * a.Cg) * plane;
    const float* __restrict__ wp = a.w + (size_t)gc * a.Cg * 9 * KT;
    const int iy0 = oy * S - 1, ix0 = ox * S - 1;

    float acc[KT][4];
#pragma unroll
    for (int k = 0; k < KT; ++k)
#pragma unroll
        for (int p = 0; p < 4; ++p) acc[k][p] = 0.f;

    for (int c = 0; c < a.Cg; ++c, xp += plane, wp += 9 * KT)
    {
#pragma unroll
        for (int r = 0; r < 3; ++r)
        {
            const int iy = iy0 + r;
            const bool row_in = iy >= 0 && iy < a.H;
            const float* row = xp + (size_t)min(max(iy, 0), a.H - 1) * a.W; // always a row of the plane
            float v[NIN];
            if constexpr (VEC)
            {
                v[0] = row[max(ix0, 0)];
                if (ix0 < 0) v[0] = 0.f;
#pragma unroll
                for (int q = 0; q < S; ++q)
                {
                    const float4 f = *reinterpret_cast<const float4*>(row + ix0 + 1 + 4 * q);
                    v[1 + 4 * q] = f.x, v[2 + 4 * q] = f.y, v[3 + 4 * q] = f.z, v[4 + 4 * q] = f.w;
                }
                if constexpr (S == 1)
                {
                    v[5] = row[min(ix0 + 5, a.W - 1)];
                    if (ix0 + 5 >= a.W) v[5] = 0.f;
                }
            }
            else
            {
#pragma unroll
                for (int j = 0; j < NIN; ++j)
                {
                    const int ix = ix0 + j;
                    v[j] = row[min(max(ix, 0), a.W - 1)];
                    if (ix < 0 || ix >= a.W) v[j] = 0.f;
                }
            }
            if (!row_in)
            {
#pragma unroll
                for (int j = 0; j < NIN; ++j) v[j] = 0.f;
            }
#pragma unroll
            for (int s = 0; s < 3; ++s)
#pragma unroll
                for (int k = 0; k < KT; ++k)
                {
                    const float wv = wp[(r * 3 + s) * KT + k]; // uniform over the wave
#pragma unroll
                    for (int p = 0; p < 4; ++p) acc[k][p] = fmaf(wv, v[p * S + s], acc[k][p]);
                }
        }
    }

    const int k0 = g * a.Kg + chunk * KT; // Kg % KT == 0 on this route
    float* yp = a.y + (((size_t)n * a.K + k0) * a.Ho + oy) * a.Wo + ox;
    const size_t oplane = (size_t)a.Ho * a.Wo;
#pragma unroll
    for (int k = 0; k < KT; ++k)
    {
        const float b = a.bias ? a.bias[k0 + k] : 0.f;
        float o[4];
#pragma unroll
        for (int p = 0; p < 4; ++p)
        {
            o[p] = acc[k][p] + b;
            if (a.relu) o[p] = fmaxf(o[p], 0.f);
        }
        if constexpr (VEC)
            *reinterpret_cast<float4*>(yp + k * oplane) = make_float4(o[0], o[1], o[2], o[3]);
        else
        {
#pragma unroll
            for (int p = 0; p < 4; ++p)
                if (ox + p < a.Wo) yp[k * oplane + p] = o[p];
        }
    }
}

// Any kernel size, stride and padding: direct_conv.h's body under this library's kernel name (the name fhip_gconv_route reports).
template <int KT>
__global__ __launch_bounds__(256) void gconv_generic_kernel(const DirectConvArgs a) { direct_conv_body<KT, UnitTaps>(a); }

__global__ __launch_bounds__(256) void gconv_pack_kernel(float* packed, const float* kernel, int Cg, int Kg, int taps, int kt, int chunks, unsigned total)
{
    direct_pack_body(packed, kernel, Cg, Kg, taps, kt, chunks, total);
}

// ---- host side ------------------------------------------------------------------------------------------------

// Every refusal of a param; 0 when the layer is one of this library's.
static int check_param(const fhip_conv_param* p)
{
    const int rc = check_sizes(p);
    if (rc) return rc;
    if (p->pad_left < 0 || p->pad_right < 0 || p->pad_top < 0 || p->pad_bottom < 0) return fail(FHIP_E_BADARG, "negative padding");
    if (p->group <= 1) return fail(FHIP_E_BADARG, "group <= 1: a dense convolution runs through fhip_conv_forward (libfeather_hip.so)");
    if (p->group == p->input_channels) return fail(FHIP_E_BADARG, "group == input_channels: a depthwise convolution runs through fhip_conv_forward (libfeather_hip.so)");
    if (p->group > p->input_channels || p->input_channels % p->group) return fail(FHIP_E_BADARG, "input_channels is not divisible by group");
    if (p->output_channels % p->group) return fail(FHIP_E_BADARG, "output_channels (of the whole layer) is not divisible by group");
    // 64-bit sums: pads near 2^31 overflowed the int form, and which refusal such a param met depended on how the compiler used that
    const long long ph = (long long)p->input_h + p->pad_top + p->pad_bottom, pw = (long long)p->input_w + p->pad_left + p->pad_right;
    if (ph < p->kernel_h || pw < p->kernel_w) return fail(FHIP_E_BADARG, "the kernel is larger than the padded input");
    const long long oh = (ph - p->kernel_h) / p->stride_h + 1, ow = (pw - p->kernel_w) / p->stride_w + 1;
    if (p->output_h != oh || p->output_w != ow) return fail(FHIP_E_BADARG, "output_h / output_w are not what fhip_conv_assign_output_dim gives");
    if (p->activation != FHIP_ACT_NONE && p->activation != FHIP_ACT_RELU) return fail(FHIP_E_BADARG, "activation must be None or ReLU");
    return FHIP_OK;
}

struct Plan
{
    int kt;     // output channels per lane
    bool tuned; // gconv3x3_kernel
};

static bool pow2_4_32(int v) { return v == 4 || v == 8 || v == 16 || v == 32; }

static Plan plan_of(const fhip_conv_param& p)
{
    const int Cg = p.input_channels / p.group, Kg = p.output_channels / p.group;
    Plan pl;
    pl.tuned = p.kernel_h == 3 && p.kernel_w == 3 && p.stride_h == p.stride_w && (p.stride_h == 1 || p.stride_h == 2) && p.pad_left == 1 &&
               p.pad_right == 1 && p.pad_top == 1 && p.pad_bottom == 1 && pow2_4_32(Cg) && pow2_4_32(Kg);
    pl.kt = pl.tuned ? (Kg >= 16 ? 16 : Kg) : kGenericKT;
    return pl;
}

static bool vec_ok(const fhip_conv_param& p, const float* out, const float* in)
{
    return p.input_w % (4 * p.stride_w) == 0 && aligned(out, 16) && aligned(in, 16);
}

typedef void (*gconv_fn)(const DirectConvArgs);
struct Route
{
    gconv_fn fn;
    char name[48];
};

template <int KT, int S>
static Route route_ks(bool vec)
{
    Route r;
    r.fn = vec ? gconv3x3_kernel<KT, S, true> : gconv3x3_kernel<KT, S, false>;
    snprintf(r.name, sizeof(r.name), "fhip::gconv3x3_kernel<%d, %d, %s>", KT, S, vec ? "true" : "false");
    return r;
}

template <int KT>
static Route route_k(int stride, bool vec)
{
    return stride == 1 ? route_ks<KT, 1>(vec) : route_ks<KT, 2>(vec);
}

// the one selection function: fhip_gconv_forward launches r.fn, fhip_gconv_route reports r.name
static Route select(const fhip_conv_param& p, const Plan& pl, const float* out, const float* in)
{
    if (!pl.tuned)
    {
        Route r;
        r.fn = gconv_generic_kernel<kGenericKT>;
        snprintf(r.name, sizeof(r.name), "fhip::gconv_generic_kernel<4>");
        return r;
    }
    const bool vec = vec_ok(p, out, in);
    return pl.kt == 16 ? route_k<16>(p.stride_h, vec) : pl.kt == 8 ? route_k<8>(p.stride_h, vec) : route_k<4>(p.stride_h, vec);
}

} // namespace fhip

using namespace fhip;

extern "C"
{

int fhip_gconv_supported(const fhip_conv_param* param) { return check_param(param) == FHIP_OK ? 1 : 0; }

int fhip_gconv_get_buffer_size(const fhip_conv_param* param, int batch, size_t* scratch_bytes, size_t* packed_bytes)
{
    const int rc = check_param(param);
    if (rc) return rc;
    if (batch < 1 || !scratch_bytes || !packed_bytes) return fail(FHIP_E_BADARG, "batch < 1 or a null size pointer");
    *scratch_bytes = 0;
    *packed_bytes = generic_packed_floats(*param, plan_of(*param).kt) * sizeof(float);
    return FHIP_OK;
}

int fhip_gconv_init(const fhip_conv_param* param, float* packed, const float* kernel, void* stream)
{
    const int rc = check_param(param);
    if (rc) return rc;
    if (!packed || !kernel) return fail(FHIP_E_BADARG, "null packed / kernel");
    if (!aligned(packed, 4) || !aligned(kernel, 4)) return fail(FHIP_E_BADARG, "device pointers must be 4-byte aligned");
    const int kt = plan_of(*param).kt;
    const size_t total = generic_packed_floats(*param, kt);
    if (total > 0x7fffffffULL) return fail(FHIP_E_BADARG, "filter tensor too large: 2^31 packed floats or more");
    launch_direct_pack(gconv_pack_kernel, *param, kt, total, packed, kernel, (hipStream_t)stream);
    FHIP_CHECK_HIP(hipGetLastError());
    return FHIP_OK;
}

int fhip_gconv_forward(const fhip_conv_param* param, int batch, float* out, const float* in, const float* packed, float* /*scratch*/,
                       const float* bias, void* stream)
{
    int rc = check_param(param);
    if (!rc) rc = check_forward_pointers(*param, batch, out, in, packed, bias, 4, "device pointers must be 4-byte aligned");
    if (rc) return rc;
    const fhip_conv_param& p = *param;
    const Plan pl = plan_of(p);
    DirectConvArgs a = direct_conv_args(p, pl.kt, out, in, packed, bias);
    if (pl.tuned) a.strips = (p.output_w + 3) / 4;
    rc = launch_direct(select(p, pl, out, in).fn, a, (size_t)batch * p.output_h * a.strips, (size_t)p.group * a.chunks, (hipStream_t)stream,
                       "tensor too large: 2^31 lanes or more, or more than 65535 channel chunks");
    if (rc) return rc;
    FHIP_CHECK_HIP(hipGetLastError());
    return FHIP_OK;
}

int fhip_gconv_route(const fhip_conv_param* param, const float* out, const float* in, char* name, int len)
{
    const int rc = check_param(param);
    if (rc) return rc;
    if (!out || !in || !name || len < 1) return fail(FHIP_E_BADARG, "null out / in / name");
    if (!aligned(out, 4) || !aligned(in, 4)) return fail(FHIP_E_BADARG, "device pointers must be 4-byte aligned");
    const Route r = select(*param, plan_of(*param), out, in);
    snprintf(name, (size_t)len, "%s", r.name);
    return FHIP_OK;
}

const char* fhip_gconv_last_error(void) { return last_error(); }

} // extern "C"
