// int8_rules.h -- the arithmetic rules of include/feather_hip/feather_qconv.h, once, for the two int8 libraries (libfeather_qconv.so and
// libfeather_q8.so): the quantisation of a value, the dequantisation of an int32 sum, the byte of a packed dword, and the host function behind
// fhip_qconv_dequant_scales and fhip_q8_dequant_scales.  Include after side_error.h (fail()).
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>

namespace fhip
{

// feather_qconv.h "Quantise an input value"
__device__ __forceinline__ int quantise(float x, float s_in)
{
    const float t = __fmul_rn(x, s_in);
    const float r = fminf(fmaxf(roundf(t), -127.f), 127.f);
    return t != t ? 0 : (int)r;
}

// feather_qconv.h "Dequantise"
__device__ __forceinline__ float dequantise(int acc, float d, const float* bias, int k, int relu)
{
    float y = __fmul_rn((float)acc, d); // v_cvt_f32_i32 rounds to nearest even
    if (bias) y = __fadd_rn(y, bias[k]);
    return relu ? fmaxf(y, 0.f) : y;
}

__device__ __forceinline__ int byte_of(int w, int k) { return (int)(signed char)((unsigned)w >> (8 * k)); }

static bool good_input_scale(float s) { return std::isfinite(s) && s > 0.f; }

// d[k] = s_w[k] == 0 ? 0 : 1.0f / (s_in * s_w[k]), on the host
static int int8_dequant_scales(float* d, const float* s_w, int K, float s_in)
{
    if (!d || !s_w || K < 1) return fail(FHIP_E_BADARG, "null d / s_w or K < 1");
    if (!good_input_scale(s_in)) return fail(FHIP_E_BADARG, "s_in must be finite and > 0");
    for (int k = 0; k < K; ++k)
        if (!std::isfinite(s_w[k]) || s_w[k] < 0.f) return fail(FHIP_E_BADARG, "a weight scale is not finite or is negative");
    for (int k = 0; k < K; ++k)
    {
        const float prod = s_in * s_w[k]; // rounded to fp32 before the reciprocal
        d[k] = s_w[k] == 0.f ? 0.f : 1.0f / prod;
    }
    return FHIP_OK;
}

} // namespace fhip
