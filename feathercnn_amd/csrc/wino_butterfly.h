// wino_butterfly.h -- the F(6x6,3x3) butterflies every transform kernel shares: one text, so that kernels of different libraries (the 2x2-canvas
// transforms of ../csrc_canvas) compute bit-identical values.
#pragma once

#include <hip/hip_runtime.h>

namespace fhip
{

// ---------------------------------------------------------------------------------------------------
// B^T d (8 -> 8) and A^T m (8 -> 6) butterflies (the NNPACK/ncnn F(6,3) variant the reference uses).
__device__ __forceinline__ void bt8(float& r0, float& r1, float& r2, float& r3, float& r4, float& r5, float& r6, float& r7)
{
    const float o0 = (r0 - r6) + 5.25f * (r4 - r2);
    const float o7 = (r7 - r1) + 5.25f * (r3 - r5);
    const float t1 = (r2 + r6) - 4.25f * r4;
    const float t2 = (r1 + r5) - 4.25f * r3;
    const float p1 = r6 + (0.25f * r2 - 1.25f * r4);
    const float p2 = (0.5f * r1 - 2.5f * r3) + 2.f * r5;
    const float q1 = r6 + 4.f * (r2 - 1.25f * r4);
    const float q2 = (2.f * r1 - 2.5f * r3) + 0.5f * r5;
    r0 = o0;
    r1 = t1 + t2;
    r2 = t1 - t2;
    r3 = p1 + p2;
    r4 = p1 - p2;
    r5 = q1 + q2;
    r6 = q1 - q2;
    r7 = o7;
}

__device__ __forceinline__ void at6(float m0, float m1, float m2, float m3, float m4, float m5, float m6, float m7,
                                    float& s0, float& s1, float& s2, float& s3, float& s4, float& s5)
{
    const float a12 = m1 + m2, d12 = m1 - m2;
    const float a34 = m3 + m4, d34 = m3 - m4;
    const float a56 = m5 + m6, d56 = m5 - m6;
    s0 = (m0 + a12) + (a34 + 32.f * a56);
    s1 = (d12 + 2.f * d34) + 16.f * d56;
    s2 = (a12 + 4.f * a34) + 8.f * a56;
    s3 = (d12 + 8.f * d34) + 4.f * d56;
    s4 = (a12 + 16.f * a34) + 2.f * a56;
    s5 = ((d12 + 32.f * d34) + d56) + m7;
}

} // namespace fhip
