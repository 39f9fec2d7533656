// pixel_resample.h -- what the pixel input (layers.hip, PixelSrc) and the pixel output (../csrc_pixout/pixout.hip) share: the reference's
// fixed-point bilinear resize of uint8 images (mat_pixel_resize.cpp) and the channel counts of ncnn's pixel formats.  Device helpers only:
// no kernel lives here.
#pragma once

#include <hip/hip_runtime.h>

namespace fhip
{

// channels of a pixel FORMAT (one half of a pixel type): RGB = 1 and BGR = 2 have 3, GRAY = 4 has 1, RGBA = 8 has 4; 0 for anything else
inline int pixel_format_channels(int format)
{
    const int ch[9] = {0, 3, 3, 0, 1, 0, 0, 0, 4};
    return format >= 1 && format <= 8 ? ch[format] : 0;
}

struct PixelResample
{
    // ncnn's coefficient of output index d along an axis of `src` source pixels (resize_bilinear_c1, mat_pixel_resize.cpp:46-71):
    // float / double steps exactly as written there, so no contraction into FMAs
    static __device__ __forceinline__ void coef(int d, int src, double scale, int& s, int& k0, int& k1)
    {
#pragma clang fp contract(off)
        float f = (float)((d + 0.5) * scale - 0.5);
        s = (int)floorf(f);
        f -= (float)s;
        if (s < 0)
        {
            s = 0;
            f = 0.f;
        }
        if (s >= src - 1)
        {
            s = src - 2;
            f = 1.f;
        }
        const float c0 = (1.f - f) * 2048.f, c1 = f * 2048.f;
        k0 = min(max((int)(c0 + (c0 >= 0.f ? 0.5f : -0.5f)), -32768), 32767); // SATURATE_CAST_SHORT
        k1 = min(max((int)(c1 + (c1 >= 0.f ? 0.5f : -0.5f)), -32768), 32767);
    }
    // one channel of the resized source at an output pixel: the horizontal pass ((S0*a0 + S1*a1) >> 4, kept as a short row value) on
    // rows sy and sy + 1, then the vertical pass of the reference's scalar loop (mat_pixel_resize.cpp:272).  at(dy, dx) is that channel's
    // byte at source pixel (sy + dy, sx + dx), dy and dx 0 or 1: raw image bytes, a plane of an NV21 frame, or RGB computed from one
    template <class At>
    static __device__ __forceinline__ int sample(const At& at, int b0, int b1, int a0, int a1)
    {
        const short row0 = (short)((at(0, 0) * a0 + at(0, 1) * a1) >> 4);
        const short row1 = (short)((at(1, 0) * a0 + at(1, 1) * a1) >> 4);
        return (unsigned char)(((short)((b0 * row0) >> 16) + (short)((b1 * row1) >> 16) + 2) >> 2);
    }
};

} // namespace fhip
