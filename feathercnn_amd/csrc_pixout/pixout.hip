// pixout.hip -- libfeather_pixout.so: fp32 device tensors to uint8 images, ncnn's Mat::to_pixels / to_pixels_resize (+
// substract_mean_normalize) for a batch (include/feather_hip/feather_pixout.h).  The mirror of fhip_pixels_to_float (../csrc/layers.hip,
// PixelSrc), with which it shares the resize arithmetic (../csrc/pixel_resample.h).  A library of its own because the main library's
// kernels all store float: this is the one that stores bytes.
//
// A pure streaming kernel, 4 bytes read per byte written.  One lane makes 4 consecutive pixels of an output row and writes them with
// dword stores (cn = 1: one, cn = 3: three, cn = 4: one 16-byte store), so a wave writes 256 / 768 / 1024 contiguous bytes; at equal size
// it reads one float4 per plane when the rows allow it.  Rows that are not a multiple of 4 pixels end in a lane that writes bytes, and
// outputs whose rows are not aligned for the vector stores take the one-pixel-per-lane kernel.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <string>

#include "feather_hip/feather_pixout.h"
#include "side_error.h"
#include "pixel_resample.h"

namespace fhip
{

// What the kernel needs, by value (nothing to upload, so the call is stream-capturable).
struct PixelDst
{
    const float* x;
    unsigned char* px;
    size_t pitch; // bytes from one output row to the next
    int w, h, tw, th;
    int per_row; // lanes per output row: ceil(tw / 4) (VEC) or tw
    int resize;  // 0: target size == source size (Mat::to_pixels)
    int reverse; // cn = 3: output channel k is plane 2 - k (RGB2BGR / BGR2RGB)
    int load4;   // VEC at equal size: w % 4 == 0 and x 16-byte aligned, one float4 per plane and lane
    double scale_x, scale_y; // (double)w / tw, (double)h / th as the reference computes them (host side, IEEE division)
    float m[4], a[4];        // plane c: v * m[c] + a[c], two roundings (see to_byte)

    // substract_mean_normalize, then SATURATE_CAST_UCHAR: v * m + a rounded twice (never an FMA; m = 1 / a = -0.f stand in for a missing
    // norm / mean, so each one-sided form is the reference's exact x - mean or x * norm), (int) truncation, clamp to 0..255.  The clamp
    // comes first, in float: its bounds are integers and truncation is monotonic, so the byte is the same wherever the reference's cast is
    // defined, and outside it (NaN, inf, |v| >= 2^31) the result is fixed: fmaxf(NaN, 0) = 0.
    __device__ __forceinline__ int to_byte(float v, int c) const
    {
#pragma clang fp contract(off)
        v = v * m[c] + a[c];
        return (int)fminf(fmaxf(v, 0.f), 255.f);
    }
};

// bytes [0, 4 * CN) of 4 pixels as dwords, little-endian
template <int CN>
__device__ __forceinline__ void store_quad(unsigned char* dst, const int (&b)[4][CN])
{
    unsigned d[CN];
#pragma unroll
    for (int i = 0; i < CN; ++i)
    {
        d[i] = 0;
#pragma unroll
        for (int s = 0; s < 4; ++s)
        {
            const int at = i * 4 + s; // byte `at` of the 4 pixels: channel at % CN of pixel at / CN
            d[i] |= (unsigned)b[at / CN][at % CN] << (8 * s);
        }
    }
    if constexpr (CN == 4)
        *reinterpret_cast<uint4*>(dst) = make_uint4(d[0], d[1], d[2], d[3]);
    else
    {
#pragma unroll
        for (int i = 0; i < CN; ++i) reinterpret_cast<unsigned*>(dst)[i] = d[i];
    }
}

// pixels[n][oy][ox .. ox + COLS) of x[n][CN][h][w]; lane i of [batch][th][per_row], no loop.  VEC: COLS = 4, every row start aligned for
// the stores of store_quad (4 bytes, 16 for CN = 4: the host checks the addresses per launch); the last lane of a row whose width is not
// a multiple of 4 writes its 1..3 pixels as bytes.
template <int CN, bool VEC>
__global__ __launch_bounds__(256) void float_to_pixels_kernel(const PixelDst q, size_t total)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    constexpr int COLS = VEC ? 4 : 1;
    const int ox = (int)(i % q.per_row) * COLS;
    const size_t t = i / q.per_row;
    const int oy = (int)(t % q.th);
    const size_t n = t / q.th;
    const size_t plane = (size_t)q.w * q.h;
    const float* img = q.x + n * CN * plane;
    const int cols = VEC ? min(4, q.tw - ox) : 1; // pixels of this lane inside the row
    int b[COLS][CN];
    if (!q.resize)
    {
        const float* p = img + (size_t)oy * q.w + ox;
#pragma unroll
        for (int k = 0; k < CN; ++k)
        {
            const int c = CN == 3 && q.reverse ? 2 - k : k;
            const float* pc = p + c * plane;
            float v[COLS];
            bool loaded = false;
            if constexpr (VEC)
                if (q.load4) // w % 4 == 0: every lane has 4 pixels
                {
                    const float4 f = *reinterpret_cast<const float4*>(pc);
                    v[0] = f.x, v[1] = f.y, v[2] = f.z, v[3] = f.w;
                    loaded = true;
                }
            if (!loaded)
            {
                // unconditional loads from addresses clamped into the row; the columns past it are not stored
#pragma unroll
                for (int j = 0; j < COLS; ++j) v[j] = pc[min(j, cols - 1)];
            }
#pragma unroll
            for (int j = 0; j < COLS; ++j) b[j][k] = q.to_byte(v[j], c);
        }
    }
    else
    {
        int sy, b0, b1;
        PixelResample::coef(oy, q.h, q.scale_y, sy, b0, b1);
#pragma unroll
        for (int j = 0; j < COLS; ++j)
        {
            int sx, a0, a1;
            PixelResample::coef(min(ox + j, q.tw - 1), q.w, q.scale_x, sx, a0, a1);
            const float* p = img + (size_t)sy * q.w + sx; // sy <= h - 2 and sx <= w - 2 (coef), so the 2 x 2 neighbours are inside the plane
#pragma unroll
            for (int k = 0; k < CN; ++k)
            {
                const int c = CN == 3 && q.reverse ? 2 - k : k;
                const float* pc = p + c * plane;
                // the converted byte of the output format at source pixel (sy + dy, sx + dx): no byte image exists in memory
                b[j][k] = PixelResample::sample([&](int dy, int dx) { return q.to_byte(pc[(size_t)dy * q.w + dx], c); }, b0, b1, a0, a1);
            }
        }
    }
    unsigned char* dst = q.px + (n * q.th + oy) * q.pitch + (size_t)ox * CN;
    if constexpr (VEC)
    {
        if (cols == 4)
        {
            store_quad<CN>(dst, b);
            return;
        }
    }
#pragma unroll
    for (int j = 0; j < COLS; ++j)
        if (j < cols)
        {
#pragma unroll
            for (int k = 0; k < CN; ++k) dst[j * CN + k] = (unsigned char)b[j][k];
        }
}

static int output_channels(int type)
{
    switch (type)
    {
    case FHIP_PIXEL_RGB:
    case FHIP_PIXEL_BGR:
    case FHIP_PIXEL_GRAY:
    case FHIP_PIXEL_RGBA:
        return pixel_format_channels(type);
    case FHIP_PIXEL_RGB2BGR:
    case FHIP_PIXEL_BGR2RGB:
        return 3;
    default:
        return 0; // Mat::to_pixels writes nothing for the rest (mat_pixel.cpp:1412-1430)
    }
}

// every refusal of fhip_float_to_pixels; *cn and the row pitch in bytes on success
static int check(const void* pixels, size_t pitch, const float* x, int batch, int type, int w, int h, int target_w, int target_h, int* cn,
                 size_t* row_pitch)
{
    *cn = output_channels(type);
    if (!*cn) return fail(FHIP_E_BADARG, "not an output pixel type: PIXEL_RGB, PIXEL_BGR, PIXEL_GRAY, PIXEL_RGBA, PIXEL_RGB2BGR or PIXEL_BGR2RGB");
    if (!pixels || !x || batch < 1 || w < 1 || h < 1 || target_w < 1 || target_h < 1) return fail(FHIP_E_BADARG, "bad argument");
    if ((uintptr_t)x & 3) return fail(FHIP_E_BADARG, "x must be 4-byte aligned");
    const size_t row = (size_t)target_w * *cn;
    if (pitch && pitch < row) return fail(FHIP_E_BADARG, "pitch is smaller than a row of target_w pixels");
    // the reference's resize reads column / row -1 for a 1-pixel source axis (sx = srcw - 2); refused as in fhip_pixels_to_float
    if ((w != target_w || h != target_h) && (w < 2 || h < 2)) return fail(FHIP_E_BADARG, "a source 1 pixel wide or high cannot be resized");
    *row_pitch = pitch ? pitch : row;
    return FHIP_OK;
}

template <int CN>
static void launch_cn(bool vec, dim3 grid, hipStream_t s, const PixelDst& q, size_t total)
{
    if (vec)
        hipLaunchKernelGGL((float_to_pixels_kernel<CN, true>), grid, dim3(256), 0, s, q, total);
    else
        hipLaunchKernelGGL((float_to_pixels_kernel<CN, false>), grid, dim3(256), 0, s, q, total);
}

// one launch over [batch][th][per_row]; arguments already checked
static int launch(unsigned char* pixels, size_t pitch, const float* x, int batch, int type, int cn, int w, int h, int target_w, int target_h,
                  const float* mean, const float* norm, void* stream)
{
    PixelDst q = {};
    q.x = x;
    q.px = pixels;
    q.pitch = pitch;
    q.w = w;
    q.h = h;
    q.tw = target_w;
    q.th = target_h;
    q.resize = w != target_w || h != target_h;
    q.reverse = type == FHIP_PIXEL_RGB2BGR || type == FHIP_PIXEL_BGR2RGB;
    q.scale_x = (double)w / target_w;
    q.scale_y = (double)h / target_h;
    for (int c = 0; c < cn; ++c)
    {
        q.m[c] = norm ? norm[c] : 1.f;
        q.a[c] = mean ? (norm ? -(mean[c] * norm[c]) : -mean[c]) : -0.f;
    }
    // the vector stores need every row start aligned: the first one and the pitch (a dense image whose rows are not a multiple of the
    // alignment puts later rows and images off it), chosen per launch from the actual addresses
    const size_t align = cn == 4 ? 16 : 4;
    const bool vec = ((uintptr_t)pixels % align) == 0 && (pitch % align) == 0;
    q.per_row = vec ? (target_w + 3) / 4 : target_w;
    q.load4 = vec && !q.resize && (w % 4) == 0 && ((uintptr_t)x & 15) == 0;
    const size_t total = (size_t)batch * target_h * q.per_row;
    if ((total + 255) / 256 > 0x7fffffffULL) return fail(FHIP_E_BADARG, "tensor too large: 2^31 blocks of 256 lanes or more");
    const dim3 grid((unsigned)((total + 255) / 256));
    hipStream_t s = (hipStream_t)stream;
    if (cn == 1)
        launch_cn<1>(vec, grid, s, q, total);
    else if (cn == 3)
        launch_cn<3>(vec, grid, s, q, total);
    else
        launch_cn<4>(vec, grid, s, q, total);
    FHIP_CHECK_HIP(hipGetLastError());
    return FHIP_OK;
}

} // namespace fhip

using namespace fhip;

extern "C"
{

int fhip_pixout_channels(int type)
{
    const int cn = output_channels(type);
    return cn ? cn : fail(FHIP_E_BADARG, "not an output pixel type");
}

int fhip_float_to_pixels(unsigned char* pixels, size_t pitch, const float* x, int batch, int type, int w, int h, int target_w, int target_h,
                         const float* mean, const float* norm, void* stream)
{
    int cn;
    size_t row_pitch;
    const int rc = check(pixels, pitch, x, batch, type, w, h, target_w, target_h, &cn, &row_pitch);
    if (rc) return rc;
    return launch(pixels, row_pitch, x, batch, type, cn, w, h, target_w, target_h, mean, norm, stream);
}

int fhip_float_to_pixels_host(unsigned char* pixels_host, size_t pitch, const float* x, int batch, int type, int w, int h, int target_w,
                              int target_h, const float* mean, const float* norm, void* stream)
{
    int cn;
    size_t row_pitch;
    int rc = check(pixels_host, pitch, x, batch, type, w, h, target_w, target_h, &cn, &row_pitch);
    if (rc) return rc;
    const size_t row = (size_t)target_w * cn, rows = (size_t)batch * target_h;
    unsigned char* staging = nullptr;
    FHIP_CHECK_HIP(hipMalloc(&staging, rows * row));
    rc = launch(staging, row, x, batch, type, cn, w, h, target_w, target_h, mean, norm, stream);
    hipError_t e = hipSuccess;
    if (!rc) e = hipMemcpy2DAsync(pixels_host, row_pitch, staging, row, row, rows, hipMemcpyDeviceToHost, (hipStream_t)stream);
    if (!rc && e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
    (void)hipFree(staging);
    if (rc) return rc;
    if (e != hipSuccess) return fail_hip(e, "copying the pixels to the host");
    return FHIP_OK;
}

const char* fhip_pixout_last_error(void) { return last_error(); }

} // extern "C"
