// layers.hip -- SURVEY.md 8(f) rank 1: the layers BETWEEN the convolutions on the device, so a whole forward pass stays
// in HBM.  All of them are HBM-bound elementwise / window kernels; each follows the reference layer it replaces
// (paths relative to /root/reference/src):
//   relu            layers/relu_layer.h:29-41
//   add (+relu)     layers/eltwise_layer.h:69-80 -> booster::add_relu<fuse_relu>, booster/avx/generic_kernels.cpp:138
//   affine (+relu)  layers/batchnorm_layer.h:43-75 (folded alpha/beta), booster::batchnorm<bias,scale,relu>
//                   generic_kernels.cpp:237-279, layers/scale_layer.h + booster::scale<bias> generic_kernels.cpp:203-233
//   pooling         layers/pooling_layer.h:37-88 (max / average / global; NB the window origin subtracts BOTH pads,
//                   :56,:67, the divisor is the number of in-range taps, output dims use ceil, :129-130)
//   softmax         layers/softmax_layer.h:33-53 (over the whole C*H*W of an image)
// InnerProduct needs no kernel of its own: it is a 1x1 convolution over a 1x1 image with C*H*W input channels and runs
// through the implicit-GEMM path (split-K takes care of the tiny N = batch).
#include <float.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>

#include "common.h"
#include "feather_hip/feather_net.h"
#include "pixel_resample.h"

namespace fhip
{

// One float4 per thread, no grid-stride loop: the fastest streaming form on this chip (tools/copy_probe.hip: 6.2 TB/s against
// 4.3-5.4 for any looped variant).  Threads [n4, n4 + tail) finish the count % 4 (or unaligned) remainder one float each.
__global__ __launch_bounds__(256) void relu_kernel(float* __restrict__ y, const float* __restrict__ x, size_t n4, size_t n)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n4)
    {
        float4 v = reinterpret_cast<const float4*>(x)[i];
        v.x = fmaxf(v.x, 0.f);
        v.y = fmaxf(v.y, 0.f);
        v.z = fmaxf(v.z, 0.f);
        v.w = fmaxf(v.w, 0.f);
        reinterpret_cast<float4*>(y)[i] = v;
        return;
    }
    const size_t t = n4 * 4 + (i - n4);
    if (t < n) y[t] = fmaxf(x[t], 0.f);
}

template <bool RELU>
__global__ __launch_bounds__(256) void add_kernel(float* __restrict__ y, const float* __restrict__ a, const float* __restrict__ b,
                                                 size_t n4, size_t n)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n4)
    {
        const float4 u = reinterpret_cast<const float4*>(a)[i], v = reinterpret_cast<const float4*>(b)[i];
        float4 r = make_float4(u.x + v.x, u.y + v.y, u.z + v.z, u.w + v.w);
        if (RELU)
        {
            r.x = fmaxf(r.x, 0.f);
            r.y = fmaxf(r.y, 0.f);
            r.z = fmaxf(r.z, 0.f);
            r.w = fmaxf(r.w, 0.f);
        }
        reinterpret_cast<float4*>(y)[i] = r;
        return;
    }
    const size_t t = n4 * 4 + (i - n4);
    if (t < n)
    {
        const float r = a[t] + b[t];
        y[t] = RELU ? fmaxf(r, 0.f) : r;
    }
}

// ---- sources of affine_kernel --------------------------------------------------------------------------------
// PlaneSrc: the layers' source, the dense fp32 tensor x itself, with mul / add as device vectors (BatchNorm, Scale, fhip_affine).
struct PlaneSrc
{
    __device__ __forceinline__ float4 load4(const float* __restrict__ x, size_t i, size_t) const { return reinterpret_cast<const float4*>(x)[i]; }
    __device__ __forceinline__ float load1(const float* __restrict__ x, size_t i) const { return x[i]; }
    __device__ __forceinline__ float mul(const float* __restrict__ m, int c) const { return m[c]; }
    __device__ __forceinline__ float add(const float* __restrict__ a, int c) const { return a ? a[c] : 0.f; }
    static __device__ __forceinline__ float map(float v, float m, float a) { return v * m + a; }
};

// PixelSrc: a batch of uint8 images [N][h][w][cin] (any byte offset) seen as the [N][cout][th][tw] fp32 tensor that ncnn's
// Mat::from_pixels_resize + substract_mean_normalize make of each (reference src/ncnn/mat_pixel.cpp:1369-1410): a bilinear resize in
// the source format when the size changes (mat_pixel_resize.cpp, 11-bit fixed-point coefficients), then the channel conversion of the
// pixel type on the resized bytes.  Coefficients are computed per output element from the by-value scales (nothing to upload, so the
// call is stream-capturable); mean / norm travel by value too.  x, mul and add of the kernel are unused (NULL).
// With yuv != 0 the images are NV21 frames (w*h Y bytes, then w/2 x h/2 interleaved V,U pairs) and the pixel type's source is the RGB
// that the reference's yuv420sp2rgb makes of them (fhip_yuv420sp_to_float):
//   yuv = 1: resize_bilinear_yuv420sp first (Y plane as c1, VU plane as c2 at half size), then yuv420sp2rgb at the target size;
//   yuv = 2: yuv420sp2rgb at the source size, then from_pixels_resize's resize in RGB (c3).
// With plan != NULL the images are a planned batch (fhip_pixels_to_float_images): image n's layout is plan[n], which stands in for the
// by-value px + n * image, w, h, resize and scales (the images differ in size, pitch and ROI); type, target and mean / norm stay by value.
struct PixelPlanEntry
{
    const unsigned char* px; // the ROI's first byte
    size_t pitch;            // bytes from one source row to the next
    int w, h;                // the ROI's size: the source from_pixels_resize sees
    int resize;              // w != tw || h != th
    int reserved;
    double scale_x, scale_y; // (double)w / tw, (double)h / th, as pixel_src computes them
};

// coef() and sample(), the reference's fixed-point bilinear resize, come from PixelResample (pixel_resample.h)
struct PixelSrc : PixelResample
{
    const unsigned char* px;
    const PixelPlanEntry* plan; // NULL but for fhip_pixels_to_float_images (device memory)
    size_t image;   // bytes per image (h*w*cin, or h*w*3/2 for an NV21 frame)
    int w, h, cin, cout, tw, th;
    int resize;     // 0: target size == source size, the bytes are read as they are
    int gray;       // 1: every output channel is (s0*wt0 + s1*wt1 + s2*wt2) >> 8; 0: output channel c is source channel sel[c]
    int yuv;        // 0: raw pixels, 1 / 2: NV21, resized before / after the conversion to RGB (above)
    int sel[4], wt[3];
    double scale_x, scale_y;       // (double)w / tw, (double)h / th as the reference computes them (host side, IEEE division)
    double uv_scale_x, uv_scale_y; // yuv = 1: (double)(w/2) / (tw/2), (double)(h/2) / (th/2), the VU plane's resize_bilinear_c2
    float m[4], a[4];              // output channel c: v * m[c] + a[c], two roundings (see map)

    // at() of a plane of `step`-byte pixels, rows of `pitch` bytes, starting at the sample's top-left byte p
    struct PlaneAt
    {
        const unsigned char* p;
        size_t pitch;
        int step;
        __device__ __forceinline__ int operator()(int dy, int dx) const { return p[dy * pitch + dx * step]; }
    };
    // channel k (0 R, 1 G, 2 B) of the reference's yuv420sp2rgb (C path, mat_pixel.cpp:1266-1320) for luma y and the block's V, U
    static __device__ __forceinline__ int yuv_rgb(int k, int y, int v, int u)
    {
        v -= 128;
        u -= 128;
        const int d = k == 0 ? 90 * v : (k == 1 ? -46 * v + -22 * u : 113 * u);
        return min(max(((y << 6) + d) >> 6, 0), 255);
    }
    // the pixel type's conversion of one (resized) pixel into output channel c (mat_pixel.cpp from_* functions)
    template <class Get>
    __device__ __forceinline__ float convert(int c, const Get& get) const
    {
        if (gray) return (float)((get(0) * wt[0] + get(1) * wt[1] + get(2) * wt[2]) >> 8);
        return (float)get(sel[c]);
    }
    // output values [e, e + COLS) of one output row (the caller keeps them inside a row); the row's coefficients are computed once
    template <int COLS>
    __device__ __forceinline__ void values(size_t e, float* out) const
    {
        const int ox = (int)(e % tw);
        const size_t t = e / tw;
        const int oy = (int)(t % th);
        const size_t nc = t / th;
        const int c = (int)(nc % cout);
        if (__builtin_expect(plan != nullptr, 0)) // keeps the raw-pixel path (fhip_pixels_to_float) the straight-line one
        {
            planned_values<COLS>((int)(nc / cout), c, oy, ox, out);
            return;
        }
        const unsigned char* img = px + (nc / cout) * image;
        if (__builtin_expect(yuv != 0, 0))
        {
            yuv_values<COLS>(img, c, oy, ox, out);
            return;
        }
        raw_values<COLS>(img, (size_t)w * cin, w, h, resize, scale_x, scale_y, c, oy, ox, out);
    }
    // values() of raw pixels: an image of sw x sh pixels at img, rows `pitch` bytes apart
    template <int COLS>
    __device__ __forceinline__ void raw_values(const unsigned char* img, size_t pitch, int sw, int sh, int rs, double sx_scale, double sy_scale,
                                               int c, int oy, int ox, float* out) const
    {
        if (!rs)
        {
#pragma unroll
            for (int j = 0; j < COLS; ++j)
            {
                const unsigned char* p = img + (size_t)oy * pitch + (size_t)(ox + j) * cin;
                out[j] = convert(c, [&](int k) { return (int)p[k]; });
            }
            return;
        }
        int sy, b0, b1;
        coef(oy, sh, sy_scale, sy, b0, b1);
#pragma unroll
        for (int j = 0; j < COLS; ++j)
        {
            int sx, a0, a1;
            coef(ox + j, sw, sx_scale, sx, a0, a1);
            const unsigned char* p = img + (size_t)sy * pitch + (size_t)sx * cin;
            out[j] = convert(c, [&](int k) { return sample(PlaneAt{p + k, pitch, cin}, b0, b1, a0, a1); });
        }
    }
    // values() of image n of a planned batch.  A wave inside one image (every wave when a plane is a multiple of 256 outputs, 224 x 224
    // among them) reads the entry at a wave-uniform index, so with scalar loads; a wave across two images reads it per lane.
    template <int COLS>
    __device__ __forceinline__ void planned_values(int n, int c, int oy, int ox, float* out) const
    {
        const int u = __builtin_amdgcn_readfirstlane(n);
        if (__builtin_amdgcn_ballot_w64(n != u) == 0)
        {
            const PixelPlanEntry& e = plan[u];
            raw_values<COLS>(e.px, e.pitch, e.w, e.h, e.resize, e.scale_x, e.scale_y, c, oy, ox, out);
            return;
        }
        const PixelPlanEntry& e = plan[n];
        raw_values<COLS>(e.px, e.pitch, e.w, e.h, e.resize, e.scale_x, e.scale_y, c, oy, ox, out);
    }
    // values() of an NV21 frame; Y at img, the VU plane (w/2 pairs per row) at img + w*h
    template <int COLS>
    __device__ __forceinline__ void yuv_values(const unsigned char* img, int c, int oy, int ox, float* out) const
    {
        const unsigned char* Y = img;
        const unsigned char* VU = img + (size_t)w * h;
        // the frame's RGB at source pixel (y, x), channel k: what yuv420sp2rgb writes there
        const auto rgb = [&](int y, int x, int k) {
            const unsigned char* vu = VU + (size_t)(y >> 1) * w + (x & ~1);
            return yuv_rgb(k, Y[(size_t)y * w + x], vu[0], vu[1]);
        };
        if (!resize)
        {
#pragma unroll
            for (int j = 0; j < COLS; ++j) out[j] = convert(c, [&](int k) { return rgb(oy, ox + j, k); });
            return;
        }
        int sy, b0, b1;
        coef(oy, h, scale_y, sy, b0, b1);
        if (yuv == 2)
        {
            // yuv420sp2rgb, then resize_bilinear_c3 of the RGB bytes
#pragma unroll
            for (int j = 0; j < COLS; ++j)
            {
                int sx, a0, a1;
                coef(ox + j, w, scale_x, sx, a0, a1);
                out[j] = convert(c, [&](int k) { return sample([&](int dy, int dx) { return rgb(sy + dy, sx + dx, k); }, b0, b1, a0, a1); });
            }
            return;
        }
        // resize_bilinear_yuv420sp: Y resized as c1 at (w, h) -> (tw, th); VU resized as c2 at (w/2, h/2) -> (tw/2, th/2); then
        // yuv420sp2rgb of the resized frame, whose output pixel (oy, ox) takes the VU pair (oy/2, ox/2)
        int uy, c0, c1;
        coef(oy >> 1, h >> 1, uv_scale_y, uy, c0, c1);
        int v = 0, u = 0;
#pragma unroll
        for (int j = 0; j < COLS; ++j)
        {
            // VEC (COLS = 4) keeps ox a multiple of 4, so columns 2i and 2i + 1 share one VU pair
            if (COLS == 1 || (j & 1) == 0)
            {
                int ux, d0, d1;
                coef((ox + j) >> 1, w >> 1, uv_scale_x, ux, d0, d1);
                const unsigned char* p = VU + (size_t)uy * w + ux * 2;
                v = sample(PlaneAt{p, (size_t)w, 2}, c0, c1, d0, d1);
                u = sample(PlaneAt{p + 1, (size_t)w, 2}, c0, c1, d0, d1);
            }
            int sx, a0, a1;
            coef(ox + j, w, scale_x, sx, a0, a1);
            const int yy = sample(PlaneAt{Y + (size_t)sy * w + sx, (size_t)w, 1}, b0, b1, a0, a1);
            out[j] = convert(c, [&](int k) { return yuv_rgb(k, yy, v, u); });
        }
    }
    __device__ __forceinline__ float4 load4(const float*, size_t, size_t e) const
    {
        float v[4];
        values<4>(e, v);
        return make_float4(v[0], v[1], v[2], v[3]);
    }
    __device__ __forceinline__ float load1(const float*, size_t i) const
    {
        float v;
        values<1>(i, &v);
        return v;
    }
    __device__ __forceinline__ float mul(const float*, int c) const { return m[c]; }
    __device__ __forceinline__ float add(const float*, int c) const { return a[c]; }
    // x * m + a rounded twice (never an FMA), as upstream ncnn's substract_mean_normalize computes it in plain C; m = 1 / a = -0.f stand in
    // for a missing norm / mean, so each one-sided form is the reference's exact x - mean or x * norm
    static __device__ __forceinline__ float map(float v, float m, float a)
    {
#pragma clang fp contract(off)
        return v * m + a;
    }
};

// y[n][c][:] = x[n][c][:] * mul[c] + add[c]  (+ ReLU); one float4 (VEC: HW % 4 == 0, so it stays inside a plane) or one
// float per lane, no loop.  Src supplies x and the per-channel mul / add: PlaneSrc (the default) reads the tensor x and the device
// vectors, PixelSrc computes x from uint8 images (fhip_pixels_to_float).
template <bool RELU, bool VEC, class Src = PlaneSrc>
__global__ __launch_bounds__(256) void affine_kernel(float* __restrict__ y, const float* __restrict__ x, const float* __restrict__ mul,
                                                    const float* __restrict__ add, int C, int HW, size_t total, const Src src = Src())
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const size_t e = VEC ? i * 4 : i;
    const int c = (int)((e / HW) % C);
    const float m = src.mul(mul, c), a = src.add(add, c);
    if (VEC)
    {
        float4 v = src.load4(x, i, e);
        v.x = Src::map(v.x, m, a);
        v.y = Src::map(v.y, m, a);
        v.z = Src::map(v.z, m, a);
        v.w = Src::map(v.w, m, a);
        if (RELU)
        {
            v.x = fmaxf(v.x, 0.f);
            v.y = fmaxf(v.y, 0.f);
            v.z = fmaxf(v.z, 0.f);
            v.w = fmaxf(v.w, 0.f);
        }
        reinterpret_cast<float4*>(y)[i] = v;
    }
    else
    {
        const float v = Src::map(src.load1(x, i), m, a);
        y[i] = RELU ? fmaxf(v, 0.f) : v;
    }
}

struct PoolParams
{
    int planes, H, W, OH, OW, KH, KW, SH, SW;
    int off_y, off_x; // window origin offset = pad_top + pad_bottom / pad_left + pad_right (reference quirk)
    int average;
};

__global__ __launch_bounds__(256) void pooling_kernel(float* __restrict__ y, const float* __restrict__ x, const PoolParams q, long long total)
{
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256)
    {
        const int ox = (int)(idx % q.OW);
        const long long t = idx / q.OW;
        const int oy = (int)(t % q.OH);
        const long long plane = t / q.OH;
        const float* xp = x + plane * q.H * q.W;
        const int y0 = oy * q.SH - q.off_y, x0 = ox * q.SW - q.off_x;
        const int ya = max(y0, 0), yb = min(y0 + q.KH, q.H);
        const int xa = max(x0, 0), xb = min(x0 + q.KW, q.W);
        float total_v = q.average ? 0.f : -FLT_MAX;
        int counter = 0;
        for (int yy = ya; yy < yb; ++yy)
            for (int xx = xa; xx < xb; ++xx)
            {
                const float v = xp[yy * q.W + xx];
                if (q.average)
                {
                    total_v += v;
                    ++counter;
                }
                else
                    total_v = total_v > v ? total_v : v;
            }
        y[idx] = q.average ? total_v / counter : total_v; // empty window: 0/0 = NaN exactly like the reference
    }
}

// 3x3 / stride 2 / unpadded MAX pooling (ResNet pool1, SqueezeNet): 4 consecutive outputs per lane from 3 rows of 9 inputs, read as
// two 16-byte vectors + one scalar per row (the generic kernel issues 36 scalar loads for the same 4 outputs).  Needs W % 4 == 0
// (aligned vectors); the clipped last window of ceil mode is handled by the column / row guards.
__global__ __launch_bounds__(256) void maxpool3s2_kernel(float* __restrict__ y, const float* __restrict__ x, int planes, int H, int W, int OH,
                                                        int OW, int ow4, long long total)
{
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256)
    {
        const int xq = (int)(idx % ow4);
        const long long t = idx / ow4;
        const int oy = (int)(t % OH);
        const long long plane = t / OH;
        const int ox = xq * 4, ix = ox * 2;
        const float* xp = x + plane * H * W;
        float m0 = -FLT_MAX, m1 = -FLT_MAX, m2 = -FLT_MAX, m3 = -FLT_MAX;
        // all nine loads unconditional, from clamped addresses (a load under a branch is waited for on the spot): a row past the image repeats
        // the last one (the maximum does not change), columns past it are replaced by -FLT_MAX after the load
        const bool has_b = ix + 4 < W, has_c = ix + 8 < W;
        float4 a[3], b[3];
        float c[3];
#pragma unroll
        for (int r = 0; r < 3; ++r)
        {
            const float* row = xp + (size_t)min(oy * 2 + r, H - 1) * W + ix;
            a[r] = *reinterpret_cast<const float4*>(row); // ix + 3 < W always (W % 4 == 0)
            b[r] = *reinterpret_cast<const float4*>(row + (has_b ? 4 : 0));
            c[r] = row[has_c ? 8 : 0];
        }
#pragma unroll
        for (int r = 0; r < 3; ++r)
        {
            if (!has_b) b[r] = make_float4(-FLT_MAX, -FLT_MAX, -FLT_MAX, -FLT_MAX);
            if (!has_c) c[r] = -FLT_MAX;
            m0 = fmaxf(m0, fmaxf(fmaxf(a[r].x, a[r].y), a[r].z));
            m1 = fmaxf(m1, fmaxf(fmaxf(a[r].z, a[r].w), b[r].x));
            m2 = fmaxf(m2, fmaxf(fmaxf(b[r].x, b[r].y), b[r].z));
            m3 = fmaxf(m3, fmaxf(fmaxf(b[r].z, b[r].w), c[r]));
        }
        float* yp = y + (plane * OH + oy) * OW + ox;
        if ((OW & 3) == 0) *reinterpret_cast<float4*>(yp) = make_float4(m0, m1, m2, m3); // whole, aligned quads
        else
        {
            yp[0] = m0;
            if (ox + 1 < OW) yp[1] = m1;
            if (ox + 2 < OW) yp[2] = m2;
            if (ox + 3 < OW) yp[3] = m3;
        }
    }
}

// global pooling: one wave per (n, c) plane, lanes stride over the plane (coalesced), butterfly reduction
template <bool AVG>
__global__ __launch_bounds__(256) void plane_reduce_kernel(float* __restrict__ y, const float* __restrict__ x, int planes, int HW)
{
    const int plane = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (plane >= planes) return;
    const float* xp = x + (size_t)plane * HW;
    float v = AVG ? 0.f : -FLT_MAX;
    for (int i = lane; i < HW; i += 64) v = AVG ? v + xp[i] : fmaxf(v, xp[i]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
    {
        const float t = __shfl_xor(v, o);
        v = AVG ? v + t : fmaxf(v, t);
    }
    if (lane == 0) y[plane] = AVG ? v / HW : v;
}

// global pooling of SMALL planes (HW < 128; the 7 x 7 planes in front of every classifier): the wave-per-plane form above spends a whole
// wave, one 4-byte load per lane and a six-step butterfly on 49 values (MobileNet-V1 b256: 262 144 planes, 34 us for 51 MB).  Here a block copies
// 128 consecutive planes -- one contiguous, 16-byte aligned run of the tensor -- to LDS with coalesced float4 loads (plane stride HW | 1: odd,
// conflict-free) and lane t sums plane t in index order, the order of the reference's loop (layers/pooling_layer.h:60-75).
constexpr int kPlaneReducePB = 128;
template <bool AVG>
__global__ __launch_bounds__(256) void plane_reduce_small_kernel(float* __restrict__ y, const float* __restrict__ x, int planes, int HW)
{
    extern __shared__ __attribute__((aligned(16))) float smem[]; // [PB][HW | 1]
    const int tid = threadIdx.x, hwp = HW | 1;
    const int plane0 = blockIdx.x * kPlaneReducePB, np = min(kPlaneReducePB, planes - plane0);
    const float* src = x + (size_t)plane0 * HW; // 128 * HW floats per block: 16-byte aligned
    const int count = np * HW, n4 = count >> 2;
    for (int i = tid; i < n4; i += 256)
    {
        const float4 v = reinterpret_cast<const float4*>(src)[i];
        const float e[4] = {v.x, v.y, v.z, v.w};
        int pl = (4 * i) / HW, r = 4 * i - pl * HW;
#pragma unroll
        for (int c = 0; c < 4; ++c)
        {
            smem[pl * hwp + r] = e[c];
            if (++r == HW)
            {
                r = 0;
                ++pl;
            }
        }
    }
    for (int i = (n4 << 2) + tid; i < count; i += 256) smem[(i / HW) * hwp + (i - (i / HW) * HW)] = src[i];
    __syncthreads();
    if (tid < np)
    {
        const float* p = smem + tid * hwp;
        float v = AVG ? 0.f : -FLT_MAX;
        for (int i = 0; i < HW; ++i) v = AVG ? v + p[i] : fmaxf(v, p[i]);
        y[plane0 + tid] = AVG ? v / HW : v;
    }
}

// one block per image: max, exp-sum, normalise over `cols` values
__global__ __launch_bounds__(256) void softmax_kernel(float* __restrict__ y, const float* __restrict__ x, int cols)
{
    __shared__ float red[256];
    const float* xp = x + (size_t)blockIdx.x * cols;
    float* yp = y + (size_t)blockIdx.x * cols;
    float m = -FLT_MAX;
    for (int i = threadIdx.x; i < cols; i += 256) m = fmaxf(m, xp[i]);
    red[threadIdx.x] = m;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1)
    {
        if (threadIdx.x < s) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + s]);
        __syncthreads();
    }
    m = red[0];
    __syncthreads();
    float sum = 0.f;
    for (int i = threadIdx.x; i < cols; i += 256)
    {
        const float e = expf(xp[i] - m);
        yp[i] = e;
        sum += e;
    }
    red[threadIdx.x] = sum;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1)
    {
        if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    sum = red[0];
    for (int i = threadIdx.x; i < cols; i += 256) yp[i] = yp[i] / sum;
}

int pixel_channels(int type, int* cin, int* cout)
{
    const int from = type & 0xffff, to = (unsigned)type >> 16;
    if (!pixel_format_channels(from) || (to && !pixel_format_channels(to))) return FHIP_E_BADARG;
    // the conversions ncnn's Mat::from_pixels knows (mat_pixel.cpp:1329-1367): none into RGBA, none from a format into itself
    if (to == FHIP_PIXEL_RGBA || to == from) return FHIP_E_BADARG;
    *cin = pixel_format_channels(from);
    *cout = pixel_format_channels(to ? to : from);
    return 0;
}

int yuv420sp_check(int type, int w, int h, int target_w, int target_h, int resize_first, int* cout)
{
    // yuv420sp2rgb gives RGB bytes; from_pixels takes them as RGB, RGB2BGR or RGB2GRAY
    if (type != FHIP_PIXEL_RGB && type != (FHIP_PIXEL_RGB | (FHIP_PIXEL_BGR << 16)) && type != (FHIP_PIXEL_RGB | (FHIP_PIXEL_GRAY << 16)))
        return fail(FHIP_E_BADARG, "an NV21 frame converts as PIXEL_RGB, PIXEL_RGB2BGR or PIXEL_RGB2GRAY");
    if (w < 1 || h < 1 || target_w < 1 || target_h < 1) return fail(FHIP_E_BADARG, "bad argument");
    if ((w | h) & 1) return fail(FHIP_E_BADARG, "an NV21 frame has an even width and height");
    // resize_bilinear_yuv420sp halves the target size for the VU plane and resizes it as c2, which reads index -1 for a 1-pair axis
    if (resize_first && ((target_w | target_h) & 1)) return fail(FHIP_E_BADARG, "resize_first needs an even target width and height");
    if (resize_first && (w < 4 || h < 4)) return fail(FHIP_E_BADARG, "resize_first needs a frame of at least 4x4 pixels");
    *cout = (type >> 16) == FHIP_PIXEL_GRAY ? 1 : 3;
    return 0;
}

// the conversion part of a PixelSrc (everything but the source layout: image, yuv, uv scales)
static PixelSrc pixel_src(const unsigned char* px, int type, int cin, int cout, int w, int h, int target_w, int target_h, const float* mean,
                          const float* norm)
{
    PixelSrc src = {};
    src.px = px;
    src.w = w;
    src.h = h;
    src.cin = cin;
    src.cout = cout;
    src.tw = target_w;
    src.th = target_h;
    src.resize = w != target_w || h != target_h;
    src.scale_x = (double)w / target_w;
    src.scale_y = (double)h / target_h;
    const int to = (type >> 16) ? (type >> 16) : type; // the output format
    const bool swap = (to == FHIP_PIXEL_BGR && (type & 0xffff) != FHIP_PIXEL_BGR) || (to == FHIP_PIXEL_RGB && (type & 0xffff) == FHIP_PIXEL_BGR);
    src.gray = cout == 1 && cin > 1;
    const bool bgr_src = (type & 0xffff) == FHIP_PIXEL_BGR; // BGR2GRAY weighs channel 0 as blue
    src.wt[0] = bgr_src ? 29 : 77;
    src.wt[1] = 150;
    src.wt[2] = bgr_src ? 77 : 29;
    for (int c = 0; c < 4; ++c)
        src.sel[c] = cin == 1 ? 0 : (swap && c < 3 ? 2 - c : c); // GRAY2RGB / GRAY2BGR replicate the one channel
    for (int c = 0; c < cout; ++c)
    {
        const bool has_norm = norm != nullptr, has_mean = mean != nullptr;
        src.m[c] = has_norm ? norm[c] : 1.f;
        src.a[c] = has_mean ? (has_norm ? -(mean[c] * norm[c]) : -mean[c]) : -0.f;
    }
    return src;
}

// one affine_kernel<false, *, PixelSrc> launch over [batch][cout][th][tw]: float4 lanes when a row is a multiple of 4 and the output
// 16-byte aligned, one float per lane otherwise
static int launch_pixels(float* output, const PixelSrc& src, int batch, void* stream)
{
    const int hw = src.tw * src.th;
    const size_t count = (size_t)batch * src.cout * hw;
    const bool vec = (src.tw % 4) == 0 && ((uintptr_t)output & 15) == 0;
    const size_t total = vec ? count / 4 : count;
    if ((total + 255) / 256 > 0x7fffffffULL) return fail(FHIP_E_BADARG, "tensor too large: 2^31 blocks of 256 lanes or more");
    const dim3 grid((unsigned)((total + 255) / 256));
    hipStream_t s = (hipStream_t)stream;
    if (vec)
        hipLaunchKernelGGL((affine_kernel<false, true, PixelSrc>), grid, dim3(256), 0, s, output, nullptr, nullptr, nullptr, src.cout, hw, total, src);
    else
        hipLaunchKernelGGL((affine_kernel<false, false, PixelSrc>), grid, dim3(256), 0, s, output, nullptr, nullptr, nullptr, src.cout, hw, total, src);
    FHIP_CHECK_HIP(hipGetLastError());
    return FHIP_OK;
}

// The opaque plan of fhip_pixel_images_plan: this header, then `batch` PixelPlanEntry.  `check` is a hash of the other fields, so a buffer
// the builder did not write is refused before any launch.
struct PixelPlanHeader
{
    unsigned magic;
    int batch, type, tw, th, cin, cout, reserved;
    unsigned long long bytes; // header + entries
    unsigned long long check;
};
static_assert(sizeof(PixelPlanHeader) % 16 == 0 && sizeof(PixelPlanEntry) % 16 == 0, "plan entries stay 16-byte aligned");
constexpr unsigned kPixelPlanMagic = 0x50504846u; // "FHPP"

static unsigned long long plan_check(const PixelPlanHeader& h)
{
    const unsigned long long v[9] = {h.magic, (unsigned)h.batch, (unsigned)h.type, (unsigned)h.tw, (unsigned)h.th, (unsigned)h.cin, (unsigned)h.cout,
                                     (unsigned)h.reserved, h.bytes};
    unsigned long long x = 0xcbf29ce484222325ULL; // FNV-1a over the fields
    for (unsigned long long f : v) x = (x ^ f) * 0x100000001b3ULL;
    return x;
}

static int bad_image(int i, const char* what)
{
    char msg[160];
    snprintf(msg, sizeof msg, "image %d: %s", i, what);
    return fail(FHIP_E_BADARG, msg);
}

// blocks needed: a thread per float4 plus one per leftover float; 0 = more than a grid holds (2^31 - 1 blocks)
static unsigned ew_grid(size_t n4, size_t n)
{
    const size_t blocks = (n4 + (n - n4 * 4) + 255) / 256;
    return blocks > 0x7fffffffULL ? 0u : (unsigned)blocks;
}
static const char* const kEwTooLarge = "tensor too large: 2^31 blocks of 256 lanes or more";

} // namespace fhip

using namespace fhip;

extern "C"
{

int fhip_relu(float* y, const float* x, size_t count, void* stream)
{
    if (!y || !x) return fail(FHIP_E_BADARG, "null pointer");
    if (count == 0) return FHIP_OK;
    const bool vec = (((uintptr_t)y | (uintptr_t)x) & 15) == 0;
    const size_t n4 = vec ? count / 4 : 0;
    const unsigned grid = ew_grid(n4, count);
    if (!grid) return fail(FHIP_E_BADARG, kEwTooLarge);
    hipLaunchKernelGGL(relu_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, y, x, n4, count);
    FHIP_CHECK_HIP(hipGetLastError());
    return FHIP_OK;
}

int fhip_add(float* y, const float* a, const float* b, size_t count, int relu, void* stream)
{
    if (!y || !a || !b) return fail(FHIP_E_BADARG, "null pointer");
    if (count == 0) return FHIP_OK;
    const bool vec = (((uintptr_t)y | (uintptr_t)a | (uintptr_t)b) & 15) == 0;
    const size_t n4 = vec ? count / 4 : 0;
    const unsigned blocks = ew_grid(n4, count);
    if (!blocks) return fail(FHIP_E_BADARG, kEwTooLarge);
    const dim3 grid(blocks);
    if (relu)
        hipLaunchKernelGGL(add_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, y, a, b, n4, count);
    else
        hipLaunchKernelGGL(add_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, y, a, b, n4, count);
    FHIP_CHECK_HIP(hipGetLastError());
    return FHIP_OK;
}

int fhip_affine(float* y, const float* x, const float* mul, const float* add, int batch, int channels, int hw, int relu, void* stream)
{
    if (!y || !x || !mul || batch < 1 || channels < 1 || hw < 1) return fail(FHIP_E_BADARG, "bad argument");
    const size_t count = (size_t)batch * channels * hw;
    const bool vec = (hw % 4) == 0 && (((uintptr_t)y | (uintptr_t)x) & 15) == 0;
    const size_t total = vec ? count / 4 : count;
    if ((total + 255) / 256 > 0x7fffffffULL) return fail(FHIP_E_BADARG, "tensor too large: 2^31 blocks of 256 lanes or more");
    const dim3 grid((unsigned)((total + 255) / 256));
    hipStream_t s = (hipStream_t)stream;
    if (relu && vec)
        hipLaunchKernelGGL((affine_kernel<true, true>), grid, dim3(256), 0, s, y, x, mul, add, channels, hw, total);
    else if (relu)
        hipLaunchKernelGGL((affine_kernel<true, false>), grid, dim3(256), 0, s, y, x, mul, add, channels, hw, total);
    else if (vec)
        hipLaunchKernelGGL((affine_kernel<false, true>), grid, dim3(256), 0, s, y, x, mul, add, channels, hw, total);
    else
        hipLaunchKernelGGL((affine_kernel<false, false>), grid, dim3(256), 0, s, y, x, mul, add, channels, hw, total);
    FHIP_CHECK_HIP(hipGetLastError());
    return FHIP_OK;
}

int fhip_pixels_to_float(float* output, const unsigned char* pixels, int batch, int type, int w, int h, int target_w, int target_h,
                         const float* mean, const float* norm, void* stream)
{
    int cin, cout;
    if (pixel_channels(type, &cin, &cout)) return fail(FHIP_E_BADARG, "unknown pixel type");
    if (!output || !pixels || batch < 1 || w < 1 || h < 1 || target_w < 1 || target_h < 1) return fail(FHIP_E_BADARG, "bad argument");
    if ((uintptr_t)output & 3) return fail(FHIP_E_BADARG, "output not 4-byte aligned");
    const bool resize = w != target_w || h != target_h;
    // the reference's resize reads column / row -1 for a 1-pixel source axis (sx = srcw - 2); refused here
    if (resize && (w < 2 || h < 2)) return fail(FHIP_E_BADARG, "a source 1 pixel wide or high cannot be resized");
    PixelSrc src = pixel_src(pixels, type, cin, cout, w, h, target_w, target_h, mean, norm);
    src.image = (size_t)h * w * cin;
    return launch_pixels(output, src, batch, stream);
}

int fhip_yuv420sp_to_float(float* output, const unsigned char* yuv, int batch, int type, int w, int h, int target_w, int target_h,
                           int resize_first, const float* mean, const float* norm, void* stream)
{
    int cout;
    if (yuv420sp_check(type, w, h, target_w, target_h, resize_first, &cout)) return FHIP_E_BADARG;
    if (!output || !yuv || batch < 1) return fail(FHIP_E_BADARG, "bad argument");
    if ((uintptr_t)output & 3) return fail(FHIP_E_BADARG, "output not 4-byte aligned");
    PixelSrc src = pixel_src(yuv, type, 3, cout, w, h, target_w, target_h, mean, norm);
    src.image = (size_t)h * w * 3 / 2;
    src.yuv = resize_first ? 1 : 2;
    src.uv_scale_x = (double)(w / 2) / (target_w / 2);
    src.uv_scale_y = (double)(h / 2) / (target_h / 2);
    return launch_pixels(output, src, batch, stream);
}

int fhip_pixel_images_plan(const fhip_pixel_image* images, int batch, int type, int target_w, int target_h, void* plan, size_t* plan_bytes)
{
    int cin, cout;
    if (pixel_channels(type, &cin, &cout)) return fail(FHIP_E_BADARG, "unknown pixel type");
    if (!images || !plan_bytes || batch < 1 || target_w < 1 || target_h < 1) return fail(FHIP_E_BADARG, "bad argument");
    for (int i = 0; i < batch; ++i)
    {
        const fhip_pixel_image& im = images[i];
        if (!im.data) return bad_image(i, "null data");
        if (im.w < 1 || im.h < 1) return bad_image(i, "w and h must be at least 1");
        if ((long long)im.w * cin > 0x7fffffff) return bad_image(i, "row longer than 2 GiB");
        if (im.stride != 0 && (long long)im.stride < (long long)im.w * cin) return bad_image(i, "stride below w * channels");
        const bool whole = im.roi_w == 0 && im.roi_h == 0;
        const long long rx = whole ? 0 : im.roi_x, ry = whole ? 0 : im.roi_y, rw = whole ? im.w : im.roi_w, rh = whole ? im.h : im.roi_h;
        if (rw < 1 || rh < 1 || rx < 0 || ry < 0 || rx + rw > im.w || ry + rh > im.h) return bad_image(i, "ROI not inside the image");
        // the reference's resize reads column / row -1 for a 1-pixel source axis (sx = srcw - 2); refused as in fhip_pixels_to_float
        if ((rw != target_w || rh != target_h) && (rw < 2 || rh < 2)) return bad_image(i, "a ROI 1 pixel wide or high cannot be resized");
    }
    const size_t need = sizeof(PixelPlanHeader) + (size_t)batch * sizeof(PixelPlanEntry);
    if (!plan)
    {
        *plan_bytes = need;
        return FHIP_OK;
    }
    if (*plan_bytes < need) return fail(FHIP_E_BADARG, "plan buffer too small");
    if ((uintptr_t)plan & 7) return fail(FHIP_E_BADARG, "plan not 8-byte aligned");
    PixelPlanHeader hd = {};
    hd.magic = kPixelPlanMagic;
    hd.batch = batch;
    hd.type = type;
    hd.tw = target_w;
    hd.th = target_h;
    hd.cin = cin;
    hd.cout = cout;
    hd.bytes = need;
    hd.check = plan_check(hd);
    memcpy(plan, &hd, sizeof hd);
    PixelPlanEntry* e = reinterpret_cast<PixelPlanEntry*>((char*)plan + sizeof hd);
    for (int i = 0; i < batch; ++i)
    {
        const fhip_pixel_image& im = images[i];
        const bool whole = im.roi_w == 0 && im.roi_h == 0;
        const int rx = whole ? 0 : im.roi_x, ry = whole ? 0 : im.roi_y, rw = whole ? im.w : im.roi_w, rh = whole ? im.h : im.roi_h;
        const size_t pitch = im.stride ? (size_t)im.stride : (size_t)im.w * cin;
        PixelPlanEntry en = {};
        en.px = im.data + (size_t)ry * pitch + (size_t)rx * cin;
        en.pitch = pitch;
        en.w = rw;
        en.h = rh;
        en.resize = rw != target_w || rh != target_h;
        en.scale_x = (double)rw / target_w; // IEEE division on the host, as pixel_src
        en.scale_y = (double)rh / target_h;
        e[i] = en;
    }
    *plan_bytes = need;
    return FHIP_OK;
}

int fhip_pixels_to_float_images(float* output, const void* plan, const void* plan_device, const float* mean, const float* norm, void* stream)
{
    if (!output || !plan || !plan_device) return fail(FHIP_E_BADARG, "bad argument");
    if (((uintptr_t)plan | (uintptr_t)plan_device) & 7) return fail(FHIP_E_BADARG, "plan not 8-byte aligned");
    if ((uintptr_t)output & 3) return fail(FHIP_E_BADARG, "output not 4-byte aligned");
    PixelPlanHeader hd;
    memcpy(&hd, plan, sizeof hd);
    int cin, cout;
    if (hd.magic != kPixelPlanMagic || hd.check != plan_check(hd) || pixel_channels(hd.type, &cin, &cout) || cin != hd.cin || cout != hd.cout ||
        hd.batch < 1 || hd.tw < 1 || hd.th < 1 || hd.bytes != sizeof(PixelPlanHeader) + (size_t)hd.batch * sizeof(PixelPlanEntry))
        return fail(FHIP_E_BADARG, "not a plan written by fhip_pixel_images_plan");
    PixelSrc src = pixel_src(nullptr, hd.type, cin, cout, hd.tw, hd.th, hd.tw, hd.th, mean, norm);
    src.plan = reinterpret_cast<const PixelPlanEntry*>((const char*)plan_device + sizeof(PixelPlanHeader));
    return launch_pixels(output, src, hd.batch, stream);
}

int fhip_pooling_output_dim(const fhip_pool_param* p, int* out_h, int* out_w)
{
    if (!p || !out_h || !out_w) return fail(FHIP_E_BADARG, "null argument");
    if (p->global_pooling)
    {
        *out_h = 1;
        *out_w = 1;
        return FHIP_OK;
    }
    if (p->stride_h < 1 || p->stride_w < 1) return fail(FHIP_E_BADARG, "stride < 1");
    // ceil, layers/pooling_layer.h:129-130
    *out_h = (int)ceilf((float)(p->input_h + p->pad_top + p->pad_bottom - p->kernel_h) / p->stride_h) + 1;
    *out_w = (int)ceilf((float)(p->input_w + p->pad_left + p->pad_right - p->kernel_w) / p->stride_w) + 1;
    return FHIP_OK;
}

int fhip_pooling(const fhip_pool_param* p, int batch, float* y, const float* x, void* stream)
{
    if (!p || !y || !x || batch < 1 || p->channels < 1) return fail(FHIP_E_BADARG, "bad argument");
    PoolParams q;
    int oh = 0, ow = 0;
    int rc = fhip_pooling_output_dim(p, &oh, &ow);
    if (rc) return rc;
    if (oh < 1 || ow < 1) return fail(FHIP_E_BADARG, "empty pooling output");
    // the kernels index planes and the pixels of one plane in int
    // (0x7fffff00, the column limit of the convolutions: the grids round the plane count up in int)
    if ((long long)batch * p->channels > 0x7fffff00LL) return fail(FHIP_E_BADARG, "N*C too large: more than 0x7fffff00 planes");
    if ((long long)oh * ow > 0x7fffffffLL) return fail(FHIP_E_BADARG, "output plane too large: 2^31 elements or more");
    if ((long long)p->input_h * p->input_w > 0x7fffffffLL) return fail(FHIP_E_BADARG, "plane too large: 2^31 elements or more");
    q.planes = batch * p->channels;
    q.H = p->input_h;
    q.W = p->input_w;
    q.OH = oh;
    q.OW = ow;
    q.KH = p->global_pooling ? p->input_h : p->kernel_h;
    q.KW = p->global_pooling ? p->input_w : p->kernel_w;
    q.SH = p->global_pooling ? 1 : p->stride_h;
    q.SW = p->global_pooling ? 1 : p->stride_w;
    q.off_y = p->pad_top + p->pad_bottom;
    q.off_x = p->pad_left + p->pad_right;
    q.average = p->pooling_type != 0;
    const long long total = (long long)q.planes * oh * ow;
    // whole-plane windows (global pooling, or a kernel covering the unpadded image): one wave per plane, coalesced
    if (oh == 1 && ow == 1 && q.off_y == 0 && q.off_x == 0 && q.KH >= q.H && q.KW >= q.W)
    {
        const int planes = q.planes;
        const int hw = q.H * q.W;
        if (hw < 128 && ((uintptr_t)x & 15) == 0) // 128 planes x (hw | 1) floats stay within the 64 KB a launch gets without asking
        {
            const dim3 grid(ceil_div(planes, kPlaneReducePB));
            const size_t lds = (size_t)kPlaneReducePB * (hw | 1) * sizeof(float);
            if (q.average) hipLaunchKernelGGL(plane_reduce_small_kernel<true>, grid, dim3(256), lds, (hipStream_t)stream, y, x, planes, hw);
            else hipLaunchKernelGGL(plane_reduce_small_kernel<false>, grid, dim3(256), lds, (hipStream_t)stream, y, x, planes, hw);
            FHIP_CHECK_HIP(hipGetLastError());
            return FHIP_OK;
        }
        if (q.average)
            hipLaunchKernelGGL(plane_reduce_kernel<true>, dim3(ceil_div(planes, 4)), dim3(256), 0, (hipStream_t)stream, y, x, planes, q.H * q.W);
        else
            hipLaunchKernelGGL(plane_reduce_kernel<false>, dim3(ceil_div(planes, 4)), dim3(256), 0, (hipStream_t)stream, y, x, planes, q.H * q.W);
        FHIP_CHECK_HIP(hipGetLastError());
        return FHIP_OK;
    }
    if (!q.average && q.KH == 3 && q.KW == 3 && q.SH == 2 && q.SW == 2 && q.off_y == 0 && q.off_x == 0 && (q.W % 4) == 0 &&
        (((uintptr_t)x | (uintptr_t)y) & 15) == 0)
    {
        const int ow4 = ceil_div(ow, 4);
        const long long items = (long long)q.planes * oh * ow4;
        hipLaunchKernelGGL(maxpool3s2_kernel, dim3((unsigned)std::min<long long>(256 * 32, (items + 255) / 256)), dim3(256), 0, (hipStream_t)stream, y,
                           x, q.planes, q.H, q.W, oh, ow, ow4, items);
        FHIP_CHECK_HIP(hipGetLastError());
        return FHIP_OK;
    }
    const int grid = (int)std::min<long long>(256 * 16, (total + 255) / 256); // looped: measured faster than one output per lane here
    hipLaunchKernelGGL(pooling_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, y, x, q, total);
    FHIP_CHECK_HIP(hipGetLastError());
    return FHIP_OK;
}

int fhip_softmax(float* y, const float* x, int batch, int count_per_image, void* stream)
{
    if (!y || !x || batch < 1 || count_per_image < 1) return fail(FHIP_E_BADARG, "bad argument");
    hipLaunchKernelGGL(softmax_kernel, dim3(batch), dim3(256), 0, (hipStream_t)stream, y, x, count_per_image);
    FHIP_CHECK_HIP(hipGetLastError());
    return FHIP_OK;
}

} // extern "C"
