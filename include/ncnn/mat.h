// ncnn/mat.h -- the part of ncnn::Mat (reference src/ncnn/mat.h, vendored there from Tencent/ncnn) that FeatherCNN's PUBLIC API
// touches: feather::Net::FeedInput(const char*, ncnn::Mat&) and Extract(std::string, ncnn::Mat&) (reference src/net.h:44,50).
// It exists so that application code written against the reference compiles unchanged against include/feather/net.h:
//
//     ncnn::Mat in(w, h, c);            // host memory, channel stride rounded up to 16 bytes (mat.h:288)
//     float* p = in.channel(0);         // fill it ...
//     net.FeedInput("data", in);  net.Forward();
//     ncnn::Mat out;  net.Extract("prob", out);   const float* prob = out.channel(0);
//
// Same include guard as the reference header: a program that already includes the real ncnn mat.h keeps using that one (the
// Net overloads only need data / w / h / c / cstep / elemsize / create() / channel()).
// Host-side fp32 container only: no allocators, no packing, no SIMD -- none of that is on the hot path, which runs on device blobs.
// The pixel entry points (from_pixels, from_pixels_resize, substract_mean_normalize) are plain host code for one image, so that
//
//     ncnn::Mat in = ncnn::Mat::from_pixels_resize(bgr, ncnn::Mat::PIXEL_BGR2RGB, w, h, 224, 224);
//     net.FeedInput("data", in);
//
// compiles and runs unchanged; their output is bit-identical to the reference's (mat_pixel.cpp, mat_pixel_resize.cpp).  The fast path
// for a batch is feather::Net::FeedPixels (include/feather/net.h), which does the same on the device.  One deliberate difference: a
// source 1 pixel wide or high that must be resized gives an empty Mat (the reference reads index -1 there).  substract_mean_normalize
// rounds x * norm and the sum separately ("both" form), like the device; build without FMA contraction (-ffp-contract=off, or no
// -mfma) for bit-equality with it.
// Mat::to_pixels / to_pixels_resize and the reference's free functions yuv420sp2rgb, resize_bilinear_c1..c4 and
// resize_bilinear_yuv420sp are host code too, bit-identical to the reference's C paths; feather::Net::FeedYUV420sp converts a batch of
// NV21 frames on the device.
#ifndef NCNN_MAT_H
#define NCNN_MAT_H

#include <math.h>
#include <stddef.h>
#include <stdlib.h>
#include <string.h>

namespace ncnn
{

inline void resize_bilinear_c1(const unsigned char* src, int srcw, int srch, unsigned char* dst, int w, int h);
inline void resize_bilinear_c2(const unsigned char* src, int srcw, int srch, unsigned char* dst, int w, int h);
inline void resize_bilinear_c3(const unsigned char* src, int srcw, int srch, unsigned char* dst, int w, int h);
inline void resize_bilinear_c4(const unsigned char* src, int srcw, int srch, unsigned char* dst, int w, int h);

class Mat
{
  public:
    Mat() : data(0), refcount(0), elemsize(0), dims(0), w(0), h(0), c(0), cstep(0) {}
    Mat(int w_, size_t elemsize_ = 4u) : data(0), refcount(0), elemsize(0), dims(0), w(0), h(0), c(0), cstep(0) { create(w_, elemsize_); }
    Mat(int w_, int h_, size_t elemsize_ = 4u) : data(0), refcount(0), elemsize(0), dims(0), w(0), h(0), c(0), cstep(0) { create(w_, h_, elemsize_); }
    Mat(int w_, int h_, int c_, size_t elemsize_ = 4u) : data(0), refcount(0), elemsize(0), dims(0), w(0), h(0), c(0), cstep(0)
    {
        create(w_, h_, c_, elemsize_);
    }
    // external data (not owned), mat.h:54
    Mat(int w_, int h_, int c_, void* data_, size_t elemsize_ = 4u)
        : data(data_), refcount(0), elemsize(elemsize_), dims(3), w(w_), h(h_), c(c_), cstep(align_size((size_t)w_ * h_ * elemsize_, 16) / elemsize_)
    {
    }
    Mat(const Mat& m) : data(m.data), refcount(m.refcount), elemsize(m.elemsize), dims(m.dims), w(m.w), h(m.h), c(m.c), cstep(m.cstep)
    {
        if (refcount) ++*refcount;
    }
    ~Mat() { release(); }
    Mat& operator=(const Mat& m)
    {
        if (this == &m) return *this;
        if (m.refcount) ++*m.refcount;
        release();
        data = m.data;
        refcount = m.refcount;
        elemsize = m.elemsize;
        dims = m.dims;
        w = m.w;
        h = m.h;
        c = m.c;
        cstep = m.cstep;
        return *this;
    }

    void create(int w_, size_t elemsize_ = 4u) { alloc(1, w_, 1, 1, elemsize_, (size_t)w_); }
    void create(int w_, int h_, size_t elemsize_ = 4u) { alloc(2, w_, h_, 1, elemsize_, (size_t)w_ * h_); }
    void create(int w_, int h_, int c_, size_t elemsize_ = 4u)
    {
        alloc(3, w_, h_, c_, elemsize_, align_size((size_t)w_ * h_ * elemsize_, 16) / elemsize_);
    }
    void release()
    {
        if (refcount && --*refcount == 0)
        {
            free(refcount); // one allocation: [refcount | padding to 64 B | data]
        }
        data = 0;
        refcount = 0;
        elemsize = 0;
        dims = w = h = c = 0;
        cstep = 0;
    }
    bool empty() const { return data == 0 || total() == 0; }
    size_t total() const { return cstep * c; }
    void fill(float v)
    {
        float* p = (float*)data;
        for (size_t i = 0, n = total(); i < n; ++i) p[i] = v;
    }
    Mat clone() const
    {
        Mat m;
        if (dims == 1) m.create(w, elemsize);
        else if (dims == 2) m.create(w, h, elemsize);
        else if (dims == 3) m.create(w, h, c, elemsize);
        if (total()) memcpy(m.data, data, total() * elemsize);
        return m;
    }

    // a 2-D view of channel q (shares the data, like the reference's, mat.h:430-440)
    Mat channel(int q)
    {
        Mat m;
        m.data = (unsigned char*)data + cstep * q * elemsize;
        m.elemsize = elemsize;
        m.dims = 2;
        m.w = w;
        m.h = h;
        m.c = 1;
        m.cstep = (size_t)w * h;
        return m;
    }
    const Mat channel(int q) const { return const_cast<Mat*>(this)->channel(q); }
    float* row(int y) { return (float*)data + (size_t)w * y; }
    const float* row(int y) const { return (const float*)data + (size_t)w * y; }
    template <typename T>
    operator T*()
    {
        return (T*)data;
    }
    template <typename T>
    operator const T*() const
    {
        return (const T*)data;
    }
    float& operator[](int i) { return ((float*)data)[i]; }
    const float& operator[](int i) const { return ((const float*)data)[i]; }

    // ---- pixels (reference mat.h:123-157; ncnn's codes and values) ----
    enum
    {
        PIXEL_CONVERT_SHIFT = 16,
        PIXEL_FORMAT_MASK = 0x0000ffff,
        PIXEL_CONVERT_MASK = 0xffff0000,

        PIXEL_RGB = 1,
        PIXEL_BGR = (1 << 1),
        PIXEL_GRAY = (1 << 2),
        PIXEL_RGBA = (1 << 3),

        PIXEL_RGB2BGR = PIXEL_RGB | (PIXEL_BGR << PIXEL_CONVERT_SHIFT),
        PIXEL_RGB2GRAY = PIXEL_RGB | (PIXEL_GRAY << PIXEL_CONVERT_SHIFT),
        PIXEL_BGR2RGB = PIXEL_BGR | (PIXEL_RGB << PIXEL_CONVERT_SHIFT),
        PIXEL_BGR2GRAY = PIXEL_BGR | (PIXEL_GRAY << PIXEL_CONVERT_SHIFT),
        PIXEL_GRAY2RGB = PIXEL_GRAY | (PIXEL_RGB << PIXEL_CONVERT_SHIFT),
        PIXEL_GRAY2BGR = PIXEL_GRAY | (PIXEL_BGR << PIXEL_CONVERT_SHIFT),
        PIXEL_RGBA2RGB = PIXEL_RGBA | (PIXEL_RGB << PIXEL_CONVERT_SHIFT),
        PIXEL_RGBA2BGR = PIXEL_RGBA | (PIXEL_BGR << PIXEL_CONVERT_SHIFT),
        PIXEL_RGBA2GRAY = PIXEL_RGBA | (PIXEL_GRAY << PIXEL_CONVERT_SHIFT)
    };
    // a (w, h, cout) fp32 Mat of the pixels, converted as `type` says; an empty Mat for an unknown type.  The allocator is ignored.
    static Mat from_pixels(const unsigned char* pixels, int type, int w_, int h_, void* allocator = 0)
    {
        (void)allocator;
        int cin, cout;
        Mat m;
        if (!pixels || w_ < 1 || h_ < 1 || !pixel_channels(type, cin, cout)) return m;
        m.create(w_, h_, cout, 4u);
        if (m.empty()) return m;
        const int from = type & PIXEL_FORMAT_MASK, to = (type >> PIXEL_CONVERT_SHIFT) ? (type >> PIXEL_CONVERT_SHIFT) : from;
        const bool swap = (to == PIXEL_BGR) != (from == PIXEL_BGR); // RGB <-> BGR, RGBA -> BGR
        const bool bgr = from == PIXEL_BGR;
        const size_t size = (size_t)w_ * h_;
        for (int q = 0; q < cout; ++q)
        {
            float* out = (float*)m.data + m.cstep * q;
            const int k = cin == 1 ? 0 : (swap && q < 3 ? 2 - q : q);
            for (size_t i = 0; i < size; ++i)
            {
                const unsigned char* p = pixels + i * cin;
                if (cout == 1 && cin > 1) // (r*77 + g*150 + b*29) >> 8
                    out[i] = (float)(((bgr ? p[2] : p[0]) * 77 + p[1] * 150 + (bgr ? p[0] : p[2]) * 29) >> 8);
                else
                    out[i] = (float)p[k];
            }
        }
        return m;
    }
    // from_pixels after ncnn's fixed-point bilinear resize in the source format (mat_pixel.cpp:1369-1410), when the size changes
    static Mat from_pixels_resize(const unsigned char* pixels, int type, int w_, int h_, int target_width, int target_height, void* allocator = 0)
    {
        if (w_ == target_width && h_ == target_height) return from_pixels(pixels, type, w_, h_, allocator);
        int cin, cout;
        if (!pixels || w_ < 2 || h_ < 2 || target_width < 1 || target_height < 1 || !pixel_channels(type, cin, cout)) return Mat();
        unsigned char* dst = new unsigned char[(size_t)target_width * target_height * cin];
        resize_bilinear(pixels, w_, h_, cin, dst, target_width, target_height);
        Mat m = from_pixels(dst, type, target_width, target_height, allocator);
        delete[] dst;
        return m;
    }
    // the Mat's values as bytes (mat_pixel.cpp:1412-1430): (int) truncation, then clamped to 0..255.  PIXEL_RGB / BGR / GRAY / RGBA write
    // the channels as they are, PIXEL_RGB2BGR / BGR2RGB in reverse order; any other type writes nothing, as in the reference
    void to_pixels(unsigned char* pixels, int type) const
    {
        int cn;
        bool reverse = false;
        if (type == PIXEL_RGB2BGR || type == PIXEL_BGR2RGB)
        {
            cn = 3;
            reverse = true;
        }
        else if (type == PIXEL_RGB || type == PIXEL_BGR)
            cn = 3;
        else if (type == PIXEL_GRAY)
            cn = 1;
        else if (type == PIXEL_RGBA)
            cn = 4;
        else
            return;
        const size_t size = (size_t)w * h;
        for (int k = 0; k < cn; ++k)
        {
            const float* p = (const float*)data + cstep * (reverse ? cn - 1 - k : k);
            for (size_t i = 0; i < size; ++i)
            {
                const int v = (int)p[i];
                pixels[i * cn + k] = (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v));
            }
        }
    }
    // to_pixels, then ncnn's bilinear resize in the output format when the size changes (mat_pixel.cpp:1432-1468).  A Mat 1 pixel wide
    // or high that must be resized writes nothing (the reference reads index -1 there).
    void to_pixels_resize(unsigned char* pixels, int type, int target_width, int target_height) const
    {
        if (w == target_width && h == target_height) return to_pixels(pixels, type);
        const int to = (type & PIXEL_CONVERT_MASK) ? (int)((unsigned)type >> PIXEL_CONVERT_SHIFT) : (type & PIXEL_FORMAT_MASK);
        const int cn = (to == PIXEL_RGB || to == PIXEL_BGR) ? 3 : (to == PIXEL_GRAY ? 1 : (to == PIXEL_RGBA ? 4 : 0));
        if (!cn || w < 2 || h < 2 || target_width < 1 || target_height < 1) return;
        unsigned char* src = new unsigned char[(size_t)w * h * cn]();
        to_pixels(src, type);
        resize_bilinear(src, w, h, cn, pixels, target_width, target_height);
        delete[] src;
    }
    // upstream ncnn (mat.cpp): per channel, mean only: x - mean; norm only: x * norm; both: x * norm + (-(mean * norm)).  NULL skips.
    void substract_mean_normalize(const float* mean_vals, const float* norm_vals)
    {
        const size_t size = (size_t)w * h;
        for (int q = 0; q < c; ++q)
        {
            float* p = (float*)data + cstep * q;
            if (mean_vals && norm_vals)
            {
                const float s = norm_vals[q], mb = -(mean_vals[q] * norm_vals[q]);
                for (size_t i = 0; i < size; ++i)
                {
                    const float t = p[i] * s;
                    p[i] = t + mb;
                }
            }
            else if (mean_vals)
            {
                const float mv = mean_vals[q];
                for (size_t i = 0; i < size; ++i) p[i] = p[i] - mv;
            }
            else if (norm_vals)
            {
                const float s = norm_vals[q];
                for (size_t i = 0; i < size; ++i) p[i] = p[i] * s;
            }
        }
    }

    void* data;
    int* refcount;
    size_t elemsize;
    int dims;
    int w, h, c;
    size_t cstep;

  private:
    friend void resize_bilinear_c1(const unsigned char*, int, int, unsigned char*, int, int);
    friend void resize_bilinear_c2(const unsigned char*, int, int, unsigned char*, int, int);
    friend void resize_bilinear_c3(const unsigned char*, int, int, unsigned char*, int, int);
    friend void resize_bilinear_c4(const unsigned char*, int, int, unsigned char*, int, int);
    static bool pixel_channels(int type, int& cin, int& cout)
    {
        static const int ch[9] = {0, 3, 3, 0, 1, 0, 0, 0, 4};
        const int from = type & PIXEL_FORMAT_MASK, to = (int)((unsigned)type >> PIXEL_CONVERT_SHIFT);
        if (from < 1 || from > 8 || !ch[from] || to > 8 || (to && !ch[to]) || to == PIXEL_RGBA || to == from) return false;
        cin = ch[from];
        cout = to ? ch[to] : ch[from];
        return true;
    }
    // 11-bit fixed-point coefficient of output index d along an axis of `src` pixels (resize_bilinear_c1 / c3 / c4)
    static void resize_coef(int d, int src, double scale, int& s, short& k0, short& k1)
    {
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
        k0 = sat_short(c0);
        k1 = sat_short(c1);
    }
    static short sat_short(float x)
    {
        int v = (int)(x + (x >= 0.f ? 0.5f : -0.5f));
        return (short)(v < -32768 ? -32768 : (v > 32767 ? 32767 : v));
    }
    // horizontal pass per source row ((S0*a0 + S1*a1) >> 4 as a short), then the vertical one; every channel alike
    static void resize_bilinear(const unsigned char* src, int sw, int sh, int cn, unsigned char* dst, int dw, int dh)
    {
        const double scale_x = (double)sw / dw, scale_y = (double)sh / dh;
        int* xofs = new int[dw];
        short* alpha = new short[dw * 2];
        short* rows = new short[(size_t)dw * cn * 2];
        for (int dx = 0; dx < dw; ++dx) resize_coef(dx, sw, scale_x, xofs[dx], alpha[dx * 2], alpha[dx * 2 + 1]);
        for (int dy = 0; dy < dh; ++dy)
        {
            int sy;
            short b0, b1;
            resize_coef(dy, sh, scale_y, sy, b0, b1);
            for (int r = 0; r < 2; ++r)
            {
                const unsigned char* S = src + (size_t)(sy + r) * sw * cn;
                short* row = rows + (size_t)r * dw * cn;
                for (int dx = 0; dx < dw; ++dx)
                    for (int k = 0; k < cn; ++k)
                    {
                        const unsigned char* p = S + (size_t)xofs[dx] * cn + k;
                        row[dx * cn + k] = (short)((p[0] * alpha[dx * 2] + p[cn] * alpha[dx * 2 + 1]) >> 4);
                    }
            }
            const short* r0 = rows;
            const short* r1 = rows + (size_t)dw * cn;
            unsigned char* D = dst + (size_t)dy * dw * cn;
            for (int i = 0; i < dw * cn; ++i) D[i] = (unsigned char)(((short)((b0 * r0[i]) >> 16) + (short)((b1 * r1[i]) >> 16) + 2) >> 2);
        }
        delete[] rows;
        delete[] alpha;
        delete[] xofs;
    }
    static size_t align_size(size_t sz, size_t n) { return (sz + n - 1) & ~(n - 1); }
    void alloc(int dims_, int w_, int h_, int c_, size_t elemsize_, size_t cstep_)
    {
        if (dims == dims_ && w == w_ && h == h_ && c == c_ && elemsize == elemsize_ && refcount) return;
        release();
        elemsize = elemsize_;
        dims = dims_;
        w = w_;
        h = h_;
        c = c_;
        cstep = cstep_;
        const size_t bytes = align_size(total() * elemsize, 4);
        if (!bytes) return;
        void* raw = 0;
        if (posix_memalign(&raw, 64, 64 + bytes) != 0) raw = 0;
        if (!raw)
        {
            dims = w = h = c = 0;
            cstep = 0;
            return;
        }
        refcount = (int*)raw;
        *refcount = 1;
        data = (unsigned char*)raw + 64;
    }
};

// ---- free pixel functions (reference mat.h:200-208) ----
// NV21 (yuv420sp: w*h Y bytes, then w/2 x h/2 interleaved V,U pairs) to w*h RGB bytes, the reference's C path (mat_pixel.cpp:1266-1320).
// w and h must be even, as the reference asserts.
inline void yuv420sp2rgb(const unsigned char* yuv420sp, int w, int h, unsigned char* rgb)
{
    const unsigned char* vuptr = yuv420sp + (size_t)w * h;
    for (int y = 0; y < h; y += 2)
    {
        const unsigned char* y0 = yuv420sp + (size_t)y * w;
        const unsigned char* y1 = y0 + w;
        unsigned char* rgb0 = rgb + (size_t)y * w * 3;
        unsigned char* rgb1 = rgb0 + (size_t)w * 3;
        for (int x = 0; x < w; x += 2)
        {
            const int v = vuptr[0] - 128, u = vuptr[1] - 128;
            const int d[3] = {90 * v, -46 * v + -22 * u, 113 * u};
            const int yy[4] = {y0[x] << 6, y0[x + 1] << 6, y1[x] << 6, y1[x + 1] << 6};
            unsigned char* out[4] = {rgb0 + x * 3, rgb0 + x * 3 + 3, rgb1 + x * 3, rgb1 + x * 3 + 3};
            for (int p = 0; p < 4; ++p)
                for (int k = 0; k < 3; ++k)
                {
                    const int r = (yy[p] + d[k]) >> 6;
                    out[p][k] = (unsigned char)(r < 0 ? 0 : (r > 255 ? 255 : r));
                }
            vuptr += 2;
        }
    }
}
// ncnn's fixed-point bilinear resize of 1 to 4 interleaved channels (mat_pixel_resize.cpp).  A source 1 pixel wide or high writes
// nothing (the reference reads index -1 there).
inline void resize_bilinear_c1(const unsigned char* src, int srcw, int srch, unsigned char* dst, int w, int h)
{
    if (srcw >= 2 && srch >= 2) Mat::resize_bilinear(src, srcw, srch, 1, dst, w, h);
}
inline void resize_bilinear_c2(const unsigned char* src, int srcw, int srch, unsigned char* dst, int w, int h)
{
    if (srcw >= 2 && srch >= 2) Mat::resize_bilinear(src, srcw, srch, 2, dst, w, h);
}
inline void resize_bilinear_c3(const unsigned char* src, int srcw, int srch, unsigned char* dst, int w, int h)
{
    if (srcw >= 2 && srch >= 2) Mat::resize_bilinear(src, srcw, srch, 3, dst, w, h);
}
inline void resize_bilinear_c4(const unsigned char* src, int srcw, int srch, unsigned char* dst, int w, int h)
{
    if (srcw >= 2 && srch >= 2) Mat::resize_bilinear(src, srcw, srch, 4, dst, w, h);
}
// an NV21 frame resized plane by plane (mat_pixel_resize.cpp:1174-1189): Y as c1, the VU plane as c2 at half the sizes.  All four
// sizes must be even; below 4 source pixels the VU plane is 1 pair wide or high and stays unwritten (see above).
inline void resize_bilinear_yuv420sp(const unsigned char* src, int srcw, int srch, unsigned char* dst, int w, int h)
{
    resize_bilinear_c1(src, srcw, srch, dst, w, h);
    resize_bilinear_c2(src + (size_t)srcw * srch, srcw / 2, srch / 2, dst + (size_t)w * h, w / 2, h / 2);
}

} // namespace ncnn

#endif // NCNN_MAT_H
