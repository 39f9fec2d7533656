// tests/cpp/yuv_mat_main.cpp -- include/ncnn/mat.h's NV21 and pixel helpers with plain g++ (tests/test_yuv_cpu.py); the stdin protocol of
// tests/golden/make_yuv_golden.py's driver, so both produce the same bytes:
//   C type w h tw th resize_first + w*h*3/2 bytes  -> cout*th*tw bytes (the whole-number values of the fp32 Mat)
//   R2 sw sh dw dh + sw*sh*2 bytes                 -> dw*dh*2 bytes of resize_bilinear_c2
//   RY sw sh dw dh + sw*sh*3/2 bytes               -> dw*dh*3/2 bytes of resize_bilinear_yuv420sp
//   P type w h c tw th + c*h*w floats              -> th*tw*cn bytes of to_pixels_resize (to_pixels at equal size)
#include <ncnn/mat.h>

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

static std::vector<unsigned char> in(size_t n)
{
    std::vector<unsigned char> p(n);
    if (fread(&p[0], 1, n, stdin) != n) exit(2);
    return p;
}

int main()
{
    char tag[4];
    while (scanf("%3s", tag) == 1)
    {
        if (!strcmp(tag, "C"))
        {
            int type, w, h, tw, th, rf;
            if (scanf("%d %d %d %d %d %d", &type, &w, &h, &tw, &th, &rf) != 6) return 3;
            getchar();
            std::vector<unsigned char> yuv = in((size_t)w * h * 3 / 2);
            ncnn::Mat m;
            if (rf)
            {
                std::vector<unsigned char> r((size_t)tw * th * 3 / 2), rgb((size_t)tw * th * 3);
                ncnn::resize_bilinear_yuv420sp(&yuv[0], w, h, &r[0], tw, th);
                ncnn::yuv420sp2rgb(&r[0], tw, th, &rgb[0]);
                m = ncnn::Mat::from_pixels(&rgb[0], type, tw, th);
            }
            else
            {
                std::vector<unsigned char> rgb((size_t)w * h * 3);
                ncnn::yuv420sp2rgb(&yuv[0], w, h, &rgb[0]);
                m = ncnn::Mat::from_pixels_resize(&rgb[0], type, w, h, tw, th);
            }
            if (m.w != tw || m.h != th) return 4;
            for (int q = 0; q < m.c; ++q)
            {
                const float* p = m.channel(q);
                for (int i = 0; i < tw * th; ++i)
                {
                    if (p[i] < 0.f || p[i] > 255.f || p[i] != (float)(int)p[i]) return 5;
                    putchar((int)p[i]);
                }
            }
        }
        else if (!strcmp(tag, "R2") || !strcmp(tag, "RY"))
        {
            int sw, sh, dw, dh;
            if (scanf("%d %d %d %d", &sw, &sh, &dw, &dh) != 4) return 6;
            getchar();
            const bool c2 = tag[1] == '2';
            std::vector<unsigned char> src = in(c2 ? (size_t)sw * sh * 2 : (size_t)sw * sh * 3 / 2);
            std::vector<unsigned char> dst(c2 ? (size_t)dw * dh * 2 : (size_t)dw * dh * 3 / 2);
            if (c2)
                ncnn::resize_bilinear_c2(&src[0], sw, sh, &dst[0], dw, dh);
            else
                ncnn::resize_bilinear_yuv420sp(&src[0], sw, sh, &dst[0], dw, dh);
            fwrite(&dst[0], 1, dst.size(), stdout);
        }
        else if (!strcmp(tag, "P"))
        {
            int type, w, h, c, tw, th;
            if (scanf("%d %d %d %d %d %d", &type, &w, &h, &c, &tw, &th) != 6) return 7;
            getchar();
            ncnn::Mat m(w, h, c);
            for (int q = 0; q < c; ++q)
                if (fread((float*)m.channel(q), sizeof(float), (size_t)w * h, stdin) != (size_t)w * h) return 8;
            std::vector<unsigned char> dst((size_t)tw * th * c);
            m.to_pixels_resize(&dst[0], type, tw, th);
            fwrite(&dst[0], 1, dst.size(), stdout);
        }
        else
            return 9;
    }
    // c1 / c3 / c4 are the resize from_pixels_resize runs: each equals it on a 3x2 -> 5x4 image
    unsigned char px[3 * 2 * 4];
    for (int i = 0; i < 24; ++i) px[i] = (unsigned char)(i * 37 + 11);
    const int types[3] = {ncnn::Mat::PIXEL_GRAY, ncnn::Mat::PIXEL_RGB, ncnn::Mat::PIXEL_RGBA};
    for (int t = 0; t < 3; ++t)
    {
        const int cn = t == 0 ? 1 : (t == 1 ? 3 : 4);
        unsigned char out[5 * 4 * 4];
        if (cn == 1) ncnn::resize_bilinear_c1(px, 3, 2, out, 5, 4);
        if (cn == 3) ncnn::resize_bilinear_c3(px, 3, 2, out, 5, 4);
        if (cn == 4) ncnn::resize_bilinear_c4(px, 3, 2, out, 5, 4);
        ncnn::Mat m = ncnn::Mat::from_pixels_resize(px, types[t], 3, 2, 5, 4);
        for (int q = 0; q < cn; ++q)
            for (int i = 0; i < 20; ++i)
                if (((const float*)m.channel(q))[i] != (float)out[i * cn + q]) return 10;
    }
    return 0;
}
