// tests/cpp/pixel_mat_main.cpp -- include/ncnn/mat.h's pixel entry points with plain g++ (tests/test_pixels_cpu.py).
// stdin, repeated: "type w h target_w target_h cin form\n" then w*h*cin bytes; form 0: no mean / norm, 1: mean, 2: norm, 3: both
// (the values below).  stdout: per case the cout*target_h*target_w floats of Mat::from_pixels_resize (+ substract_mean_normalize),
// channel after channel, raw.
#include <ncnn/mat.h>

#include <stdio.h>
#include <stdlib.h>

int main()
{
    static const float mean[4] = {104.f, 116.67f, 122.68f, 0.5f}, norm[4] = {0.017f, 1.f / 58.8f, 0.0175f, -2.f};
    int type, w, h, tw, th, cin, form;
    while (scanf("%d %d %d %d %d %d %d", &type, &w, &h, &tw, &th, &cin, &form) == 7)
    {
        getchar();
        unsigned char* px = (unsigned char*)malloc((size_t)w * h * cin);
        if (fread(px, 1, (size_t)w * h * cin, stdin) != (size_t)w * h * cin) return 2;
        ncnn::Mat m = ncnn::Mat::from_pixels_resize(px, type, w, h, tw, th);
        if (m.empty() || m.w != tw || m.h != th || m.dims != 3) return 3;
        m.substract_mean_normalize(form & 1 ? mean : NULL, form & 2 ? norm : NULL);
        for (int q = 0; q < m.c; ++q) fwrite((const float*)m.channel(q), sizeof(float), (size_t)tw * th, stdout);
        free(px);
    }
    // a 1-pixel source axis that must be resized is refused (empty Mat), an unknown type too
    unsigned char one[12] = {0};
    if (!ncnn::Mat::from_pixels_resize(one, ncnn::Mat::PIXEL_RGB, 1, 4, 3, 3).empty()) return 4;
    if (!ncnn::Mat::from_pixels_resize(one, ncnn::Mat::PIXEL_RGB, 4, 1, 3, 3).empty()) return 5;
    if (ncnn::Mat::from_pixels_resize(one, ncnn::Mat::PIXEL_RGB, 1, 4, 1, 4).empty()) return 6; // no resize: fine
    if (!ncnn::Mat::from_pixels(one, ncnn::Mat::PIXEL_RGB | (ncnn::Mat::PIXEL_RGBA << 16), 2, 2).empty()) return 7;
    return 0;
}
