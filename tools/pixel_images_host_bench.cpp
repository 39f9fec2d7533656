// tools/pixel_images_host_bench.cpp -- host side of tools/pixel_images_bench.py: what an application does today for a mixed-size batch
// with crops, without FeedPixelImages.  N images cycling through the sizes given, each cropped to its centre square (a dense copy of the
// crop), then ncnn::Mat::from_pixels_resize + substract_mean_normalize (include/ncnn/mat.h) on T threads into one dense
// [N][3][th][tw] fp32 buffer (what FeedInput uploads).  usage: pixel_images_host_bench N tw th threads reps w1xh1 [w2xh2 ...]
// prints "seconds_per_batch <s>" (best of reps).
#include <ncnn/mat.h>

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <chrono>
#include <thread>
#include <vector>

int main(int argc, char* argv[])
{
    if (argc < 7) return 2;
    const int n = atoi(argv[1]), tw = atoi(argv[2]), th = atoi(argv[3]), threads = atoi(argv[4]), reps = atoi(argv[5]);
    std::vector<int> ws, hs;
    for (int a = 6; a < argc; ++a)
    {
        int w = 0, h = 0;
        if (sscanf(argv[a], "%dx%d", &w, &h) != 2) return 2;
        ws.push_back(w);
        hs.push_back(h);
    }
    std::vector<std::vector<unsigned char> > images(ws.size());
    unsigned s = 12345;
    for (size_t k = 0; k < ws.size(); ++k)
    {
        images[k].resize((size_t)ws[k] * hs[k] * 3);
        for (size_t i = 0; i < images[k].size(); ++i) images[k][i] = (unsigned char)((s = s * 1103515245u + 12345u) >> 16);
    }
    std::vector<float> out((size_t)n * 3 * tw * th);
    const float mean[3] = {104.f, 117.f, 123.f}, norm[3] = {0.017f, 0.017f, 0.017f};
    double best = 1e30;
    for (int r = 0; r < reps; ++r)
    {
        const auto t0 = std::chrono::steady_clock::now();
        std::vector<std::thread> pool;
        for (int t = 0; t < threads; ++t)
            pool.emplace_back([&, t]() {
                std::vector<unsigned char> crop;
                for (int i = t; i < n; i += threads)
                {
                    const int k = i % (int)ws.size(), w = ws[k], h = hs[k], side = w < h ? w : h, x0 = (w - side) / 2, y0 = (h - side) / 2;
                    crop.resize((size_t)side * side * 3);
                    for (int y = 0; y < side; ++y) memcpy(&crop[(size_t)y * side * 3], &images[k][((size_t)(y0 + y) * w + x0) * 3], (size_t)side * 3);
                    ncnn::Mat m = ncnn::Mat::from_pixels_resize(&crop[0], ncnn::Mat::PIXEL_BGR2RGB, side, side, tw, th);
                    m.substract_mean_normalize(mean, norm);
                    for (int q = 0; q < 3; ++q)
                        memcpy(&out[((size_t)i * 3 + q) * tw * th], (const float*)m.channel(q), sizeof(float) * tw * th);
                }
            });
        for (auto& p : pool) p.join();
        const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (sec < best) best = sec;
    }
    printf("seconds_per_batch %.6f\n", best);
    return 0;
}
