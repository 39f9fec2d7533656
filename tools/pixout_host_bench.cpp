// tools/pixout_host_bench.cpp -- host side of tools/pixout_bench.py: what an application does without ExtractPixels.
// ncnn::Mat::substract_mean_normalize + Mat::to_pixels_resize (include/ncnn/mat.h) of N extracted fp32 images [3][h][w] on T threads into
// one dense [N][th][tw][3] uint8 buffer.  usage: pixout_host_bench N w h tw th threads reps
// prints "seconds_per_batch <median> <min> <max>".
#include <ncnn/mat.h>

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <thread>
#include <vector>

int main(int argc, char* argv[])
{
    if (argc < 8) return 2;
    const int n = atoi(argv[1]), w = atoi(argv[2]), h = atoi(argv[3]), tw = atoi(argv[4]), th = atoi(argv[5]), threads = atoi(argv[6]),
              reps = atoi(argv[7]);
    const size_t plane = (size_t)w * h;
    std::vector<float> x((size_t)n * 3 * plane);
    unsigned s = 12345;
    for (size_t i = 0; i < x.size(); ++i) x[i] = (float)((s = s * 1103515245u + 12345u) >> 16) * (380.f / 65536.f) - 60.f;
    std::vector<unsigned char> out((size_t)n * tw * th * 3);
    const float mean[3] = {-1.5f, 2.25f, 0.5f}, norm[3] = {0.5f, 2.f, 1.25f};
    std::vector<double> secs;
    for (int r = 0; r < reps; ++r)
    {
        const auto t0 = std::chrono::steady_clock::now();
        std::vector<std::thread> pool;
        for (int t = 0; t < threads; ++t)
            pool.emplace_back([&, t]() {
                for (int i = t; i < n; i += threads)
                {
                    ncnn::Mat m(w, h, 3);
                    for (int q = 0; q < 3; ++q) memcpy((float*)m.channel(q), &x[((size_t)i * 3 + q) * plane], sizeof(float) * plane);
                    m.substract_mean_normalize(mean, norm);
                    m.to_pixels_resize(&out[(size_t)i * tw * th * 3], ncnn::Mat::PIXEL_RGB2BGR, tw, th);
                }
            });
        for (auto& p : pool) p.join();
        secs.push_back(std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    }
    std::sort(secs.begin(), secs.end());
    printf("seconds_per_batch %.6f %.6f %.6f\n", secs[secs.size() / 2], secs.front(), secs.back());
    return 0;
}
