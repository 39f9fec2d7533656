// tools/yuv_host_bench.cpp -- host side of tools/yuv_bench.py: what an application does without FeedYUV420sp.
// ncnn::yuv420sp2rgb + Mat::from_pixels_resize(PIXEL_RGB2BGR) + substract_mean_normalize (include/ncnn/mat.h) of N NV21 frames on T
// threads, written into one dense [N][3][th][tw] fp32 buffer (what FeedInput uploads).  usage: yuv_host_bench N w h tw th threads reps
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
    if (argc < 8) return 2;
    const int n = atoi(argv[1]), w = atoi(argv[2]), h = atoi(argv[3]), tw = atoi(argv[4]), th = atoi(argv[5]), threads = atoi(argv[6]),
              reps = atoi(argv[7]);
    const size_t frame = (size_t)w * h * 3 / 2;
    std::vector<unsigned char> yuv(frame * n);
    unsigned s = 12345;
    for (size_t i = 0; i < yuv.size(); ++i) yuv[i] = (unsigned char)((s = s * 1103515245u + 12345u) >> 16);
    std::vector<float> out((size_t)n * 3 * tw * th);
    const float mean[3] = {104.f, 117.f, 123.f}, norm[3] = {0.017f, 0.017f, 0.017f};
    double best = 1e30;
    for (int r = 0; r < reps; ++r)
    {
        const auto t0 = std::chrono::steady_clock::now();
        std::vector<std::thread> pool;
        for (int t = 0; t < threads; ++t)
            pool.emplace_back([&, t]() {
                std::vector<unsigned char> rgb((size_t)w * h * 3);
                for (int i = t; i < n; i += threads)
                {
                    ncnn::yuv420sp2rgb(&yuv[frame * i], w, h, &rgb[0]);
                    ncnn::Mat m = ncnn::Mat::from_pixels_resize(&rgb[0], ncnn::Mat::PIXEL_RGB2BGR, w, h, tw, th);
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
