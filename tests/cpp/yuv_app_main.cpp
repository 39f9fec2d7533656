// tests/cpp/yuv_app_main.cpp -- an application that feeds a camera frame the way reference / ncnn programs do:
//     resize_bilinear_yuv420sp(nv21, w, h, small, tw, th);  yuv420sp2rgb(small, tw, th, rgb);
//     ncnn::Mat in = ncnn::Mat::from_pixels(rgb, ncnn::Mat::PIXEL_RGB2BGR, tw, th);  net.FeedInput("data", in);
// It must compile against include/ unchanged.  Then the same frame through feather::Net::FeedYUV420sp (the device path); both outputs
// are written for the test to compare.
// usage: yuv_app_main model.param model.bin frame.nv21 w h target_w target_h input_blob output_blob out_mat.f32 out_yuv.f32
#include <net.h>

#include <stdio.h>
#include <stdlib.h>

#include <vector>

static int run(feather::Net& net, const char* blob, const char* path)
{
    if (net.Forward() != 0) return 20;
    ncnn::Mat out;
    if (net.Extract(std::string(blob), out) != 0) return 21;
    FILE* fp = fopen(path, "wb");
    if (!fp) return 22;
    for (int q = 0; q < out.c; ++q) fwrite((const float*)out.channel(q), sizeof(float), (size_t)out.w * out.h, fp);
    fclose(fp);
    return 0;
}

int main(int argc, char* argv[])
{
    if (argc < 12) return 2;
    const int w = atoi(argv[4]), h = atoi(argv[5]), tw = atoi(argv[6]), th = atoi(argv[7]);
    std::vector<unsigned char> nv21((size_t)w * h * 3 / 2);
    FILE* fp = fopen(argv[3], "rb");
    if (!fp || fread(&nv21[0], 1, nv21.size(), fp) != nv21.size()) return 3;
    fclose(fp);
    feather::Net net;
    if (net.LoadParam(argv[1]) != 0 || net.LoadWeights(argv[2]) != 0) return 4;

    const float mean_vals[3] = {104.f, 117.f, 123.f};
    const float norm_vals[3] = {0.017f, 0.017f, 0.017f};
    std::vector<unsigned char> small((size_t)tw * th * 3 / 2), rgb((size_t)tw * th * 3);
    ncnn::resize_bilinear_yuv420sp(&nv21[0], w, h, &small[0], tw, th);
    ncnn::yuv420sp2rgb(&small[0], tw, th, &rgb[0]);
    ncnn::Mat in = ncnn::Mat::from_pixels(&rgb[0], ncnn::Mat::PIXEL_RGB2BGR, tw, th);
    in.substract_mean_normalize(mean_vals, norm_vals);
    if (net.FeedInput(argv[8], in) != 0) return 5;
    int rc = run(net, argv[9], argv[10]);
    if (rc) return rc;

    if (net.FeedYUV420sp(argv[8], &nv21[0], w, h, tw, th, ncnn::Mat::PIXEL_RGB2BGR, 1, mean_vals, norm_vals) != 0) return 6;
    rc = run(net, argv[9], argv[11]);
    if (rc) return rc;
    printf("yuv app ok %d %d\n", tw, th);
    return 0;
}
