// tests/cpp/pixout_app_main.cpp -- an application whose net produces an image, written the way reference / ncnn programs show one:
//     ncnn::Mat out;  net.Extract("blob", out);  out.substract_mean_normalize(mean, norm);  out.to_pixels_resize(bgr, PIXEL_RGB2BGR, tw, th);
// It must compile against include/ unchanged.  Then the same blob through feather::Net::ExtractPixels (the device path, host and device
// destination); all three results are written for the test to compare.
// usage: pixout_app_main model.param model.bin image.u8 w h target_w target_h input_blob output_blob out_mat.u8 out_host.u8 out_device.u8
//        mean0 mean1 mean2 norm0 norm1 norm2   (of the output, as C99 hex floats)
#include <net.h>

#include <hip/hip_runtime_api.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

static int save(const char* path, const std::vector<unsigned char>& px)
{
    FILE* fp = fopen(path, "wb");
    if (!fp) return 30;
    fwrite(&px[0], 1, px.size(), fp);
    fclose(fp);
    return 0;
}

int main(int argc, char* argv[])
{
    if (argc < 19) return 2;
    const int w = atoi(argv[4]), h = atoi(argv[5]), tw = atoi(argv[6]), th = atoi(argv[7]);
    std::vector<unsigned char> rgb((size_t)w * h * 3);
    FILE* fp = fopen(argv[3], "rb");
    if (!fp || fread(&rgb[0], 1, rgb.size(), fp) != rgb.size()) return 3;
    fclose(fp);
    feather::Net net;
    if (net.LoadParam(argv[1]) != 0 || net.LoadWeights(argv[2]) != 0) return 4;
    const float in_mean[3] = {104.f, 117.f, 123.f}, in_norm[3] = {0.017f, 0.017f, 0.017f};
    if (net.FeedPixels(argv[8], &rgb[0], ncnn::Mat::PIXEL_RGB, w, h, w, h, in_mean, in_norm) != 0) return 5;
    if (net.Forward() != 0) return 6;

    // back into 0..255 (and beyond: the clamps are part of the conversion)
    float out_mean[3], out_norm[3];
    for (int q = 0; q < 3; ++q)
    {
        out_mean[q] = strtof(argv[13 + q], NULL);
        out_norm[q] = strtof(argv[16 + q], NULL);
    }
    std::vector<unsigned char> a((size_t)tw * th * 3), b(a.size()), c(a.size());
    ncnn::Mat out;
    if (net.Extract(std::string(argv[9]), out) != 0) return 7;
    if (out.c != 3) return 8;
    out.substract_mean_normalize(out_mean, out_norm);
    out.to_pixels_resize(&a[0], ncnn::Mat::PIXEL_RGB2BGR, tw, th);

    int n = 0;
    if (net.ExtractPixels(std::string(argv[9]), &n, &b[0], ncnn::Mat::PIXEL_RGB2BGR, tw, th, out_mean, out_norm) != 0 || n != 1)
    {
        fprintf(stderr, "ExtractPixels: %s / %s\n", feather::Net::LastError(), feather::Net::LastPixelError());
        return 9;
    }
    unsigned char* dev = NULL;
    if (hipMalloc((void**)&dev, c.size()) != hipSuccess) return 10;
    if (net.ExtractPixelsDevice(std::string(argv[9]), &n, dev, ncnn::Mat::PIXEL_RGB2BGR, tw, th, out_mean, out_norm) != 0) return 11;
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(&c[0], dev, c.size(), hipMemcpyDeviceToHost) != hipSuccess) return 12;
    hipFree(dev);
    // a type Mat::to_pixels writes nothing for, and a type whose channels are not the blob's, are refused
    if (net.ExtractPixels(std::string(argv[9]), &n, &b[0], ncnn::Mat::PIXEL_RGB2GRAY, tw, th) != FHIP_E_BADARG) return 13;
    if (net.ExtractPixels(std::string(argv[9]), &n, &b[0], ncnn::Mat::PIXEL_RGBA, tw, th) != FHIP_E_BADARG) return 14;
    if (save(argv[10], a) || save(argv[11], b) || save(argv[12], c)) return 30;
    printf("pixout app ok %d %d\n", tw, th);
    return 0;
}
