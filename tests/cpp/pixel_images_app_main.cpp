// tests/cpp/pixel_images_app_main.cpp -- an application that feeds a mixed-size batch with ROIs: each image's ROI copied dense on the
// host, ncnn::Mat::from_pixels_resize + substract_mean_normalize of it, the batch through feather::Net::FeedInput; then the same
// descriptors through feather::Net::FeedPixelImages (the device path).  Both outputs are written for the test to compare.
// usage: pixel_images_app_main model.param model.bin images.u8 target_w target_h input_blob output_blob out_mat.f32 out_images.f32
//        [then one line per image on stdin: w h stride roi_x roi_y roi_w roi_h; images.u8 holds the images back to back, h * stride bytes each]
#include <net.h>

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

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
    if (argc < 10) return 2;
    const int tw = atoi(argv[4]), th = atoi(argv[5]);
    std::vector<fhip_pixel_image> images;
    std::vector<size_t> offsets;
    size_t total = 0;
    fhip_pixel_image im;
    memset(&im, 0, sizeof im);
    while (scanf("%d %d %d %d %d %d %d", &im.w, &im.h, &im.stride, &im.roi_x, &im.roi_y, &im.roi_w, &im.roi_h) == 7)
    {
        images.push_back(im);
        offsets.push_back(total);
        total += (size_t)im.h * im.stride;
    }
    if (images.empty()) return 3;
    std::vector<unsigned char> bytes(total);
    FILE* fp = fopen(argv[3], "rb");
    if (!fp || fread(&bytes[0], 1, total, fp) != total) return 3;
    fclose(fp);
    for (size_t i = 0; i < images.size(); ++i) images[i].data = &bytes[offsets[i]];
    feather::Net net;
    if (net.LoadParam(argv[1]) != 0 || net.LoadWeights(argv[2]) != 0) return 4;

    const float mean_vals[3] = {104.f, 117.f, 123.f};
    const float norm_vals[3] = {0.017f, 0.017f, 0.017f};
    const int n = (int)images.size();
    std::vector<float> batch((size_t)n * 3 * th * tw);
    for (int i = 0; i < n; ++i)
    {
        const fhip_pixel_image& m = images[i];
        std::vector<unsigned char> roi((size_t)m.roi_w * m.roi_h * 3);
        for (int y = 0; y < m.roi_h; ++y)
            memcpy(&roi[(size_t)y * m.roi_w * 3], m.data + (size_t)(m.roi_y + y) * m.stride + (size_t)m.roi_x * 3, (size_t)m.roi_w * 3);
        ncnn::Mat in = ncnn::Mat::from_pixels_resize(&roi[0], ncnn::Mat::PIXEL_BGR2RGB, m.roi_w, m.roi_h, tw, th);
        in.substract_mean_normalize(mean_vals, norm_vals);
        for (int q = 0; q < 3; ++q) memcpy(&batch[((size_t)i * 3 + q) * th * tw], (const float*)in.channel(q), sizeof(float) * th * tw);
    }
    if (net.FeedInput(argv[6], n, 3, th, tw, &batch[0]) != 0) return 5;
    int rc = run(net, argv[7], argv[8]);
    if (rc) return rc;

    if (net.FeedPixelImages(argv[6], n, &images[0], ncnn::Mat::PIXEL_BGR2RGB, tw, th, mean_vals, norm_vals) != 0) return 6;
    rc = run(net, argv[7], argv[9]);
    if (rc) return rc;
    printf("pixel images app ok %d %d %d\n", n, tw, th);
    return 0;
}
