// tests/cpp/atrous_app_main.cpp -- a host application that runs a dilated convolution the way reference programs run ConvBooster,
// through booster::AtrousConv (include/booster/atrous.h), and a net that holds dilated Convolution layers through feather::Net after
// SetDilated(true).  It must compile against include/ unchanged and link against libfeather_hip.so and libfeather_atrous.so.
// usage: atrous_app_main model.param model.bin input.f32 n c h w input_blob output_blob out_net.f32  x.f32 w.f32 b.f32 out_layer.f32
//   the layer: 32 -> 64 channels, k3 / dilation 2 / pad 2, bias + ReLU, on x [2][32][5][8]
#include <booster/atrous.h>
#include <net.h>

#include <hip/hip_runtime_api.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

static bool load(const char* path, std::vector<float>& v)
{
    FILE* fp = fopen(path, "rb");
    if (!fp) return false;
    const size_t got = fread(&v[0], sizeof(float), v.size(), fp);
    fclose(fp);
    return got == v.size();
}

static bool save(const char* path, const std::vector<float>& v)
{
    FILE* fp = fopen(path, "wb");
    if (!fp) return false;
    fwrite(&v[0], sizeof(float), v.size(), fp);
    fclose(fp);
    return true;
}

static float* to_device(const std::vector<float>& v)
{
    float* d = NULL;
    if (hipMalloc((void**)&d, v.size() * sizeof(float)) != hipSuccess) return NULL;
    if (hipMemcpy(d, &v[0], v.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) return NULL;
    return d;
}

int main(int argc, char* argv[])
{
    if (argc < 15) return 2;
    // ---- a net with dilated layers
    const int n = atoi(argv[4]), c = atoi(argv[5]), h = atoi(argv[6]), w = atoi(argv[7]);
    std::vector<float> image((size_t)n * c * h * w);
    if (!load(argv[3], image)) return 3;
    feather::Net net;
    if (net.SetDilated(true) != 0) return 10;
    if (net.LoadParam(argv[1]) != 0 || net.LoadWeights(argv[2]) != 0) return 4;
    if (net.FeedInput(argv[8], n, c, h, w, &image[0]) != 0) return 5;
    if (net.Forward() != 0)
    {
        fprintf(stderr, "Forward: %s\n", feather::Net::LastError());
        return 6;
    }
    float* dev = NULL;
    int on = 0, oc = 0, oh = 0, ow = 0;
    if (net.Extract(std::string(argv[9]), &dev, &on, &oc, &oh, &ow) != 0) return 7;
    std::vector<float> out((size_t)on * oc * oh * ow);
    if (net.ExtractHost(std::string(argv[9]), &out[0], out.size()) != 0) return 8;
    if (!save(argv[10], out)) return 9;

    // ---- one layer through the operator interface
    booster::AtrousParam p;
    p.input_channels = 32;
    p.output_channels = 64;
    p.input_h = 5;
    p.input_w = 8;
    p.kernel_h = p.kernel_w = 3;
    p.dilation_h = p.dilation_w = 2;
    p.pad_left = p.pad_right = p.pad_top = p.pad_bottom = 2;
    p.bias_term = true;
    p.activation = booster::ReLU;
    p.batch = 2;
    if (p.AssignOutputDim() != 0 || p.output_h != 5 || p.output_w != 8) return 20;
    booster::AtrousConv conv;
    if (!conv.Supported(&p)) return 21;
    size_t buffer_bytes = 0, packed_bytes = 0;
    if (conv.GetBufferSizeBytes(&p, &buffer_bytes, &packed_bytes) != 0) return 22;
    std::vector<float> x((size_t)2 * 32 * 5 * 8), wt((size_t)64 * 32 * 9), b(64), y((size_t)2 * 64 * p.output_h * p.output_w);
    if (!load(argv[11], x) || !load(argv[12], wt) || !load(argv[13], b)) return 23;
    float *dx = to_device(x), *dw = to_device(wt), *db = to_device(b), *dy = NULL, *packed = NULL, *buffer = NULL;
    if (!dx || !dw || !db) return 24;
    if (hipMalloc((void**)&dy, y.size() * sizeof(float)) != hipSuccess || hipMalloc((void**)&packed, packed_bytes) != hipSuccess) return 25;
    if (buffer_bytes && hipMalloc((void**)&buffer, buffer_bytes) != hipSuccess) return 26;
    if (conv.Init(&p, packed, dw) != 0 || conv.Forward(&p, dy, dx, packed, buffer, db, 1) != 0)
    {
        fprintf(stderr, "AtrousConv: %s\n", booster::AtrousConv::LastError());
        return 27;
    }
    if (hipMemcpy(&y[0], dy, y.size() * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) return 28;
    if (!save(argv[14], y)) return 29;
    return 0;
}
