// tests/cpp/resample_app_main.cpp -- a host application that runs a net with Interp and HardSwish layers through feather::Net after
// SetExtendedLayers(true), and one up-sample-add-ReLU through the C-ABI of libfeather_resample.so (include/feather_hip/feather_resample.h).
// It must compile against include/ unchanged and link against libfeather_hip.so and libfeather_resample.so.
// usage: resample_app_main model.param model.bin input.f32 n c h w input_blob output_blob out_net.f32  x.f32 residual.f32 out_layer.f32
//   the layer: x [2][3][5][6] -> nearest x2 -> + residual [2][3][10][12] -> ReLU
#include <feather_hip/feather_resample.h>
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
    if (argc < 14) return 2;
    // ---- a net with Interp and HardSwish layers
    const int n = atoi(argv[4]), c = atoi(argv[5]), h = atoi(argv[6]), w = atoi(argv[7]);
    std::vector<float> image((size_t)n * c * h * w);
    if (!load(argv[3], image)) return 3;
    feather::Net net;
    if (net.SetFusion(2) != 0 || net.SetExtendedLayers(true) != 0) return 10;
    if (net.LoadParam(argv[1]) != 0 || net.LoadWeights(argv[2]) != 0)
    {
        fprintf(stderr, "Load: %s\n", feather::Net::LastError());
        return 4;
    }
    if (net.SetExtendedLayers(false) == 0) return 11; // the switch is refused once a param file is loaded
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

    // ---- one fused layer through the C-ABI
    int out_h = 0, out_w = 0;
    if (fhip_interp_output_dim(5, 6, 2.f, 2.f, 0, 0, &out_h, &out_w) != 0 || out_h != 10 || out_w != 12) return 20;
    std::vector<float> x((size_t)2 * 3 * 5 * 6), r((size_t)2 * 3 * out_h * out_w), y(r.size());
    if (!load(argv[11], x) || !load(argv[12], r)) return 21;
    float *dx = to_device(x), *dr = to_device(r), *dy = NULL;
    if (!dx || !dr || hipMalloc((void**)&dy, y.size() * sizeof(float)) != hipSuccess) return 22;
    char route[96];
    if (fhip_interp_route(FHIP_INTERP_NEAREST, 2, 3, 5, 6, out_h, out_w, 2.f, 2.f, dy, dx, dr, route, sizeof(route)) != 0) return 23;
    if (strcmp(route, "fhip::interp_nearest2x_kernel") != 0) return 24;
    if (fhip_interp_forward(FHIP_INTERP_NEAREST, 0, 2, 3, 5, 6, out_h, out_w, 2.f, 2.f, dy, dx, dr, 1, NULL) != 0)
    {
        fprintf(stderr, "fhip_interp_forward: %s\n", fhip_resample_last_error());
        return 25;
    }
    if (hipDeviceSynchronize() != hipSuccess) return 26;
    if (hipMemcpy(&y[0], dy, y.size() * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) return 27;
    if (!save(argv[13], y)) return 28;
    return 0;
}
