// tests/cpp/gate_app_main.cpp -- a host application that runs a net with squeeze-and-excitation blocks through feather::Net the way
// reference programs run a net, and one SE block (squeeze, excite, channel gate with a residual and ReLU) through the C-ABI of
// libfeather_gate.so (include/feather_hip/feather_gate.h).  It must compile against include/ unchanged and link against
// libfeather_hip.so and libfeather_gate.so.
// usage: gate_app_main model.param model.bin input.f32 n c h w input_blob output_blob out_net.f32  x.f32 res.f32 w1.f32 b1.f32 w2.f32 b2.f32 out_block.f32
//   the block: x and res [2][8][6][6], reduction to 3, ReLU between the dense layers, Sigmoid gate
#include <feather_hip/feather_gate.h>
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
    if (argc < 18) return 2;
    // ---- a net with SE blocks, at the fusion level that collapses them
    const int n = atoi(argv[4]), c = atoi(argv[5]), h = atoi(argv[6]), w = atoi(argv[7]);
    std::vector<float> image((size_t)n * c * h * w);
    if (!load(argv[3], image)) return 3;
    feather::Net net;
    if (net.SetFusion(2) != 0) return 10;
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

    // ---- one block through the C-ABI
    const int N = 2, C = 8, R = 3, H = 6, W = 6;
    std::vector<float> x((size_t)N * C * H * W), res(x.size()), w1((size_t)R * C), b1(R), w2((size_t)C * R), b2(C), y(x.size());
    if (!load(argv[11], x) || !load(argv[12], res) || !load(argv[13], w1) || !load(argv[14], b1) || !load(argv[15], w2) || !load(argv[16], b2)) return 23;
    float *dx = to_device(x), *dres = to_device(res), *dw1 = to_device(w1), *db1 = to_device(b1), *dw2 = to_device(w2), *db2 = to_device(b2);
    float *dy = NULL, *mean = NULL, *gate = NULL, *scratch = NULL;
    if (!dx || !dres || !dw1 || !db1 || !dw2 || !db2) return 24;
    size_t scratch_bytes = 0;
    if (fhip_squeeze_get_buffer_size(N, C, H, W, &scratch_bytes) != 0) return 22;
    if (hipMalloc((void**)&dy, y.size() * sizeof(float)) != hipSuccess || hipMalloc((void**)&mean, N * C * sizeof(float)) != hipSuccess ||
        hipMalloc((void**)&gate, N * C * sizeof(float)) != hipSuccess)
        return 25;
    if (scratch_bytes && hipMalloc((void**)&scratch, scratch_bytes) != hipSuccess) return 26;
    if (fhip_squeeze_forward(N, C, H, W, mean, dx, scratch, NULL) != 0 ||
        fhip_excite_forward(N, C, R, gate, mean, dw1, db1, dw2, db2, FHIP_EXCITE_MACT_RELU, FHIP_EXCITE_GACT_SIGMOID, 0.f, 0.f, NULL) != 0 ||
        fhip_channel_gate_forward(N, C, H, W, dy, dx, gate, dres, FHIP_GATE_ACT_RELU, NULL) != 0)
    {
        fprintf(stderr, "gate: %s\n", fhip_gate_last_error());
        return 27;
    }
    if (hipMemcpy(&y[0], dy, y.size() * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) return 28;
    if (!save(argv[17], y)) return 29;
    return 0;
}
