// tests/cpp/rnn_loader_hostile_main.cpp -- plain C++ against include/feather_hip/feather_net.h: the param and weight readers of the recurrent
// layers (LSTM, GRU, RNN) on hostile files.
// usage: rnn_loader_hostile_main DIR COUNT
// DIR holds the cases 0000 .. COUNT-1 of tests/test_rnn_cpu.py as NNNN.param / NNNN.bin pairs.  Each case gets a fresh net with the
// recurrent, detection and transformer switches on: create, load_param_mem, load_weights_mem (skipped when the param load failed), destroy.
// One line per case: "case NNNN param RC weights RC|skip | first 120 characters of the last error".  No feed, forward or extract call is
// made: host side only, no GPU needed.  Exit status 0 when every case ran to its end.
#include <feather_hip/feather_hip.h>
#include <feather_hip/feather_net.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static bool read_file(const std::string& path, std::vector<char>& out)
{
    FILE* fp = fopen(path.c_str(), "rb");
    if (!fp) return false;
    fseek(fp, 0, SEEK_END);
    const long sz = ftell(fp);
    fseek(fp, 0, SEEK_SET);
    out.resize(sz > 0 ? (size_t)sz : 0);
    const size_t got = out.empty() ? 0 : fread(&out[0], 1, out.size(), fp);
    fclose(fp);
    return got == out.size();
}

int main(int argc, char** argv)
{
    if (argc < 3) return 2;
    const std::string dir = argv[1];
    const int count = atoi(argv[2]);
    int refused = 0, loaded = 0;
    for (int i = 0; i < count; ++i)
    {
        char stem[32];
        snprintf(stem, sizeof(stem), "/%04d", i);
        std::vector<char> param, weights;
        if (!read_file(dir + stem + ".param", param) || !read_file(dir + stem + ".bin", weights))
        {
            printf("case %04d missing\n", i);
            return 3;
        }
        // exact-size heap copies without a terminator: a reader that runs past either image runs into the allocator's red zone
        char* text = (char*)malloc(param.size() ? param.size() : 1);
        char* blob = (char*)malloc(weights.size() ? weights.size() : 1);
        if (!param.empty()) memcpy(text, &param[0], param.size());
        if (!weights.empty()) memcpy(blob, &weights[0], weights.size());
        fhip_net* net = NULL;
        if (fhip_net_create(&net) != 0 || !net) return 4;
        if (fhip_net_set_recurrent(net, 1) != 0 || fhip_net_set_detection(net, 1) != 0 || fhip_net_set_transformer(net, 1) != 0) return 5;
        std::string err;
        const int rp = fhip_net_load_param_mem(net, text, param.size());
        if (rp) err = fhip_last_error();
        int rw = 0;
        if (!rp)
        {
            rw = fhip_net_load_weights_mem(net, blob, weights.size());
            if (rw) err = fhip_last_error();
        }
        if (fhip_net_destroy(net) != 0) return 6;
        free(text);
        free(blob);
        for (size_t k = 0; k < err.size(); ++k)
            if ((unsigned char)err[k] < 32 || (unsigned char)err[k] > 126) err[k] = '?';
        if (rp)
            printf("case %04d param %d weights skip | %.120s\n", i, rp, err.c_str());
        else
            printf("case %04d param 0 weights %d | %.120s\n", i, rw, err.c_str());
        fflush(stdout); // a crash in a later case leaves this line behind
        refused += rp != 0 || rw != 0;
        loaded += !rp && !rw;
    }
    printf("hostile recurrent loader: %d cases, %d refused, %d loaded\n", count, refused, loaded);
    return 0;
}
