// The host side of booster::Q8Conv (include/booster/q8.h) from a plain C++11 application: the param, the output size, what the library takes
// and what it leaves to booster::QuantConv, the packed size and the q8 tensor's size.  No device call: tests/test_q8_contract_cpu.py
// compiles and runs it without a GPU.
#include <stdio.h>

#include "booster/q8.h"

#define CHECK(cond)                                             \
    do                                                          \
    {                                                           \
        if (!(cond))                                            \
        {                                                       \
            fprintf(stderr, "line %d: %s\n", __LINE__, #cond);  \
            return 1;                                           \
        }                                                       \
    } while (0)

int main()
{
    booster::Q8Param p;
    p.input_channels = 24;
    p.output_channels = 20;
    p.input_h = 7;
    p.input_w = 5;
    p.kernel_h = p.kernel_w = 3;
    p.pad_left = p.pad_right = p.pad_top = p.pad_bottom = 1;
    p.bias_term = true;
    p.batch = 3;
    CHECK(p.AssignOutputDim() == 0 && p.output_h == 7 && p.output_w == 5);
    booster::Q8Conv conv;
    CHECK(conv.Supported(&p)); // int8 in, int8 out: any C
    size_t buffer = 1, packed = 0;
    CHECK(conv.GetBufferSizeBytes(&p, &buffer, &packed) == 0 && buffer == 0 && packed % 16 == 0 && packed >= 20 * 24 * 9);
    p.output_int8 = false;
    CHECK(conv.Supported(&p));
    p.input_int8 = false; // fp32 in and out is booster::QuantConv's layer
    CHECK(!conv.Supported(&p) && booster::Q8Conv::LastError()[0] != 0);
    size_t bytes = 0;
    CHECK(booster::Q8Conv::TensorBytes(3, 24, 7, 5, &bytes) == 0 && bytes == 3 * 2 * 7 * 5 * 16);
    float d[2], s_w[2] = {0.f, 4.f};
    CHECK(booster::Q8Conv::DequantScales(d, s_w, 2, 0.5f) == 0 && d[0] == 0.f && d[1] == 0.5f);
    printf("q8 app ok\n");
    return 0;
}
