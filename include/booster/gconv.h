// booster/gconv.h -- C++ host mirror of the grouped-convolution route (feather_hip/feather_gconv.h, libfeather_gconv.so): a layer with
// 1 < group < input_channels, which booster::ConvBooster::SelectAlgo refuses with -1 exactly as the reference does.  Header-only over the
// C-ABI, used the way ConvBooster is:
//
//     booster::ConvParam p = ...;          // output_channels / input_channels of the WHOLE layer, group in between
//     p.AssignOutputDim();
//     booster::GroupedConv gconv;
//     if (!gconv.Supported(&p)) ...        // group == 1 and group == C go through ConvBooster
//     gconv.GetBufferSizeBytes(&p, &buffer_bytes, &processed_kernel_bytes);
//     gconv.Init(&p, processed_kernel, kernel);                                   // kernel [K][C/group][kh][kw]
//     gconv.Forward(&p, output, input, processed_kernel, buffer, bias, 1);
//
// Every pointer is a DEVICE pointer; Init / Forward run on booster::GetStream() (booster.h), allocate nothing and can be captured into a
// hipGraph.  Link with -lfeather_gconv next to -lfeather_hip.
#pragma once

#include <stddef.h>

#include "booster/booster.h"
#include "feather_hip/feather_gconv.h"

namespace booster
{

class GroupedConv
{
public:
    static fhip_conv_param ToC(const ConvParam* p)
    {
        fhip_conv_param c;
        c.output_channels = p->output_channels;
        c.input_channels = p->input_channels;
        c.input_h = p->input_h;
        c.input_w = p->input_w;
        c.kernel_h = p->kernel_h;
        c.kernel_w = p->kernel_w;
        c.output_h = p->output_h;
        c.output_w = p->output_w;
        c.stride_h = p->stride_h;
        c.stride_w = p->stride_w;
        c.pad_left = p->pad_left;
        c.pad_bottom = p->pad_bottom;
        c.pad_right = p->pad_right;
        c.pad_top = p->pad_top;
        c.group = p->group;
        c.bias_term = p->bias_term ? 1 : 0;
        c.activation = (int)p->activation;
        return c;
    }
    static int Batch(const ConvParam* p) { return p->batch > 0 ? p->batch : 1; }

    bool Supported(const ConvParam* param) const
    {
        const fhip_conv_param c = ToC(param);
        return fhip_gconv_supported(&c) == 1;
    }
    int GetBufferSizeBytes(ConvParam* param, size_t* buffer_bytes, size_t* processed_kernel_bytes) const
    {
        const fhip_conv_param c = ToC(param);
        return fhip_gconv_get_buffer_size(&c, Batch(param), buffer_bytes, processed_kernel_bytes);
    }
    // float counts as the reference's GET_BUFFER_SIZE_FUNC reports them
    int GetBufferSize(ConvParam* param, int* buffer_size, int* processed_kernel_size) const
    {
        size_t b = 0, k = 0;
        const int rc = GetBufferSizeBytes(param, &b, &k);
        if (rc) return rc;
        if (b / sizeof(float) > 0x7fffffffu || k / sizeof(float) > 0x7fffffffu) return -1;
        *buffer_size = (int)(b / sizeof(float));
        *processed_kernel_size = (int)(k / sizeof(float));
        return 0;
    }
    int Init(ConvParam* param, float* processed_kernel, float* kernel) const
    {
        const fhip_conv_param c = ToC(param);
        return fhip_gconv_init(&c, processed_kernel, kernel, GetStream());
    }
    int Forward(ConvParam* param, float* output, float* input, float* processed_kernel, float* buffer, float* bias_arr, int /*num_threads*/) const
    {
        const fhip_conv_param c = ToC(param);
        return fhip_gconv_forward(&c, Batch(param), output, input, processed_kernel, buffer, bias_arr, GetStream());
    }
    static const char* LastError() { return fhip_gconv_last_error(); }
};

} // namespace booster
