// booster/atrous.h -- C++ host mirror of the dilated-convolution route (feather_hip/feather_atrous.h, libfeather_atrous.so): a convolution
// with dilation > 1, which the reference's ConvParam cannot express.  Header-only over the C-ABI, used the way ConvBooster is:
//
//     booster::AtrousParam p;              // ConvParam's fields (channels of the WHOLE layer) + dilation_h / dilation_w
//     p.input_channels = 512; p.output_channels = 1024; p.input_h = p.input_w = 41; p.kernel_h = p.kernel_w = 3; p.dilation_h = p.dilation_w = 12; ...
//     p.AssignOutputDim();
//     booster::AtrousConv conv;
//     if (!conv.Supported(&p)) ...
//     conv.GetBufferSizeBytes(&p, &buffer_bytes, &processed_kernel_bytes);
//     conv.Init(&p, processed_kernel, kernel);                                    // kernel [K][C/group][kh][kw]
//     conv.Forward(&p, output, input, processed_kernel, buffer, bias, 1);
//
// Every pointer is a DEVICE pointer; Init / Forward run on booster::GetStream() (booster.h), allocate nothing and can be captured into a
// hipGraph.  Link with -lfeather_atrous next to -lfeather_hip.
#pragma once

#include <stddef.h>

#include "booster/booster.h"
#include "feather_hip/feather_atrous.h"

namespace booster
{

struct AtrousParam
{
    int output_channels, input_channels, input_h, input_w, kernel_h, kernel_w, output_h, output_w, stride_h, stride_w;
    int pad_left, pad_bottom, pad_right, pad_top, group;
    bool bias_term;
    ActivationType activation;
    int dilation_h, dilation_w;
    int batch; // 0 / 1: one image
    AtrousParam()
        : output_channels(0), input_channels(0), input_h(0), input_w(0), kernel_h(0), kernel_w(0), output_h(0), output_w(0), stride_h(1), stride_w(1),
          pad_left(0), pad_bottom(0), pad_right(0), pad_top(0), group(1), bias_term(false), activation(None), dilation_h(1), dilation_w(1),
          batch(1)
    {
    }
    fhip_atrous_param ToC() const
    {
        fhip_atrous_param c;
        c.output_channels = output_channels;
        c.input_channels = input_channels;
        c.input_h = input_h;
        c.input_w = input_w;
        c.kernel_h = kernel_h;
        c.kernel_w = kernel_w;
        c.output_h = output_h;
        c.output_w = output_w;
        c.stride_h = stride_h;
        c.stride_w = stride_w;
        c.pad_left = pad_left;
        c.pad_bottom = pad_bottom;
        c.pad_right = pad_right;
        c.pad_top = pad_top;
        c.group = group;
        c.bias_term = bias_term ? 1 : 0;
        c.activation = (int)activation;
        c.dilation_h = dilation_h;
        c.dilation_w = dilation_w;
        return c;
    }
    int AssignOutputDim()
    {
        fhip_atrous_param c = ToC();
        const int rc = fhip_atrous_assign_output_dim(&c);
        if (rc) return rc;
        output_h = c.output_h;
        output_w = c.output_w;
        return 0;
    }
};

class AtrousConv
{
public:
    static int Batch(const AtrousParam* p) { return p->batch > 0 ? p->batch : 1; }

    bool Supported(const AtrousParam* param) const
    {
        const fhip_atrous_param c = param->ToC();
        return fhip_atrous_supported(&c) == 1;
    }
    int GetBufferSizeBytes(AtrousParam* param, size_t* buffer_bytes, size_t* processed_kernel_bytes) const
    {
        const fhip_atrous_param c = param->ToC();
        return fhip_atrous_get_buffer_size(&c, Batch(param), buffer_bytes, processed_kernel_bytes);
    }
    // float counts as the reference's GET_BUFFER_SIZE_FUNC reports them
    int GetBufferSize(AtrousParam* param, int* buffer_size, int* processed_kernel_size) const
    {
        size_t b = 0, k = 0;
        const int rc = GetBufferSizeBytes(param, &b, &k);
        if (rc) return rc;
        if (b / sizeof(float) > 0x7fffffffu || k / sizeof(float) > 0x7fffffffu) return -1;
        *buffer_size = (int)(b / sizeof(float));
        *processed_kernel_size = (int)(k / sizeof(float));
        return 0;
    }
    int Init(AtrousParam* param, float* processed_kernel, float* kernel) const
    {
        const fhip_atrous_param c = param->ToC();
        return fhip_atrous_init(&c, processed_kernel, kernel, GetStream());
    }
    int Forward(AtrousParam* param, float* output, float* input, float* processed_kernel, float* buffer, float* bias_arr, int /*num_threads*/) const
    {
        const fhip_atrous_param c = param->ToC();
        return fhip_atrous_forward(&c, Batch(param), output, input, processed_kernel, buffer, bias_arr, GetStream());
    }
    static const char* LastError() { return fhip_atrous_last_error(); }
};

} // namespace booster
