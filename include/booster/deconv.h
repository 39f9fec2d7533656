// booster/deconv.h -- C++ host mirror of the transposed-convolution route (feather_hip/feather_deconv.h, libfeather_deconv.so): ncnn's
// Deconvolution / DeconvolutionDepthWise, a layer the reference does not have.  Header-only over the C-ABI, used the way ConvBooster is:
//
//     booster::DeconvParam p;              // ConvParam's fields (input_* is the SMALL tensor) + output_pad_right / output_pad_bottom
//     p.input_channels = 128; p.output_channels = 64; p.input_h = p.input_w = 32; p.kernel_h = p.kernel_w = 4; ...
//     p.AssignOutputDim();
//     booster::Deconv deconv;
//     if (!deconv.Supported(&p)) ...
//     deconv.GetBufferSizeBytes(&p, &buffer_bytes, &processed_kernel_bytes);
//     deconv.Init(&p, processed_kernel, kernel);                                  // kernel [K][C/group][kh][kw], not flipped
//     deconv.Forward(&p, output, input, processed_kernel, buffer, bias, 1);
//
// Every pointer is a DEVICE pointer; Init / Forward run on booster::GetStream() (booster.h), allocate nothing and can be captured into a
// hipGraph.  Link with -lfeather_deconv next to -lfeather_hip.
#pragma once

#include <stddef.h>

#include "booster/booster.h"
#include "feather_hip/feather_deconv.h"

namespace booster
{

struct DeconvParam
{
    int output_channels, input_channels, input_h, input_w, kernel_h, kernel_w, output_h, output_w, stride_h, stride_w;
    int pad_left, pad_bottom, pad_right, pad_top, group;
    bool bias_term;
    ActivationType activation;
    int output_pad_right, output_pad_bottom;
    int batch; // 0 / 1: one image
    DeconvParam()
        : output_channels(0), input_channels(0), input_h(0), input_w(0), kernel_h(0), kernel_w(0), output_h(0), output_w(0), stride_h(1), stride_w(1),
          pad_left(0), pad_bottom(0), pad_right(0), pad_top(0), group(1), bias_term(false), activation(None), output_pad_right(0), output_pad_bottom(0),
          batch(1)
    {
    }
    fhip_deconv_param ToC() const
    {
        fhip_deconv_param c;
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
        c.output_pad_right = output_pad_right;
        c.output_pad_bottom = output_pad_bottom;
        return c;
    }
    int AssignOutputDim()
    {
        fhip_deconv_param c = ToC();
        const int rc = fhip_deconv_assign_output_dim(&c);
        if (rc) return rc;
        output_h = c.output_h;
        output_w = c.output_w;
        return 0;
    }
};

class Deconv
{
public:
    static int Batch(const DeconvParam* p) { return p->batch > 0 ? p->batch : 1; }

    bool Supported(const DeconvParam* param) const
    {
        const fhip_deconv_param c = param->ToC();
        return fhip_deconv_supported(&c) == 1;
    }
    int GetBufferSizeBytes(DeconvParam* param, size_t* buffer_bytes, size_t* processed_kernel_bytes) const
    {
        const fhip_deconv_param c = param->ToC();
        return fhip_deconv_get_buffer_size(&c, Batch(param), buffer_bytes, processed_kernel_bytes);
    }
    // float counts as the reference's GET_BUFFER_SIZE_FUNC reports them
    int GetBufferSize(DeconvParam* param, int* buffer_size, int* processed_kernel_size) const
    {
        size_t b = 0, k = 0;
        const int rc = GetBufferSizeBytes(param, &b, &k);
        if (rc) return rc;
        if (b / sizeof(float) > 0x7fffffffu || k / sizeof(float) > 0x7fffffffu) return -1;
        *buffer_size = (int)(b / sizeof(float));
        *processed_kernel_size = (int)(k / sizeof(float));
        return 0;
    }
    int Init(DeconvParam* param, float* processed_kernel, float* kernel) const
    {
        const fhip_deconv_param c = param->ToC();
        return fhip_deconv_init(&c, processed_kernel, kernel, GetStream());
    }
    int Forward(DeconvParam* param, float* output, float* input, float* processed_kernel, float* buffer, float* bias_arr, int /*num_threads*/) const
    {
        const fhip_deconv_param c = param->ToC();
        return fhip_deconv_forward(&c, Batch(param), output, input, processed_kernel, buffer, bias_arr, GetStream());
    }
    static const char* LastError() { return fhip_deconv_last_error(); }
};

} // namespace booster
