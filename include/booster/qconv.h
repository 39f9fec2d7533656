// booster/qconv.h -- C++ host mirror of the int8 convolution route (feather_hip/feather_qconv.h, libfeather_qconv.so): a convolution with
// int8 weights and fp32 input and output, which the reference refuses.  Header-only over the C-ABI, used the way ConvBooster is:
//
//     booster::QuantParam p;               // ConvParam's fields (channels of the WHOLE layer); group is 1 or depthwise
//     p.input_channels = 256; p.output_channels = 256; p.input_h = p.input_w = 56; p.kernel_h = p.kernel_w = 3; ...
//     p.AssignOutputDim();
//     booster::QuantConv conv;
//     if (!conv.Supported(&p)) ...
//     conv.GetBufferSizeBytes(&p, &buffer_bytes, &processed_kernel_bytes);
//     booster::QuantConv::DequantScales(d_host, weight_scales_host, p.output_channels, input_scale);   // host; upload d_host yourself
//     conv.Init(&p, processed_kernel, kernel);                                    // kernel: signed char [K][C/group][kh][kw]
//     conv.Forward(&p, output, input, processed_kernel, buffer, dequant, bias, input_scale, 1);
//
// Every pointer but DequantScales' is a DEVICE pointer; Init / Forward run on booster::GetStream() (booster.h), allocate nothing and can
// be captured into a hipGraph.  Link with -lfeather_qconv next to -lfeather_hip.
#pragma once

#include <stddef.h>

#include "booster/booster.h"
#include "feather_hip/feather_qconv.h"

namespace booster
{

struct QuantParam
{
    int output_channels, input_channels, input_h, input_w, kernel_h, kernel_w, output_h, output_w, stride_h, stride_w;
    int pad_left, pad_bottom, pad_right, pad_top, group;
    bool bias_term;
    ActivationType activation;
    int int8_scale_term; // the model's value, 1 .. 100
    int batch;           // 0 / 1: one image
    QuantParam()
        : output_channels(0), input_channels(0), input_h(0), input_w(0), kernel_h(0), kernel_w(0), output_h(0), output_w(0), stride_h(1), stride_w(1),
          pad_left(0), pad_bottom(0), pad_right(0), pad_top(0), group(1), bias_term(false), activation(None), int8_scale_term(1), batch(1)
    {
    }
    fhip_qconv_param ToC() const
    {
        fhip_qconv_param c;
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
        c.dilation_h = c.dilation_w = 1;
        c.int8_scale_term = int8_scale_term;
        return c;
    }
    int AssignOutputDim()
    {
        fhip_qconv_param c = ToC();
        const int rc = fhip_qconv_assign_output_dim(&c);
        if (rc) return rc;
        output_h = c.output_h;
        output_w = c.output_w;
        return 0;
    }
};

class QuantConv
{
public:
    static int Batch(const QuantParam* p) { return p->batch > 0 ? p->batch : 1; }

    bool Supported(const QuantParam* param) const
    {
        const fhip_qconv_param c = param->ToC();
        return fhip_qconv_supported(&c) == 1;
    }
    int GetBufferSizeBytes(QuantParam* param, size_t* buffer_bytes, size_t* processed_kernel_bytes) const
    {
        const fhip_qconv_param c = param->ToC();
        return fhip_qconv_get_buffer_size(&c, Batch(param), buffer_bytes, processed_kernel_bytes);
    }
    // byte counts: the packed weights are int8
    int GetBufferSize(QuantParam* param, int* buffer_size, int* processed_kernel_size) const
    {
        size_t b = 0, k = 0;
        const int rc = GetBufferSizeBytes(param, &b, &k);
        if (rc) return rc;
        if (b > 0x7fffffffu || k > 0x7fffffffu) return -1;
        *buffer_size = (int)b;
        *processed_kernel_size = (int)k;
        return 0;
    }
    // d[k] = 1 / (input_scale * weight_scales[k]) on the host, as feather_qconv.h defines it
    static int DequantScales(float* d, const float* weight_scales, int channels, float input_scale)
    {
        return fhip_qconv_dequant_scales(d, weight_scales, channels, input_scale);
    }
    int Init(QuantParam* param, void* processed_kernel, const signed char* kernel) const
    {
        const fhip_qconv_param c = param->ToC();
        return fhip_qconv_init(&c, processed_kernel, kernel, GetStream());
    }
    int Forward(QuantParam* param, float* output, float* input, const void* processed_kernel, float* buffer, const float* dequant, const float* bias_arr,
                float input_scale, int /*num_threads*/) const
    {
        const fhip_qconv_param c = param->ToC();
        return fhip_qconv_forward(&c, Batch(param), output, input, processed_kernel, buffer, dequant, bias_arr, input_scale, GetStream());
    }
    static const char* LastError() { return fhip_qconv_last_error(); }
};

} // namespace booster
