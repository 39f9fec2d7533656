// booster/q8.h -- C++ host mirror of the int8 route on q8 tensors (feather_hip/feather_q8.h, libfeather_q8.so): a convolution with int8
// weights whose input, output or both are int8 tensors signed char [n][ceil(C/16)][h][w][16], and the layers between two of them.
// Header-only over the C-ABI, used the way booster::QuantConv (booster/qconv.h) is:
//
//     booster::Q8Param p;                  // QuantParam's fields, + input_int8 / output_int8 (both true by default)
//     p.input_channels = 256; p.output_channels = 256; p.input_h = p.input_w = 56; p.kernel_h = p.kernel_w = 3; ...
//     p.AssignOutputDim();
//     booster::Q8Conv conv;
//     if (!conv.Supported(&p)) ...         // fp32 in AND out is booster::QuantConv's layer
//     conv.GetBufferSizeBytes(&p, &buffer_bytes, &processed_kernel_bytes);
//     booster::Q8Conv::DequantScales(d_host, weight_scales_host, p.output_channels, input_scale);   // host; upload d_host yourself
//     conv.Init(&p, processed_kernel, kernel);                                    // kernel: signed char [K][C/group][kh][kw]
//     conv.Forward(&p, output, input, processed_kernel, buffer, dequant, bias, input_scale, output_scale, 1);
//
// Every pointer but DequantScales' is a DEVICE pointer; every call runs on booster::GetStream() (booster.h), allocates nothing and can be
// captured into a hipGraph.  Link with -lfeather_q8 next to -lfeather_hip.
#pragma once

#include <stddef.h>

#include "booster/booster.h"
#include "feather_hip/feather_q8.h"

namespace booster
{

struct Q8Param
{
    int output_channels, input_channels, input_h, input_w, kernel_h, kernel_w, output_h, output_w, stride_h, stride_w;
    int pad_left, pad_bottom, pad_right, pad_top, group;
    bool bias_term;
    ActivationType activation;
    int int8_scale_term;           // the model's value, 1 .. 200
    bool input_int8, output_int8;  // the form of the input and of the output: a q8 tensor, else dense NCHW fp32
    int batch;                     // 0 / 1: one image
    Q8Param()
        : output_channels(0), input_channels(0), input_h(0), input_w(0), kernel_h(0), kernel_w(0), output_h(0), output_w(0), stride_h(1), stride_w(1),
          pad_left(0), pad_bottom(0), pad_right(0), pad_top(0), group(1), bias_term(false), activation(None), int8_scale_term(101), input_int8(true), output_int8(true), batch(1)
    {
    }
    fhip_q8_param ToC() const
    {
        fhip_q8_param c;
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
        c.input_int8 = input_int8 ? 1 : 0;
        c.output_int8 = output_int8 ? 1 : 0;
        return c;
    }
    int AssignOutputDim()
    {
        fhip_q8_param c = ToC();
        const int rc = fhip_q8_assign_output_dim(&c);
        if (rc) return rc;
        output_h = c.output_h;
        output_w = c.output_w;
        return 0;
    }
};

class Q8Conv
{
public:
    static int Batch(const Q8Param* p) { return p->batch > 0 ? p->batch : 1; }

    bool Supported(const Q8Param* param) const
    {
        const fhip_q8_param c = param->ToC();
        return fhip_q8_supported(&c) == 1;
    }
    int GetBufferSizeBytes(Q8Param* param, size_t* buffer_bytes, size_t* processed_kernel_bytes) const
    {
        const fhip_q8_param c = param->ToC();
        return fhip_q8_get_buffer_size(&c, Batch(param), buffer_bytes, processed_kernel_bytes);
    }
    // byte counts: the packed weights are int8
    int GetBufferSize(Q8Param* param, int* buffer_size, int* processed_kernel_size) const
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
        return fhip_q8_dequant_scales(d, weight_scales, channels, input_scale);
    }
    int Init(Q8Param* param, void* processed_kernel, const signed char* kernel) const
    {
        const fhip_q8_param c = param->ToC();
        return fhip_q8_init(&c, processed_kernel, kernel, GetStream());
    }
    // output / input: float NCHW or a q8 tensor, as the param says; input_scale is read with an fp32 input, output_scale with an int8 output
    int Forward(Q8Param* param, void* output, const void* input, const void* processed_kernel, void* buffer, const float* dequant, const float* bias_arr,
                float input_scale, float output_scale, int /*num_threads*/) const
    {
        const fhip_q8_param c = param->ToC();
        return fhip_q8_forward(&c, Batch(param), output, input, processed_kernel, buffer, dequant, bias_arr, input_scale, output_scale, GetStream());
    }
    // bytes of the q8 tensor of [batch][channels][h][w]
    static int TensorBytes(int batch, int channels, int h, int w, size_t* bytes) { return fhip_q8_tensor_bytes(batch, channels, h, w, bytes); }
    // fp32 NCHW <-> q8 tensor, ReLU and max pooling on a q8 tensor (feather_q8.h)
    static int Quantize(void* out, const float* in, int batch, int channels, int h, int w, float scale) { return fhip_q8_quantize_forward(out, in, batch, channels, h, w, scale, GetStream()); }
    static int Dequantize(float* out, const void* in, int batch, int channels, int h, int w, float scale) { return fhip_q8_dequantize_forward(out, in, batch, channels, h, w, scale, GetStream()); }
    static int Relu(void* out, const void* in, size_t bytes) { return fhip_q8_relu_forward(out, in, bytes, GetStream()); }
    static int MaxPool(const fhip_pool_param* pool, int batch, void* out, const void* in) { return fhip_q8_max_pool_forward(pool, batch, out, in, GetStream()); }
    static const char* LastError() { return fhip_q8_last_error(); }
};

} // namespace booster
