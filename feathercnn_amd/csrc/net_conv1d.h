// net_conv1d.h -- the layers of a net with fhip_net_set_conv1d (Net::conv1d): ncnn's Convolution1D, ConvolutionDepthWise1D and Pooling1D.
// include/feather_hip/feather_conv1d.h defines them, libfeather_conv1d.so holds them (conv1d_api); the layers report the route
// FHIP_CONV1D_NET_ROUTE.  A 1-D blob is a blob of rank 2, [n][1][C][L] (Blob::dims, which fhip_net_set_detection maintains: the switch
// needs it); the rank-3 blob [1][C][L] an Input yields is taken for one.  Nothing fuses into these layers: the convolutions have ncnn's
// built-in activation.  A default net never creates one of these classes.
#pragma once
#include "feather_hip/feather_conv1d.h" // declarations only: the library is opened at run time (conv1d_api)
#include "net_rnn.h"

namespace fhip::net
{

// libfeather_conv1d.so, the layers of a net with fhip_net_set_conv1d
struct Conv1dApi
{
    decltype(&fhip_conv1d_output_dim) conv_output_dim = nullptr;
    decltype(&fhip_conv1d_forward) conv_forward = nullptr;
    decltype(&fhip_pool1d_output_dim) pool_output_dim = nullptr;
    decltype(&fhip_pool1d_forward) pool_forward = nullptr;
    decltype(&fhip_conv1d_last_error) last_error = nullptr;
    SideLibrary library()
    {
        return {"libfeather_conv1d.so", "a 1-D layer (Convolution1D, ConvolutionDepthWise1D, Pooling1D)", "feather_conv1d.h",
                {{&conv_output_dim, "fhip_conv1d_output_dim"}, {&conv_forward, "fhip_conv1d_forward"}, {&pool_output_dim, "fhip_pool1d_output_dim"},
                 {&pool_forward, "fhip_pool1d_forward"}, {&last_error, "fhip_conv1d_last_error"}}};
    }
};
static const Conv1dApi* conv1d_api() { return side_api<Conv1dApi>(); }

// the bottom of a 1-D layer: rank 2 [C][L], or the rank-3 [1][C][L] of an Input
static int conv1d_bottom(const Layer* l, const Blob* b)
{
    if (b->dims == 2 || (b->dims == 3 && b->c == 1)) return 0;
    return failf(NET_E_SHAPE, "layer %s: %s needs a blob of rank 2 [C][L], blob %s has rank %d and (%d, %d, %d)", l->name.c_str(), l->type.c_str(), b->name.c_str(), b->dims, b->c,
                 b->h, b->w);
}

// ncnn's Convolution1D (0=num_output 1=kernel_w 2=dilation_w 3=stride_w 4=pad_left 15=pad_right 18=pad_value 5=bias_term 6=weight_data_size
// 9=activation_type 10=activation_params 19=dynamic_weight) and ConvolutionDepthWise1D (the same and 7=group); weights tagged
// [num_output][C / group][kernel_w], then the raw bias.
struct Conv1dLayer : Layer
{
    int K = 0, kw = 0, d = 1, s = 1, pl = 0, pr = 0, bias_term = 0, group = 1, act = 0, Cg = 0;
    int left = 0, right = 0; // the pads resolved at Reshape
    long long wsize = 0;
    float pad_value = 0.f, a0 = 0.f, a1 = 0.f;
    std::vector<float> w, bias;
    DeviceVec d_w, d_bias;
    bool built = false;
    int algo() const override { return FHIP_CONV1D_NET_ROUTE; }
    bool needs_weights() const override { return true; }
    int LoadParam(const ParamDict& pd) override
    {
        const char *ln = name.c_str(), *ty = type.c_str();
        if (bottoms.size() != 1 || tops.size() != 1) return failf(NET_E_SHAPE, "layer %s: %s needs 1 bottom and 1 top, got %zu and %zu", ln, ty, bottoms.size(), tops.size());
        K = pd.get(0, 0), kw = pd.get(1, 0), d = pd.get(2, 1), s = pd.get(3, 1), pl = pd.get(4, 0), pr = pd.get(15, pl), pad_value = pd.get(18, 0.f);
        bias_term = pd.get(5, 0), wsize = pd.get(6, 0), act = pd.get(9, 0);
        group = type == "ConvolutionDepthWise1D" ? pd.get(7, 1) : 1;
        if (pd.get(19, 0) != 0) return failf(NET_E_SHAPE, "layer %s: %s with dynamic_weight (19=%d) is not supported", ln, ty, pd.get(19, 0));
        if (pd.get(8, 0) != 0) return failf(NET_E_SHAPE, "layer %s: %s with int8 weights (8=%d) is not supported", ln, ty, pd.get(8, 0));
        if (K < 1) return failf(NET_E_SHAPE, "layer %s: %s num_output (0=%d) must be positive", ln, ty, K);
        if (kw < 1) return failf(NET_E_SHAPE, "layer %s: %s kernel_w (1=%d) must be positive", ln, ty, kw);
        if (d < 1) return failf(NET_E_SHAPE, "layer %s: %s dilation_w (2=%d) must be positive", ln, ty, d);
        if (s < 1) return failf(NET_E_SHAPE, "layer %s: %s stride_w (3=%d) must be positive", ln, ty, s);
        if (pl < 0 && pl != FHIP_CONV1D_SAME_UPPER && pl != FHIP_CONV1D_SAME_LOWER)
            return failf(NET_E_SHAPE, "layer %s: %s pad_left (4=%d) must be >= 0, -233 (SAME_UPPER) or -234 (SAME_LOWER)", ln, ty, pl);
        if (pl >= 0 && pr < 0) return failf(NET_E_SHAPE, "layer %s: %s pad_right (15=%d) must be >= 0", ln, ty, pr);
        if (group < 1 || K % group) return failf(NET_E_SHAPE, "layer %s: %s group (7=%d) must divide num_output (0=%d)", ln, ty, group, K);
        if (act < 0 || act > 6) return failf(NET_E_SHAPE, "layer %s: %s activation_type (9=%d) must be 0 .. 6", ln, ty, act);
        const long long per = (long long)(K / group) * kw; // weights per input channel: < 2^62
        if (per >= (1ll << 31) || wsize >= (1ll << 31)) return failf(NET_E_SHAPE, "layer %s: %s weight_data_size (6=%lld): tensors of 2^31 elements or more are not supported", ln, ty, wsize);
        if (wsize < 1 || wsize % per || (wsize / per) % group)
            return failf(NET_E_SHAPE, "layer %s: %s weight_data_size (6=%lld) must be num_output / group * C * kernel_w for input channels C that group divides", ln, ty, wsize);
        Cg = (int)(wsize / per / group);
        if (pd.has_array(10))
        {
            const std::vector<float>& v = pd.e[10].array;
            a0 = v[0], a1 = v.size() > 1 ? v[1] : 0.f;
        }
        return 0;
    }
    int LoadWeights(ModelBin& mb) override
    {
        built = false;
        int rc = mb.load((size_t)wsize, 0, w);
        if (!rc && bias_term) rc = mb.load((size_t)K, 1, bias);
        return rc;
    }
    int Reshape() override
    {
        const Conv1dApi* api = conv1d_api();
        if (!api) return FHIP_E_UNSUPPORTED; // message set by conv1d_api
        const Blob* b = bottoms[0];
        if (const int rc = conv1d_bottom(this, b)) return rc;
        if (b->h != Cg * group)
            return failf(NET_E_SHAPE, "layer %s: %s has weights for %d input channels, blob %s has %d", name.c_str(), type.c_str(), Cg * group, b->name.c_str(), b->h);
        int lo = 0;
        if (api->conv_output_dim(b->w, kw, d, s, pl, pr, &left, &right, &lo))
            return failf(NET_E_SHAPE, "layer %s: %s of blob %s, a row of %d: %s", name.c_str(), type.c_str(), b->name.c_str(), b->w, api->last_error());
        if (b->count() >= ((size_t)1 << 31) || (long long)b->n * K * lo >= (1ll << 31))
            return failf(NET_E_SHAPE, "layer %s: %s: tensors of 2^31 elements or more are not supported", name.c_str(), type.c_str());
        const int rc = tops[0]->reshape(b->n, 1, K, lo);
        tops[0]->dims = 2;
        return rc;
    }
    int Init(hipStream_t st) override
    {
        if (built) return 0;
        int rc = d_w.upload(w.data(), w.size(), st);
        if (!rc && bias_term) rc = d_bias.upload(bias.data(), bias.size(), st);
        if (rc) return rc;
        FHIP_CHECK_HIP(hipStreamSynchronize(st));
        built = true;
        return 0;
    }
    int Forward(hipStream_t st) override
    {
        const Blob *b = bottoms[0], *t = tops[0];
        return side(conv1d_api(), [&](const Conv1dApi* api) {
            return api->conv_forward(b->n, b->h, b->w, K, kw, d, s, left, right, pad_value, group, act, a0, a1, b->data, b->w, d_w.d, bias_term ? d_bias.d : nullptr, t->data,
                                     t->w, t->w, st);
        });
    }
    size_t weight_bytes() const override { return d_w.bytes + d_bias.bytes; }
};

// ncnn's Pooling1D: 0=pooling_type 1=kernel_w 2=stride_w 3=pad_left 14=pad_right 4=global_pooling 5=pad_mode 6=avgpool_count_include_pad
// 7=adaptive_pooling 8=out_w.  Global pooling writes ncnn's blob of rank 1, [n][1][1][C].
struct Pool1dLayer : Layer
{
    int type_ = 0, kw = 0, s = 1, pl = 0, pr = 0, global = 0, pad_mode = 0, include_pad = 0, adaptive = 0, out_w = 0;
    int left = 0, right = 0, lo = 0;
    int algo() const override { return FHIP_CONV1D_NET_ROUTE; }
    int LoadParam(const ParamDict& pd) override
    {
        const char* ln = name.c_str();
        if (bottoms.size() != 1 || tops.size() != 1) return failf(NET_E_SHAPE, "layer %s: Pooling1D needs 1 bottom and 1 top, got %zu and %zu", ln, bottoms.size(), tops.size());
        type_ = pd.get(0, 0), kw = pd.get(1, 0), s = pd.get(2, 1), pl = pd.get(3, 0), pr = pd.get(14, pl), global = pd.get(4, 0), pad_mode = pd.get(5, 0);
        include_pad = pd.get(6, 0), adaptive = pd.get(7, 0), out_w = pd.get(8, 0);
        if (type_ < 0 || type_ > 1) return failf(NET_E_SHAPE, "layer %s: Pooling1D pooling_type (0=%d) must be 0 (max) or 1 (average)", ln, type_);
        if (global) return 0;
        if (adaptive) return out_w < 1 ? failf(NET_E_SHAPE, "layer %s: Pooling1D out_w (8=%d) must be positive", ln, out_w) : 0;
        if (kw < 1) return failf(NET_E_SHAPE, "layer %s: Pooling1D kernel_w (1=%d) must be positive", ln, kw);
        if (s < 1) return failf(NET_E_SHAPE, "layer %s: Pooling1D stride_w (2=%d) must be positive", ln, s);
        if (pl < 0 || pr < 0) return failf(NET_E_SHAPE, "layer %s: Pooling1D pads (3=%d 14=%d) must be >= 0", ln, pl, pr);
        if (pad_mode < 0 || pad_mode > 3) return failf(NET_E_SHAPE, "layer %s: Pooling1D pad_mode (5=%d) must be 0 .. 3", ln, pad_mode);
        return 0;
    }
    int Reshape() override
    {
        const Conv1dApi* api = conv1d_api();
        if (!api) return FHIP_E_UNSUPPORTED; // message set by conv1d_api
        const Blob* b = bottoms[0];
        if (const int rc = conv1d_bottom(this, b)) return rc;
        if (b->count() >= ((size_t)1 << 31)) return failf(NET_E_SHAPE, "layer %s: Pooling1D: tensors of 2^31 elements or more are not supported", name.c_str());
        left = right = 0;
        if (global) lo = 1;
        else if (adaptive) lo = out_w;
        else if (api->pool_output_dim(b->w, kw, s, pl, pr, pad_mode, &left, &right, &lo))
            return failf(NET_E_SHAPE, "layer %s: Pooling1D of blob %s, a row of %d: %s", name.c_str(), b->name.c_str(), b->w, api->last_error());
        if ((long long)b->n * b->h * lo >= (1ll << 31)) return failf(NET_E_SHAPE, "layer %s: Pooling1D: tensors of 2^31 elements or more are not supported", name.c_str());
        const int rc = global ? tops[0]->reshape(b->n, 1, 1, b->h) : tops[0]->reshape(b->n, 1, b->h, lo);
        tops[0]->dims = global ? 1 : 2;
        return rc;
    }
    int Forward(hipStream_t st) override
    {
        const Blob* b = bottoms[0];
        return side(conv1d_api(), [&](const Conv1dApi* api) {
            return api->pool_forward(type_, b->n * b->h, b->w, global || adaptive ? 0 : kw, s, left, right, include_pad, b->data, b->w, tops[0]->data, lo, lo, st);
        });
    }
};

// The layer types of a net with fhip_net_set_conv1d (Net::conv1d).
static Layer* create_conv1d_layer(const std::string& type)
{
    if (type == "Convolution1D" || type == "ConvolutionDepthWise1D") return new Conv1dLayer;
    if (type == "Pooling1D") return new Pool1dLayer;
    return nullptr;
}

} // namespace fhip::net
