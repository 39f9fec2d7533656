// net_conv3d.h -- the layers of a net with fhip_net_set_conv3d (Net::conv3d): ncnn's Convolution3D, ConvolutionDepthWise3D and Pooling3D.
// include/feather_hip/feather_conv3d.h defines them, libfeather_conv3d.so holds them (conv3d_api); the layers report the route
// FHIP_CONV3D_NET_ROUTE.  A volume is a blob of rank 4, [n][C][D][H][W] (Blob::d, Blob::dims == 4); fhip_net_feed_volume makes one of an
// Input.  Nothing fuses into or out of these layers: the convolutions have ncnn's built-in activation.  A default net never creates one of
// these classes.
#pragma once
#include "feather_hip/feather_conv3d.h" // declarations only: the library is opened at run time (conv3d_api)
#include "net_dcn.h"

namespace fhip::net
{

// libfeather_conv3d.so, the layers of a net with fhip_net_set_conv3d
struct Conv3dApi
{
    decltype(&fhip_conv3d_output_dim) conv_output_dim = nullptr;
    decltype(&fhip_conv3d_packed_floats) packed_floats = nullptr;
    decltype(&fhip_conv3d_pack_weights) pack_weights = nullptr;
    decltype(&fhip_conv3d_forward) conv_forward = nullptr;
    decltype(&fhip_pool3d_output_dim) pool_output_dim = nullptr;
    decltype(&fhip_pool3d_forward) pool_forward = nullptr;
    decltype(&fhip_conv3d_last_error) last_error = nullptr;
    SideLibrary library()
    {
        return {"libfeather_conv3d.so", "a 3-D layer (Convolution3D, ConvolutionDepthWise3D, Pooling3D)", "feather_conv3d.h",
                {{&conv_output_dim, "fhip_conv3d_output_dim"}, {&packed_floats, "fhip_conv3d_packed_floats"}, {&pack_weights, "fhip_conv3d_pack_weights"},
                 {&conv_forward, "fhip_conv3d_forward"}, {&pool_output_dim, "fhip_pool3d_output_dim"}, {&pool_forward, "fhip_pool3d_forward"},
                 {&last_error, "fhip_conv3d_last_error"}}};
    }
};
static const Conv3dApi* conv3d_api() { return side_api<Conv3dApi>(); }

// n * c * d * h * w, or 2^31 for anything at or past it
static long long volume_elements(int n, int c, int d, int h, int w)
{
    long long v = 1;
    for (const int e : {n, c, d, h, w}) v = v >= (1ll << 31) || e < 1 ? (1ll << 31) : v * e;
    return std::min(v, 1ll << 31);
}

static int conv3d_bottom(const Layer* l, const Blob* b)
{
    if (b->dims == 4) return 0;
    return failf(NET_E_SHAPE, "layer %s: %s needs a volume, a blob of rank 4 [C][D][H][W] (fhip_net_feed_volume), blob %s has rank %d and (%d, %d, %d)", l->name.c_str(),
                 l->type.c_str(), b->name.c_str(), b->dims, b->c, b->h, b->w);
}

// ncnn's Convolution3D (0=num_output 1/11/21=kernel w/h/d 2/12/22=dilation 3/13/23=stride 4/15=pad left/right 14/16=pad top/bottom
// 24/17=pad front/behind 18=pad_value 5=bias_term 6=weight_data_size 9=activation_type 10=activation_params 19=dynamic_weight) and
// ConvolutionDepthWise3D (the same and 7=group); an id of h or d that is absent takes the value of its w counterpart.  Weights tagged
// [num_output][C / group][kd][kh][kw], then the raw bias.
struct Conv3dLayer : Layer
{
    int K = 0, k[3] = {0, 0, 0}, dil[3] = {1, 1, 1}, s[3] = {1, 1, 1}, lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0}; // axes: depth, row, column
    int bias_term = 0, group = 1, act = 0, Cg = 0;
    int rlo[3] = {0, 0, 0}, rhi[3] = {0, 0, 0}, out[3] = {0, 0, 0}; // the pads resolved and the output volume, at Reshape
    long long wsize = 0, packed_floats = 0;
    float pad_value = 0.f, a0 = 0.f, a1 = 0.f;
    std::vector<float> w, bias;
    DeviceVec d_w, d_bias, d_packed;
    bool built = false;
    int algo() const override { return FHIP_CONV3D_NET_ROUTE; }
    bool needs_weights() const override { return true; }
    bool reads_volume() const override { return true; }
    int LoadParam(const ParamDict& pd) override
    {
        const char *ln = name.c_str(), *ty = type.c_str();
        if (bottoms.size() != 1 || tops.size() != 1) return failf(NET_E_SHAPE, "layer %s: %s needs 1 bottom and 1 top, got %zu and %zu", ln, ty, bottoms.size(), tops.size());
        K = pd.get(0, 0);
        k[2] = pd.get(1, 0), k[1] = pd.get(11, k[2]), k[0] = pd.get(21, k[2]);
        dil[2] = pd.get(2, 1), dil[1] = pd.get(12, dil[2]), dil[0] = pd.get(22, dil[2]);
        s[2] = pd.get(3, 1), s[1] = pd.get(13, s[2]), s[0] = pd.get(23, s[2]);
        lo[2] = pd.get(4, 0), hi[2] = pd.get(15, lo[2]), lo[1] = pd.get(14, lo[2]), hi[1] = pd.get(16, lo[1]), lo[0] = pd.get(24, lo[2]), hi[0] = pd.get(17, lo[0]);
        pad_value = pd.get(18, 0.f), bias_term = pd.get(5, 0), wsize = pd.get(6, 0), act = pd.get(9, 0);
        group = type == "ConvolutionDepthWise3D" ? pd.get(7, 1) : 1;
        if (pd.get(19, 0) != 0) return failf(NET_E_SHAPE, "layer %s: %s with dynamic_weight (19=%d) is not supported", ln, ty, pd.get(19, 0));
        if (pd.get(8, 0) != 0) return failf(NET_E_SHAPE, "layer %s: %s with int8 weights (8=%d) is not supported", ln, ty, pd.get(8, 0));
        if (K < 1) return failf(NET_E_SHAPE, "layer %s: %s num_output (0=%d) must be positive", ln, ty, K);
        static const int kid[3] = {21, 11, 1}, did[3] = {22, 12, 2}, sid[3] = {23, 13, 3}, loid[3] = {24, 14, 4}, hiid[3] = {17, 16, 15};
        const bool same = lo[2] == FHIP_CONV3D_SAME_UPPER || lo[2] == FHIP_CONV3D_SAME_LOWER; // on every axis, as ncnn's pad_left says it
        for (int i = 0; i < 3; ++i)
        {
            if (k[i] < 1) return failf(NET_E_SHAPE, "layer %s: %s kernel extent (%d=%d) must be positive", ln, ty, kid[i], k[i]);
            if (dil[i] < 1) return failf(NET_E_SHAPE, "layer %s: %s dilation (%d=%d) must be positive", ln, ty, did[i], dil[i]);
            if (s[i] < 1) return failf(NET_E_SHAPE, "layer %s: %s stride (%d=%d) must be positive", ln, ty, sid[i], s[i]);
            if (same) lo[i] = lo[2], hi[i] = 0;
            else if (lo[i] < 0) return failf(NET_E_SHAPE, "layer %s: %s pad (%d=%d) must be >= 0, or pad_left -233 (SAME_UPPER) or -234 (SAME_LOWER)", ln, ty, loid[i], lo[i]);
            else if (hi[i] < 0) return failf(NET_E_SHAPE, "layer %s: %s pad (%d=%d) must be >= 0", ln, ty, hiid[i], hi[i]);
        }
        if (group < 1 || K % group) return failf(NET_E_SHAPE, "layer %s: %s group (7=%d) must divide num_output (0=%d)", ln, ty, group, K);
        if (act < 0 || act > 6) return failf(NET_E_SHAPE, "layer %s: %s activation_type (9=%d) must be 0 .. 6", ln, ty, act);
        const long long taps = (long long)k[0] * k[1]; // < 2^62
        if (taps >= (1ll << 31) || taps * k[2] >= (1ll << 31) || taps * k[2] * (K / group) >= (1ll << 31) || wsize >= (1ll << 31))
            return failf(NET_E_SHAPE, "layer %s: %s weight_data_size (6=%lld): tensors of 2^31 elements or more are not supported", ln, ty, wsize);
        const long long per = taps * k[2] * (K / group); // weights per input channel
        if (wsize < 1 || wsize % per || (wsize / per) % group)
            return failf(NET_E_SHAPE, "layer %s: %s weight_data_size (6=%lld) must be num_output / group * C * kernel_d * kernel_h * kernel_w for input channels C that group divides", ln,
                         ty, wsize);
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
        const Conv3dApi* api = conv3d_api();
        if (!api) return FHIP_E_UNSUPPORTED; // message set by conv3d_api
        const Blob* b = bottoms[0];
        if (const int rc = conv3d_bottom(this, b)) return rc;
        if (b->c != Cg * group)
            return failf(NET_E_SHAPE, "layer %s: %s has weights for %d input channels, blob %s has %d", name.c_str(), type.c_str(), Cg * group, b->name.c_str(), b->c);
        const int in[3] = {b->d, b->h, b->w};
        for (int i = 0; i < 3; ++i)
            if (api->conv_output_dim(in[i], k[i], dil[i], s[i], lo[i], hi[i], &rlo[i], &rhi[i], &out[i]))
                return failf(NET_E_SHAPE, "layer %s: %s of blob %s, a volume of (%d, %d, %d): %s", name.c_str(), type.c_str(), b->name.c_str(), b->d, b->h, b->w, api->last_error());
        if (b->count() >= ((size_t)1 << 31) || volume_elements(b->n, K, out[0], out[1], out[2]) >= (1ll << 31))
            return failf(NET_E_SHAPE, "layer %s: %s: tensors of 2^31 elements or more are not supported", name.c_str(), type.c_str());
        return tops[0]->reshape_volume(b->n, K, out[0], out[1], out[2]);
    }
    int Init(hipStream_t st) override
    {
        if (built) return 0;
        const Conv3dApi* api = conv3d_api();
        if (!api) return FHIP_E_UNSUPPORTED;
        int rc = d_w.upload(w.data(), w.size(), st);
        if (!rc && bias_term) rc = d_bias.upload(bias.data(), bias.size(), st);
        packed_floats = api->packed_floats(Cg * group, K, k[0], k[1], k[2], dil[1], dil[2], s[1], s[2], group);
        if (!rc && packed_floats) rc = d_packed.resize((size_t)packed_floats * 4);
        if (!rc && packed_floats) rc = side(api, [&](const Conv3dApi* a) { return a->pack_weights(Cg * group, K, k[0], k[1], k[2], d_w.d, d_packed.d, st); });
        if (rc) return rc;
        FHIP_CHECK_HIP(hipStreamSynchronize(st));
        built = true;
        return 0;
    }
    int Forward(hipStream_t st) override
    {
        const Blob *b = bottoms[0], *t = tops[0];
        return side(conv3d_api(), [&](const Conv3dApi* api) {
            return api->conv_forward(b->n, b->c, b->d, b->h, b->w, K, k[0], k[1], k[2], dil[0], dil[1], dil[2], s[0], s[1], s[2], rlo[0], rhi[0], rlo[1], rhi[1], rlo[2], rhi[2],
                                     pad_value, group, act, a0, a1, b->data, d_w.d, packed_floats ? d_packed.d : nullptr, bias_term ? d_bias.d : nullptr, t->data, out[0], out[1],
                                     out[2], st);
        });
    }
    size_t weight_bytes() const override { return d_w.bytes + d_bias.bytes + d_packed.bytes; }
};

// ncnn's Pooling3D: 0=pooling_type 1/11/21=kernel w/h/d 2/12/22=stride 3/14=pad left/right 13/15=pad top/bottom 23/16=pad front/behind
// 4=global_pooling 5=pad_mode 6=avgpool_count_include_pad 7=adaptive_pooling 8/18/28=out w/h/d.  Global pooling writes ncnn's blob of rank
// 1, [n][1][1][C].
struct Pool3dLayer : Layer
{
    int type_ = 0, k[3] = {0, 0, 0}, s[3] = {1, 1, 1}, lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0}, want[3] = {0, 0, 0}; // axes: depth, row, column
    int global = 0, pad_mode = 0, include_pad = 0, adaptive = 0;
    int rlo[3] = {0, 0, 0}, rhi[3] = {0, 0, 0}, out[3] = {0, 0, 0};
    int algo() const override { return FHIP_CONV3D_NET_ROUTE; }
    bool reads_volume() const override { return true; }
    int LoadParam(const ParamDict& pd) override
    {
        const char* ln = name.c_str();
        if (bottoms.size() != 1 || tops.size() != 1) return failf(NET_E_SHAPE, "layer %s: Pooling3D needs 1 bottom and 1 top, got %zu and %zu", ln, bottoms.size(), tops.size());
        type_ = pd.get(0, 0);
        k[2] = pd.get(1, 0), k[1] = pd.get(11, k[2]), k[0] = pd.get(21, k[2]);
        s[2] = pd.get(2, 1), s[1] = pd.get(12, s[2]), s[0] = pd.get(22, s[2]);
        lo[2] = pd.get(3, 0), hi[2] = pd.get(14, lo[2]), lo[1] = pd.get(13, lo[2]), hi[1] = pd.get(15, lo[1]), lo[0] = pd.get(23, lo[2]), hi[0] = pd.get(16, lo[0]);
        global = pd.get(4, 0), pad_mode = pd.get(5, 0), include_pad = pd.get(6, 0), adaptive = pd.get(7, 0);
        want[2] = pd.get(8, 0), want[1] = pd.get(18, want[2]), want[0] = pd.get(28, want[2]);
        if (type_ < 0 || type_ > 1) return failf(NET_E_SHAPE, "layer %s: Pooling3D pooling_type (0=%d) must be 0 (max) or 1 (average)", ln, type_);
        if (global) return 0;
        static const int kid[3] = {21, 11, 1}, sid[3] = {22, 12, 2}, loid[3] = {23, 13, 3}, hiid[3] = {16, 15, 14}, oid[3] = {28, 18, 8};
        for (int i = 0; i < 3; ++i)
        {
            if (adaptive && want[i] < 1) return failf(NET_E_SHAPE, "layer %s: Pooling3D output extent (%d=%d) must be positive", ln, oid[i], want[i]);
            if (adaptive) continue;
            if (k[i] < 1) return failf(NET_E_SHAPE, "layer %s: Pooling3D kernel extent (%d=%d) must be positive", ln, kid[i], k[i]);
            if (s[i] < 1) return failf(NET_E_SHAPE, "layer %s: Pooling3D stride (%d=%d) must be positive", ln, sid[i], s[i]);
            if (lo[i] < 0 || hi[i] < 0) return failf(NET_E_SHAPE, "layer %s: Pooling3D pads (%d=%d %d=%d) must be >= 0", ln, loid[i], lo[i], hiid[i], hi[i]);
        }
        if (pad_mode < 0 || pad_mode > 3) return failf(NET_E_SHAPE, "layer %s: Pooling3D pad_mode (5=%d) must be 0 .. 3", ln, pad_mode);
        return 0;
    }
    int Reshape() override
    {
        const Conv3dApi* api = conv3d_api();
        if (!api) return FHIP_E_UNSUPPORTED; // message set by conv3d_api
        const Blob* b = bottoms[0];
        if (const int rc = conv3d_bottom(this, b)) return rc;
        if (b->count() >= ((size_t)1 << 31)) return failf(NET_E_SHAPE, "layer %s: Pooling3D: tensors of 2^31 elements or more are not supported", name.c_str());
        const int in[3] = {b->d, b->h, b->w};
        for (int i = 0; i < 3; ++i)
        {
            rlo[i] = rhi[i] = 0;
            if (global) out[i] = 1;
            else if (adaptive) out[i] = want[i];
            else if (api->pool_output_dim(in[i], k[i], s[i], lo[i], hi[i], pad_mode, &rlo[i], &rhi[i], &out[i]))
                return failf(NET_E_SHAPE, "layer %s: Pooling3D of blob %s, a volume of (%d, %d, %d): %s", name.c_str(), b->name.c_str(), b->d, b->h, b->w, api->last_error());
        }
        if (volume_elements(b->n, b->c, out[0], out[1], out[2]) >= (1ll << 31)) return failf(NET_E_SHAPE, "layer %s: Pooling3D: tensors of 2^31 elements or more are not supported", name.c_str());
        if (!global) return tops[0]->reshape_volume(b->n, b->c, out[0], out[1], out[2]);
        const int rc = tops[0]->reshape(b->n, 1, 1, b->c);
        tops[0]->dims = 1;
        return rc;
    }
    int Forward(hipStream_t st) override
    {
        const Blob* b = bottoms[0];
        const bool window = !global && !adaptive;
        return side(conv3d_api(), [&](const Conv3dApi* api) {
            return api->pool_forward(type_, b->n * b->c, b->d, b->h, b->w, window ? k[0] : 0, window ? k[1] : 0, window ? k[2] : 0, s[0], s[1], s[2], rlo[0], rhi[0], rlo[1], rhi[1],
                                     rlo[2], rhi[2], include_pad, b->data, tops[0]->data, out[0], out[1], out[2], st);
        });
    }
};

// The layer types of a net with fhip_net_set_conv3d (Net::conv3d).
static Layer* create_conv3d_layer(const std::string& type)
{
    if (type == "Convolution3D" || type == "ConvolutionDepthWise3D") return new Conv3dLayer;
    if (type == "Pooling3D") return new Pool3dLayer;
    return nullptr;
}

} // namespace fhip::net
