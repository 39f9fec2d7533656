// net_dcn.h -- the layer of a net with fhip_net_set_deformable (Net::deformable): ncnn's DeformableConv2D.
// include/feather_hip/feather_dcn.h defines it, libfeather_dcn.so holds it (dcn_api); the layer reports the route FHIP_DCN_NET_ROUTE.
// Nothing fuses into or out of the layer: it has ncnn's built-in activation.  A default net never creates this class.
#pragma once
#include "feather_hip/feather_dcn.h" // declarations only: the library is opened at run time (dcn_api)
#include "net_conv1d.h"

namespace fhip::net
{

// libfeather_dcn.so, the layer of a net with fhip_net_set_deformable
struct DcnApi
{
    decltype(&fhip_dcn_output_dim) output_dim = nullptr;
    decltype(&fhip_dcn_packed_floats) packed_floats = nullptr;
    decltype(&fhip_dcn_pack_weights) pack_weights = nullptr;
    decltype(&fhip_dcn_forward) forward = nullptr;
    decltype(&fhip_dcn_last_error) last_error = nullptr;
    SideLibrary library()
    {
        return {"libfeather_dcn.so", "a deformable convolution (DeformableConv2D)", "feather_dcn.h",
                {{&output_dim, "fhip_dcn_output_dim"}, {&packed_floats, "fhip_dcn_packed_floats"}, {&pack_weights, "fhip_dcn_pack_weights"}, {&forward, "fhip_dcn_forward"},
                 {&last_error, "fhip_dcn_last_error"}}};
    }
};
static const DcnApi* dcn_api() { return side_api<DcnApi>(); }

// ncnn's DeformableConv2D (0=num_output 1=kernel_w 11=kernel_h 2=dilation_w 12=dilation_h 3=stride_w 13=stride_h 4=pad_left 15=pad_right
// 14=pad_top 16=pad_bottom 5=bias_term 6=weight_data_size 9=activation_type 10=activation_params); bottoms x, offset [2 kh kw][Ho][Wo] and,
// optionally, mask [kh kw][Ho][Wo]; weights tagged [num_output][C][kernel_h][kernel_w], then the raw bias.  One offset group, as in ncnn.
struct DeformConvLayer : Layer
{
    int K = 0, kw = 0, kh = 0, dw = 1, dh = 1, sw = 1, sh = 1, pl = 0, pr = 0, pt = 0, pb = 0, bias_term = 0, act = 0, C = 0;
    int ho = 0, wo = 0;
    long long wsize = 0;
    float a0 = 0.f, a1 = 0.f;
    std::vector<float> w, bias;
    DeviceVec d_packed, d_bias;
    bool built = false;
    int algo() const override { return FHIP_DCN_NET_ROUTE; }
    bool needs_weights() const override { return true; }
    int LoadParam(const ParamDict& pd) override
    {
        const char* ln = name.c_str();
        if (bottoms.size() < 2 || bottoms.size() > 3 || tops.size() != 1)
            return failf(NET_E_SHAPE, "layer %s: DeformableConv2D needs 2 or 3 bottoms (x, offset, mask) and 1 top, got %zu and %zu", ln, bottoms.size(), tops.size());
        K = pd.get(0, 0), kw = pd.get(1, 0), kh = pd.get(11, kw), dw = pd.get(2, 1), dh = pd.get(12, dw), sw = pd.get(3, 1), sh = pd.get(13, sw);
        pl = pd.get(4, 0), pr = pd.get(15, pl), pt = pd.get(14, pl), pb = pd.get(16, pt), bias_term = pd.get(5, 0), wsize = pd.get(6, 0), act = pd.get(9, 0);
        if (pd.get(19, 0) != 0) return failf(NET_E_SHAPE, "layer %s: DeformableConv2D with dynamic_weight (19=%d) is not supported", ln, pd.get(19, 0));
        if (pd.get(8, 0) != 0) return failf(NET_E_SHAPE, "layer %s: DeformableConv2D with int8 weights (8=%d) is not supported", ln, pd.get(8, 0));
        if (pd.get(7, 1) != 1) return failf(NET_E_SHAPE, "layer %s: DeformableConv2D with a group (7=%d) is not supported", ln, pd.get(7, 1));
        if (K < 1) return failf(NET_E_SHAPE, "layer %s: DeformableConv2D num_output (0=%d) must be positive", ln, K);
        if (kw < 1 || kh < 1) return failf(NET_E_SHAPE, "layer %s: DeformableConv2D kernel (1=%d 11=%d) must be positive", ln, kw, kh);
        if (dw < 1 || dh < 1) return failf(NET_E_SHAPE, "layer %s: DeformableConv2D dilation (2=%d 12=%d) must be positive", ln, dw, dh);
        if (sw < 1 || sh < 1) return failf(NET_E_SHAPE, "layer %s: DeformableConv2D stride (3=%d 13=%d) must be positive", ln, sw, sh);
        if (pl < 0 || pr < 0 || pt < 0 || pb < 0) return failf(NET_E_SHAPE, "layer %s: DeformableConv2D pads (4=%d 15=%d 14=%d 16=%d) must be >= 0", ln, pl, pr, pt, pb);
        if (act < 0 || act > 6) return failf(NET_E_SHAPE, "layer %s: DeformableConv2D activation_type (9=%d) must be 0 .. 6", ln, act);
        const long long taps = (long long)kh * kw, per = taps < (1ll << 31) ? taps * K : (1ll << 31); // weights per input channel
        if (per >= (1ll << 31) || wsize >= (1ll << 31))
            return failf(NET_E_SHAPE, "layer %s: DeformableConv2D weight_data_size (6=%lld): tensors of 2^31 elements or more are not supported", ln, wsize);
        if (wsize < 1 || wsize % per) return failf(NET_E_SHAPE, "layer %s: DeformableConv2D weight_data_size (6=%lld) must be num_output * C * kernel_h * kernel_w", ln, wsize);
        C = (int)(wsize / per);
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
    // a bottom beside x: `planes` channels of the output's extent, the batch of x
    int beside(const Blob* b, const Blob* x, int planes, const char* what) const
    {
        if (b->n == x->n && b->c == planes && b->h == ho && b->w == wo) return 0;
        return failf(NET_E_SHAPE, "layer %s: DeformableConv2D needs %s of (%d, %d, %d), blob %s has (%d, %d, %d)", name.c_str(), what, planes, ho, wo, b->name.c_str(), b->c, b->h, b->w);
    }
    int Reshape() override
    {
        const DcnApi* api = dcn_api();
        if (!api) return FHIP_E_UNSUPPORTED; // message set by dcn_api
        const Blob* b = bottoms[0];
        if (b->c != C) return failf(NET_E_SHAPE, "layer %s: DeformableConv2D has weights for %d input channels, blob %s has %d", name.c_str(), C, b->name.c_str(), b->c);
        if (api->output_dim(b->h, b->w, kh, kw, dh, dw, sh, sw, pt, pb, pl, pr, &ho, &wo))
            return failf(NET_E_SHAPE, "layer %s: DeformableConv2D of blob %s, a plane of %d x %d: %s", name.c_str(), b->name.c_str(), b->h, b->w, api->last_error());
        if (const int rc = beside(bottoms[1], b, 2 * kh * kw, "an offset blob")) return rc;
        if (bottoms.size() > 2)
            if (const int rc = beside(bottoms[2], b, kh * kw, "a mask blob")) return rc;
        if (b->count() >= ((size_t)1 << 31) || bottoms[1]->count() >= ((size_t)1 << 31) || (long long)b->n * K * ho * wo >= (1ll << 31))
            return failf(NET_E_SHAPE, "layer %s: DeformableConv2D: tensors of 2^31 elements or more are not supported", name.c_str());
        return tops[0]->reshape(b->n, K, ho, wo);
    }
    // uploads and packs once: ncnn's layout goes through a device buffer of this call into the kernel's
    int Init(hipStream_t st) override
    {
        if (built) return 0;
        const DcnApi* api = dcn_api();
        if (!api) return FHIP_E_UNSUPPORTED;
        const long long floats = api->packed_floats(C, K, kh, kw, 1);
        if (floats < 1) return failf(NET_E_SHAPE, "layer %s: %s", name.c_str(), api->last_error());
        DeviceVec raw;
        int rc = raw.upload(w.data(), w.size(), st);
        if (!rc) rc = d_packed.resize((size_t)floats * 4);
        if (!rc && bias_term) rc = d_bias.upload(bias.data(), bias.size(), st);
        if (!rc) rc = side(api, [&](const DcnApi* a) { return a->pack_weights(C, K, kh, kw, 1, raw.d, d_packed.d, st); });
        if (rc) return rc;
        FHIP_CHECK_HIP(hipStreamSynchronize(st)); // raw leaves with this call
        built = true;
        return 0;
    }
    int Forward(hipStream_t st) override
    {
        const Blob *b = bottoms[0], *t = tops[0];
        return side(dcn_api(), [&](const DcnApi* api) {
            return api->forward(b->n, C, b->h, b->w, K, kh, kw, dh, dw, sh, sw, pt, pb, pl, pr, 1, act, a0, a1, b->data, bottoms[1]->data, bottoms.size() > 2 ? bottoms[2]->data : nullptr,
                                d_packed.d, bias_term ? d_bias.d : nullptr, t->data, ho, wo, st);
        });
    }
    size_t weight_bytes() const override { return d_packed.bytes + d_bias.bytes; }
};

// The layer type of a net with fhip_net_set_deformable (Net::deformable).
static Layer* create_deformable_layer(const std::string& type) { return type == "DeformableConv2D" ? new DeformConvLayer : nullptr; }

} // namespace fhip::net
