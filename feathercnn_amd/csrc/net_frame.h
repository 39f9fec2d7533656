// net_frame.h -- the layers of a net with fhip_net_set_frame (Net::frame): ncnn's Padding, Crop and PixelShuffle, the layers that frame an
// image-to-image net.  include/feather_hip/feather_frame.h defines every layer; the kernels are libfeather_frame.so's (frame_api).  Every layer
// here reports the route FHIP_FRAME_NET_ROUTE.  Padding and Crop are one operation there, the window: both classes below hold six signed
// margins and differ in how they read them.  A layer that changes nothing -- all margins 0, a crop of the whole blob, an upscale factor of
// 1 -- aliases its bottom as Split does and launches nothing.  Two fusions touch these layers (net_plan.h, level >= 2): a plain zero Padding
// in front of a convolution folds into the convolution's pads (fold_zero_paddings), and PixelShuffle absorbs the ReLU behind it.  A default
// net never creates one of these classes.
#pragma once
#include "feather_hip/feather_frame.h" // declarations only: the library is opened at run time (frame_api)
#include "net_layers.h"

namespace fhip::net
{

// libfeather_frame.so, the layers of a net with fhip_net_set_frame
struct FrameApi
{
    decltype(&fhip_frame_window_output_dim) window_output_dim = nullptr;
    decltype(&fhip_frame_window_forward) window = nullptr;
    decltype(&fhip_pixel_shuffle_output_dim) shuffle_output_dim = nullptr;
    decltype(&fhip_pixel_shuffle_forward) shuffle = nullptr;
    decltype(&fhip_frame_last_error) last_error = nullptr;
    SideLibrary library()
    {
        return {"libfeather_frame.so", "a framing layer (Padding, Crop, PixelShuffle)", "feather_frame.h",
                {{&window_output_dim, "fhip_frame_window_output_dim"}, {&window, "fhip_frame_window_forward"},
                 {&shuffle_output_dim, "fhip_pixel_shuffle_output_dim"}, {&shuffle, "fhip_pixel_shuffle_forward"}, {&last_error, "fhip_frame_last_error"}}};
    }
};
static const FrameApi* frame_api() { return side_api<FrameApi>(); }

struct FrameLayer : Layer
{
    bool noop = false; // this shape changes nothing: the top shares the bottom's storage (Reshape), Forward launches nothing
    int algo() const override { return FHIP_FRAME_NET_ROUTE; }
    // a q8 bottom never gets here (reshape_all refuses it: reads_q8 is false); under fhip_net_set_detection a blob knows its rank
    int check_bottom(const Blob* b) const
    {
        if (b->dims != 3) return failf(NET_E_SHAPE, "layer %s: %s needs a blob of rank 3 (c, h, w), blob %s has rank %d", name.c_str(), type.c_str(), b->name.c_str(), b->dims);
        return 0;
    }
};

// The window both Padding and Crop run: margins (front, behind, top, bottom, left, right), set by the derived class's Reshape.
struct WindowLayer : FrameLayer
{
    int border = FHIP_FRAME_CONSTANT;
    float value = 0.f;
    int m[6] = {0, 0, 0, 0, 0, 0};
    const float* per_channel_dev = nullptr;
    int reshape_window()
    {
        const FrameApi* api = frame_api();
        if (!api) return FHIP_E_UNSUPPORTED; // message set by frame_api
        const Blob* b = bottoms[0];
        int oc, oh, ow;
        if (api->window_output_dim(b->c, b->h, b->w, m[0], m[1], m[2], m[3], m[4], m[5], &oc, &oh, &ow))
            return failf(NET_E_SHAPE, "layer %s: %s of a blob (%d, %d, %d): %s", name.c_str(), type.c_str(), b->c, b->h, b->w, api->last_error());
        if (border == FHIP_FRAME_REFLECT && (m[2] >= b->h || m[3] >= b->h || m[4] >= b->w || m[5] >= b->w))
            return failf(NET_E_SHAPE, "layer %s: a reflect pad (%d, %d, %d, %d) must be smaller than the plane (%d, %d) it pads", name.c_str(), m[2], m[3], m[4], m[5],
                         b->h, b->w);
        long long total = (long long)b->n * oc; // every factor is below 2^31: the running product is checked before the next one
        if (total < (1ll << 31)) total *= oh;
        if (total < (1ll << 31)) total *= ow;
        if (total >= (1ll << 31) || b->count() >= ((size_t)1 << 31))
            return failf(NET_E_SHAPE, "layer %s: %s: tensors of 2^31 elements or more are not supported", name.c_str(), type.c_str());
        noop = !(m[0] | m[1] | m[2] | m[3] | m[4] | m[5]);
        if (noop)
        {
            tops[0]->share(bottoms[0]);
            return 0;
        }
        return tops[0]->reshape(b->n, oc, oh, ow);
    }
    int Forward(hipStream_t s) override
    {
        if (noop) return 0;
        const Blob* b = bottoms[0];
        return side(frame_api(), [&](const FrameApi* api) {
            return api->window(border, value, per_channel_dev, b->n, b->c, b->h, b->w, m[0], m[1], m[2], m[3], m[4], m[5], tops[0]->data, b->data, s);
        });
    }
};

// ncnn's Padding: 0=top 1=bottom 2=left 3=right 4=type 5=value 6=per_channel_pad_data_size 7=front 8=behind; with 6 > 0 that many raw floats
// in the .bin.  The dynamic form (a second bottom, or -233 margins) is refused.
struct PaddingLayer : WindowLayer
{
    int per_channel_size = 0;
    std::vector<float> per_channel;
    DeviceVec d_per_channel;
    bool inited = false;
    int pads[4] = {0, 0, 0, 0}; // top, bottom, left, right
    int LoadParam(const ParamDict& pd) override
    {
        if (bottoms.size() == 2) return failf(NET_E_SHAPE, "layer %s: Padding with a second bottom (dynamic pads) is not supported", name.c_str());
        if (bottoms.size() != 1 || tops.size() != 1)
            return failf(NET_E_SHAPE, "layer %s: Padding needs one bottom and one top, got %zu and %zu", name.c_str(), bottoms.size(), tops.size());
        const int ids[6] = {7, 8, 0, 1, 2, 3};
        for (int k = 0; k < 6; ++k)
        {
            m[k] = pd.get(ids[k], 0);
            if (m[k] == -233) return failf(NET_E_SHAPE, "layer %s: Padding margin %d=-233 (dynamic pads) is not supported", name.c_str(), ids[k]);
            if (m[k] < 0) return failf(NET_E_SHAPE, "layer %s: Padding margin (%d=%d) must be >= 0", name.c_str(), ids[k], m[k]);
        }
        for (int k = 0; k < 4; ++k) pads[k] = m[2 + k];
        border = pd.get(4, 0);
        value = pd.get(5, 0.f);
        per_channel_size = pd.get(6, 0);
        if (border < FHIP_FRAME_CONSTANT || border > FHIP_FRAME_REFLECT)
            return failf(NET_E_SHAPE, "layer %s: Padding type (4=%d) must be 0 (constant), 1 (replicate) or 2 (reflect)", name.c_str(), border);
        if (per_channel_size < 0) return failf(NET_E_SHAPE, "layer %s: Padding per_channel_pad_data_size (6=%d) must be >= 0", name.c_str(), per_channel_size);
        if (border != FHIP_FRAME_CONSTANT && (per_channel_size > 0 || m[0] > 0 || m[1] > 0))
            return failf(NET_E_SHAPE, "layer %s: Padding per-channel values (6=) and channel pads (7=, 8=) are defined for type 0 only, got type %d", name.c_str(), border);
        return 0;
    }
    bool needs_weights() const override { return per_channel_size > 0; }
    int LoadWeights(ModelBin& mb) override
    {
        if (per_channel_size <= 0) return 0;
        inited = false;
        return mb.load((size_t)per_channel_size, 1, per_channel);
    }
    int Reshape() override
    {
        const Blob* b = bottoms[0];
        int rc = check_bottom(b);
        if (rc) return rc;
        if (per_channel_size > 0 && per_channel_size != b->c)
            return failf(NET_E_SHAPE, "layer %s: Padding holds %d per-channel values (6=) while bottom blob %s has %d channels", name.c_str(), per_channel_size,
                         b->name.c_str(), b->c);
        return reshape_window();
    }
    int Init(hipStream_t s) override
    {
        if (inited || per_channel_size <= 0) return 0;
        const int rc = d_per_channel.upload(per_channel.data(), per_channel.size(), s);
        if (rc) return rc;
        FHIP_CHECK_HIP(hipStreamSynchronize(s));
        per_channel_dev = d_per_channel.d;
        inited = true;
        return 0;
    }
    size_t weight_bytes() const override { return d_per_channel.bytes; }
    // the four margins where this is a plain zero padding of the plane: what a convolution's own pads would do (fold_zero_paddings)
    const int* zero_pad_margins() const override
    {
        uint32_t bits;
        memcpy(&bits, &value, 4);
        return border == FHIP_FRAME_CONSTANT && bits == 0 && per_channel_size == 0 && m[0] == 0 && m[1] == 0 ? pads : nullptr;
    }
};

// ncnn's Crop: 0=woffset 1=hoffset 2=coffset 3=outw 4=outh 5=outc 6=woffset2 7=hoffset2 8=coffset2; out = -233: dim - offset - offset2.
// With a second bottom, the reference: its (c, h, w) are (outc, outh, outw) and the offsets those of 0 / 1 / 2; only its shape is read.
// The starts / ends / axes form (9 / 10 / 11) is refused.
struct CropLayer : WindowLayer
{
    int off[3] = {0, 0, 0}, out[3] = {-233, -233, -233}, off2[3] = {0, 0, 0}; // w, h, c
    int LoadParam(const ParamDict& pd) override
    {
        if (bottoms.empty() || bottoms.size() > 2 || tops.size() != 1)
            return failf(NET_E_SHAPE, "layer %s: Crop needs one or two bottoms and one top, got %zu and %zu", name.c_str(), bottoms.size(), tops.size());
        for (int id = 9; id <= 11; ++id)
            if (pd.e[id].loaded)
                return failf(NET_E_SHAPE, "layer %s: Crop by starts / ends / axes (%d=) is not supported", name.c_str(), -23300 - id);
        for (int k = 0; k < 3; ++k)
        {
            off[k] = pd.get(k, 0);
            out[k] = pd.get(3 + k, -233);
            off2[k] = pd.get(6 + k, 0);
            if (off[k] < 0 || off2[k] < 0) return failf(NET_E_SHAPE, "layer %s: Crop offsets (%d=%d, %d=%d) must be >= 0", name.c_str(), k, off[k], 6 + k, off2[k]);
            if (out[k] != -233 && out[k] < 1) return failf(NET_E_SHAPE, "layer %s: Crop size (%d=%d) must be >= 1 or -233", name.c_str(), 3 + k, out[k]);
        }
        return 0;
    }
    int Reshape() override
    {
        const Blob* b = bottoms[0];
        int rc = check_bottom(b);
        if (rc) return rc;
        if (bottoms.size() == 2 && (rc = check_bottom(bottoms[1]))) return rc;
        if (bottoms.size() == 2 && bottoms[1]->n != b->n)
            return failf(NET_E_SHAPE, "layer %s: Crop reference %s has a batch of %d, the blob one of %d", name.c_str(), bottoms[1]->name.c_str(), bottoms[1]->n, b->n);
        const int dim[3] = {b->w, b->h, b->c};
        const int ref[3] = {bottoms.size() == 2 ? bottoms[1]->w : 0, bottoms.size() == 2 ? bottoms[1]->h : 0, bottoms.size() == 2 ? bottoms[1]->c : 0};
        int lo[3], hi[3];
        for (int k = 0; k < 3; ++k)
        {
            const long long size = bottoms.size() == 2 ? ref[k] : (out[k] == -233 ? (long long)dim[k] - off[k] - off2[k] : out[k]);
            if (size < 1 || (long long)off[k] + size > dim[k])
                return failf(NET_E_SHAPE, "layer %s: Crop window (offset %d, size %lld) leaves the %s of %d of blob %s", name.c_str(), off[k], size,
                             k == 0 ? "width" : (k == 1 ? "height" : "channels"), dim[k], b->name.c_str());
            lo[k] = -off[k];
            hi[k] = (int)((long long)off[k] + size - dim[k]);
        }
        m[0] = lo[2], m[1] = hi[2], m[2] = lo[1], m[3] = hi[1], m[4] = lo[0], m[5] = hi[0];
        return reshape_window();
    }
};

// ncnn's PixelShuffle: 0=upscale_factor 1=mode.  Absorbs the ReLU behind it (level >= 2), plain or with a slope: one launch, bit for bit the two.
struct PixelShuffleLayer : FrameLayer
{
    int r = 1, mode = 0, relu = FHIP_FRAME_RELU_NONE;
    float slope = 0.f;
    int LoadParam(const ParamDict& pd) override
    {
        if (bottoms.size() != 1 || tops.size() != 1)
            return failf(NET_E_SHAPE, "layer %s: PixelShuffle needs one bottom and one top, got %zu and %zu", name.c_str(), bottoms.size(), tops.size());
        r = pd.get(0, 1);
        mode = pd.get(1, 0);
        if (r < 1) return failf(NET_E_SHAPE, "layer %s: PixelShuffle upscale_factor (0=%d) must be at least 1", name.c_str(), r);
        if (mode != 0 && mode != 1) return failf(NET_E_SHAPE, "layer %s: PixelShuffle mode (1=%d) must be 0 or 1", name.c_str(), mode);
        return 0;
    }
    int Reshape() override
    {
        const FrameApi* api = frame_api();
        if (!api) return FHIP_E_UNSUPPORTED; // message set by frame_api
        const Blob* b = bottoms[0];
        const int rc = check_bottom(b);
        if (rc) return rc;
        int oc, oh, ow;
        if (api->shuffle_output_dim(r, b->c, b->h, b->w, &oc, &oh, &ow))
            return failf(NET_E_SHAPE, "layer %s: PixelShuffle with upscale_factor %d of a blob (%d, %d, %d): %s", name.c_str(), r, b->c, b->h, b->w, api->last_error());
        if (b->count() >= ((size_t)1 << 31)) return failf(NET_E_SHAPE, "layer %s: PixelShuffle: tensors of 2^31 elements or more are not supported", name.c_str());
        noop = r == 1 && relu == FHIP_FRAME_RELU_NONE;
        if (noop)
        {
            tops[0]->share(bottoms[0]);
            return 0;
        }
        return tops[0]->reshape(b->n, oc, oh, ow);
    }
    int Forward(hipStream_t s) override
    {
        if (noop) return 0;
        const Blob* b = bottoms[0];
        return side(frame_api(), [&](const FrameApi* api) { return api->shuffle(r, mode, relu, slope, b->n, b->c, b->h, b->w, tops[0]->data, b->data, s); });
    }
    int Fuse(Layer* next, int level) override
    {
        if (level < 2 || relu != FHIP_FRAME_RELU_NONE || !next->relu_slope()) return 0;
        slope = *next->relu_slope();
        relu = is_plain_relu(next) ? FHIP_FRAME_RELU_PLAIN : FHIP_FRAME_RELU_SLOPE; // fhip_relu's fmaxf, or the leaky layer's x > 0 ? x : x * slope
        return 1;
    }
};

// The layer types of a net with fhip_net_set_frame (Net::frame).  load_param_text asks here last, and only when the switch is on.
static Layer* create_frame_layer(const std::string& type)
{
    if (type == "Padding") return new PaddingLayer;
    if (type == "Crop") return new CropLayer;
    if (type == "PixelShuffle") return new PixelShuffleLayer;
    return nullptr;
}

} // namespace fhip::net
