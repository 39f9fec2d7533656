// net_detect.h -- the layers of a net with fhip_net_set_detection (Net::detection): ncnn's SSD head -- Permute, Flatten, Reshape, Normalize,
// PriorBox, DetectionOutput, and the Concat and Softmax that know a blob's rank (Blob::dims) -- and the two level-2 rules that only move data.
// include/feather_hip/feather_detect.h defines every layer; the kernels are libfeather_detect.so's (detect_api).  Every layer here reports
// the route FHIP_DETECT_NET_ROUTE.  A default net never creates one of these classes.
#pragma once
#include "net_layers.h"

namespace fhip::net
{

// the extents of a blob as [n][c][h][w] and the place of axis 0 of its rank in them
struct Extents
{
    int e[4];
    int first; // rank 3: 1 (c), rank 2: 2 (h), rank 1: 3 (w)
    explicit Extents(const Blob* b) : e{b->n, b->c, b->h, b->w}, first(4 - b->dims) {}
    // a layer's axis (negative: from the end) as an index into e, or -1
    int at(int axis, int dims) const
    {
        if (axis < -dims || axis >= dims) return -1;
        return first + (axis < 0 ? axis + dims : axis);
    }
    size_t outer(int a) const // the product of the extents between n and a
    {
        size_t p = 1;
        for (int i = 1; i < a; ++i) p *= (size_t)e[i];
        return p;
    }
    size_t inner(int a) const
    {
        size_t p = 1;
        for (int i = a + 1; i < 4; ++i) p *= (size_t)e[i];
        return p;
    }
};

// top becomes a view of src's data with another shape: no storage, no launch (the way Split shares)
static void view_as(Blob* top, Blob* src, int c, int h, int w, int dims)
{
    top->share(src);
    top->c = c;
    top->h = h;
    top->w = w;
    top->dims = dims;
}

static int one_to_one_counts(const Layer* l)
{
    if (l->bottoms.size() == 1 && l->tops.size() == 1) return 0;
    return failf(NET_E_SHAPE, "layer %s: %s needs one bottom and one top, got %zu and %zu", l->name.c_str(), l->type.c_str(), l->bottoms.size(), l->tops.size());
}

struct DetectLayer : Layer
{
    int algo() const override { return FHIP_DETECT_NET_ROUTE; }
};

struct PermuteLayer : DetectLayer
{
    int order = 0;
    int LoadParam(const ParamDict& pd) override
    {
        if (const int rc = one_to_one_counts(this)) return rc;
        order = pd.get(0, 0);
        if (order < 0 || order > 5) return failf(NET_E_SHAPE, "layer %s: Permute order_type %d is not 0 .. 5", name.c_str(), order);
        return 0;
    }
    int Reshape() override
    {
        const DetectApi* api = detect_api();
        if (!api) return FHIP_E_UNSUPPORTED; // message set by detect_api
        const Blob* b = bottoms[0];
        int oc, oh, ow;
        if (b->dims == 1 || api->permute_output_dim(order, b->dims, b->c, b->h, b->w, &oc, &oh, &ow))
            return failf(NET_E_SHAPE, "layer %s: Permute order_type %d of a blob of rank %d (%d, %d, %d) is not supported", name.c_str(), order, b->dims, b->c, b->h, b->w);
        if (b->count() >= ((size_t)1 << 31)) return failf(NET_E_SHAPE, "layer %s: Permute: tensors of 2^31 elements or more are not supported", name.c_str());
        const int dims = b->dims;
        const int rc = tops[0]->reshape(b->n, oc, oh, ow);
        tops[0]->dims = dims;
        return rc;
    }
    int Forward(hipStream_t s) override
    {
        const Blob* b = bottoms[0];
        return side(detect_api(), [&](const DetectApi* api) { return api->permute(order, b->dims, b->n, b->c, b->h, b->w, tops[0]->data, b->data, s); });
    }
};

struct FlattenLayer : DetectLayer
{
    int LoadParam(const ParamDict&) override { return one_to_one_counts(this); }
    int Reshape() override
    {
        Blob* b = bottoms[0];
        if (b->count() / std::max(b->n, 1) >= ((size_t)1 << 31)) return failf(NET_E_SHAPE, "layer %s: Flatten: an image of 2^31 elements or more", name.c_str());
        view_as(tops[0], b, 1, 1, b->c * b->h * b->w, 1);
        return 0;
    }
    int Forward(hipStream_t) override { return 0; } // the top aliases the bottom
};

// ncnn's Reshape: 0=w 1=h 2=c, -233 (or absent) = the dimension does not exist, 0 = the bottom's extent, -1 = inferred; 3=permute must be 0
struct ReshapeLayer : DetectLayer
{
    int w = -233, h = -233, c = -233;
    int LoadParam(const ParamDict& pd) override
    {
        if (const int rc = one_to_one_counts(this)) return rc;
        w = pd.get(0, -233);
        h = pd.get(1, -233);
        c = pd.get(2, -233);
        if (pd.get(3, 0) != 0) return failf(NET_E_SHAPE, "layer %s: Reshape with permute (3=%d) is not supported", name.c_str(), pd.get(3, 0));
        if (w == -233 || (h == -233 && c != -233)) return failf(NET_E_SHAPE, "layer %s: Reshape needs w (0=), and h (1=) where it has c (2=)", name.c_str());
        int inferred = 0;
        for (int v : {w, h, c})
        {
            if (v < -1 && v != -233) return failf(NET_E_SHAPE, "layer %s: a Reshape extent must be positive, 0, -1 or -233, got %d", name.c_str(), v);
            inferred += v == -1;
        }
        if (inferred > 1) return failf(NET_E_SHAPE, "layer %s: Reshape infers at most one extent (-1)", name.c_str());
        return 0;
    }
    int Reshape() override
    {
        Blob* b = bottoms[0];
        const long long total = (long long)b->c * b->h * b->w;
        long long ext[3] = {w == 0 ? b->w : w, h == -233 ? 1 : (h == 0 ? b->h : h), c == -233 ? 1 : (c == 0 ? b->c : c)};
        // the extents are file values of up to 2^31 each: no product is formed that could pass `total` (a wrapped product could equal it)
        long long known = 1;
        bool fits = total >= 1;
        for (long long v : ext)
            if (v != -1)
            {
                fits = fits && v >= 1 && v <= total / known;
                if (fits) known *= v;
            }
        for (long long& v : ext)
            if (v == -1) v = fits && total % known == 0 ? total / known : 0;
        if (!fits || ext[0] < 1 || ext[1] < 1 || ext[2] < 1 || ext[0] > INT_MAX || ext[1] > INT_MAX || ext[2] > INT_MAX || ext[0] * ext[1] != total / ext[2] ||
            total % ext[2] != 0)
            return failf(NET_E_TOPOLOGY, "layer %s: Reshape of %lld elements into (w %d, h %d, c %d) does not keep the element count", name.c_str(), total, w, h, c);
        view_as(tops[0], b, (int)ext[2], (int)ext[1], (int)ext[0], c != -233 ? 3 : (h != -233 ? 2 : 1));
        return 0;
    }
    int Forward(hipStream_t) override { return 0; }
};

// Concat along any axis of the bottoms' rank.  It is a ConcatLayer whose `axis` never reads 0, so that no pass takes it for a channel
// concat before the ranks are known; rank 3 and axis 0 issue the copies ConcatLayer issues.  at_reshape (level 2, all bottoms PriorBox
// tops): the copies run once, at Reshape, and Forward launches nothing.
struct AxisConcatLayer : ConcatLayer
{
    int det_axis = 0;
    bool at_reshape = false;
    size_t rows = 0, inner = 0;
    int total = 0;
    std::vector<int> extent;
    int LoadParam(const ParamDict& pd) override
    {
        if (bottoms.empty() || tops.size() != 1)
            return failf(NET_E_SHAPE, "layer %s: Concat needs bottoms and one top, got %zu and %zu", name.c_str(), bottoms.size(), tops.size());
        det_axis = pd.get(0, 0);
        axis = -1;
        return 0;
    }
    int copies(hipStream_t s)
    {
        Blob* t = tops[0];
        size_t off = 0;
        for (size_t i = 0; i < bottoms.size(); ++i)
        {
            const size_t row = (size_t)extent[i] * inner * sizeof(float);
            FHIP_CHECK_HIP(hipMemcpy2DAsync(t->data + off * inner, (size_t)total * inner * sizeof(float), bottoms[i]->data, row, row, rows, hipMemcpyDeviceToDevice, s));
            off += extent[i];
        }
        return 0;
    }
    int Reshape() override
    {
        const Blob* a = bottoms[0];
        const Extents ea(a);
        const int at = ea.at(det_axis, a->dims);
        if (at < 0) return failf(NET_E_SHAPE, "layer %s: concat axis %d of blobs of rank %d", name.c_str(), det_axis, a->dims);
        long long sum = 0;
        extent.clear();
        for (const Blob* b : bottoms)
        {
            const Extents eb(b);
            bool same = b->dims == a->dims;
            for (int i = 0; i < 4; ++i) same = same && (i == at || eb.e[i] == ea.e[i]);
            if (!same) return failf(NET_E_SHAPE, "layer %s: blobs of different ranks, batches or other extents cannot be concatenated together", name.c_str());
            extent.push_back(eb.e[at]);
            sum += eb.e[at];
        }
        if (sum > INT_MAX) return failf(NET_E_SHAPE, "layer %s: the concatenated extent passes 2^31", name.c_str());
        total = (int)sum;
        rows = (size_t)a->n * ea.outer(at);
        inner = ea.inner(at);
        int e[4] = {a->n, a->c, a->h, a->w};
        e[at] = total;
        const int dims = a->dims;
        const int rc = tops[0]->reshape(e[0], e[1], e[2], e[3]);
        tops[0]->dims = dims;
        if (rc || !at_reshape) return rc;
        if (const int rc2 = copies(net->stream)) return rc2; // the PriorBox layers above have uploaded on the same stream
        FHIP_CHECK_HIP(hipStreamSynchronize(net->stream));
        return 0;
    }
    int Forward(hipStream_t s) override { return at_reshape ? 0 : copies(s); }
    int algo() const override { return FHIP_DETECT_NET_ROUTE; }
};

// Level 2: Concat(axis 0) of Flatten of Permute(order 3) of up to FHIP_PERMUTE_CONCAT_MAX blobs, one launch (collapse_detection_heads)
struct PermuteConcatLayer : DetectLayer
{
    int Reshape() override
    {
        if (!detect_api()) return FHIP_E_UNSUPPORTED; // message set by detect_api
        const Blob* a = bottoms[0];
        long long total = 0;
        for (const Blob* b : bottoms)
        {
            if (b->dims != 3) return failf(NET_E_SHAPE, "layer %s: Permute order_type 3 of a blob of rank %d is not supported", name.c_str(), b->dims);
            if (b->n != a->n) return failf(NET_E_SHAPE, "layer %s: blobs of different batches cannot be concatenated together", name.c_str());
            total += (long long)b->c * b->h * b->w;
        }
        if (total * a->n >= (1ll << 31)) return failf(NET_E_SHAPE, "layer %s: tensors of 2^31 elements or more are not supported", name.c_str());
        const int rc = tops[0]->reshape(a->n, 1, 1, (int)total);
        tops[0]->dims = 1;
        return rc;
    }
    int Forward(hipStream_t s) override
    {
        int c[FHIP_PERMUTE_CONCAT_MAX], hw[FHIP_PERMUTE_CONCAT_MAX];
        const float* in[FHIP_PERMUTE_CONCAT_MAX];
        for (size_t i = 0; i < bottoms.size(); ++i)
        {
            c[i] = bottoms[i]->c;
            hw[i] = bottoms[i]->h * bottoms[i]->w;
            in[i] = bottoms[i]->data;
        }
        return side(detect_api(), [&](const DetectApi* api) { return api->permute_concat((int)bottoms.size(), c, hw, bottoms[0]->n, tops[0]->data, in, s); });
    }
};

// Softmax along an axis of the bottom's rank: 0=axis, 1=fixbug0 (an axis other than 0 from a file without fixbug0 meant another axis in old
// ncnn versions: refused).  Where the axis is the innermost it is fhip_softmax over rows; else the strided kernel of libfeather_detect.so.
struct AxisSoftmaxLayer : Layer
{
    int axis = 0, len = 0;
    size_t outer = 0, inner = 0;
    int LoadParam(const ParamDict& pd) override
    {
        if (const int rc = one_to_one_counts(this)) return rc;
        axis = pd.get(0, 0);
        if (axis != 0 && pd.get(1, 0) == 0) return failf(NET_E_SHAPE, "layer %s: Softmax axis %d without fixbug0: param is too old, please regenerate", name.c_str(), axis);
        return 0;
    }
    int Reshape() override
    {
        const Blob* b = bottoms[0];
        const Extents e(b);
        // no params on a [n][c][1][1] blob: today's softmax over the whole image
        const int at = e.at(axis, b->dims);
        if (at < 0) return failf(NET_E_SHAPE, "layer %s: softmax axis %d of a blob of rank %d", name.c_str(), axis, b->dims);
        outer = (size_t)b->n * e.outer(at);
        len = e.e[at];
        inner = e.inner(at);
        if (b->count() >= ((size_t)1 << 31)) return failf(NET_E_SHAPE, "layer %s: Softmax: tensors of 2^31 elements or more are not supported", name.c_str());
        if (inner > 1 && !detect_api()) return FHIP_E_UNSUPPORTED; // message set by detect_api
        const int dims = b->dims;
        const int rc = tops[0]->reshape(b->n, b->c, b->h, b->w);
        tops[0]->dims = dims;
        return rc;
    }
    int Forward(hipStream_t s) override
    {
        const Blob* b = bottoms[0];
        if (inner == 1) return fhip_softmax(tops[0]->data, b->data, (int)outer, len, s);
        return side(detect_api(), [&](const DetectApi* api) { return api->axis_softmax((int)outer, len, (int)inner, tops[0]->data, b->data, s); });
    }
    int algo() const override { return FHIP_DETECT_NET_ROUTE; }
};

// ncnn's Normalize, the SSD form: 0=across_spatial (0) 1=channel_shared 2=eps 3=scale_data_size 4=across_channel (1) 9=eps_mode (0); one
// raw array of scale_data_size floats
struct NormalizeLayer : DetectLayer
{
    int channel_shared = 0, scale_size = 0;
    float eps = 1e-4f;
    std::vector<float> scale;
    DeviceVec d_scale;
    bool needs_weights() const override { return true; }
    int LoadParam(const ParamDict& pd) override
    {
        if (const int rc = one_to_one_counts(this)) return rc;
        channel_shared = pd.get(1, 0);
        eps = pd.get(2, 1e-4f);
        scale_size = pd.get(3, 0);
        if (pd.get(0, 0) != 0) return failf(NET_E_SHAPE, "layer %s: Normalize across_spatial (0=%d) is not supported", name.c_str(), pd.get(0, 0));
        if (pd.get(4, 1) != 1) return failf(NET_E_SHAPE, "layer %s: Normalize without across_channel (4=%d) is not supported", name.c_str(), pd.get(4, 1));
        if (pd.get(9, 0) != 0) return failf(NET_E_SHAPE, "layer %s: Normalize eps_mode (9=%d) other than 0 is not supported", name.c_str(), pd.get(9, 0));
        if (channel_shared != 0 && channel_shared != 1) return failf(NET_E_SHAPE, "layer %s: Normalize channel_shared (1=%d) must be 0 or 1", name.c_str(), channel_shared);
        if (!std::isfinite(eps) || !(eps > 0.f)) return failf(NET_E_SHAPE, "layer %s: Normalize eps (2=%g) must be finite and > 0", name.c_str(), (double)eps);
        if (scale_size < 1 || scale_size > (1 << 24)) return failf(NET_E_SHAPE, "layer %s: Normalize scale_data_size (3=%d) must be 1 .. 2^24", name.c_str(), scale_size);
        return 0;
    }
    int LoadWeights(ModelBin& mb) override { return mb.load((size_t)scale_size, 1, scale); }
    int Reshape() override
    {
        const Blob* b = bottoms[0];
        if (scale_size != 1 && scale_size != b->c)
            return failf(NET_E_TOPOLOGY, "layer %s: Normalize has %d scales for %d channels (1 or as many as channels)", name.c_str(), scale_size, b->c);
        if (!channel_shared && scale_size != b->c)
            return failf(NET_E_TOPOLOGY, "layer %s: Normalize without channel_shared has %d scales for %d channels", name.c_str(), scale_size, b->c);
        if (b->count() >= ((size_t)1 << 31)) return failf(NET_E_SHAPE, "layer %s: Normalize: tensors of 2^31 elements or more are not supported", name.c_str());
        const int dims = b->dims;
        const int rc = reshape_with(detect_api());
        tops[0]->dims = dims;
        return rc;
    }
    int Init(hipStream_t s) override
    {
        if (d_scale.d) return 0;
        const int rc = d_scale.upload(scale.data(), scale.size(), s);
        if (rc) return rc;
        FHIP_CHECK_HIP(hipStreamSynchronize(s));
        return 0;
    }
    int Forward(hipStream_t s) override
    {
        const Blob* b = bottoms[0];
        return side(detect_api(), [&](const DetectApi* api) { return api->normalize(b->n, b->c, b->h, b->w, channel_shared, eps, tops[0]->data, b->data, d_scale.d, s); });
    }
    size_t weight_bytes() const override { return d_scale.bytes; }
};

// ncnn's PriorBox: -23300=min_sizes -23301=max_sizes -23302=aspect_ratios 3..6=variances 7=flip 8=clip 9=image_width 10=image_height
// 11=step_width 12=step_height 13=offset; -233 (and an image extent of 0) = from the bottoms: the feature map and the image blob.  It depends
// on shapes only: Reshape fills it on the host (fhip_priorbox_fill), uploads it once, and Forward launches nothing.  The top is
// [1][1][2][4 * h * w * num_prior] whatever the batch.
struct PriorBoxLayer : DetectLayer
{
    std::vector<float> min_sizes, max_sizes, ratios, host;
    int built[4] = {0, 0, 0, 0}; // the feature map's and the image's extents `host` was filled for (everything else is fixed at LoadParam)
    float variances[4] = {0.1f, 0.1f, 0.2f, 0.2f}, step_w = -233.f, step_h = -233.f, offset = 0.f;
    int flip = 1, clip = 0, image_w = 0, image_h = 0;
    int LoadParam(const ParamDict& pd) override
    {
        if (bottoms.size() != 2 || tops.size() != 1)
            return failf(NET_E_SHAPE, "layer %s: PriorBox needs two bottoms (feature map, image) and one top, got %zu and %zu", name.c_str(), bottoms.size(), tops.size());
        min_sizes = pd.has_array(0) ? pd.e[0].array : std::vector<float>();
        max_sizes = pd.has_array(1) ? pd.e[1].array : std::vector<float>();
        ratios = pd.has_array(2) ? pd.e[2].array : std::vector<float>();
        if (min_sizes.empty() || min_sizes.size() > 64 || ratios.size() > 64)
            return failf(NET_E_SHAPE, "layer %s: PriorBox needs 1 .. 64 min_sizes (-23300=) and at most 64 aspect_ratios (-23302=)", name.c_str());
        if (!max_sizes.empty() && max_sizes.size() != min_sizes.size())
            return failf(NET_E_SHAPE, "layer %s: PriorBox max_sizes (-23301=) must be absent or as many as min_sizes", name.c_str());
        const auto positive = [](float v) { return std::isfinite(v) && v > 0.f; };
        for (const std::vector<float>* a : {&min_sizes, &max_sizes, &ratios})
            for (float v : *a)
                if (!positive(v)) return failf(NET_E_SHAPE, "layer %s: PriorBox sizes and aspect ratios must be finite and > 0, got %g", name.c_str(), (double)v);
        for (int k = 0; k < 4; ++k)
        {
            variances[k] = pd.get(3 + k, variances[k]);
            if (!std::isfinite(variances[k])) return failf(NET_E_SHAPE, "layer %s: PriorBox variance (%d=) must be finite", name.c_str(), 3 + k);
        }
        flip = pd.get(7, 1) != 0;
        clip = pd.get(8, 0) != 0;
        image_w = pd.get(9, 0);
        image_h = pd.get(10, 0);
        step_w = pd.get(11, -233.f);
        step_h = pd.get(12, -233.f);
        offset = pd.get(13, 0.f);
        if ((image_w < 0 && image_w != -233) || (image_h < 0 && image_h != -233))
            return failf(NET_E_SHAPE, "layer %s: PriorBox image_width / image_height (9=, 10=) must be positive, or 0 / -233 for the image blob's", name.c_str());
        for (float st : {step_w, step_h})
            if (st != -233.f && !positive(st)) return failf(NET_E_SHAPE, "layer %s: PriorBox steps (11=, 12=) must be finite and > 0, or -233", name.c_str());
        if (!std::isfinite(offset)) return failf(NET_E_SHAPE, "layer %s: PriorBox offset (13=) must be finite", name.c_str());
        return 0;
    }
    int Reshape() override
    {
        const DetectApi* api = detect_api();
        if (!api) return FHIP_E_UNSUPPORTED; // message set by detect_api
        const Blob *f = bottoms[0], *im = bottoms[1];
        const int iw = image_w > 0 ? image_w : im->w, ih = image_h > 0 ? image_h : im->h;
        const auto fill = [&](float* out, size_t capacity, int* per) {
            return api->priorbox(f->h, f->w, iw, ih, min_sizes.data(), (int)min_sizes.size(), max_sizes.data(), (int)max_sizes.size(), ratios.data(),
                                 (int)ratios.size(), variances, flip, clip, step_w == -233.f ? 0.f : step_w, step_h == -233.f ? 0.f : step_h, offset, per, out, capacity);
        };
        int per = 0;
        if (fill(nullptr, 0, &per)) return failf(NET_E_SHAPE, "layer %s: %s", name.c_str(), api->last_error());
        const size_t floats = (size_t)8 * f->h * f->w * per;
        Blob* t = tops[0];
        const float* before = t->data;
        const int rc = t->reshape(1, 1, 2, (int)(floats / 2));
        t->dims = 2;
        if (rc) return rc;
        const int now[4] = {f->h, f->w, iw, ih};
        if (before == t->data && host.size() == floats && !memcmp(now, built, sizeof(built))) return 0; // the same shapes: what the device holds is current
        host.resize(floats);
        if (fill(host.data(), floats, &per))
        {
            host.clear();
            return failf(NET_E_SHAPE, "layer %s: %s", name.c_str(), api->last_error());
        }
        memcpy(built, now, sizeof(built));
        FHIP_CHECK_HIP(hipMemcpyAsync(t->data, host.data(), floats * sizeof(float), hipMemcpyHostToDevice, net->stream));
        FHIP_CHECK_HIP(hipStreamSynchronize(net->stream));
        return 0;
    }
    int Forward(hipStream_t) override { return 0; }
};

// ncnn's DetectionOutput: 0=num_class 1=nms_threshold 2=nms_top_k 3=keep_top_k 4=confidence_threshold; bottoms location (4 * P per image),
// confidence (P * num_class, prior-major), priorbox ([2][4 * P], n = 1 or the batch); the top is [n][1][keep_top_k][6] of rank 2, zero rows
// past an image's count (feather_detect.h).  Two launches, the scratch between them in the net's arena.
struct DetectionOutputLayer : DetectLayer
{
    int num_class = 0, nms_top_k = 300, keep_top_k = 100, priors = 0;
    float nms_threshold = 0.05f, confidence_threshold = 0.5f;
    size_t scratch_bytes = 0;
    int LoadParam(const ParamDict& pd) override
    {
        if (bottoms.size() != 3 || tops.size() != 1)
            return failf(NET_E_SHAPE, "layer %s: DetectionOutput needs three bottoms (location, confidence, priorbox) and one top, got %zu and %zu", name.c_str(),
                         bottoms.size(), tops.size());
        num_class = pd.get(0, 0);
        nms_threshold = pd.get(1, 0.05f);
        nms_top_k = pd.get(2, 300);
        keep_top_k = pd.get(3, 100);
        confidence_threshold = pd.get(4, 0.5f);
        if (num_class < 2 || num_class > FHIP_DETECT_MAX_CLASSES)
            return failf(NET_E_SHAPE, "layer %s: DetectionOutput num_class (0=%d) must be 2 .. %d", name.c_str(), num_class, FHIP_DETECT_MAX_CLASSES);
        if (nms_top_k < 1 || nms_top_k > FHIP_DETECT_MAX_TOP_K || keep_top_k < 1 || keep_top_k > FHIP_DETECT_MAX_TOP_K)
            return failf(NET_E_SHAPE, "layer %s: DetectionOutput nms_top_k (2=%d) and keep_top_k (3=%d) must be 1 .. %d", name.c_str(), nms_top_k, keep_top_k,
                         FHIP_DETECT_MAX_TOP_K);
        if (!std::isfinite(nms_threshold) || !std::isfinite(confidence_threshold))
            return failf(NET_E_SHAPE, "layer %s: DetectionOutput thresholds (1=, 4=) must be finite", name.c_str());
        return 0;
    }
    int Reshape() override
    {
        const DetectApi* api = detect_api();
        if (!api) return FHIP_E_UNSUPPORTED; // message set by detect_api
        const Blob *loc = bottoms[0], *conf = bottoms[1], *pb = bottoms[2];
        const size_t per_image = (size_t)loc->c * loc->h * loc->w;
        if (loc->n < 1 || per_image < 4 || per_image % 4 || per_image / 4 > (size_t)FHIP_DETECT_MAX_PRIORS)
            return failf(NET_E_SHAPE, "layer %s: the location blob holds %zu values per image, not 4 per prior for 1 .. %d priors", name.c_str(), per_image,
                         FHIP_DETECT_MAX_PRIORS);
        priors = (int)(per_image / 4);
        if (conf->n != loc->n || (size_t)conf->c * conf->h * conf->w != (size_t)priors * num_class)
            return failf(NET_E_SHAPE, "layer %s: the confidence blob does not hold %d classes for each of %d priors of %d images", name.c_str(), num_class, priors, loc->n);
        if ((pb->n != 1 && pb->n != loc->n) || pb->c != 1 || pb->h != 2 || pb->w != 4 * priors)
            return failf(NET_E_SHAPE, "layer %s: the priorbox blob is not [2][4 * %d] once or per image", name.c_str(), priors);
        if (api->detection_buffer_size(loc->n, priors, num_class, nms_top_k, keep_top_k, &scratch_bytes))
            return failf(NET_E_SHAPE, "layer %s: %s", name.c_str(), api->last_error());
        const int rc = tops[0]->reshape(loc->n, 1, keep_top_k, 6);
        tops[0]->dims = 2;
        return rc;
    }
    int Forward(hipStream_t s) override
    {
        return side(detect_api(), [&](const DetectApi* api) {
            return api->detection_output(bottoms[0]->n, priors, num_class, nms_threshold, nms_top_k, keep_top_k, confidence_threshold, bottoms[2]->n, tops[0]->data,
                                         bottoms[0]->data, bottoms[1]->data, bottoms[2]->data, net->arena.d, s);
        });
    }
    size_t arena_bytes() const override { return scratch_bytes; }
};

// The layer types of a net with fhip_net_set_detection (Net::detection).  load_param_text asks here FIRST when the switch is on: Concat and
// Softmax are overridden by the classes that know a blob's rank.  PixelShuffle and Padding stay unknown.
static Layer* create_detection_layer(const std::string& type)
{
    if (type == "Permute") return new PermuteLayer;
    if (type == "Flatten") return new FlattenLayer;
    if (type == "Reshape") return new ReshapeLayer;
    if (type == "Normalize") return new NormalizeLayer;
    if (type == "PriorBox") return new PriorBoxLayer;
    if (type == "DetectionOutput") return new DetectionOutputLayer;
    if (type == "Concat") return new AxisConcatLayer;
    if (type == "Softmax") return new AxisSoftmaxLayer;
    return nullptr;
}

static int producer_of(const Net& net, const Blob* b)
{
    for (size_t j = 0; j < net.layers.size(); ++j)
        for (const Blob* t : net.layers[j]->tops)
            if (t == b) return (int)j;
    return -1;
}

// Fusion level 2 in a net with fhip_net_set_detection; both rules only move data, so results stay bit-identical.
//   1. a Concat (axis 0 or -1) whose bottoms are all Flatten of Permute order 3 -- up to FHIP_PERMUTE_CONCAT_MAX of them, every linking blob
//      with one consumer -- becomes one PermuteConcatLayer of one launch that keeps the Concat's type, name and place; the blobs inside
//      cannot be extracted.  A link with a second consumer leaves the Concat as written.
//   2. a Concat whose bottoms are all PriorBox tops copies at Reshape and launches nothing.
static void collapse_detection_heads(Net& net)
{
    if (!net.detection) return;
    for (size_t i = 0; i < net.layers.size(); ++i)
    {
        AxisConcatLayer* cat = dynamic_cast<AxisConcatLayer*>(net.layers[i].get());
        if (!cat) continue;
        bool priors = true;
        for (const Blob* b : cat->bottoms)
        {
            const int p = producer_of(net, b);
            priors = priors && p >= 0 && dynamic_cast<PriorBoxLayer*>(net.layers[p].get());
        }
        if (priors)
        {
            cat->at_reshape = true;
            continue;
        }
        if ((cat->det_axis != 0 && cat->det_axis != -1) || cat->bottoms.size() > FHIP_PERMUTE_CONCAT_MAX) continue;
        std::vector<int> drop;
        std::vector<Blob*> sources, inner;
        bool all = true;
        for (Blob* b : cat->bottoms)
        {
            const int f = producer_of(net, b);
            FlattenLayer* flat = f >= 0 ? dynamic_cast<FlattenLayer*>(net.layers[f].get()) : nullptr;
            const int p = flat && readers(net, b).count == 1 ? producer_of(net, flat->bottoms[0]) : -1;
            PermuteLayer* perm = p >= 0 ? dynamic_cast<PermuteLayer*>(net.layers[p].get()) : nullptr;
            if (!perm || perm->order != 3 || readers(net, flat->bottoms[0]).count != 1 || f > (int)i || p > f)
            {
                all = false;
                break;
            }
            drop.push_back(f);
            drop.push_back(p);
            inner.push_back(b);
            inner.push_back(flat->bottoms[0]);
            sources.push_back(perm->bottoms[0]);
        }
        if (!all) continue;
        std::unique_ptr<PermuteConcatLayer> one(new PermuteConcatLayer);
        one->type = cat->type;
        one->name = cat->name;
        one->net = &net;
        one->bottoms = sources;
        one->tops = cat->tops;
        for (Blob* b : inner) b->fused_away = true;
        net.layers[i] = std::move(one);
        std::sort(drop.begin(), drop.end());
        for (size_t k = drop.size(); k-- > 0;) net.layers.erase(net.layers.begin() + drop[k]);
        i -= drop.size();
    }
}

} // namespace fhip::net
