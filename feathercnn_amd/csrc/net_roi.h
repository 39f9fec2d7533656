// net_roi.h -- the layers of a net with fhip_net_set_roi (Net::roi): the second stage of ncnn's two-stage detectors -- Proposal, ROIPooling,
// ROIAlign and PSROIPooling.  include/feather_hip/feather_roi.h defines every layer; the kernels are libfeather_roi.so's (roi_api).  Every
// layer here reports the route FHIP_ROI_NET_ROUTE.  Nothing fuses into these layers and they absorb nothing, so every fusion level runs
// them as written; a default net never creates one of these classes.  A Proposal top is [n][R][1][4] and an ROI layer's top [n * R][c][ph][pw]:
// the layers behind it (InnerProduct, Pooling, Softmax) see a batch of n * R, and a sub-batch replica's share of the images is its share
// of the rows.
#pragma once
#include "feather_hip/feather_roi.h" // declarations only: the library is opened at run time (roi_api)
#include "net_layers.h"

namespace fhip::net
{

// libfeather_roi.so, the layers of a net with fhip_net_set_roi
struct RoiApi
{
    decltype(&fhip_roi_generate_anchors) generate_anchors = nullptr;
    decltype(&fhip_proposal_get_buffer_size) buffer_size = nullptr;
    decltype(&fhip_proposal_forward) proposal = nullptr;
    decltype(&fhip_roi_pool_forward) roi_pool = nullptr;
    decltype(&fhip_roi_align_forward) roi_align = nullptr;
    decltype(&fhip_psroi_pool_forward) psroi_pool = nullptr;
    decltype(&fhip_roi_last_error) last_error = nullptr;
    SideLibrary library()
    {
        return {"libfeather_roi.so", "a two-stage detection layer (Proposal, ROIPooling, ROIAlign, PSROIPooling)", "feather_roi.h",
                {{&generate_anchors, "fhip_roi_generate_anchors"}, {&buffer_size, "fhip_proposal_get_buffer_size"}, {&proposal, "fhip_proposal_forward"},
                 {&roi_pool, "fhip_roi_pool_forward"}, {&roi_align, "fhip_roi_align_forward"}, {&psroi_pool, "fhip_psroi_pool_forward"},
                 {&last_error, "fhip_roi_last_error"}}};
    }
};
static const RoiApi* roi_api() { return side_api<RoiApi>(); }

struct RoiNetLayer : Layer
{
    int algo() const override { return FHIP_ROI_NET_ROUTE; }
};

// ncnn's Proposal: 0=feat_stride 1=base_size 2=pre_nms_topN 3=after_nms_topN 4=nms_thresh 5=min_size; bottoms score [n][2A][h][w], bbox
// [n][4A][h][w] and im_info [n][3] (a second Input), A = 9: ncnn's ratios 0.5, 1, 2 and scales 8, 16, 32.  Tops rois [n][R][1][4] and,
// optionally, scores [n][R][1][1], R = after_nms_topN, sentinel rows past an image's count (feather_roi.h).  Two launches, the keys between
// them in the net's arena.
struct ProposalLayer : RoiNetLayer
{
    static constexpr int kAnchors = 9;
    int feat_stride = 16, base_size = 16, pre_nms_topN = 6000, after_nms_topN = 300;
    float nms_thresh = 0.7f, min_size = 16.f;
    float anchors[kAnchors][4] = {};
    size_t scratch_bytes = 0;
    int LoadParam(const ParamDict& pd) override
    {
        if (bottoms.size() != 3 || tops.empty() || tops.size() > 2)
            return failf(NET_E_SHAPE, "layer %s: Proposal needs three bottoms (score, bbox, im_info) and one or two tops, got %zu and %zu", name.c_str(),
                         bottoms.size(), tops.size());
        feat_stride = pd.get(0, 16);
        base_size = pd.get(1, 16);
        pre_nms_topN = pd.get(2, 6000);
        after_nms_topN = pd.get(3, 300);
        nms_thresh = pd.get(4, 0.7f);
        const int min_size_read = pd.get(5, 16); // an int, as in ncnn
        if (feat_stride < 1 || feat_stride > (1 << 16)) return failf(NET_E_SHAPE, "layer %s: Proposal feat_stride (0=%d) must be 1 .. 65536", name.c_str(), feat_stride);
        if (base_size < 1 || base_size > (1 << 16)) return failf(NET_E_SHAPE, "layer %s: Proposal base_size (1=%d) must be 1 .. 65536", name.c_str(), base_size);
        if (after_nms_topN < 1 || after_nms_topN > FHIP_ROI_MAX_ROIS)
            return failf(NET_E_SHAPE, "layer %s: Proposal after_nms_topN (3=%d) must be 1 .. %d", name.c_str(), after_nms_topN, FHIP_ROI_MAX_ROIS);
        if (!std::isfinite(nms_thresh)) return failf(NET_E_SHAPE, "layer %s: Proposal nms_thresh (4=) must be finite", name.c_str());
        if (min_size_read < -(1 << 24) || min_size_read > (1 << 24))
            return failf(NET_E_SHAPE, "layer %s: Proposal min_size (5=%d) must be an integer of at most 2^24 in magnitude", name.c_str(), min_size_read);
        min_size = (float)min_size_read;
        return 0;
    }
    int Reshape() override
    {
        const RoiApi* api = roi_api();
        if (!api) return FHIP_E_UNSUPPORTED; // message set by roi_api
        const Blob *score = bottoms[0], *bbox = bottoms[1], *info = bottoms[2];
        if (score->c != 2 * kAnchors || bbox->c != 4 * kAnchors)
            return failf(NET_E_SHAPE, "layer %s: Proposal needs a score of 2 * %d and a bbox of 4 * %d channels, got %d and %d", name.c_str(), kAnchors, kAnchors,
                         score->c, bbox->c);
        if (score->h != bbox->h || score->w != bbox->w || score->n != bbox->n)
            return failf(NET_E_SHAPE, "layer %s: Proposal score (%d, %d, %d) and bbox (%d, %d, %d) differ in batch or extent", name.c_str(), score->n, score->h,
                         score->w, bbox->n, bbox->h, bbox->w);
        if (info->n != score->n || (long long)info->c * info->h * info->w != 3)
            return failf(NET_E_SHAPE, "layer %s: Proposal im_info must hold (height, width, scale) for each of %d images, got %d x (%d, %d, %d)", name.c_str(),
                         score->n, info->n, info->c, info->h, info->w);
        const float ratios[3] = {0.5f, 1.f, 2.f}, scales[3] = {8.f, 16.f, 32.f};
        if (api->generate_anchors(base_size, ratios, 3, scales, 3, &anchors[0][0]) ||
            api->buffer_size(score->n, kAnchors, score->h, score->w, &scratch_bytes))
            return failf(NET_E_SHAPE, "layer %s: %s", name.c_str(), api->last_error());
        const int rc = tops[0]->reshape(score->n, after_nms_topN, 1, 4);
        if (rc || tops.size() < 2) return rc;
        return tops[1]->reshape(score->n, after_nms_topN, 1, 1);
    }
    int Forward(hipStream_t s) override
    {
        const Blob* score = bottoms[0];
        return side(roi_api(), [&](const RoiApi* api) {
            return api->proposal(score->n, kAnchors, score->h, score->w, feat_stride, pre_nms_topN, after_nms_topN, nms_thresh, min_size, &anchors[0][0],
                                 tops[0]->data, tops.size() > 1 ? tops[1]->data : nullptr, score->data, bottoms[1]->data, bottoms[2]->data, net->arena.d, s);
        });
    }
    size_t arena_bytes() const override { return scratch_bytes; }
};

// ncnn's ROIPooling (0=pooled_width 1=pooled_height 2=spatial_scale), ROIAlign (+ 3=sampling_ratio 4=aligned 5=version) and PSROIPooling
// (+ 3=output_dim): bottoms features [n][C][h][w] and rois [n][R][1][4] -- a Proposal top or an Input the caller feeds -- the top
// [n * R][channels][pooled_h][pooled_w], row i * R + r from image i.  One launch.
struct RoiPoolLayer : RoiNetLayer
{
    enum Kind { POOL, ALIGN, PSROI } kind = POOL;
    int pooled_w = 7, pooled_h = 7, sampling_ratio = 0, aligned = 0, version = 0, output_dim = 0, num_rois = 0;
    float spatial_scale = 0.0625f;
    int LoadParam(const ParamDict& pd) override
    {
        if (bottoms.size() != 2 || tops.size() != 1)
            return failf(NET_E_SHAPE, "layer %s: %s needs two bottoms (features, rois) and one top, got %zu and %zu", name.c_str(), type.c_str(), bottoms.size(),
                         tops.size());
        kind = type == "ROIAlign" ? ALIGN : (type == "PSROIPooling" ? PSROI : POOL);
        pooled_w = pd.get(0, 7);
        pooled_h = pd.get(1, 7);
        spatial_scale = pd.get(2, 0.0625f);
        if (pooled_w < 1 || pooled_w > FHIP_ROI_MAX_POOLED)
            return failf(NET_E_SHAPE, "layer %s: %s pooled_width (0=%d) must be 1 .. %d", name.c_str(), type.c_str(), pooled_w, FHIP_ROI_MAX_POOLED);
        if (pooled_h < 1 || pooled_h > FHIP_ROI_MAX_POOLED)
            return failf(NET_E_SHAPE, "layer %s: %s pooled_height (1=%d) must be 1 .. %d", name.c_str(), type.c_str(), pooled_h, FHIP_ROI_MAX_POOLED);
        if (!std::isfinite(spatial_scale)) return failf(NET_E_SHAPE, "layer %s: %s spatial_scale (2=) must be finite", name.c_str(), type.c_str());
        if (kind == PSROI)
        {
            output_dim = pd.get(3, 0);
            if (output_dim < 1 || output_dim > (1 << 20)) return failf(NET_E_SHAPE, "layer %s: PSROIPooling output_dim (3=%d) must be 1 .. 2^20", name.c_str(), output_dim);
        }
        if (kind == ALIGN)
        {
            sampling_ratio = pd.get(3, 0);
            aligned = pd.get(4, 0);
            version = pd.get(5, 0);
            if (sampling_ratio < 0 || sampling_ratio > FHIP_ROI_MAX_GRID)
                return failf(NET_E_SHAPE, "layer %s: ROIAlign sampling_ratio (3=%d) must be 0 .. %d", name.c_str(), sampling_ratio, FHIP_ROI_MAX_GRID);
            if (aligned != 0 && aligned != 1) return failf(NET_E_SHAPE, "layer %s: ROIAlign aligned (4=%d) must be 0 or 1", name.c_str(), aligned);
            if (version != 0 && version != 1) return failf(NET_E_SHAPE, "layer %s: ROIAlign version (5=%d) must be 0 or 1", name.c_str(), version);
        }
        return 0;
    }
    int Reshape() override
    {
        if (!roi_api()) return FHIP_E_UNSUPPORTED; // message set by roi_api
        const Blob *f = bottoms[0], *r = bottoms[1];
        if (r->n != f->n || r->h != 1 || r->w != 4 || r->c < 1)
            return failf(NET_E_SHAPE, "layer %s: rois must be [n][R][1][4] with the features' n = %d, got %d x (%d, %d, %d)", name.c_str(), f->n, r->n, r->c, r->h,
                         r->w);
        if (kind == PSROI && (long long)output_dim * pooled_h * pooled_w != f->c)
            return failf(NET_E_SHAPE, "layer %s: PSROIPooling needs output_dim * pooled_height * pooled_width = %d * %d * %d feature channels, got %d", name.c_str(),
                         output_dim, pooled_h, pooled_w, f->c);
        num_rois = r->c;
        const int channels = kind == PSROI ? output_dim : f->c;
        const long long rows = (long long)f->n * num_rois;
        if (rows * channels * pooled_h * pooled_w >= (1ll << 31) || f->count() >= ((size_t)1 << 31))
            return failf(NET_E_SHAPE, "layer %s: %s: tensors of 2^31 elements or more are not supported", name.c_str(), type.c_str());
        return tops[0]->reshape((int)rows, channels, pooled_h, pooled_w);
    }
    int Forward(hipStream_t s) override
    {
        const Blob *f = bottoms[0], *r = bottoms[1];
        return side(roi_api(), [&](const RoiApi* api) {
            if (kind == ALIGN)
                return api->roi_align(f->n, f->c, f->h, f->w, num_rois, pooled_w, pooled_h, spatial_scale, sampling_ratio, aligned, version, tops[0]->data, f->data,
                                      r->data, s);
            if (kind == PSROI)
                return api->psroi_pool(f->n, f->c, f->h, f->w, num_rois, pooled_w, pooled_h, spatial_scale, output_dim, tops[0]->data, f->data, r->data, s);
            return api->roi_pool(f->n, f->c, f->h, f->w, num_rois, pooled_w, pooled_h, spatial_scale, tops[0]->data, f->data, r->data, s);
        });
    }
};

// The layer types of a net with fhip_net_set_roi (Net::roi).  load_param_text asks here last, and only when the switch is on.
static Layer* create_roi_layer(const std::string& type)
{
    if (type == "Proposal") return new ProposalLayer;
    if (type == "ROIPooling" || type == "ROIAlign" || type == "PSROIPooling") return new RoiPoolLayer;
    return nullptr;
}

} // namespace fhip::net
