// net_yolo.h -- the layers of a net with fhip_net_set_yolo (Net::yolo): ncnn's YOLO heads -- Reorg, YoloDetectionOutput (YOLOv2) and
// Yolov3DetectionOutput.  include/feather_hip/feather_yolo.h defines every layer; the kernels are libfeather_yolo.so's (yolo_api).  Every
// layer here reports the route FHIP_YOLO_NET_ROUTE.  Nothing fuses into these layers and they absorb nothing, so every fusion level runs
// them as written; a default net never creates one of these classes.
#pragma once
#include "feather_hip/feather_yolo.h" // declarations only: the library is opened at run time (yolo_api)
#include "net_layers.h"

namespace fhip::net
{

// libfeather_yolo.so, the layers of a net with fhip_net_set_yolo: Reorg and the two detection outputs
struct YoloApi
{
    decltype(&fhip_reorg_output_dim) reorg_output_dim = nullptr;
    decltype(&fhip_reorg_forward) reorg = nullptr;
    decltype(&fhip_yolo_get_buffer_size) buffer_size = nullptr;
    decltype(&fhip_yolo_detection_forward) detection = nullptr;
    decltype(&fhip_yolo_last_error) last_error = nullptr;
    SideLibrary library()
    {
        return {"libfeather_yolo.so", "a YOLO-head layer (Reorg, YoloDetectionOutput, Yolov3DetectionOutput)", "feather_yolo.h",
                {{&reorg_output_dim, "fhip_reorg_output_dim"}, {&reorg, "fhip_reorg_forward"}, {&buffer_size, "fhip_yolo_get_buffer_size"},
                 {&detection, "fhip_yolo_detection_forward"}, {&last_error, "fhip_yolo_last_error"}}};
    }
};
static const YoloApi* yolo_api() { return side_api<YoloApi>(); }

struct YoloLayer : Layer
{
    int algo() const override { return FHIP_YOLO_NET_ROUTE; }
};

// ncnn's Reorg: 0=stride 1=mode
struct ReorgLayer : YoloLayer
{
    int stride = 1, mode = 0;
    int LoadParam(const ParamDict& pd) override
    {
        if (bottoms.size() != 1 || tops.size() != 1)
            return failf(NET_E_SHAPE, "layer %s: Reorg needs one bottom and one top, got %zu and %zu", name.c_str(), bottoms.size(), tops.size());
        stride = pd.get(0, 1);
        mode = pd.get(1, 0);
        if (stride < 1) return failf(NET_E_SHAPE, "layer %s: Reorg stride (0=%d) must be at least 1", name.c_str(), stride);
        if (mode != 0 && mode != 1) return failf(NET_E_SHAPE, "layer %s: Reorg mode (1=%d) must be 0 or 1", name.c_str(), mode);
        return 0;
    }
    int Reshape() override
    {
        const YoloApi* api = yolo_api();
        if (!api) return FHIP_E_UNSUPPORTED; // message set by yolo_api
        const Blob* b = bottoms[0];
        int oc, oh, ow;
        if (api->reorg_output_dim(stride, b->c, b->h, b->w, &oc, &oh, &ow))
            return failf(NET_E_SHAPE, "layer %s: Reorg with stride %d of a blob (%d, %d, %d): %s", name.c_str(), stride, b->c, b->h, b->w, api->last_error());
        if (b->count() >= ((size_t)1 << 31)) return failf(NET_E_SHAPE, "layer %s: Reorg: tensors of 2^31 elements or more are not supported", name.c_str());
        return tops[0]->reshape(b->n, oc, oh, ow);
    }
    int Forward(hipStream_t s) override
    {
        const Blob* b = bottoms[0];
        return side(yolo_api(), [&](const YoloApi* api) { return api->reorg(stride, mode, b->n, b->c, b->h, b->w, tops[0]->data, b->data, s); });
    }
};

// ncnn's YoloDetectionOutput and Yolov3DetectionOutput: 0=num_class 1=num_box 2=confidence_threshold 3=nms_threshold -23304=biases, and for
// Yolov3DetectionOutput -23305=mask -23306=anchors_scale; 1 .. FHIP_YOLO_MAX_SCALES bottoms [n][num_box * (5 + num_class)][h][w].  The top is
// [n][1][rows][6] of rank 2, rows = the value of fhip_net_set_yolo, zero rows past an image's count (feather_yolo.h).  Two launches, the keys
// between them in the net's arena.
struct YoloDetectionOutputLayer : YoloLayer
{
    int version = 2, num_class = 20, num_box = 5, rows = 0;
    float confidence_threshold = 0.01f, nms_threshold = 0.45f;
    std::vector<float> biases, anchors_scale;
    std::vector<int> mask, hs, ws;
    size_t scratch_bytes = 0;
    int LoadParam(const ParamDict& pd) override
    {
        if (bottoms.empty() || bottoms.size() > FHIP_YOLO_MAX_SCALES || tops.size() != 1)
            return failf(NET_E_SHAPE, "layer %s: %s needs 1 .. %d bottoms and one top, got %zu and %zu", name.c_str(), type.c_str(), FHIP_YOLO_MAX_SCALES,
                         bottoms.size(), tops.size());
        version = type == "Yolov3DetectionOutput" ? 3 : 2;
        rows = net->yolo;
        num_class = pd.get(0, 20);
        num_box = pd.get(1, 5);
        confidence_threshold = pd.get(2, 0.01f);
        nms_threshold = pd.get(3, 0.45f);
        if (num_class < 1 || num_class > FHIP_YOLO_MAX_CLASSES)
            return failf(NET_E_SHAPE, "layer %s: %s num_class (0=%d) must be 1 .. %d", name.c_str(), type.c_str(), num_class, FHIP_YOLO_MAX_CLASSES);
        if (num_box < 1 || num_box > FHIP_YOLO_MAX_BOXES)
            return failf(NET_E_SHAPE, "layer %s: %s num_box (1=%d) must be 1 .. %d", name.c_str(), type.c_str(), num_box, FHIP_YOLO_MAX_BOXES);
        if (!std::isfinite(confidence_threshold)) return failf(NET_E_SHAPE, "layer %s: %s confidence_threshold (2=) must be finite", name.c_str(), type.c_str());
        if (!std::isfinite(nms_threshold)) return failf(NET_E_SHAPE, "layer %s: %s nms_threshold (3=) must be finite", name.c_str(), type.c_str());
        biases = pd.has_array(4) ? pd.e[4].array : std::vector<float>();
        const size_t anchors = biases.size() / 2;
        if (biases.empty() || biases.size() % 2 || anchors > (size_t)FHIP_YOLO_MAX_SCALES * FHIP_YOLO_MAX_BOXES || (version == 2 && anchors < (size_t)num_box))
            return failf(NET_E_SHAPE, "layer %s: %s biases (-23304=) must be pairs, %s, got %zu values", name.c_str(), type.c_str(),
                         version == 2 ? "at least num_box of them" : "at most 64 of them", biases.size());
        for (float v : biases)
            if (!std::isfinite(v)) return failf(NET_E_SHAPE, "layer %s: %s biases (-23304=) must be finite", name.c_str(), type.c_str());
        mask.clear();
        anchors_scale.clear();
        if (version == 2) return 0;
        const std::vector<float> m = pd.has_array(5) ? pd.e[5].array : std::vector<float>();
        if (m.size() != bottoms.size() * (size_t)num_box)
            return failf(NET_E_SHAPE, "layer %s: %s mask (-23305=) must hold num_box = %d entries for each of %zu bottoms, got %zu", name.c_str(), type.c_str(),
                         num_box, bottoms.size(), m.size());
        for (float v : m)
        {
            if (!(v >= 0.f) || !(v < (float)anchors) || v != floorf(v))
                return failf(NET_E_SHAPE, "layer %s: %s mask (-23305=) entry %g is not one of the %zu anchors", name.c_str(), type.c_str(), (double)v, anchors);
            mask.push_back((int)v);
        }
        anchors_scale = pd.has_array(6) ? pd.e[6].array : std::vector<float>();
        if (anchors_scale.size() != bottoms.size())
            return failf(NET_E_SHAPE, "layer %s: %s anchors_scale (-23306=) must hold one value for each of %zu bottoms, got %zu", name.c_str(), type.c_str(),
                         bottoms.size(), anchors_scale.size());
        for (float v : anchors_scale)
            if (!std::isfinite(v) || !(v > 0.f)) return failf(NET_E_SHAPE, "layer %s: %s anchors_scale (-23306=) must be finite and > 0", name.c_str(), type.c_str());
        return 0;
    }
    int Reshape() override
    {
        const YoloApi* api = yolo_api();
        if (!api) return FHIP_E_UNSUPPORTED; // message set by yolo_api
        const Blob* a = bottoms[0];
        hs.clear();
        ws.clear();
        for (const Blob* b : bottoms)
        {
            if (b->c != num_box * (5 + num_class))
                return failf(NET_E_SHAPE, "layer %s: bottom %s has %d channels, not num_box * (5 + num_class) = %d * (5 + %d)", name.c_str(), b->name.c_str(), b->c,
                             num_box, num_class);
            if (b->n != a->n) return failf(NET_E_SHAPE, "layer %s: the bottoms have different batches (%d and %d)", name.c_str(), a->n, b->n);
            hs.push_back(b->h);
            ws.push_back(b->w);
        }
        if (api->buffer_size(a->n, (int)bottoms.size(), num_box, num_class, hs.data(), ws.data(), &scratch_bytes))
            return failf(NET_E_SHAPE, "layer %s: %s", name.c_str(), api->last_error());
        const int rc = tops[0]->reshape(a->n, 1, rows, 6);
        tops[0]->dims = 2;
        return rc;
    }
    int Forward(hipStream_t s) override
    {
        const float* in[FHIP_YOLO_MAX_SCALES];
        for (size_t i = 0; i < bottoms.size(); ++i) in[i] = bottoms[i]->data;
        return side(yolo_api(), [&](const YoloApi* api) {
            return api->detection(version, bottoms[0]->n, (int)bottoms.size(), num_box, num_class, hs.data(), ws.data(), confidence_threshold, nms_threshold,
                                  biases.data(), (int)biases.size(), mask.data(), anchors_scale.data(), rows, tops[0]->data, in, net->arena.d, s);
        });
    }
    size_t arena_bytes() const override { return scratch_bytes; }
};

// The layer types of a net with fhip_net_set_yolo (Net::yolo).  load_param_text asks here last, and only when the switch is on.
static Layer* create_yolo_layer(const std::string& type)
{
    if (type == "Reorg") return new ReorgLayer;
    if (type == "YoloDetectionOutput" || type == "Yolov3DetectionOutput") return new YoloDetectionOutputLayer;
    return nullptr;
}

} // namespace fhip::net
