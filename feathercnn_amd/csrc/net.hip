// net.hip -- feather::Net on device blobs.
//
// The host runtime either side of the ConvBooster hot path: the ncnn .param/.bin readers, the layer objects
// with the reference's LoadParam / LoadWeights / Reshape / Init / Forward life cycle, one shared device scratch
// arena in place of CommonMemPool, and the layer-fusion pass the reference declares but never runs.
// Reference (paths relative to /root/reference/src): net.cpp:31-349, layer.cpp:24-142, layers/*.h,
// ncnn/paramdict.cpp:92-174, ncnn/modelbin.cpp:47-197, mempool.cpp:88-92.
//
// What differs from the reference on purpose:
//   * blobs carry a batch dimension (the reference hard-codes num = 1 in every Reshape);
//   * blob data lives in HBM, weights are uploaded once at Init and the packed conv weights stay resident;
//   * everything is enqueued on one HIP stream; Forward returns after enqueueing (Extract-to-host synchronises);
//   * Reshape runs only when the fed input shape changed (the reference re-runs it every Forward, net.cpp:299);
//   * Split tops and Dropout(scale = 1) tops alias their bottom instead of copying it -- no layer writes in place,
//     so an aliased blob is never modified;
//   * optional hipGraph replay of the whole forward.
//
// One translation unit, read in this order (no header includes a later one): net_side.h -- errors, the side libraries; net_model.h --
// ParamDict, ModelBin; net_core.h -- Blob, DeviceVec, Layer, Net, the graph queries; net_conv.h -- the convolution layer, its side routes
// and the weight staging it shares; net_layers.h -- the other layer classes; net_detect.h -- the detection-head layers and their factory; net_yolo.h -- the YOLO-head layers and
// theirs; net_roi.h -- the two-stage detection layers and theirs; net_frame.h -- Padding, Crop, PixelShuffle and theirs; net_attn.h -- the transformer layers and theirs; net_rnn.h -- the recurrent layers and theirs; net_plan.h -- the fusion and planning passes, prepare,
// forward.  Here: the layer factories, the loaders that call them, and the fhip_net_* C-ABI.
#include "net_side.h"
#include "net_model.h"
#include "net_core.h"
#include "net_conv.h"
#include "net_layers.h"
#include "net_detect.h"
#include "net_yolo.h"
#include "net_roi.h"
#include "net_frame.h"
#include "net_attn.h"
#include "net_rnn.h"
#include "net_plan.h"

namespace fhip::net
{

// The layer types of a net with fhip_net_set_extended_layers (Net::extended); load_param_text asks here only when create_layer knows no
// such type and the switch is on.
static Layer* create_extended_layer(const std::string& type)
{
    if (type == "Interp") return new InterpLayer;
    if (type == "HardSwish") return new HardSwishLayer;
    if (type == "LRN") return new LRNLayer;
    return nullptr;
}

static Layer* create_layer(const std::string& type) // layer_factory.cpp:55-67
{
    if (type == "Input") return new InputLayer;
    if (type == "Convolution" || type == "ConvolutionDepthWise") return new ConvLayer;
    if (type == "Deconvolution" || type == "DeconvolutionDepthWise") return new DeconvLayer;
    if (type == "ReLU") return new ReluLayer;
    if (type == "InstanceNorm") return new InstanceNormLayer;
    if (type == "PReLU" || type == "Sigmoid" || type == "TanH" || type == "Clip") return new ActivationLayer;
    if (type == "Pooling") return new PoolingLayer;
    if (type == "InnerProduct") return new InnerProductLayer;
    if (type == "Dropout") return new DropoutLayer;
    if (type == "Softmax") return new SoftmaxLayer;
    if (type == "BatchNorm") return new BatchNormLayer;
    if (type == "Scale") return new ScaleLayer;
    if (type == "Split") return new SplitLayer;
    if (type == "Eltwise") return new EltwiseLayer;
    if (type == "Concat") return new ConcatLayer;
    if (type == "ShuffleChannel" || type == "Slice") return new ChannelMapLayer;
    if (type == "BinaryOp") return new BinaryOpLayer;
    if (type == "Swish" || type == "HardSigmoid") return new GateActivationLayer;
    return nullptr;
}

// ---- Net::LoadParam (net.cpp:67-170) over a token stream: fscanf("%s") semantics ------------------------------------
static int load_param_text(Net& net, const char* text, size_t len)
{
    if (net.param_loaded) return failf(NET_E_IO, "a param file is already loaded");
    std::vector<std::string> tok;
    {
        size_t i = 0;
        while (i < len)
        {
            while (i < len && isspace((unsigned char)text[i])) ++i;
            const size_t a = i;
            while (i < len && !isspace((unsigned char)text[i])) ++i;
            if (i > a) tok.emplace_back(text + a, i - a);
        }
    }
    size_t t = 0;
    auto next = [&](std::string& out) {
        if (t >= tok.size()) return false;
        out = tok[t++];
        return true;
    };
    std::string s;
    if (!next(s)) return failf(NET_E_IO, "issue with param file");
    if (atoi(s.c_str()) != 7767517) return failf(NET_E_IO, "param is too old, please regenerate"); // utils.cpp:27-44
    std::string a, b;
    if (!next(a) || !next(b)) return failf(NET_E_IO, "issue with param file");
    const int layer_count = atoi(a.c_str()), blob_count = atoi(b.c_str());
    if (layer_count <= 0 || blob_count <= 0) return failf(NET_E_IO, "issue with param file");

    ParamDict pd;
    for (int i = 0; i < layer_count; ++i)
    {
        std::string type, name, nb, nt;
        if (!next(type) || !next(name) || !next(nb) || !next(nt)) return failf(NET_E_IO, "param file ends after %d of %d layers", i, layer_count);
        std::unique_ptr<Layer> layer(net.detection ? create_detection_layer(type) : nullptr); // asked first: it overrides Concat and Softmax
        if (!layer && net.transformer) // asked before create_layer: it overrides BinaryOp and InnerProduct
        {
            layer.reset(create_transformer_layer(type));
            // without the blob ranks BinaryOp and InnerProduct stay what a default net knows; the new types are refused
            if (layer && !net.detection && (type == "BinaryOp" || type == "InnerProduct")) layer.reset();
            else if (layer && !net.detection)
                return failf(NET_E_UNKNOWN_LAYER, "layer %s: the layers of fhip_net_set_transformer need the blob ranks fhip_net_set_detection maintains: set both", type.c_str());
        }
        if (!layer) layer.reset(create_layer(type));
        if (!layer && net.extended) layer.reset(create_extended_layer(type));
        if (!layer && net.yolo) layer.reset(create_yolo_layer(type));
        if (!layer && net.roi) layer.reset(create_roi_layer(type));
        if (!layer && net.frame) layer.reset(create_frame_layer(type));
        if (!layer && net.recurrent)
        {
            layer.reset(create_recurrent_layer(type));
            if (layer && !net.detection)
                return failf(NET_E_UNKNOWN_LAYER, "layer %s: the layers of fhip_net_set_recurrent need the blob ranks fhip_net_set_detection maintains: set both", type.c_str());
        }
        if (!layer)
        {
            std::unique_ptr<Layer> opt_in(create_extended_layer(type)), detect(create_detection_layer(type)), yolo(create_yolo_layer(type)),
                roi(create_roi_layer(type)), frame(create_frame_layer(type)), transformer(create_transformer_layer(type)), recurrent(create_recurrent_layer(type));
            return failf(NET_E_UNKNOWN_LAYER, "layer %s not exists or registered%s", type.c_str(),
                         opt_in ? " (fhip_net_set_extended_layers lifts this)"
                                : (detect ? " (fhip_net_set_detection lifts this)" : (yolo ? " (fhip_net_set_yolo lifts this)" : (roi ? " (fhip_net_set_roi lifts this)" : (frame ? " (fhip_net_set_frame enables it)" : (transformer ? " (fhip_net_set_transformer lifts this)" : (recurrent ? " (fhip_net_set_recurrent lifts this)" : "")))))));
        }
        layer->type = type;
        layer->name = name;
        layer->net = &net;
        const int bottom_count = atoi(nb.c_str()), top_count = atoi(nt.c_str());
        // the reference uses both counts as read (net.cpp:98-137) and a layer without bottoms or tops faults at its first Reshape
        if (bottom_count < 0 || top_count < 1 || (bottom_count == 0 && type != "Input" && type != "MemoryData"))
            return failf(NET_E_TOPOLOGY, "Topology error: layer %s type %s has %d bottoms and %d tops.", name.c_str(), type.c_str(), bottom_count, top_count);
        for (int j = 0; j < bottom_count; ++j)
        {
            std::string bn;
            if (!next(bn)) return failf(NET_E_IO, "param file truncated in layer %s", name.c_str());
            Blob* blob = net.find(bn);
            if (!blob) return failf(NET_E_TOPOLOGY, "Topology error: bottom blob %s of layer %s type %s not found in map.", bn.c_str(), name.c_str(), type.c_str());
            layer->bottoms.push_back(blob);
        }
        for (int j = 0; j < top_count; ++j)
        {
            std::string tn;
            if (!next(tn)) return failf(NET_E_IO, "param file truncated in layer %s", name.c_str());
            std::unique_ptr<Blob> blob(new Blob);
            blob->name = tn;
            layer->tops.push_back(blob.get());
            auto& slot = net.blobs[tn];
            if (slot) net.shadowed.push_back(std::move(slot)); // earlier layers (and this layer's bottoms) still point at it
            slot = std::move(blob);
        }
        pd.clear();
        while (t < tok.size() && ParamDict::looks_like_pair(tok[t]))
        {
            const int rc = pd.parse(tok[t++]);
            if (rc) return rc;
        }
        const int rc = layer->LoadParam(pd);
        if (rc) return rc;
        net.layers.push_back(std::move(layer));
    }
    net.param_loaded = true;
    return 0;
}

static int load_weights_mem(Net& net, const void* data, size_t len)
{
    if (net.initialized) return failf(NET_E_IO, "Net is already initialized. Are you repeatedly loading models?");
    if (net.layers.empty()) return failf(NET_E_IO, "Network has not been loaded. Please load the param file first.");
    ModelBin mb{(const unsigned char*)data, (const unsigned char*)data + len};
    for (auto& l : net.layers)
    {
        const int rc = l->LoadWeights(mb);
        if (rc)
        {
            const std::string why = fhip_last_error();
            return failf(NET_E_IO, "Layer %s loading weights failed: %s", l->name.c_str(), why.c_str());
        }
    }
    net.weights_loaded = true;
    return 0;
}

static int read_file(const char* path, std::vector<char>& out)
{
    FILE* fp = fopen(path, "rb");
    if (!fp) return failf(NET_E_IO, "Cannot open file, path: %s", path);
    fseek(fp, 0, SEEK_END);
    const long sz = ftell(fp);
    fseek(fp, 0, SEEK_SET);
    out.resize(sz > 0 ? (size_t)sz : 0);
    const size_t got = out.empty() ? 0 : fread(out.data(), 1, out.size(), fp);
    fclose(fp);
    if (got != out.size()) return failf(NET_E_IO, "short read on %s", path);
    return 0;
}

} // namespace fhip::net

using namespace fhip;
using namespace fhip::net;

struct fhip_net
{
    Net impl; // the net -- or, with fhip_net_set_sub_batches(R > 1), the replica that takes the first share of every batch
    // Sub-batch replicas: R - 1 further complete nets (own layers, weights, blobs, arena, stream, graph).  FeedInput deals the images
    // out in contiguous shares, Forward runs all replicas concurrently (fork / join events against impl.stream), Extract puts the
    // shares back together.  Images are independent, so no replica ever reads another's data.
    std::vector<std::unique_ptr<fhip_net>> more;
    std::vector<hipStream_t> more_streams;
    hipEvent_t fork = nullptr;
    std::vector<hipEvent_t> joins;
    std::vector<int> share;                    // images per replica at the last FeedInput (index 0 = impl)
    std::map<std::string, DeviceVec> gathered; // Extract: blobs put back together (device pointer API)
    unsigned char* staging = nullptr;          // FeedPixels from host memory: the uint8 images, uploaded once (FeedPixelImages: + plans)
    size_t staging_bytes = 0;
    std::vector<unsigned char> plans;          // FeedPixelImages: the host plans, the source of their upload into the staging buffer
    hipEvent_t plans_read = nullptr;           // recorded after that upload; `plans` is rewritten only once it has passed
    ~fhip_net()
    {
        if (staging) (void)hipFree(staging);
        if (plans_read) (void)hipEventDestroy(plans_read);
        more.clear();
        for (hipStream_t st : more_streams) (void)hipStreamDestroy(st);
        if (fork) (void)hipEventDestroy(fork);
        for (hipEvent_t e : joins) (void)hipEventDestroy(e);
    }
};

// contiguous shares of `num` images for `parts` replicas, the remainder dealt to the first ones (feathercnn_amd/shard.py's rule)
static void deal(int num, int parts, std::vector<int>& share)
{
    share.assign(parts, num / parts);
    for (int r = 0; r < num % parts; ++r) ++share[r];
}

// n's staging buffer holds at least `bytes`
static int reserve_staging(fhip_net* n, size_t bytes)
{
    if (bytes <= n->staging_bytes) return FHIP_OK;
    // the old buffer may still be read by conversions queued earlier (every replica's is joined into the net's stream)
    FHIP_CHECK_HIP(hipStreamSynchronize(n->impl.stream));
    if (n->staging) FHIP_CHECK_HIP(hipFree(n->staging));
    n->staging = nullptr;
    n->staging_bytes = 0;
    FHIP_CHECK_HIP(hipMalloc((void**)&n->staging, bytes));
    n->staging_bytes = bytes;
    return FHIP_OK;
}

// The shares of fhip_net_feed_input for `num` images converted into blob_name as [num][cout][target_h][target_w]: with sub-batch replicas
// contiguous shares, each converted by its replica on its own stream after a fork from the net's stream and joined back; each net's blob
// is reshaped (and its graph dropped) only when its shape changes.  convert(output, first image, count, stream).
template <class Convert>
static int feed_shares(fhip_net* n, const char* blob_name, int num, int cout, int target_w, int target_h, const Convert& convert)
{
    const auto into_blob = [&](fhip_net* m, int first, int cnt) -> int {
        Blob* b = m->impl.find(blob_name);
        if (!b) return failf(NET_E_IO, "Invalid input blob %s, not found in map.", blob_name);
        if (b->n != cnt || b->c != cout || b->h != target_h || b->w != target_w)
        {
            const float* old = b->data;
            const int rc = b->reshape(cnt, cout, target_h, target_w);
            if (rc) return rc;
            m->impl.shapes_dirty = true;
            if (old != b->data) m->impl.drop_graph();
        }
        return convert(b->data, first, cnt, m->impl.stream);
    };
    if (!n->more.empty())
    {
        deal(num, (int)n->more.size() + 1, n->share);
        FHIP_CHECK_HIP(hipEventRecord(n->fork, n->impl.stream));
        int first = n->share[0];
        for (size_t r = 0; r < n->more.size(); ++r)
        {
            const int cnt = n->share[r + 1];
            if (cnt > 0)
            {
                FHIP_CHECK_HIP(hipStreamWaitEvent(n->more[r]->impl.stream, n->fork, 0));
                const int rc = into_blob(n->more[r].get(), first, cnt);
                if (rc) return rc;
                FHIP_CHECK_HIP(hipEventRecord(n->joins[r], n->more[r]->impl.stream));
                FHIP_CHECK_HIP(hipStreamWaitEvent(n->impl.stream, n->joins[r], 0));
            }
            first += cnt;
        }
        num = n->share[0];
    }
    return into_blob(n, 0, num);
}

// The body of fhip_net_feed_pixels / fhip_net_feed_yuv420sp once the arguments are checked: `num` images of `image` bytes (host memory
// unless on_device) into blob_name, each net converting its share with convert(output, device bytes, count, stream).
template <class Convert>
static int feed_bytes(fhip_net* n, const char* blob_name, int num, const unsigned char* bytes_in, size_t image, int cout, int target_w,
                      int target_h, int on_device, const Convert& convert)
{
    if (!n->impl.find(blob_name)) return failf(NET_E_IO, "Invalid input blob %s, not found in map.", blob_name);
    const unsigned char* pixels = bytes_in;
    if (!on_device)
    {
        // one uint8 upload of the whole batch on the net's stream; the replicas then read their shares from the staging buffer
        const int rc = reserve_staging(n, image * num);
        if (rc) return rc;
        FHIP_CHECK_HIP(hipMemcpyAsync(n->staging, pixels, image * num, hipMemcpyHostToDevice, n->impl.stream));
        pixels = n->staging;
    }
    return feed_shares(n, blob_name, num, cout, target_w, target_h, [&](float* out, int first, int cnt, hipStream_t s) {
        return convert(out, pixels + first * image, cnt, s);
    });
}

#define NET_GUARD(n) \
    if (!(n)) return fail(FHIP_E_BADARG, "null net")

extern "C"
{

int fhip_net_create(fhip_net** out)
{
    if (!out) return fail(FHIP_E_BADARG, "null argument");
    *out = new fhip_net;
    return FHIP_OK;
}

int fhip_net_destroy(fhip_net* n)
{
    NET_GUARD(n);
    for (auto& m : n->more)
        if (m->impl.stream) (void)hipStreamSynchronize(m->impl.stream);
    if (n->impl.stream || n->impl.initialized) (void)hipStreamSynchronize(n->impl.stream);
    delete n;
    return FHIP_OK;
}

int fhip_net_set_sub_batches(fhip_net* n, int replicas)
{
    NET_GUARD(n);
    if (replicas < 1 || replicas > 16) return fail(FHIP_E_BADARG, "1 .. 16 sub-batches");
    if (n->impl.param_loaded || !n->more.empty()) return fail(FHIP_E_BADARG, "set the number of sub-batches once, before LoadParam");
    for (int r = 1; r < replicas; ++r)
    {
        hipStream_t st = nullptr;
        FHIP_CHECK_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        n->more_streams.push_back(st);
        hipEvent_t e = nullptr;
        FHIP_CHECK_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        n->joins.push_back(e);
        std::unique_ptr<fhip_net> m(new fhip_net);
        m->impl.stream = st;
        m->impl.fusion = n->impl.fusion;
        m->impl.use_graph = n->impl.use_graph;
        m->impl.tuned_selection = n->impl.tuned_selection;
        m->impl.dilated = n->impl.dilated;
        m->impl.extended = n->impl.extended;
        m->impl.detection = n->impl.detection;
        m->impl.quantized = n->impl.quantized;
        m->impl.requantized = n->impl.requantized;
        m->impl.concurrency = n->impl.concurrency;
        m->impl.colpass = n->impl.colpass;
        m->impl.yolo = n->impl.yolo;
        m->impl.roi = n->impl.roi;
        m->impl.frame = n->impl.frame;
        m->impl.transformer = n->impl.transformer;
        m->impl.recurrent = n->impl.recurrent;
        n->more.push_back(std::move(m));
    }
    if (replicas > 1 && !n->fork) FHIP_CHECK_HIP(hipEventCreateWithFlags(&n->fork, hipEventDisableTiming));
    return FHIP_OK;
}

int fhip_net_set_stream(fhip_net* n, void* stream)
{
    NET_GUARD(n);
    n->impl.stream = (hipStream_t)stream;
    n->impl.drop_graph();
    return FHIP_OK;
}

int fhip_net_get_stream(fhip_net* n, void** stream)
{
    NET_GUARD(n);
    if (!stream) return fail(FHIP_E_BADARG, "null argument");
    *stream = (void*)n->impl.stream;
    return FHIP_OK;
}

int fhip_net_set_fusion(fhip_net* n, int on)
{
    NET_GUARD(n);
    if (n->impl.fused) return fail(FHIP_E_BADARG, "fusion already ran; set it before the first Forward");
    n->impl.fusion = on;
    for (auto& m : n->more) m->impl.fusion = on;
    return FHIP_OK;
}

int fhip_net_set_tuned_selection(fhip_net* n, int on)
{
    NET_GUARD(n);
    n->impl.tuned_selection = on != 0;
    n->impl.shapes_dirty = true;
    for (auto& m : n->more) (void)fhip_net_set_tuned_selection(m.get(), on);
    return FHIP_OK;
}

int fhip_net_set_dilated(fhip_net* n, int on)
{
    NET_GUARD(n);
    if (n->impl.param_loaded) return fail(FHIP_E_BADARG, "set the dilated-convolution switch before LoadParam");
    n->impl.dilated = on != 0;
    for (auto& m : n->more) m->impl.dilated = on != 0;
    return FHIP_OK;
}

int fhip_net_set_extended_layers(fhip_net* n, int on)
{
    NET_GUARD(n);
    if (n->impl.param_loaded) return fail(FHIP_E_BADARG, "set the extended-layers switch before LoadParam");
    n->impl.extended = on != 0;
    for (auto& m : n->more) m->impl.extended = on != 0;
    return FHIP_OK;
}

int fhip_net_set_detection(fhip_net* n, int on)
{
    NET_GUARD(n);
    if (n->impl.param_loaded) return fail(FHIP_E_BADARG, "set the detection-layers switch before LoadParam");
    n->impl.detection = on != 0;
    for (auto& m : n->more) m->impl.detection = on != 0;
    return FHIP_OK;
}

int fhip_net_set_yolo(fhip_net* n, int rows)
{
    NET_GUARD(n);
    if (n->impl.param_loaded) return fail(FHIP_E_BADARG, "set the YOLO-layers switch before LoadParam");
    if (rows < 0 || rows > FHIP_YOLO_MAX_ROWS) return fail(FHIP_E_BADARG, "rows of the YOLO detection top: 0 (off) or 1 .. FHIP_YOLO_MAX_ROWS (1024)");
    n->impl.yolo = rows;
    for (auto& m : n->more) m->impl.yolo = rows;
    return FHIP_OK;
}

int fhip_net_set_roi(fhip_net* n, int on)
{
    NET_GUARD(n);
    if (n->impl.param_loaded) return fail(FHIP_E_BADARG, "set the two-stage-detection-layers switch before LoadParam");
    n->impl.roi = on != 0;
    for (auto& m : n->more) m->impl.roi = on != 0;
    return FHIP_OK;
}

int fhip_net_set_frame(fhip_net* n, int on)
{
    NET_GUARD(n);
    if (n->impl.param_loaded) return fail(FHIP_E_BADARG, "set the framing-layers switch (Padding, Crop, PixelShuffle) before LoadParam");
    n->impl.frame = on != 0;
    for (auto& m : n->more) m->impl.frame = on != 0;
    return FHIP_OK;
}

int fhip_net_set_transformer(fhip_net* n, int on)
{
    NET_GUARD(n);
    if (n->impl.param_loaded) return fail(FHIP_E_BADARG, "set the transformer-layers switch (MemoryData, LayerNorm, GELU, MultiHeadAttention, BinaryOp) before LoadParam");
    n->impl.transformer = on != 0;
    for (auto& m : n->more) m->impl.transformer = on != 0;
    return FHIP_OK;
}

int fhip_net_set_recurrent(fhip_net* n, int on)
{
    NET_GUARD(n);
    if (n->impl.param_loaded) return fail(FHIP_E_BADARG, "set the recurrent-layers switch (LSTM, GRU, RNN) before LoadParam");
    n->impl.recurrent = on != 0;
    for (auto& m : n->more) m->impl.recurrent = on != 0;
    return FHIP_OK;
}

int fhip_net_set_quantized(fhip_net* n, int on)
{
    NET_GUARD(n);
    if (n->impl.param_loaded) return fail(FHIP_E_BADARG, "set the quantized-layers switch before LoadParam");
    n->impl.quantized = on != 0;
    for (auto& m : n->more) m->impl.quantized = on != 0;
    return FHIP_OK;
}

int fhip_net_set_requantized(fhip_net* n, int on)
{
    NET_GUARD(n);
    if (n->impl.param_loaded) return fail(FHIP_E_BADARG, "set the requantized-layers switch before LoadParam");
    n->impl.requantized = on != 0;
    for (auto& m : n->more) m->impl.requantized = on != 0;
    return FHIP_OK;
}

int fhip_net_set_concurrency(fhip_net* n, int on)
{
    NET_GUARD(n);
    n->impl.concurrency = on != 0;
    n->impl.shapes_dirty = true; // re-plan (and drop a captured graph) at the next Forward
    for (auto& m : n->more) (void)fhip_net_set_concurrency(m.get(), on);
    return FHIP_OK;
}

int fhip_net_set_colpass(fhip_net* n, int mode)
{
    NET_GUARD(n);
    if (mode < 0 || mode > 2) return fail(FHIP_E_BADARG, "colpass mode: 0 never, 1 where M is HBM-bound, 2 wherever the library accepts the layer");
    n->impl.colpass = mode;
    n->impl.shapes_dirty = true; // re-plan (and drop a captured graph) at the next Forward
    for (auto& m : n->more) (void)fhip_net_set_colpass(m.get(), mode);
    return FHIP_OK;
}

int fhip_net_set_graph(fhip_net* n, int on)
{
    NET_GUARD(n);
    n->impl.use_graph = on != 0;
    if (!on) n->impl.drop_graph();
    if (on && !n->impl.stream)
    {
        if (!n->impl.owned_stream) FHIP_CHECK_HIP(hipStreamCreateWithFlags(&n->impl.owned_stream, hipStreamNonBlocking));
        n->impl.stream = n->impl.owned_stream;
    }
    for (auto& m : n->more) (void)fhip_net_set_graph(m.get(), on); // the replicas already run on streams of their own
    return FHIP_OK;
}

int fhip_net_load_param_mem(fhip_net* n, const char* text, size_t len)
{
    NET_GUARD(n);
    if (!text) return fail(FHIP_E_BADARG, "null text");
    for (auto& m : n->more)
    {
        const int rc = load_param_text(m->impl, text, len);
        if (rc) return rc;
    }
    return load_param_text(n->impl, text, len);
}

int fhip_net_load_param(fhip_net* n, const char* path)
{
    NET_GUARD(n);
    if (!path) return fail(FHIP_E_BADARG, "null path");
    std::vector<char> buf;
    const int rc = read_file(path, buf);
    if (rc) return rc;
    return fhip_net_load_param_mem(n, buf.data(), buf.size());
}

int fhip_net_load_weights_mem(fhip_net* n, const void* data, size_t len)
{
    NET_GUARD(n);
    if (!data && len) return fail(FHIP_E_BADARG, "null data");
    for (auto& m : n->more)
    {
        const int rc = load_weights_mem(m->impl, data, len);
        if (rc) return rc;
    }
    return load_weights_mem(n->impl, data, len);
}

// The .bin image handed over in DEVICE memory -- the buffer an RCCL broadcast (ncclBroadcast of the model from rank 0)
// delivered on this rank's GPU.  The image is staged through host memory once, because the loaders keep the raw weights on the host
// until Init (BatchNorm / Scale folding into the convolution weights happens there); the caller keeps ownership of `device_data` and
// may free it when the call returns.
int fhip_net_load_weights_device(fhip_net* n, const void* device_data, size_t len)
{
    NET_GUARD(n);
    if (!device_data && len) return fail(FHIP_E_BADARG, "null data");
    std::vector<char> host(len);
    if (len) FHIP_CHECK_HIP(hipMemcpy(host.data(), device_data, len, hipMemcpyDeviceToHost));
    return fhip_net_load_weights_mem(n, host.data(), len);
}

int fhip_net_load_weights(fhip_net* n, const char* path)
{
    NET_GUARD(n);
    if (!path) return fail(FHIP_E_BADARG, "null path");
    std::vector<char> buf;
    const int rc = read_file(path, buf);
    if (rc) return rc;
    return fhip_net_load_weights_mem(n, buf.data(), buf.size());
}

int fhip_net_feed_input(fhip_net* n, const char* blob_name, int num, int c, int h, int w, const float* data, int on_device)
{
    NET_GUARD(n);
    if (!blob_name || !data || num < 1 || c < 1 || h < 1 || w < 1) return fail(FHIP_E_BADARG, "bad argument");
    if (!n->more.empty())
    {
        // deal the images out; a replica left without images (batch < replicas) sits the forward out
        deal(num, (int)n->more.size() + 1, n->share);
        if (on_device) FHIP_CHECK_HIP(hipEventRecord(n->fork, n->impl.stream)); // the caller's data is ordered on the net's stream
        const size_t chw = (size_t)c * h * w;
        size_t first = n->share[0];
        for (size_t r = 0; r < n->more.size(); ++r)
        {
            const int cnt = n->share[r + 1];
            if (cnt > 0)
            {
                if (on_device) FHIP_CHECK_HIP(hipStreamWaitEvent(n->more[r]->impl.stream, n->fork, 0));
                const int rc = fhip_net_feed_input(n->more[r].get(), blob_name, cnt, c, h, w, data + first * chw, on_device);
                if (rc) return rc;
                // join the replica's copy back into the net's stream: whatever the caller enqueues there next (re-using or overwriting
                // the source buffer, a synchronize of the net's stream only) is ordered behind it -- "the caller's stream order is
                // unchanged" holds for FeedInput too
                FHIP_CHECK_HIP(hipEventRecord(n->joins[r], n->more[r]->impl.stream));
                FHIP_CHECK_HIP(hipStreamWaitEvent(n->impl.stream, n->joins[r], 0));
            }
            first += cnt;
        }
        num = n->share[0];
    }
    Blob* b = n->impl.find(blob_name);
    if (!b) return failf(NET_E_IO, "Invalid input blob %s, not found in map.", blob_name);
    if (b->n != num || b->c != c || b->h != h || b->w != w)
    {
        const float* old = b->data;
        const int rc = b->reshape(num, c, h, w);
        if (rc) return rc;
        n->impl.shapes_dirty = true;
        if (old != b->data) n->impl.drop_graph();
    }
    FHIP_CHECK_HIP(hipMemcpyAsync(b->data, data, b->count() * sizeof(float), on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, n->impl.stream));
    return FHIP_OK;
}

int fhip_net_feed_pixels(fhip_net* n, const char* blob_name, int num, const unsigned char* pixels, int type, int w, int h, int target_w,
                         int target_h, const float* mean, const float* norm, int on_device)
{
    NET_GUARD(n);
    int cin, cout;
    if (pixel_channels(type, &cin, &cout)) return fail(FHIP_E_BADARG, "unknown pixel type");
    if (!blob_name || !pixels || num < 1 || w < 1 || h < 1 || target_w < 1 || target_h < 1) return fail(FHIP_E_BADARG, "bad argument");
    if ((w != target_w || h != target_h) && (w < 2 || h < 2)) return fail(FHIP_E_BADARG, "a source 1 pixel wide or high cannot be resized");
    return feed_bytes(n, blob_name, num, pixels, (size_t)h * w * cin, cout, target_w, target_h, on_device,
                      [&](float* out, const unsigned char* px, int cnt, hipStream_t s) {
                          return fhip_pixels_to_float(out, px, cnt, type, w, h, target_w, target_h, mean, norm, s);
                      });
}

int fhip_net_feed_yuv420sp(fhip_net* n, const char* blob_name, int num, const unsigned char* yuv, int w, int h, int target_w, int target_h,
                           int type, int resize_first, const float* mean, const float* norm, int on_device)
{
    NET_GUARD(n);
    int cout;
    if (yuv420sp_check(type, w, h, target_w, target_h, resize_first, &cout)) return FHIP_E_BADARG;
    if (!blob_name || !yuv || num < 1) return fail(FHIP_E_BADARG, "bad argument");
    return feed_bytes(n, blob_name, num, yuv, (size_t)h * w * 3 / 2, cout, target_w, target_h, on_device,
                      [&](float* out, const unsigned char* px, int cnt, hipStream_t s) {
                          return fhip_yuv420sp_to_float(out, px, cnt, type, w, h, target_w, target_h, resize_first, mean, norm, s);
                      });
}

int fhip_net_feed_pixel_images(fhip_net* n, const char* blob_name, int num, const fhip_pixel_image* images, int type, int target_w,
                               int target_h, const float* mean, const float* norm, int on_device)
{
    NET_GUARD(n);
    if (!blob_name) return fail(FHIP_E_BADARG, "bad argument");
    size_t bytes = 0;
    int rc = fhip_pixel_images_plan(images, num, type, target_w, target_h, nullptr, &bytes); // every descriptor checked here
    if (rc) return rc;
    if (!n->impl.find(blob_name)) return failf(NET_E_IO, "Invalid input blob %s, not found in map.", blob_name);
    int cin, cout;
    pixel_channels(type, &cin, &cout);
    // one plan per replica's share (feed_shares deals them the same way), then, from host memory, the ROIs packed dense
    std::vector<int> share;
    deal(num, (int)n->more.size() + 1, share);
    std::vector<size_t> plan_at(share.size(), 0);
    size_t plans = 0;
    for (size_t r = 0, first = 0; r < share.size(); first += share[r++])
    {
        plan_at[r] = plans;
        if (!share[r]) continue;
        rc = fhip_pixel_images_plan(images + first, share[r], type, target_w, target_h, nullptr, &bytes);
        if (rc) return rc;
        plans += round_up_sz(bytes, 16);
    }
    std::vector<size_t> roi_at(on_device ? 0 : num);
    size_t total = round_up_sz(plans, 256);
    for (size_t i = 0; i < roi_at.size(); ++i)
    {
        const fhip_pixel_image& im = images[i];
        const bool whole = im.roi_w == 0 && im.roi_h == 0;
        const size_t pitch = im.stride ? (size_t)im.stride : (size_t)im.w * cin;
        roi_at[i] = total;
        total += (size_t)((whole ? im.h : im.roi_h) - 1) * pitch + (size_t)(whole ? im.w : im.roi_w) * cin; // the ROI's row span
    }
    // the previous feed's plan upload reads n->plans until it has run
    if (n->plans_read) FHIP_CHECK_HIP(hipEventSynchronize(n->plans_read));
    else FHIP_CHECK_HIP(hipEventCreateWithFlags(&n->plans_read, hipEventDisableTiming));
    rc = reserve_staging(n, total);
    if (rc) return rc;
    // host images: one copy per ROI of its rows, from its first byte to its last, pitch kept (one 2-D copy per ROI of only its columns
    // measured 0.7 ms per image: DESIGN.md 9.1); described in the staging buffer as images that are their ROI
    std::vector<fhip_pixel_image> dense(roi_at.size());
    for (size_t i = 0; i < roi_at.size(); ++i)
    {
        const fhip_pixel_image& im = images[i];
        const bool whole = im.roi_w == 0 && im.roi_h == 0;
        const int rx = whole ? 0 : im.roi_x, ry = whole ? 0 : im.roi_y, rw = whole ? im.w : im.roi_w, rh = whole ? im.h : im.roi_h;
        const size_t pitch = im.stride ? (size_t)im.stride : (size_t)im.w * cin;
        FHIP_CHECK_HIP(hipMemcpyAsync(n->staging + roi_at[i], im.data + (size_t)ry * pitch + (size_t)rx * cin, (size_t)(rh - 1) * pitch + (size_t)rw * cin,
                                      hipMemcpyHostToDevice, n->impl.stream));
        dense[i] = fhip_pixel_image{n->staging + roi_at[i], rw, rh, (int)pitch, 0, 0, 0, 0};
    }
    const fhip_pixel_image* planned = on_device ? images : dense.data();
    n->plans.resize(plans);
    for (size_t r = 0, first = 0; r < share.size(); first += share[r++])
    {
        if (!share[r]) continue;
        bytes = plans - plan_at[r];
        rc = fhip_pixel_images_plan(planned + first, share[r], type, target_w, target_h, n->plans.data() + plan_at[r], &bytes);
        if (rc) return rc;
    }
    FHIP_CHECK_HIP(hipMemcpyAsync(n->staging, n->plans.data(), plans, hipMemcpyHostToDevice, n->impl.stream));
    FHIP_CHECK_HIP(hipEventRecord(n->plans_read, n->impl.stream));
    return feed_shares(n, blob_name, num, cout, target_w, target_h, [&](float* out, int first, int, hipStream_t s) {
        size_t r = 0; // the share that starts at `first`
        for (int f = 0; f < first; f += share[r++]) {}
        return fhip_pixels_to_float_images(out, n->plans.data() + plan_at[r], n->staging + plan_at[r], mean, norm, s);
    });
}

int fhip_net_forward(fhip_net* n)
{
    NET_GUARD(n);
    if (n->more.empty()) return forward(n->impl);
    if (n->share.empty()) return failf(NET_E_SHAPE, "no input has been fed");
    // fork: whatever the caller enqueued on the net's stream happens before every replica's forward; join: whatever the caller
    // enqueues next (Extract, the next FeedInput) happens after all of them
    FHIP_CHECK_HIP(hipEventRecord(n->fork, n->impl.stream));
    for (size_t r = 0; r < n->more.size(); ++r)
    {
        if (n->share[r + 1] < 1) continue;
        Net& m = n->more[r]->impl;
        FHIP_CHECK_HIP(hipStreamWaitEvent(m.stream, n->fork, 0));
        const int rc = forward(m);
        if (rc) return rc;
        FHIP_CHECK_HIP(hipEventRecord(n->joins[r], m.stream));
    }
    const int rc = forward(n->impl);
    if (rc) return rc;
    for (size_t r = 0; r < n->more.size(); ++r)
        if (n->share[r + 1] > 0) FHIP_CHECK_HIP(hipStreamWaitEvent(n->impl.stream, n->joins[r], 0));
    return FHIP_OK;
}

int fhip_net_extract(fhip_net* n, const char* blob_name, float** ptr, int* num, int* c, int* h, int* w)
{
    NET_GUARD(n);
    if (!blob_name || !ptr) return fail(FHIP_E_BADARG, "null argument");
    Blob* b = n->impl.find(blob_name);
    if (!b) return failf(NET_E_IO, "Cannot find output blob %s", blob_name);
    if (b->fused_away) return failf(NET_E_IO, "blob %s was fused into its consumer; disable fusion to extract it", blob_name);
    if (b->chained)
        return failf(NET_E_IO, "blob %s exists only as the next layer's transformed input at fusion level 3; use level 2 to extract it", blob_name);
    if (b->q8) return failf(NET_E_TOPOLOGY, "blob %s holds the int8 output of a requantised layer: it has no fp32 values to extract", blob_name);
    if (b->alias) b->data = b->alias->data;
    *ptr = b->data;
    if (num) *num = b->n;
    if (c) *c = b->c;
    if (h) *h = b->h;
    if (w) *w = b->w;
    if (n->more.empty() || n->share.size() < 2 || n->share[1] < 1) return FHIP_OK;
    // the blob lives in one piece per replica: put the pieces together (device-to-device, on the net's stream, after the join)
    size_t total = b->count();
    int images = b->n;
    std::vector<std::pair<float*, size_t>> pieces(1, std::make_pair(b->data, b->count()));
    for (size_t r = 0; r < n->more.size(); ++r)
    {
        if (n->share[r + 1] < 1) continue;
        float* d = nullptr;
        int pn, pc, ph, pw;
        const int rc = fhip_net_extract(n->more[r].get(), blob_name, &d, &pn, &pc, &ph, &pw);
        if (rc) return rc;
        if (pc != b->c || ph != b->h || pw != b->w) return failf(NET_E_SHAPE, "blob %s has different shapes in the sub-batch replicas", blob_name);
        pieces.push_back(std::make_pair(d, (size_t)pn * pc * ph * pw));
        total += pieces.back().second;
        images += pn;
    }
    // The returned pointer stays valid until the next FeedInput with a different shape (like a blob pointer of a plain net): the
    // buffer of a name is only ever re-allocated when that blob's total size grows, which takes a new input shape.
    DeviceVec& g = n->gathered[blob_name];
    if (g.bytes < total * sizeof(float))
    {
        FHIP_CHECK_HIP(hipStreamSynchronize(n->impl.stream)); // earlier gathers of this name may still be in flight
        const int rc = g.resize(total * sizeof(float));
        if (rc) return rc;
    }
    size_t at = 0;
    for (auto& pc_ : pieces)
    {
        if (pc_.first && pc_.second)
            FHIP_CHECK_HIP(hipMemcpyAsync(g.d + at, pc_.first, pc_.second * sizeof(float), hipMemcpyDeviceToDevice, n->impl.stream));
        at += pc_.second;
    }
    *ptr = g.d;
    if (num) *num = images;
    return FHIP_OK;
}

int fhip_net_extract_host(fhip_net* n, const char* blob_name, float* host, size_t capacity)
{
    float* d = nullptr;
    int num, c, h, w;
    const int rc = fhip_net_extract(n, blob_name, &d, &num, &c, &h, &w);
    if (rc) return rc;
    const size_t count = (size_t)num * c * h * w;
    if (!host || capacity < count) return fail(FHIP_E_BADARG, "host buffer too small");
    if (!d) return fail(FHIP_E_BADARG, "blob has no data yet (run Forward first)");
    FHIP_CHECK_HIP(hipMemcpyAsync(host, d, count * sizeof(float), hipMemcpyDeviceToHost, n->impl.stream));
    FHIP_CHECK_HIP(hipStreamSynchronize(n->impl.stream));
    return FHIP_OK;
}

int fhip_net_layer_count(fhip_net* n)
{
    NET_GUARD(n);
    return (int)n->impl.layers.size();
}

int fhip_net_layer_info(fhip_net* n, int index, char* type, char* name, int len, int* algo)
{
    NET_GUARD(n);
    if (index < 0 || index >= (int)n->impl.layers.size()) return fail(FHIP_E_BADARG, "layer index out of range");
    Layer* l = n->impl.layers[index].get();
    if (type && len > 0) snprintf(type, len, "%s", l->type.c_str());
    if (name && len > 0) snprintf(name, len, "%s", l->name.c_str());
    if (algo) *algo = l->algo();
    return FHIP_OK;
}

int fhip_net_layer_conv_param(fhip_net* n, int index, fhip_conv_param* param, int* batch)
{
    NET_GUARD(n);
    if (index < 0 || index >= (int)n->impl.layers.size() || !param) return fail(FHIP_E_BADARG, "layer index out of range");
    Layer* l = n->impl.layers[index].get();
    const fhip_conv_param* cp = l->conv_param();
    if (!cp) return fail(FHIP_E_BADARG, "not a convolution layer");
    *param = *cp;
    if (batch) *batch = l->bottoms.empty() ? 0 : l->bottoms[0]->n;
    return FHIP_OK;
}

int fhip_net_layer_fused_pointwise(fhip_net* n, int index, fhip_conv_param* param, int* one_kernel)
{
    NET_GUARD(n);
    if (index < 0 || index >= (int)n->impl.layers.size() || !param) return fail(FHIP_E_BADARG, "layer index out of range");
    const fhip_conv_param* cp = n->impl.layers[index]->fused_pointwise(one_kernel);
    if (!cp) return fail(FHIP_E_BADARG, "no pointwise convolution was absorbed into this layer");
    *param = *cp;
    return FHIP_OK;
}

int fhip_net_layer_sibling(fhip_net* n, int index, int* state)
{
    NET_GUARD(n);
    if (index < 0 || index >= (int)n->impl.layers.size() || !state) return fail(FHIP_E_BADARG, "layer index out of range");
    *state = n->impl.layers[index]->sibling_state();
    return FHIP_OK;
}

int fhip_net_layer_residual(fhip_net* n, int index, int* state)
{
    NET_GUARD(n);
    if (index < 0 || index >= (int)n->impl.layers.size() || !state) return fail(FHIP_E_BADARG, "layer index out of range");
    *state = n->impl.layers[index]->residual_state();
    return FHIP_OK;
}

int fhip_net_layer_chain(fhip_net* n, int index, int* v_from_previous, int* writes_next_v)
{
    NET_GUARD(n);
    if (index < 0 || index >= (int)n->impl.layers.size() || !v_from_previous || !writes_next_v) return fail(FHIP_E_BADARG, "layer index out of range");
    n->impl.layers[index]->chain_state(v_from_previous, writes_next_v);
    return FHIP_OK;
}

int fhip_net_layer_canvas(fhip_net* n, int index, int* canvas)
{
    NET_GUARD(n);
    if (index < 0 || index >= (int)n->impl.layers.size() || !canvas) return fail(FHIP_E_BADARG, "layer index out of range");
    *canvas = n->impl.layers[index]->canvas_state();
    return FHIP_OK;
}

int fhip_net_layer_colpass(fhip_net* n, int index, int* colpass)
{
    NET_GUARD(n);
    if (index < 0 || index >= (int)n->impl.layers.size() || !colpass) return fail(FHIP_E_BADARG, "layer index out of range");
    *colpass = n->impl.layers[index]->colpass_state();
    return FHIP_OK;
}

int fhip_net_forward_timed(fhip_net* n, float* ms)
{
    NET_GUARD(n);
    if (!ms) return fail(FHIP_E_BADARG, "null argument");
    if (!n->more.empty())
        return fail(FHIP_E_UNSUPPORTED, "per-layer timing of a net with sub-batch replicas: kernels of concurrent replicas share the chip, "
                                        "so their durations are not layer times -- time a net created without fhip_net_set_sub_batches");
    Net& net = n->impl;
    int rc = prepare(net);
    if (rc) return rc;
    const size_t L = net.layers.size();
    std::vector<hipEvent_t> ev(L + 1);
    for (auto& e : ev) FHIP_CHECK_HIP(hipEventCreate(&e));
    FHIP_CHECK_HIP(hipEventRecord(ev[0], net.stream));
    for (size_t i = 0; i < L && rc == 0; ++i)
    {
        rc = net.layers[i]->Forward(net.stream);
        (void)hipEventRecord(ev[i + 1], net.stream);
    }
    (void)hipStreamSynchronize(net.stream);
    if (rc == 0)
        for (size_t i = 0; i < L; ++i) (void)hipEventElapsedTime(&ms[i], ev[i], ev[i + 1]);
    for (auto& e : ev) (void)hipEventDestroy(e);
    return rc;
}

int fhip_net_memory(fhip_net* n, size_t* blob_bytes, size_t* weight_bytes, size_t* arena_bytes)
{
    NET_GUARD(n);
    size_t bb = 0, wb = 0;
    for (auto& kv : n->impl.blobs) bb += kv.second->capacity * sizeof(float);
    for (auto& b : n->impl.shadowed) bb += b->capacity * sizeof(float);
    for (auto& l : n->impl.layers) wb += l->weight_bytes();
    size_t ab = n->impl.arena.bytes;
    for (auto& m : n->more)
    {
        size_t b2 = 0, w2 = 0, a2 = 0;
        (void)fhip_net_memory(m.get(), &b2, &w2, &a2);
        bb += b2;
        wb += w2;
        ab += a2;
    }
    for (auto& kv : n->gathered) bb += kv.second.bytes;
    if (blob_bytes) *blob_bytes = bb;
    if (weight_bytes) *weight_bytes = wb;
    if (arena_bytes) *arena_bytes = ab;
    return FHIP_OK;
}

} // extern "C"
