// net_core.h -- what every layer and pass of the Net runtime stands on: Blob, DeviceVec, Layer, Net, and the graph queries.
#pragma once
#include "net_model.h"

namespace fhip::net
{

// ---- blobs ---------------------------------------------------------------------------------------------------
struct Blob
{
    std::string name;
    int n = 0, c = 0, h = 0, w = 0;
    int dims = 3; // ncnn's Mat::dims: 3 = (c, h, w), 2 = (h, w) with c = 1, 1 = (w) with c = h = 1; only the layers of net_detect.h set or read it
    float* data = nullptr;
    size_t capacity = 0;   // floats owned
    Blob* alias = nullptr; // data is another blob's
    bool fused_away = false;
    bool chained = false; // fusion level 3: lives only as the next layer's Winograd-domain input (plan_chains); shape kept, no storage
    bool q8 = false;      // a q8 tensor (feather_q8.h: signed char [n][ceil(c / 16)][h][w][16]) instead of fp32 NCHW; reshape_all sets it before the producer's Reshape

    size_t count() const { return (size_t)n * c * h * w; }
    size_t q8_bytes() const { return (size_t)n * ((c + 15) / 16) * h * w * 16; }
    size_t floats() const { return q8 ? q8_bytes() / 4 : count(); } // the storage, in floats
    int reshape(int n_, int c_, int h_, int w_)
    {
        n = n_;
        c = c_;
        h = h_;
        w = w_;
        dims = 3;
        alias = nullptr;
        // a blob the previous plan chained away has no storage and, as a rule, will have none after this Reshape either: plan_chains
        // allocates it afterwards if the new shapes un-chain it (no device malloc + free per chained blob and shape change)
        if (chained && !data) return 0;
        if (floats() > capacity)
        {
            if (data && capacity) (void)hipFree(data);
            data = nullptr;
            capacity = 0;
            FHIP_CHECK_HIP(hipMalloc((void**)&data, floats() * sizeof(float)));
            capacity = floats();
        }
        return 0;
    }
    void drop_storage()
    {
        if (data && capacity) (void)hipFree(data);
        data = nullptr;
        capacity = 0;
    }
    void share(Blob* src)
    {
        n = src->n;
        c = src->c;
        h = src->h;
        w = src->w;
        dims = src->dims;
        if (data && capacity) (void)hipFree(data);
        capacity = 0;
        alias = src;
        data = src->data;
    }
    ~Blob()
    {
        if (data && capacity) (void)hipFree(data);
    }
};

struct DeviceVec
{
    float* d = nullptr;
    size_t bytes = 0;
    int upload(const float* h, size_t count, hipStream_t s)
    {
        if (bytes != count * 4)
        {
            release();
            FHIP_CHECK_HIP(hipMalloc((void**)&d, std::max<size_t>(count, 1) * 4));
            bytes = count * 4;
        }
        if (count) FHIP_CHECK_HIP(hipMemcpyAsync(d, h, count * 4, hipMemcpyHostToDevice, s));
        return 0;
    }
    int resize(size_t nbytes)
    {
        if (bytes != nbytes)
        {
            release();
            FHIP_CHECK_HIP(hipMalloc((void**)&d, std::max<size_t>(nbytes, 4)));
            bytes = nbytes;
        }
        return 0;
    }
    void release()
    {
        if (d) (void)hipFree(d);
        d = nullptr;
        bytes = 0;
    }
    ~DeviceVec() { release(); }
};

struct Net;
struct ConvLayer;
struct PoolingLayer;
struct AffineLayer;
struct EltwiseLayer;
struct InterpLayer;

// ---- layers (reference layer.h:28-86) -------------------------------------------------------------------------
struct Layer
{
    std::string type, name;
    std::vector<Blob*> bottoms, tops;
    Net* net = nullptr;

    virtual ~Layer() {}
    // What a layer is, said by the layer: the passes ask here instead of comparing `type` and casting.  Each as_x() is the object
    // itself in the classes derived from X (a collapsed squeeze-and-excitation block is a PoolingLayer, a pointwise layer a depthwise
    // layer adopted is not in the list at all), so it answers what `type == "..."` plus static_cast answered.
    virtual bool needs_weights() const { return false; } // LoadWeights reads the .bin: Forward refuses the net until a weight file is loaded
    virtual ConvLayer* as_conv() { return nullptr; }         // Convolution, ConvolutionDepthWise
    virtual PoolingLayer* as_pooling() { return nullptr; }   // Pooling
    virtual AffineLayer* as_affine() { return nullptr; }     // BatchNorm, Scale (a gated Scale too: see AffineLayer::gated)
    virtual EltwiseLayer* as_eltwise() { return nullptr; }   // Eltwise
    virtual InterpLayer* as_interp() { return nullptr; }     // Interp
    virtual const float* relu_slope() const { return nullptr; } // ReLU: its slope
    virtual const int* zero_pad_margins() const { return nullptr; } // Padding that only zero-pads the plane: its (top, bottom, left, right)
    // q8 blobs (Blob::q8, the int8 activation between two int8 layers): a layer that can read one says so, every other layer that meets
    // one is refused by reshape_all; writes_q8() is asked there too, after the layer's bottoms are settled and before its Reshape
    virtual bool reads_q8() const { return false; }
    virtual bool writes_q8() const { return false; }
    // The one form of a call into a side library: FHIP_E_UNSUPPORTED where the library is missing (side_api has set the message), else
    // the call's code -- `code` in its place, for an entry point that only says yes or no -- with the library's message behind the
    // layer's name and `prefix`.
    template <class Api, class Call>
    int side(const Api* api, const Call& call, int code = 0, const char* prefix = "") const
    {
        if (!api) return FHIP_E_UNSUPPORTED;
        const int rc = call(api);
        return rc ? failf(code ? code : rc, "layer %s: %s%s", name.c_str(), prefix, api->last_error()) : 0;
    }
    virtual int LoadParam(const ParamDict&) { return 0; }
    virtual int LoadWeights(ModelBin&) { return 0; }
    // default (layer.cpp:103-114): one bottom, one top of the same shape
    virtual int Reshape()
    {
        if (tops.size() != 1 || bottoms.size() != 1) return failf(NET_E_BASE_RESHAPE, "layer %s: base Reshape needs 1 bottom and 1 top", name.c_str());
        return tops[0]->reshape(bottoms[0]->n, bottoms[0]->c, bottoms[0]->h, bottoms[0]->w);
    }
    int reshape_with(const void* side_library) { return side_library ? Layer::Reshape() : FHIP_E_UNSUPPORTED; } // (message set by side_api)
    virtual int Init(hipStream_t) { return 0; }
    virtual int Forward(hipStream_t) = 0;
    virtual int Fuse(Layer*, int /*level*/) { return 0; }
    virtual size_t weight_bytes() const { return 0; }
    virtual size_t arena_bytes() const { return 0; }
    virtual int algo() const { return -1; }
    virtual const fhip_conv_param* conv_param() const { return nullptr; }
    virtual const fhip_conv_param* fused_pointwise(int*) const { return nullptr; } // the 1x1 convolution a depthwise layer absorbed
    virtual void chain_state(int* v_from_previous, int* writes_next_v) const { *v_from_previous = *writes_next_v = 0; }
    virtual int canvas_state() const { return 0; }
    virtual int colpass_state() const { return 0; }
    virtual int sibling_state() const { return 0; } // 1: launches the GEMM that also computes the NEXT layer; 2: computed by the layer before
    virtual int residual_state() const { return 0; } // 1: an Eltwise SUM operand is added in this layer's GEMM epilogue; 2: absorbed, added by a separate launch
};

// A ReLU layer without a slope: the only ReLU the fused epilogues of the convolution, deconvolution, InnerProduct, affine and Eltwise
// layers compute.  A leaky one (ncnn's `ReLU 0=slope`) stays a layer of its own behind them.
static bool is_plain_relu(const Layer* l)
{
    const float* slope = l->relu_slope();
    return slope && *slope == 0.f;
}

struct Net
{
    std::vector<std::unique_ptr<Layer>> layers;
    std::map<std::string, std::unique_ptr<Blob>> blobs;
    // Blobs whose NAME was taken over by a later top (in-place style files: `ReLU r 1 1 conv1 conv1`, or two layers with the
    // same top).  The reference leaks the old Blob and replaces the map entry (net.cpp:135-139), so earlier layers keep
    // using it; here it stays owned, the name resolves to the newest blob exactly like the reference's blob_map.
    std::vector<std::unique_ptr<Blob>> shadowed;
    hipStream_t stream = nullptr;
    int fusion = 1;
    bool use_graph = false;
    bool tuned_selection = false; // fhip_conv_select_algo_tuned instead of the reference's SelectAlgo rule
    bool dilated = false;         // fhip_net_set_dilated: a Convolution with dilation > 1 is loaded (libfeather_atrous.so) instead of refused
    bool extended = false;        // fhip_net_set_extended_layers: Interp, HardSwish (libfeather_resample.so) and LRN (libfeather_lrn.so) are loaded instead of refused
    bool quantized = false;       // fhip_net_set_quantized: Convolution / InnerProduct layers with int8 weights (8=int8_scale_term) are loaded (libfeather_qconv.so) instead of refused
    bool detection = false;       // fhip_net_set_detection: the SSD head's layers (net_detect.h, libfeather_detect.so) are loaded instead of refused, Concat and Softmax know a blob's rank
    bool requantized = false;     // fhip_net_set_requantized: an int8 Convolution with int8_scale_term 101 .. 200 (requantised int8 output) is loaded (libfeather_q8.so) instead of refused
    int yolo = 0;                 // fhip_net_set_yolo: > 0: Reorg, YoloDetectionOutput and Yolov3DetectionOutput (net_yolo.h, libfeather_yolo.so) are loaded instead of refused; the rows of the detection top
    bool roi = false;             // fhip_net_set_roi: Proposal, ROIPooling, ROIAlign and PSROIPooling (net_roi.h, libfeather_roi.so) are loaded instead of refused
    bool frame = false;           // fhip_net_set_frame: Padding, Crop and PixelShuffle (net_frame.h, libfeather_frame.so) are loaded instead of refused
    bool transformer = false;     // fhip_net_set_transformer: MemoryData, LayerNorm, GELU, MultiHeadAttention, the element-wise BinaryOp and the token-wise InnerProduct (net_attn.h, libfeather_attn.so) are loaded instead of refused
    bool recurrent = false;       // fhip_net_set_recurrent: LSTM, GRU and RNN (net_rnn.h, libfeather_rnn.so) are loaded instead of refused
    int colpass = 1;              // fhip_net_set_colpass: chained 64-input-channel Winograd layers through libfeather_colpass.so -- 0 never, 1 where M is HBM-bound, 2 wherever accepted
    bool param_loaded = false, weights_loaded = false, fused = false, initialized = false, shapes_dirty = true;
    DeviceVec arena;
    // fusion level 3 (plan_chains): runs of Winograd layers hand their transformed input from one to the next; the arena then holds two V
    // slots (layers at even / odd positions of a run) and M
    size_t chain_slot[2] = {0, 0}, chain_m = 0;
    hipGraphExec_t graph_exec = nullptr;
    hipStream_t owned_stream = nullptr; // graph capture is not allowed on the NULL stream
    // Branch concurrency (fhip_net_set_concurrency): a convolution that needs no scratch arena and whose output is consumed
    // only further down the layer list (ResNet's projection shortcut, SqueezeNet's expand1x1) runs on a second stream while the
    // main stream continues with the layers in between; fork / join are events, so the pattern is hipGraph-capturable.
    bool concurrency = false;
    hipStream_t side_stream = nullptr;
    std::vector<hipEvent_t> events;        // [2 * pair]: fork, join
    std::vector<int> side;                 // per layer: its event pair, or -1 (runs on the main stream)
    std::vector<std::vector<int>> waits;   // per layer: pairs whose join event the main stream waits for first

    ~Net()
    {
        drop_graph();
        for (hipEvent_t e : events) (void)hipEventDestroy(e);
        if (side_stream) (void)hipStreamDestroy(side_stream);
        if (owned_stream) (void)hipStreamDestroy(owned_stream);
    }
    void drop_graph()
    {
        if (graph_exec) (void)hipGraphExecDestroy(graph_exec);
        graph_exec = nullptr;
    }
    Blob* find(const std::string& n)
    {
        auto it = blobs.find(n);
        return it == blobs.end() ? nullptr : it->second.get();
    }
};

// ---- graph queries: who reads a blob --------------------------------------------------------------------------------------------------
// readers(): how many bottoms of the layers [from_layer, end) are `b` -- with through_alias also those whose data is b's (a Split or
// Dropout top, Blob::alias) -- and the index of the last such layer.  Every pass asks here; each keeps the scope and the match it had
// when it scanned by hand, and what is known about them is this:
//   * Blob::alias is set only by Reshape (Blob::share) and cleared by Blob::reshape.  fuse_layers and the collapse passes it calls run
//     once, before the first Reshape of any layer, so every alias is null there and the exact match is the alias-aware one.  plan_chains
//     and plan_concurrency run after Reshape and need through_alias: a Split top is another reader of the blob it shares.
//   * a reader never precedes its producer: load_param_text resolves a layer's bottoms before it creates its tops, and the passes that
//     move a layer (collapse_gate_blocks, collapse_upsample_adds) move it down to its chain's last place, behind every producer of what
//     it reads.  So for a top of layer i, from_layer = i + 1 counts what from_layer = 0 counts; the passes that said "after i" still do.
struct Readers
{
    int count = 0, last = -1;
    int sole() const { return count == 1 ? last : -1; } // the index of the only layer that reads the blob (once), or -1
};

static Readers readers(const Net& net, const Blob* b, size_t from_layer = 0, bool through_alias = false)
{
    Readers r;
    for (size_t j = from_layer; j < net.layers.size(); ++j)
        for (const Blob* x : net.layers[j]->bottoms)
            if (x == b || (through_alias && x->alias == b))
            {
                ++r.count;
                r.last = (int)j;
            }
    return r;
}

// The tail three fusions absorb behind what they produce (collapse_gate_blocks, collapse_upsample_adds, the residual add of fuse_layers):
//
//   b -> Eltwise SUM (two bottoms, no coefficients) with ANOTHER blob [-> plain ReLU that alone reads the sum]
//
// `sum` is the layer that alone reads b (the caller has found it, in its own scope).  Yields the other operand, the blob the tail ends in,
// the blobs inside it (b, and the sum's top where a ReLU layer follows) and the tail's last layer.  Conditions of one fusion alone -- the
// other operand is produced earlier, the tail runs down the list -- stay with that fusion.
struct SumTail
{
    Blob *other = nullptr, *sum_top = nullptr, *top = nullptr;
    std::vector<Blob*> inner;
    int sum = -1, relu_layer = -1, last = -1; // relu_layer: the ReLU LAYER behind the sum, or -1 (none, or the sum has absorbed it: relu)
    bool relu = false;
};

static bool sum_tail(const Net& net, Blob* b, int sum, SumTail& t);

} // namespace fhip::net
