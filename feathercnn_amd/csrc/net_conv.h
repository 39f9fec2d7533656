// net_conv.h -- the convolution layer of the Net runtime and what it shares with the InnerProduct and Deconvolution layers: the fold of a
// BatchNorm / Scale (AffineFold), the one weight staging sequence (stage_weights, BuiltFor), the life cycles of the side-library convolutions
// (SideConv, QuantRoute).  AffineFold::absorb and ConvLayer::Fuse are defined in net_layers.h, where AffineLayer and PoolingLayer are complete.
#pragma once
#include "net_core.h"

namespace fhip::net
{

// A BatchNorm / Scale folded into the convolution or deconvolution before it (fusion level 2): y = y * mul[k] + add[k] per output
// channel k, applied to the filters and the bias at Init.  K is the caller's business: the layers count their channels differently.
struct AffineFold
{
    std::vector<float> mul, add;
    bool empty() const { return mul.empty(); }
    // composes nx behind what is folded already; false, with nothing changed, if nx is no plain affine map over K channels
    bool absorb(const AffineLayer& nx, int K);
    // w = [K][...] filters, b = K biases or none (then a zero bias is created); does nothing while no layer was absorbed
    void apply(std::vector<float>& w, std::vector<float>& b, int K) const
    {
        if (mul.empty()) return;
        const size_t per = w.size() / K;
        if (b.empty()) b.assign(K, 0.f);
        for (int k = 0; k < K; ++k)
        {
            for (size_t i = 0; i < per; ++i) w[k * per + i] *= mul[k];
            b[k] = b[k] * mul[k] + add[k];
        }
    }
};

// What a packed weight buffer was built for: the route or algorithm, the layout (fhip_conv_packed_layout: a 1x1 layer's streamed image and its
// InnerProduct image have the same size) and the byte count.  Init packs again where it differs from what the layer runs now; LoadWeights
// assigns a fresh one, which equals nothing a layer asks for (no algorithm or route code is -2): never packed before the first Reshape.
struct BuiltFor
{
    int algo = -2, layout = -1;
    size_t bytes = 0;
    bool done() const { return algo != -2; }
    bool operator==(const BuiltFor& o) const { return algo == o.algo && layout == o.layout && bytes == o.bytes; }
};

// The one weight staging sequence of Init: host weights `w` -> a raw device copy -> `packed` through the caller's pack(raw) -> the bias `b`
// (where the layer has one) -> one stream synchronize, after which the raw copy and the caller's host copies may go.
template <class T, class Pack>
static int stage_weights(const std::vector<T>& w, DeviceVec& packed, size_t packed_bytes, const std::vector<float>* b, DeviceVec& bias, hipStream_t s, const Pack& pack)
{
    DeviceVec raw;
    int rc = raw.resize(w.size() * sizeof(T));
    if (rc) return rc;
    if (!w.empty()) FHIP_CHECK_HIP(hipMemcpyAsync(raw.d, w.data(), raw.bytes, hipMemcpyHostToDevice, s));
    if ((rc = packed.resize(packed_bytes))) return rc;
    if ((rc = pack(reinterpret_cast<const T*>(raw.d)))) return rc;
    if (b && (rc = bias.upload(b->data(), b->size(), s))) return rc;
    FHIP_CHECK_HIP(hipStreamSynchronize(s));
    return 0;
}

// The same on the main library (a convolution on route `algo`, an InnerProduct on the implicit GEMM)
static int init_main(const fhip_conv_param& p, int algo, const std::vector<float>& w, const std::vector<float>& b, DeviceVec& packed, size_t packed_bytes, DeviceVec& bias, hipStream_t s)
{
    return stage_weights(w, packed, packed_bytes, p.bias_term ? &b : nullptr, bias, s, [&](const float* raw) { return fhip_conv_init(&p, algo, packed.d, raw, s); });
}

// The geometry a side library's param shares with fhip_conv_param; what is the route's own (dilation, int8_scale_term, who assigns
// output_h / output_w) stays with the caller.
template <class Param>
static void copy_geometry(Param& a, const fhip_conv_param& p)
{
    a.output_channels = p.output_channels, a.input_channels = p.input_channels, a.input_h = p.input_h, a.input_w = p.input_w;
    a.kernel_h = p.kernel_h, a.kernel_w = p.kernel_w, a.stride_h = p.stride_h, a.stride_w = p.stride_w;
    a.pad_left = p.pad_left, a.pad_bottom = p.pad_bottom, a.pad_right = p.pad_right, a.pad_top = p.pad_top;
    a.group = p.group, a.bias_term = p.bias_term, a.activation = p.activation;
}

// The life cycle of a convolution that runs through a side library -- grouped (GconvApi on fhip_conv_param), dilated (AtrousApi on
// fhip_atrous_param), transposed (DeconvApi on fhip_deconv_param) -- once.  The layer decides that it takes the route and keeps the
// library's param `p`; its own checks (the bottom's channels, an empty output) stay in front of these calls.
template <class Api, class Param>
struct SideConv
{
    // the tail of Reshape, with the input size in `p`: the library's output size where it has its own rule (else the caller has set it),
    // its verdict on the geometry, the top, the scratch and packed sizes
    template <bool Assign>
    static int reshape(Layer* l, const Api* api, Param& p, const char* refusal, size_t* buffer_bytes, size_t* packed_bytes)
    {
        if (!api) return FHIP_E_UNSUPPORTED; // message set by side_api
        const Blob* b = l->bottoms[0];
        int rc;
        if constexpr (Assign)
            if ((rc = l->side(api, [&](const Api* a) { return a->assign_output_dim(&p); }, NET_E_SHAPE))) return rc;
        if ((rc = l->side(api, [&](const Api* a) { return a->supported(&p) != 1; }, FHIP_E_UNSUPPORTED, refusal))) return rc;
        if ((rc = l->tops[0]->reshape(b->n, p.output_channels, p.output_h, p.output_w))) return rc;
        return l->side(api, [&](const Api* a) { return a->get_buffer_size(&p, b->n, buffer_bytes, packed_bytes); });
    }
    // Init: filters `w` and bias `b` with the layer's fold applied -> the library's packed form and the bias on the device
    static int init(Layer* l, const Api* api, const Param& p, const std::vector<float>& w, const std::vector<float>& b, DeviceVec& packed,
                    size_t packed_bytes, DeviceVec& bias, hipStream_t s)
    {
        if (!api) return FHIP_E_UNSUPPORTED;
        return stage_weights(w, packed, packed_bytes, p.bias_term ? &b : nullptr, bias, s,
                             [&](const float* raw) { return l->side(api, [&](const Api* a) { return a->init(&p, packed.d, raw, s); }); });
    }
    static int forward(const Layer* l, const Api* api, const Param& p, const DeviceVec& packed, const DeviceVec& bias, hipStream_t s)
    {
        return l->side(api, [&](const Api* a) {
            return a->forward(&p, l->bottoms[0]->n, l->tops[0]->data, l->bottoms[0]->data, packed.d, nullptr, p.bias_term ? bias.d : nullptr, s);
        });
    }
};

// The int8 side of a Convolution / ConvolutionDepthWise / InnerProduct layer of a net with fhip_net_set_quantized: it runs through
// libfeather_qconv.so (qconv_api) with route code FHIP_NET_ROUTE_QCONV.  Init and Forward do not fit SideConv (int8 weights, the
// dequantisation scales and the input scale ride along), so those calls stand here, once for both layer types.  The layer fills `q`
// at Reshape; a BatchNorm / Scale fold goes into d[] and the bias as feather_qconv.h defines it, never into the weights.
// A layer whose input or output is a q8 blob (Blob::q8; the output of a layer with int8_scale_term 101 .. 200 in a net with
// fhip_net_set_requantized is one) makes the same calls on libfeather_q8.so (q8_api) with `q8`, which is `q` plus the two forms; the route
// code stays FHIP_NET_ROUTE_QCONV.
struct QuantRoute
{
    fhip_qconv_param q = {};
    fhip_q8_param q8 = {};
    bool on_q8 = false; // this shape runs on libfeather_q8.so (Reshape)
    int scale_term = 0;
    std::vector<signed char> w;
    std::vector<float> s_w, b;
    float s_in = 0.f, s_out = 0.f;
    DeviceVec packed, d, bias;
    size_t packed_bytes = 0;
    BuiltFor built;

    // ncnn's param 8 of the layer, 0 where the file does not set it
    int read_scale_term(const ParamDict& pd) { return scale_term = pd.get(8, 0); }
    bool requant() const { return scale_term > 100; } // the output is a q8 blob
    // the .bin of a quantised layer: int8-tagged weights, the bias, K weight scales, one input scale (the last three raw fp32); behind them
    // the output scale of a requantised layer
    int load(const Layer* l, ModelBin& mb, size_t wsize, int K, bool bias_term)
    {
        built = BuiltFor();
        int rc = mb.load_int8(wsize, w);
        if (rc) return rc;
        if (bias_term && (rc = mb.load(K, 1, b))) return rc;
        if ((rc = mb.load(K, 1, s_w))) return rc;
        std::vector<float> one;
        if ((rc = mb.load(1, 1, one))) return rc;
        s_in = one[0];
        if (!std::isfinite(s_in) || !(s_in > 0.f)) return failf(NET_E_SHAPE, "layer %s: the int8 input scale must be finite and > 0", l->name.c_str());
        for (float v : s_w)
            if (!std::isfinite(v) || v < 0.f) return failf(NET_E_SHAPE, "layer %s: an int8 weight scale is not finite or is negative", l->name.c_str());
        if (!requant()) return 0;
        if ((rc = mb.load(1, 1, one))) return rc;
        s_out = one[0];
        if (!std::isfinite(s_out) || !(s_out > 0.f)) return failf(NET_E_SHAPE, "layer %s: the int8 output scale must be finite and > 0", l->name.c_str());
        return 0;
    }
    // the tail of Reshape, with the geometry and the input size in `q`: SideConv's, on the library's own rule for the output size
    int reshape(Layer* l)
    {
        q.dilation_h = q.dilation_w = 1;
        q.int8_scale_term = scale_term;
        size_t scratch = 0;
        on_q8 = requant() || l->bottoms[0]->q8;
        if (!on_q8) return SideConv<QconvApi, fhip_qconv_param>::reshape<true>(l, qconv_api(), q, "int8 convolution refused: ", &scratch, &packed_bytes);
        static_assert(sizeof(fhip_q8_param) == sizeof(fhip_qconv_param) + 2 * sizeof(int), "fhip_q8_param is fhip_qconv_param and the two forms");
        memcpy(&q8, &q, sizeof(q));
        q8.input_int8 = l->bottoms[0]->q8 ? 1 : 0;
        q8.output_int8 = requant() ? 1 : 0;
        const int rc = SideConv<Q8Api, fhip_q8_param>::reshape<true>(l, q8_api(), q8, "int8 convolution refused: ", &scratch, &packed_bytes);
        q.output_h = q8.output_h, q.output_w = q8.output_w;
        return rc;
    }
    // what the packed weights were built for: the library and the forms pick the layout
    int layout() const { return on_q8 ? 1 + q8.input_int8 + 2 * q8.output_int8 : 0; }
    int init(Layer* l, const AffineFold& fold, hipStream_t s)
    {
        const BuiltFor want{FHIP_NET_ROUTE_QCONV, layout(), packed_bytes};
        if (built == want) return 0;
        const QconvApi* api = on_q8 ? nullptr : qconv_api();
        const Q8Api* api8 = on_q8 ? q8_api() : nullptr;
        if (!api && !api8) return FHIP_E_UNSUPPORTED;
        const int K = q.output_channels;
        std::vector<float> dq(K), bq = b;
        int rc = on_q8 ? l->side(api8, [&](const Q8Api* a) { return a->dequant_scales(dq.data(), s_w.data(), K, s_in); })
                       : l->side(api, [&](const QconvApi* a) { return a->dequant_scales(dq.data(), s_w.data(), K, s_in); });
        if (rc) return rc;
        if (!fold.empty())
        {
            if (bq.empty()) bq.assign(K, 0.f);
            for (int k = 0; k < K; ++k)
            {
                dq[k] = dq[k] * fold.mul[k];
                const float scaled = bq[k] * fold.mul[k]; // rounded before the sum: no contraction
                bq[k] = scaled + fold.add[k];
            }
            q.bias_term = q8.bias_term = 1;
        }
        // the raw copy is int8; d[] goes up behind the pack call, in front of the bias
        rc = stage_weights(w, packed, packed_bytes, q.bias_term ? &bq : nullptr, bias, s, [&](const signed char* raw) {
            const int e = on_q8 ? l->side(api8, [&](const Q8Api* a) { return a->init(&q8, packed.d, raw, s); })
                                : l->side(api, [&](const QconvApi* a) { return a->init(&q, packed.d, raw, s); });
            return e ? e : d.upload(dq.data(), dq.size(), s);
        });
        if (!rc) built = want;
        return rc;
    }
    int forward(const Layer* l, hipStream_t s) const
    {
        if (on_q8)
            return l->side(q8_api(), [&](const Q8Api* a) {
                return a->forward(&q8, l->bottoms[0]->n, l->tops[0]->data, l->bottoms[0]->data, packed.d, nullptr, d.d, q8.bias_term ? bias.d : nullptr, s_in, s_out, s);
            });
        return l->side(qconv_api(), [&](const QconvApi* a) {
            return a->forward(&q, l->bottoms[0]->n, l->tops[0]->data, l->bottoms[0]->data, packed.d, nullptr, d.d, q.bias_term ? bias.d : nullptr, s_in, s);
        });
    }
    size_t bytes() const { return packed.bytes + d.bytes + bias.bytes; }
};

// Which library runs a convolution layer, decided once by LoadParam: the main one, or a side route -- libfeather_gconv.so (1 < group < input
// channels), libfeather_atrous.so (dilation > 1 in a net with fhip_net_set_dilated, whatever the group), libfeather_qconv.so
// (8=int8_scale_term in a net with fhip_net_set_quantized; group 1 or depthwise).  A side route reports its route code as algo().
enum ConvRoute { ROUTE_MAIN, ROUTE_GROUPED, ROUTE_DILATED, ROUTE_INT8 };
static const int ROUTE_CODE[] = {-1, FHIP_NET_ROUTE_GCONV, FHIP_NET_ROUTE_ATROUS, FHIP_NET_ROUTE_QCONV};

enum ConvClaim { CLAIM_POOL = 1, CLAIM_RESIDUAL = 2, CLAIM_PAIR = 4, CLAIM_CHAIN = 8, CLAIM_HEAD = 16, CLAIM_SIBLING = 32 }; // ConvLayer::claims

// The state of a ConvLayer by its writer; DESIGN.md ("ConvLayer's state") has the table of who resets and reads each.
// What Fuse / FuseResidual absorbed (fusion level 2, once); Reshape decides how each runs at the current shape (the *_fast flags).
struct ConvEpilogues
{
    bool fuse_pool = false, pool_fast = false; // a 2x2 / stride-2 max pooling: in the route's kernel, else conv -> pre_pool -> fhip_pooling
    fhip_pool_param poolq = {};
    DeviceVec pre_pool;
    Blob* residual = nullptr; // an Eltwise SUM (+ReLU) with an earlier blob: in the GEMM epilogue, else by fhip_add on the top
    bool res_fast = false;
    std::unique_ptr<ConvLayer> pw; // the 1x1 layer this 3x3 depthwise layer adopted: ONE kernel, else dw -> `mid` -> pw
    bool pair_fast = false;
    DeviceVec mid;
};

// Fusion level 3, written by plan_chains alone after every Reshape (see there for the rules).
struct ChainPlan
{
    ConvLayer* next = nullptr; // this Winograd layer's output leaves as `next`'s transformed input
    bool in = false;           // the input arrives already transformed
    int pos = 0;               // position in the run (picks the V slot)
    size_t bytes = 0;          // arena the run needs (reported instead of buffer_bytes)
    bool canvas = false;       // V and M hold 2x2 image canvases (feather_canvas.h): the tile GEMM runs on canvas_p at a quarter of the batch
    fhip_conv_param canvas_p = {};
    fhip_winograd_plan run_plan = {}; // the plan this chained layer runs with (plain or canvas)
    bool colpass = false;             // tile GEMM and boundary run through libfeather_colpass.so: M holds 48 column-passed planes (feather_colpass.h)
    ConvLayer* head_of = nullptr;     // on a first layer: the consumer that computes it inside its input transform (this layer launches nothing)
    ConvLayer* head = nullptr;        // on that consumer: the first layer

    void reset() { *this = ChainPlan(); }
    bool runs() const { return in || next || head; } // the layer launches as part of a run
    static void link(ConvLayer* a, ConvLayer* b);
    static void absorb_first(ConvLayer* first, ConvLayer* consumer);
    void to_canvas(const fhip_conv_param& p, int n) { canvas = fhip_winograd_f63_canvas_param(&p, n, &canvas_p) == FHIP_OK; } // (the scan has asked)
    int plan_run(const fhip_conv_param& p, int n) { return fhip_winograd_f63_plan_canvas(&p, n, canvas ? 2 : 1, &run_plan); }
    void arena(size_t run_bytes) { bytes = run_bytes; }
};

// Fusion level 2, written by plan_siblings alone after every Reshape: `sib` (on the first 1x1 layer of a pair) = the NEXT layer of the list,
// `sib_of` (on that layer, which launches nothing) = the first.  The stacked filters are staged by the first layer's Init.
struct SiblingPlan
{
    ConvLayer *sib = nullptr, *sib_of = nullptr;
    ConvLayer* packed_for = nullptr; // the partner packed / bias were built with
    DeviceVec packed, bias;
    bool has_bias = false;

    void reset() { sib = sib_of = nullptr; } // the stacked copy outlives a re-plan that keeps the pair
    static void pair(ConvLayer* a, ConvLayer* b);
    // a layer the new plan leaves without a partner keeps no stacked copy (the layers' own packed weights stay: they are what the pair
    // falls back to, and what Extract-driven level changes run)
    void unpaired()
    {
        if (!packed.bytes) return;
        packed.release();
        bias.release();
        packed_for = nullptr;
    }
};

// feather::ConvLayer, layers/conv_layer.h:26-193 (also registered as ConvolutionDepthWise, layer_factory.cpp)
struct ConvLayer : Layer
{
    typedef SideConv<GconvApi, fhip_conv_param> Grouped;
    typedef SideConv<AtrousApi, fhip_atrous_param> Dilated;
    fhip_conv_param p = {};
    ConvRoute route = ROUTE_MAIN;
    int algo_ = -1, layout = 0; // the main library's algorithm and packed layout at the current shape (Reshape)
    int dilation_h = 1, dilation_w = 1;
    fhip_atrous_param dilated = {}; // the dilated route's param, filled from p at every Reshape (Init adds the bias a fold created)
    QuantRoute qr;
    std::vector<float> w_host, b_host;
    AffineFold fold; // folded BatchNorm/Scale (fusion level 2)
    DeviceVec packed, bias;
    DeviceVec first_raw; // a first_candidate()'s filters as loaded, for the layer that computes it (ChainPlan::head)
    BuiltFor built;
    size_t buffer_bytes = 0, packed_bytes = 0;
    ConvEpilogues ep;
    ChainPlan chain;
    SiblingPlan sibs;

    bool needs_weights() const override { return true; }
    ConvLayer* as_conv() override { return this; }
    bool reads_q8() const override { return route == ROUTE_INT8; }
    bool writes_q8() const override { return route == ROUTE_INT8 && qr.requant(); }
    bool first_candidate() const
    {
        return p.kernel_h == 3 && p.kernel_w == 3 && p.stride_h == 1 && p.stride_w == 1 && p.group == 1 && p.input_channels >= 2 && p.input_channels <= 4 && p.pad_left == 1 &&
               p.pad_right == 1 && p.pad_top == 1 && p.pad_bottom == 1;
    }
    // p.output_channels counts the whole layer, its filters are [K][C / group][kh][kw]
    bool whole_k() const { return route != ROUTE_MAIN; }
    // a side route: ReLU and affine epilogues only, every other fusion and plan declines the layer
    bool side_epilogues_only() const { return route != ROUTE_MAIN; }
    // the channels a bias or a fold counts (conv_layer.h:69-75 leaves a depthwise layer's K / group in p.output_channels)
    int bias_channels() const { return !whole_k() && p.group == p.input_channels ? p.input_channels : p.output_channels; }
    int claims() const
    {
        return (ep.fuse_pool ? CLAIM_POOL : 0) | (ep.residual ? CLAIM_RESIDUAL : 0) | (ep.pw ? CLAIM_PAIR : 0) | (chain.in || chain.next ? CLAIM_CHAIN : 0) |
               (chain.head || chain.head_of ? CLAIM_HEAD : 0) | (sibs.sib || sibs.sib_of ? CLAIM_SIBLING : 0);
    }
    // no other fusion or plan has claimed this layer -- but for the claims a site names, with its reason
    bool unclaimed(int but = 0) const { return !(claims() & ~but); }

    int LoadParam(const ParamDict& pd) override
    {
        dilation_w = pd.get(2, 1);
        dilation_h = pd.get(12, dilation_w);
        const bool atrous = dilation_w > 1 || dilation_h > 1;
        if (atrous && !(net && net->dilated))
            return failf(NET_E_UNKNOWN_LAYER, "layer %s: dilated convolution is not supported (fhip_net_set_dilated lifts this)", name.c_str());
        if (dilation_w < 1 || dilation_h < 1) return failf(NET_E_SHAPE, "layer %s: dilation must be >= 1", name.c_str());
        qr.scale_term = pd.get(8, 0);
        const bool quant = qr.scale_term != 0 && net && net->quantized;
        if (qr.scale_term && !quant) return failf(NET_E_UNKNOWN_LAYER, "layer %s: int8 convolution is not supported", name.c_str());
        if (quant && (qr.scale_term < 0 || (qr.scale_term > 100 && !net->requantized)))
            return failf(NET_E_UNKNOWN_LAYER, "layer %s: int8_scale_term %d (requantised int8 output) is not supported", name.c_str(), qr.scale_term);
        if (quant && qr.scale_term > 200) return failf(NET_E_UNKNOWN_LAYER, "layer %s: int8_scale_term %d is not one of 0 .. 200", name.c_str(), qr.scale_term);
        if (quant && atrous) return failf(NET_E_UNKNOWN_LAYER, "layer %s: a dilated int8 convolution is not supported", name.c_str());
        p.kernel_w = pd.get(1, 0);
        p.kernel_h = pd.get(11, p.kernel_w);
        p.stride_w = pd.get(3, 1);
        p.stride_h = pd.get(13, p.stride_w);
        p.pad_left = pd.get(4, 0);
        p.pad_bottom = pd.get(14, p.pad_left);
        p.pad_right = pd.get(4, 0);
        p.pad_top = pd.get(14, p.pad_left);
        p.group = pd.get(7, 1);
        p.output_channels = pd.get(0, 0);
        p.bias_term = pd.get(5, 0);
        p.activation = FHIP_ACT_NONE;
        const int weight_data_size = pd.get(6, 0);
        // conv_layer.h:69-75: output_channels is divided by group (AssignOutputDim restores it for depthwise)
        if (p.group < 1 || p.output_channels % p.group) return failf(NET_E_SHAPE, "layer %s: output_channels is not divisible by its group", name.c_str());
        p.output_channels /= p.group;
        if (p.output_channels <= 0 || p.kernel_h <= 0 || p.kernel_w <= 0) return failf(NET_E_SHAPE, "layer %s: bad convolution geometry", name.c_str());
        // the reference truncates here (conv_layer.h:75); a size that is no whole number of input channels would leave the weight stream
        // out of step with the file for every later layer
        long long per_channel = (long long)p.output_channels * p.kernel_h; // three ints: the product is taken in two steps, each below 2^62
        if (per_channel <= INT_MAX) per_channel *= p.kernel_w;
        if (weight_data_size < 0 || per_channel > INT_MAX || weight_data_size % per_channel)
            return failf(NET_E_SHAPE, "layer %s: weight_data_size does not fit the convolution geometry", name.c_str());
        p.input_channels = (int)(weight_data_size / per_channel);
        route = quant ? ROUTE_INT8 : atrous ? ROUTE_DILATED : p.group > 1 && p.group < p.input_channels ? ROUTE_GROUPED : ROUTE_MAIN;
        if (whole_k()) p.output_channels *= p.group;
        // a depthwise layer has ONE filter per channel (conv_layer.h:69-75 and AssignOutputDim give it input_channels outputs whatever 0= says): with
        // a channel multiplier the top would have a fraction of the channels the .param states and the rest of the filters would be ignored
        if (route == ROUTE_MAIN && p.group > 1 && p.group == p.input_channels && p.output_channels != 1)
            return failf(NET_E_UNKNOWN_LAYER, "layer %s: a depthwise convolution with a channel multiplier (%d filters per channel) is not supported", name.c_str(),
                         p.output_channels);
        if ((route == ROUTE_INT8 || route == ROUTE_DILATED) && (p.pad_left < 0 || p.pad_top < 0))
            return failf(NET_E_UNKNOWN_LAYER, "layer %s: automatic padding is not supported", name.c_str());
        if (route == ROUTE_INT8)
        {
            if (p.input_channels < 1) return failf(NET_E_SHAPE, "layer %s: weight_data_size does not fit the convolution geometry", name.c_str());
            if (p.group != 1 && (p.group != p.input_channels || p.group != p.output_channels))
                return failf(NET_E_UNKNOWN_LAYER, "layer %s: an int8 convolution with a partial group (1 < group < channels) is not supported", name.c_str());
        }
        if (route == ROUTE_DILATED && (p.input_channels < 1 || p.input_channels % p.group))
            return failf(NET_E_SHAPE, "layer %s: weight_data_size does not fit the convolution geometry", name.c_str());
        return 0;
    }
    int LoadWeights(ModelBin& mb) override
    {
        const size_t wsize = (size_t)p.input_channels * p.output_channels * p.kernel_h * p.kernel_w / (whole_k() ? p.group : 1);
        built = BuiltFor(); // new weights: every packed form is rebuilt at the next Init
        sibs.packed_for = nullptr;
        if (route == ROUTE_INT8) return qr.load(this, mb, wsize, p.output_channels, p.bias_term != 0);
        int rc = mb.load(wsize, 0, w_host);
        if (rc) return rc;
        if (p.bias_term) rc = mb.load(bias_channels(), 1, b_host);
        return rc;
    }

    // the side routes; else the main library's output size and algorithm, then the pair or the epilogues
    int Reshape() override
    {
        const Blob* b = bottoms[0];
        p.input_w = b->w;
        p.input_h = b->h;
        if (p.input_channels != b->c)
            return failf(NET_E_TOPOLOGY, "convolution layer %s has %d input channels while bottom blob has %d channels", name.c_str(), p.input_channels, b->c);
        if (route == ROUTE_INT8 || route == ROUTE_DILATED) return reshape_own_output();
        fhip_conv_assign_output_dim(&p);
        if (p.output_h < 1 || p.output_w < 1) return failf(NET_E_SHAPE, "layer %s: empty output", name.c_str());
        if (route == ROUTE_GROUPED) return Grouped::reshape<false>(this, gconv_api(), p, "grouped convolution refused: ", &buffer_bytes, &packed_bytes);
        int rc = net->tuned_selection ? fhip_conv_select_algo_tuned(&p, &algo_) : fhip_conv_select_algo(&p, &algo_);
        if (rc) return rc;
        if ((rc = ep.pw ? reshape_pair() : reshape_epilogues())) return rc;
        return fhip_conv_packed_layout(&p, algo_, &layout);
    }
    // the int8 and the dilated library have their own rule for the output size; it is kept where conv_param() reports it
    int reshape_own_output()
    {
        int rc;
        if (route == ROUTE_INT8)
        {
            copy_geometry(qr.q, p);
            rc = qr.reshape(this);
            p.output_h = qr.q.output_h, p.output_w = qr.q.output_w;
            return rc;
        }
        copy_geometry(dilated, p);
        dilated.output_h = p.output_h, dilated.output_w = p.output_w;
        dilated.dilation_h = dilation_h, dilated.dilation_w = dilation_w;
        rc = Dilated::reshape<true>(this, atrous_api(), dilated, "dilated convolution refused: ", &buffer_bytes, &packed_bytes);
        p.output_h = dilated.output_h, p.output_w = dilated.output_w;
        return rc;
    }
    size_t output_bytes() const { return (size_t)bottoms[0]->n * p.output_channels * p.output_h * p.output_w * sizeof(float); }
    // Runs `step` of the absorbed 1x1 convolution against a stand-in for the depthwise output (the pair has no blob for it) and this
    // layer's top; pw's bottoms are set per call and cleared behind it.
    template <class Step>
    int with_pair_input(float* data, const Step& step)
    {
        Blob dwout;
        dwout.n = bottoms[0]->n, dwout.c = p.output_channels, dwout.h = p.output_h, dwout.w = p.output_w;
        dwout.data = data; // not owned: capacity stays 0
        ep.pw->bottoms.assign(1, &dwout);
        ep.pw->tops = tops;
        ep.pw->net = net;
        const int rc = step();
        ep.pw->bottoms.clear();
        return rc;
    }
    int reshape_pair()
    {
        ConvLayer* pw = ep.pw.get();
        int rc = with_pair_input(nullptr, [&] { return pw->Reshape(); }); // reshapes this layer's top
        if (rc) return rc;
        ep.pair_fast = fhip_conv_can_fuse_dw_pw(&p, &pw->p, bottoms[0]->n) != 0 && pw->unclaimed() && pw->algo_ == FHIP_IM2COL;
        if (!ep.pair_fast && (rc = ep.mid.resize(output_bytes()))) return rc;
        size_t bb = 0;
        if ((rc = fhip_conv_get_buffer_size(&p, algo_, bottoms[0]->n, &bb, &packed_bytes))) return rc;
        buffer_bytes = std::max(bb, pw->buffer_bytes);
        return 0;
    }
    int reshape_epilogues()
    {
        const Blob* b = bottoms[0];
        const Blob* r = ep.residual;
        int rc, oh = p.output_h, ow = p.output_w;
        ep.res_fast = r && fhip_conv_can_fuse_residual(&p, algo_) != 0;
        if (r && (r->n != b->n || r->c != p.output_channels || r->h != p.output_h || r->w != p.output_w))
            return failf(NET_E_SHAPE, "Shape mismatch among bottoms of layer %s.", name.c_str());
        if (ep.fuse_pool)
        {
            ep.poolq.channels = p.output_channels, ep.poolq.input_h = p.output_h, ep.poolq.input_w = p.output_w;
            if ((rc = fhip_pooling_output_dim(&ep.poolq, &oh, &ow))) return rc;
            ep.pool_fast = fhip_conv_can_fuse_maxpool2(&p, algo_) != 0;
            if (!ep.pool_fast && (rc = ep.pre_pool.resize(output_bytes()))) return rc;
        }
        if ((rc = tops[0]->reshape(b->n, p.output_channels, oh, ow))) return rc;
        return fhip_conv_get_buffer_size(&p, algo_, b->n, &buffer_bytes, &packed_bytes);
    }

    // filters and bias with the folded BatchNorm / Scale (fusion level 2) applied
    void folded(std::vector<float>& w, std::vector<float>& b) const
    {
        w = w_host;
        b = b_host;
        fold.apply(w, b, p.output_channels);
    }
    // the pair's filters and biases stacked (a zero bias for the layer that has none, where the other has one), packed as one IM2COL layer
    int init_siblings(hipStream_t s)
    {
        ConvLayer* o = sibs.sib;
        std::vector<float> wa, ba, wb, bb;
        folded(wa, ba);
        o->folded(wb, bb);
        fhip_conv_param pa = p, pb = o->p, both;
        pa.bias_term = ba.empty() ? 0 : 1;
        pb.bias_term = bb.empty() ? 0 : 1;
        int rc = fhip_conv_siblings_geometry(&pa, &pb, &both);
        if (rc) return rc;
        wa.insert(wa.end(), wb.begin(), wb.end());
        sibs.has_bias = both.bias_term != 0;
        if (sibs.has_bias)
        {
            if (ba.empty()) ba.assign(p.output_channels, 0.f);
            if (bb.empty()) bb.assign(o->p.output_channels, 0.f);
            ba.insert(ba.end(), bb.begin(), bb.end());
        }
        size_t bytes = 0, pk = 0;
        if ((rc = fhip_conv_get_buffer_size(&both, FHIP_IM2COL, bottoms[0]->n, &bytes, &pk))) return rc;
        if ((rc = init_main(both, FHIP_IM2COL, wa, ba, sibs.packed, pk, sibs.bias, s))) return rc;
        sibs.packed_for = o;
        return 0;
    }
    int Init(hipStream_t s) override
    {
        int rc;
        if (ep.pw && (rc = ep.pw->Init(s))) return rc;
        if (sibs.sib && sibs.packed_for != sibs.sib && (rc = init_siblings(s))) return rc;
        if (route == ROUTE_INT8)
        {
            rc = qr.init(this, fold, s);
            if (!rc && !fold.empty()) p.bias_term = 1;
            return rc;
        }
        const BuiltFor want{algo(), layout, packed_bytes};
        if (built == want) return 0;
        std::vector<float> w, b;
        folded(w, b);
        if (!fold.empty()) p.bias_term = dilated.bias_term = 1; // the next Reshape copies p.bias_term into the side params
        if (first_candidate() && (rc = first_raw.upload(w.data(), w.size(), s))) return rc; // 27 floats per output channel
        if ((rc = route == ROUTE_DILATED   ? Dilated::init(this, atrous_api(), dilated, w, b, packed, packed_bytes, bias, s)
                  : route == ROUTE_GROUPED ? Grouped::init(this, gconv_api(), p, w, b, packed, packed_bytes, bias, s)
                                           : init_main(p, algo_, w, b, packed, packed_bytes, bias, s)))
            return rc;
        built = want;
        return 0;
    }

    // ---- Forward: one function per way a layer runs; the order of the tests is part of the behaviour ----------------------------------
    int Forward(hipStream_t s) override
    {
        if (route != ROUTE_MAIN) return forward_side(s);
        if (chain.head_of) return 0; // computed inside head_of's input transform
        if (sibs.sib_of) return 0;   // computed by the layer before, in the same GEMM
        if (sibs.sib) return forward_siblings(s);
        if (ep.pw) return forward_pair(s);
        if (chain.runs()) return forward_chained(s);
        return forward_plain(s);
    }
    const float* bias_d() const { return p.bias_term ? bias.d : nullptr; }
    float* arena() const { return (float*)net->arena.d; }
    // the pooling a route could not take into its kernel, behind the convolution that wrote pre_pool
    int pool_tail(int rc, hipStream_t s) { return rc ? rc : fhip_pooling(&ep.poolq, bottoms[0]->n, tops[0]->data, ep.pre_pool.d, s); }
    int forward_side(hipStream_t s)
    {
        if (route == ROUTE_INT8) return qr.forward(this, s);
        if (route == ROUTE_DILATED) return Dilated::forward(this, atrous_api(), dilated, packed, bias, s);
        return Grouped::forward(this, gconv_api(), p, packed, bias, s);
    }
    int forward_siblings(hipStream_t s)
    {
        return fhip_conv_forward_siblings(&p, &sibs.sib->p, bottoms[0]->n, tops[0]->data, sibs.sib->tops[0]->data, bottoms[0]->data, sibs.packed.d,
                                          sibs.has_bias ? sibs.bias.d : nullptr, s);
    }
    int forward_pair(hipStream_t s)
    {
        ConvLayer* pw = ep.pw.get();
        if (ep.pair_fast)
            return fhip_conv_forward_dw_pw(&p, &pw->p, bottoms[0]->n, tops[0]->data, bottoms[0]->data, packed.d, bias_d(), pw->packed.d, pw->bias_d(), s);
        const int rc = fhip_conv_forward(&p, algo_, bottoms[0]->n, ep.mid.d, bottoms[0]->data, packed.d, arena(), bias_d(), s);
        return rc ? rc : with_pair_input(ep.mid.d, [&] { return pw->Forward(s); });
    }
    int forward_chained(hipStream_t s)
    {
        char* base = reinterpret_cast<char*>(net->arena.d);
        float* v = reinterpret_cast<float*>(base + net->chain_slot[chain.pos & 1]);
        float* vn = reinterpret_cast<float*>(base + net->chain_slot[(chain.pos + 1) & 1]);
        float* m = reinterpret_cast<float*>(base + net->chain_m);
        const float* in = chain.in || chain.head ? nullptr : bottoms[0]->data;
        const float* b = bias_d();
        const int n = bottoms[0]->n, pool = ep.fuse_pool ? 1 : 0;
        if (const ConvLayer* h = chain.head)
        {
            const int rc = fhip_winograd_f63_input_from_first(&h->p, &p, n, v, h->bottoms[0]->data, h->first_raw.d, h->bias_d(), s);
            if (rc) return rc;
        }
        if (chain.canvas || (chain.next && chain.next->chain.canvas)) return forward_canvas(n, in, v, m, vn, b, s);
        if (chain.colpass) return forward_colpass(n, in, v, m, vn, b, s);
        if (chain.next) return fhip_conv_forward_chained(&p, n, nullptr, in, packed.d, v, m, b, &chain.next->p, vn, pool, s);
        if (!ep.fuse_pool || ep.pool_fast) return fhip_conv_forward_chained(&p, n, tops[0]->data, in, packed.d, v, m, b, nullptr, nullptr, pool, s);
        return pool_tail(fhip_conv_forward_chained(&p, n, ep.pre_pool.d, in, packed.d, v, m, b, nullptr, nullptr, 0, s), s);
    }
    // One layer of a chained run that is, or is followed by, a canvas layer: input transform (a plain first layer only) -> tile GEMM on the
    // geometry the layer runs with -> the boundary's form of the chained transform, or the canvas output transform at the end of the run.
    int forward_canvas(int n, const float* in, float* v, float* m, float* vn, const float* b, hipStream_t s)
    {
        const CanvasApi* api = canvas_api();
        if (!api) return FHIP_E_UNSUPPORTED; // message set by canvas_api
        int rc;
        if (in)
        {
            // plan_chains enters a canvas stretch through a chained boundary only: a layer that transforms its own input is plain
            if (chain.canvas) return failf(FHIP_E_UNSUPPORTED, "layer %s: a canvas layer takes its input from the chained transform before it", name.c_str());
            if ((rc = fhip_winograd_f63_input_transform(&p, n, v, in, s))) return rc;
        }
        rc = chain.canvas ? fhip_winograd_f63_tile_gemm(&chain.canvas_p, n / 4, m, packed.d, v, s) : fhip_winograd_f63_tile_gemm(&p, n, m, packed.d, v, s);
        if (rc) return rc;
        if (const ConvLayer* nx = chain.next)
        {
            const int form = !chain.canvas ? FHIP_CANVAS_ENTRY : nx->chain.canvas ? FHIP_CANVAS_INSIDE : FHIP_CANVAS_EXIT;
            rc = api->chain(form, &p, &nx->p, n, &chain.run_plan, &nx->chain.run_plan, vn, m, b, s);
        }
        else
            rc = api->output(&p, n, &chain.run_plan, tops[0]->data, m, b, ep.fuse_pool ? 1 : 0, s);
        return rc ? failf(rc, "layer %s: %s", name.c_str(), api->last_error()) : 0;
    }
    // A chained layer with a plain chained successor on the column-passed tile GEMM (plan_chains): input transform (a first layer of a run
    // only) -> the library's GEMM, 48 planes into the M slot -> the library's chained transform.
    int forward_colpass(int n, const float* in, float* v, float* m, float* vn, const float* b, hipStream_t s)
    {
        const ColpassApi* api = colpass_api();
        if (!api) return FHIP_E_UNSUPPORTED; // message set by colpass_api
        int rc;
        if (in && (rc = fhip_winograd_f63_input_transform(&p, n, v, in, s))) return rc;
        const ConvLayer* nx = chain.next;
        rc = api->tile_gemm(&p, n, &chain.run_plan, m, packed.d, v, s);
        if (!rc) rc = api->chain(&p, &nx->p, n, &chain.run_plan, &nx->chain.run_plan, vn, m, b, ep.fuse_pool ? 1 : 0, s);
        return rc ? failf(rc, "layer %s: %s", name.c_str(), api->last_error()) : 0;
    }
    // the main library's route with the epilogues Fuse absorbed: a residual add, a pooling, or neither
    int forward_plain(hipStream_t s)
    {
        const int n = bottoms[0]->n;
        const float *in = bottoms[0]->data, *b = bias_d();
        if (Blob* r = ep.residual)
        {
            if (r->alias) r->data = r->alias->data;
            if (ep.res_fast) return fhip_conv_forward_residual(&p, algo_, n, tops[0]->data, in, packed.d, arena(), b, r->data, s);
            fhip_conv_param q = p; // route without the fused epilogue: conv, then the add (+ReLU) in place on the top
            q.activation = FHIP_ACT_NONE;
            const int rc = fhip_conv_forward(&q, algo_, n, tops[0]->data, in, packed.d, arena(), b, s);
            return rc ? rc : fhip_add(tops[0]->data, tops[0]->data, r->data, tops[0]->count(), p.activation == FHIP_ACT_RELU, s);
        }
        if (!ep.fuse_pool) return fhip_conv_forward(&p, algo_, n, tops[0]->data, in, packed.d, arena(), b, s);
        if (ep.pool_fast) return fhip_conv_forward_maxpool2(&p, algo_, n, tops[0]->data, in, packed.d, arena(), b, s);
        return pool_tail(fhip_conv_forward(&p, algo_, n, ep.pre_pool.d, in, packed.d, arena(), b, s), s);
    }

    int Fuse(Layer* next, int level) override;
    // absorb `elt` = Eltwise SUM of this layer's top and `other` (a blob produced earlier in the layer list)
    bool FuseResidual(Blob* other)
    {
        if (ep.pw)
        {
            // behind an absorbed 1x1 convolution (MobileNet-V2 style dw -> pw(linear) -> add): the add goes into the POINTWISE layer's
            // epilogue; the pair then runs its two kernels one after the other (Reshape: pair_fast needs a pointwise layer without residual)
            if (!unclaimed(CLAIM_PAIR) || !ep.pw->FuseResidual(other)) return false;
            ep.pw->bottoms.pop_back(); // the pointwise layer's bottoms are set per call (a stand-in for the depthwise output)
            bottoms.push_back(other);  // dependency scans look at THIS layer
            return true;
        }
        if (side_epilogues_only() || !unclaimed() || p.activation != FHIP_ACT_NONE) return false;
        ep.residual = other;
        bottoms.push_back(other); // so that dependency scans (fusion, branch concurrency) see the second input
        return true;
    }
    // take over the (top, bottom, left, right) margins of a Padding layer that only zero-pads this layer's input (fold_zero_paddings, before
    // any other fusion): the main and the grouped fp32 route alone, and only onto pads that are pads (>= 0)
    bool FoldPadding(const int* m)
    {
        if ((route != ROUTE_MAIN && route != ROUTE_GROUPED) || p.pad_top < 0 || p.pad_bottom < 0 || p.pad_left < 0 || p.pad_right < 0) return false;
        const long long sums[4] = {(long long)p.pad_top + m[0], (long long)p.pad_bottom + m[1], (long long)p.pad_left + m[2], (long long)p.pad_right + m[3]};
        for (long long v : sums)
            if (v > (1 << 16)) return false; // a pad no plane has: the Padding layer stays and answers for it
        p.pad_top = (int)sums[0], p.pad_bottom = (int)sums[1], p.pad_left = (int)sums[2], p.pad_right = (int)sums[3];
        return true;
    }
    size_t weight_bytes() const override
    {
        return packed.bytes + bias.bytes + ep.pre_pool.bytes + ep.mid.bytes + first_raw.bytes + sibs.packed.bytes + sibs.bias.bytes + qr.bytes() +
               (ep.pw ? ep.pw->weight_bytes() : 0);
    }
    const fhip_conv_param* fused_pointwise(int* one_kernel) const override
    {
        if (one_kernel) *one_kernel = ep.pair_fast ? 1 : 0;
        return ep.pw ? &ep.pw->p : nullptr;
    }
    size_t arena_bytes() const override { return std::max(buffer_bytes, chain.bytes); }
    const fhip_conv_param* conv_param() const override { return &p; }
    int algo() const override { return route == ROUTE_MAIN ? algo_ : ROUTE_CODE[route]; }
    int sibling_state() const override { return sibs.sib ? 1 : sibs.sib_of ? 2 : 0; }
    int residual_state() const override { return !ep.residual ? 0 : ep.res_fast ? 1 : 2; }
    void chain_state(int* v_from_previous, int* writes_next_v) const override
    {
        *v_from_previous = chain.head ? 2 : chain.in ? 1 : 0;
        *writes_next_v = chain.head_of ? 2 : chain.next ? 1 : 0;
    }
    int canvas_state() const override { return chain.canvas ? 1 : 0; }
    int colpass_state() const override { return chain.colpass ? 1 : 0; }
};

inline void ChainPlan::link(ConvLayer* a, ConvLayer* b) { a->chain.next = b, b->chain.in = true, b->chain.pos = a->chain.pos + 1; }
inline void ChainPlan::absorb_first(ConvLayer* first, ConvLayer* consumer) { first->chain.head_of = consumer, consumer->chain.head = first; }
inline void SiblingPlan::pair(ConvLayer* a, ConvLayer* b) { a->sibs.sib = b, b->sibs.sib_of = a; }

} // namespace fhip::net
