// net_layers.h -- the layer classes of the Net runtime but the convolution's (net_conv.h), and the two definitions of net_conv.h that need them.
#pragma once
#include "net_conv.h"

namespace fhip::net
{

struct InputLayer : Layer
{
    int Reshape() override { return 0; } // shape comes from FeedInput (input_layer.h:33-46)
    int Forward(hipStream_t) override { return 0; }
};

// feather::InnerProductLayer, layers/inner_product_layer.h:28-171: y = W x + b, W [out][in].  On the device it is a
// 1x1 convolution over a 1x1 image with `in` channels, i.e. one GEMM [out x in] * [in x batch] through the implicit
// GEMM path (the reference's GEMV, booster/avx/sgemv.cpp:317-395, is the batch = 1 case).
struct InnerProductLayer : Layer
{
    fhip_conv_param p;
    size_t input_size = 0, output_size = 0, weight_data_size = 0;
    std::vector<float> w_host, b_host;
    DeviceVec packed, bias;
    size_t buffer_bytes = 0, packed_bytes = 0;
    BuiltFor built; // never built again once done: the packed copy is shape independent
    // 8=int8_scale_term in a net with fhip_net_set_quantized: the 1x1 convolution over a 1x1 image runs through libfeather_qconv.so
    // (QuantRoute, route code FHIP_NET_ROUTE_QCONV) with the same ReLU fusion; the int8 weights stay int8 on the device
    bool quant = false;
    QuantRoute qr;

    InnerProductLayer() { memset(&p, 0, sizeof(p)); }
    bool needs_weights() const override { return true; }
    int LoadParam(const ParamDict& pd) override
    {
        output_size = pd.get(0, 0);
        p.bias_term = pd.get(1, 0);
        weight_data_size = pd.get(2, 0);
        if (pd.get(0, 0) < 1) return failf(NET_E_SHAPE, "layer %s: num_output must be positive", name.c_str());
        if (pd.get(2, 0) < 0 || weight_data_size % output_size)
            return failf(NET_E_SHAPE, "layer %s: weight_data_size is no whole number of rows of num_output", name.c_str());
        input_size = weight_data_size / output_size;
        p.input_channels = (int)input_size;
        p.output_channels = (int)output_size;
        p.input_h = p.input_w = p.kernel_h = p.kernel_w = p.stride_h = p.stride_w = p.group = 1;
        fhip_conv_assign_output_dim(&p);
        // with the switch off nothing changes, not even a message: the weight reader refuses the int8 tag as it always has
        quant = qr.read_scale_term(pd) != 0 && net && net->quantized;
        if (quant && (qr.scale_term < 0 || qr.scale_term > 100))
            return failf(NET_E_UNKNOWN_LAYER, "layer %s: int8_scale_term %d (requantised int8 output) is not supported", name.c_str(), qr.scale_term);
        return 0;
    }
    int LoadWeights(ModelBin& mb) override
    {
        if (quant) return qr.load(this, mb, weight_data_size, (int)output_size, p.bias_term != 0);
        int rc = mb.load(weight_data_size, 0, w_host);
        if (rc) return rc;
        if (p.bias_term) rc = mb.load(output_size, 1, b_host);
        return rc;
    }
    int Reshape() override
    {
        const Blob* b = bottoms[0];
        const size_t per_image = (size_t)b->c * b->h * b->w;
        if (input_size != per_image)
            return failf(NET_E_SHAPE, "In Layer %s: Bottom %s data size %zu is inconsistant with expected input size %zu.", name.c_str(), b->name.c_str(), per_image, input_size);
        if (quant)
        {
            copy_geometry(qr.q, p); // a 1x1 convolution over a 1x1 image without padding, as LoadParam left p
            return qr.reshape(this);
        }
        int rc = tops[0]->reshape(b->n, (int)output_size, 1, 1);
        if (rc) return rc;
        return fhip_conv_get_buffer_size(&p, FHIP_IM2COL, b->n, &buffer_bytes, &packed_bytes);
    }
    int Init(hipStream_t s) override
    {
        if (quant) return qr.init(this, AffineFold(), s);
        if (built.done()) return 0;
        const int rc = init_main(p, FHIP_IM2COL, w_host, b_host, packed, packed_bytes, bias, s);
        if (rc) return rc;
        std::vector<float>().swap(w_host); // the raw weights are not needed again
        built = BuiltFor{FHIP_IM2COL, 0, packed_bytes};
        return 0;
    }
    int Forward(hipStream_t s) override
    {
        if (quant) return qr.forward(this, s);
        return fhip_conv_forward(&p, FHIP_IM2COL, bottoms[0]->n, tops[0]->data, bottoms[0]->data, packed.d, (float*)net->arena.d,
                                 p.bias_term ? bias.d : nullptr, s);
    }
    int Fuse(Layer* next, int) override
    {
        if (!is_plain_relu(next)) return 0;
        p.activation = FHIP_ACT_RELU;
        return 1;
    }
    size_t weight_bytes() const override { return packed.bytes + bias.bytes + qr.bytes(); }
    size_t arena_bytes() const override { return buffer_bytes; }
    int algo() const override { return quant ? FHIP_NET_ROUTE_QCONV : FHIP_IM2COL; }
};

// ncnn's ReLU: 0=slope.  Slope 0 is the reference's layer (fhip_relu); a leaky one runs through libfeather_inorm.so.
struct ReluLayer : Layer
{
    float slope = 0.f;
    int LoadParam(const ParamDict& pd) override
    {
        slope = pd.get(0, 0.f);
        return 0;
    }
    // a plain ReLU on a q8 blob is max(q, 0) on its bytes (libfeather_q8.so): quantise commutes with it
    bool reads_q8() const override { return slope == 0.f; }
    bool writes_q8() const override { return bottoms[0]->q8; }
    int Reshape() override
    {
        if (slope != 0.f) return reshape_with(inorm_api());
        if (!bottoms[0]->q8) return Layer::Reshape();
        if (!q8_api()) return FHIP_E_UNSUPPORTED; // (message set by side_api)
        // in place where this layer alone reads the blob and the blob owns its bytes (a Split top's are its siblings' too): the top shares
        // them and no second q8 blob exists; else a top of its own
        Blob* b = bottoms[0];
        if (tops.size() != 1 || bottoms.size() != 1) return failf(NET_E_BASE_RESHAPE, "layer %s: base Reshape needs 1 bottom and 1 top", name.c_str());
        if (b->alias || readers(*net, b).count != 1) return Layer::Reshape(); // (exact readers: what shares b reads it as a Split does, by name)
        tops[0]->share(b);
        return 0;
    }
    int Forward(hipStream_t s) override
    {
        if (bottoms[0]->q8) return side(q8_api(), [&](const Q8Api* api) { return api->relu(tops[0]->data, bottoms[0]->data, bottoms[0]->q8_bytes(), s); });
        if (slope == 0.f) return fhip_relu(tops[0]->data, bottoms[0]->data, bottoms[0]->count(), s);
        const Blob* b = bottoms[0];
        return side(inorm_api(), [&](const InormApi* api) {
            return api->activation(FHIP_ACTIVATION_LEAKY_RELU, tops[0]->data, b->data, b->n, b->c, b->h * b->w, slope, 0.f, nullptr, s);
        });
    }
    const float* relu_slope() const override { return &slope; }
};

// ncnn's InstanceNorm (no reference counterpart; the definition is include/feather_hip/feather_inorm.h): 0=channels, 1=eps, 2=affine,
// gamma and beta in the .bin when affine.  Runs through libfeather_inorm.so with route code FHIP_NET_ROUTE_INORM; the scratch of the
// split-plane route comes out of the net's arena, so the layer stays on the main stream.  Absorbs a following ReLU, plain or leaky.
struct InstanceNormLayer : Layer
{
    int channels = 0, affine = 1, act = FHIP_INORM_ACT_NONE;
    float eps = 0.001f, slope = 0.f;
    std::vector<float> gamma, beta;
    DeviceVec d_gamma, d_beta;
    size_t scratch_bytes = 0;
    bool inited = false;

    int LoadParam(const ParamDict& pd) override
    {
        channels = pd.get(0, 0);
        eps = pd.get(1, 0.001f);
        affine = pd.get(2, 1);
        if (channels < 1) return failf(NET_E_SHAPE, "layer %s: InstanceNorm needs at least one channel", name.c_str());
        if (!(eps >= 0.f)) return failf(NET_E_SHAPE, "layer %s: InstanceNorm eps must not be negative", name.c_str());
        return 0;
    }
    int LoadWeights(ModelBin& mb) override
    {
        inited = false;
        if (!affine) return 0;
        const int rc = mb.load(channels, 1, gamma);
        return rc ? rc : mb.load(channels, 1, beta);
    }
    int Reshape() override
    {
        const Blob* b = bottoms[0];
        if (b->c != channels)
            return failf(NET_E_TOPOLOGY, "InstanceNorm layer %s has %d channels while bottom blob %s has %d", name.c_str(), channels, b->name.c_str(), b->c);
        const int rc = side(inorm_api(), [&](const InormApi* api) { return api->get_buffer_size(b->n, b->c, b->h, b->w, &scratch_bytes); });
        return rc ? rc : Layer::Reshape();
    }
    bool needs_weights() const override { return true; } // also with affine = 0, where LoadWeights reads nothing
    int Init(hipStream_t s) override
    {
        if (inited || !affine) return 0;
        int rc = d_gamma.upload(gamma.data(), gamma.size(), s);
        if (rc) return rc;
        if ((rc = d_beta.upload(beta.data(), beta.size(), s))) return rc;
        FHIP_CHECK_HIP(hipStreamSynchronize(s));
        inited = true;
        return 0;
    }
    int Forward(hipStream_t s) override
    {
        const Blob* b = bottoms[0];
        return side(inorm_api(), [&](const InormApi* api) {
            return api->forward(b->n, b->c, b->h, b->w, tops[0]->data, b->data, affine ? d_gamma.d : nullptr, affine ? d_beta.d : nullptr, eps, act, slope,
                                scratch_bytes ? net->arena.d : nullptr, s);
        });
    }
    int Fuse(Layer* next, int) override
    {
        if (!next->relu_slope() || act != FHIP_INORM_ACT_NONE) return 0;
        slope = *next->relu_slope();
        act = slope == 0.f ? FHIP_INORM_ACT_RELU : FHIP_INORM_ACT_LEAKY;
        return 1;
    }
    size_t weight_bytes() const override { return d_gamma.bytes + d_beta.bytes; }
    size_t arena_bytes() const override { return scratch_bytes; }
    int algo() const override { return FHIP_NET_ROUTE_INORM; }
};

// ncnn's PReLU (0=num_slope, slope[num_slope] in the .bin), Sigmoid, TanH and Clip (0=min, 1=max): one element-wise launch of
// libfeather_inorm.so each; nothing fuses with them.
struct ActivationLayer : Layer
{
    int kind = -1, num_slope = 0;
    float p0 = 0.f, p1 = 0.f;
    std::vector<float> slopes;
    DeviceVec d_slopes;
    bool inited = false;

    int LoadParam(const ParamDict& pd) override
    {
        if (type == "PReLU")
        {
            kind = FHIP_ACTIVATION_PRELU;
            num_slope = pd.get(0, 0);
            if (num_slope < 1) return failf(NET_E_SHAPE, "layer %s: PReLU needs num_slope >= 1", name.c_str());
        }
        else if (type == "Sigmoid")
            kind = FHIP_ACTIVATION_SIGMOID;
        else if (type == "TanH")
            kind = FHIP_ACTIVATION_TANH;
        else
        {
            kind = FHIP_ACTIVATION_CLIP;
            p0 = pd.get(0, -FLT_MAX);
            p1 = pd.get(1, FLT_MAX);
            if (!(p0 <= p1)) return failf(NET_E_SHAPE, "layer %s: Clip needs min <= max", name.c_str());
        }
        return 0;
    }
    int LoadWeights(ModelBin& mb) override
    {
        if (kind != FHIP_ACTIVATION_PRELU) return 0;
        inited = false;
        const int rc = mb.load(num_slope, 1, slopes);
        if (!rc && num_slope == 1) p0 = slopes[0];
        return rc;
    }
    int Reshape() override
    {
        if (kind == FHIP_ACTIVATION_PRELU && num_slope != 1 && num_slope != bottoms[0]->c)
            return failf(NET_E_TOPOLOGY, "PReLU layer %s has %d slopes while bottom blob %s has %d channels", name.c_str(), num_slope,
                         bottoms[0]->name.c_str(), bottoms[0]->c);
        return reshape_with(inorm_api());
    }
    int Init(hipStream_t s) override
    {
        if (inited || num_slope <= 1) return 0;
        const int rc = d_slopes.upload(slopes.data(), slopes.size(), s);
        if (rc) return rc;
        FHIP_CHECK_HIP(hipStreamSynchronize(s));
        inited = true;
        return 0;
    }
    int Forward(hipStream_t s) override
    {
        const Blob* b = bottoms[0];
        return side(inorm_api(), [&](const InormApi* api) {
            return api->activation(kind, tops[0]->data, b->data, b->n, b->c, b->h * b->w, p0, p1, num_slope > 1 ? d_slopes.d : nullptr, s);
        });
    }
    bool needs_weights() const override { return kind == FHIP_ACTIVATION_PRELU; }
    size_t weight_bytes() const override { return d_slopes.bytes; }
};

struct PoolingLayer : Layer
{
    fhip_pool_param q;
    PoolingLayer() { memset(&q, 0, sizeof(q)); }
    PoolingLayer* as_pooling() override { return this; }
    // a max pooling on a q8 blob is the byte-wise max (libfeather_q8.so): quantise commutes with it; its top is q8
    bool reads_q8() const override { return q.pooling_type == 0; }
    bool writes_q8() const override { return bottoms[0]->q8; }
    int LoadParam(const ParamDict& pd) override // pooling_layer.h:90-107
    {
        q.pooling_type = pd.get(0, 0);
        q.kernel_w = pd.get(1, 0);
        q.kernel_h = pd.get(11, q.kernel_w);
        q.stride_w = pd.get(2, 1);
        q.stride_h = pd.get(12, q.stride_w);
        q.pad_left = pd.get(3, 0);
        q.pad_right = pd.get(14, q.pad_left);
        q.pad_top = pd.get(13, q.pad_left);
        q.pad_bottom = pd.get(15, q.pad_top);
        q.global_pooling = pd.get(4, 0) != 0;
        return 0;
    }
    int Reshape() override
    {
        const Blob* b = bottoms[0];
        q.channels = b->c;
        q.input_h = b->h;
        q.input_w = b->w;
        int oh, ow;
        int rc = fhip_pooling_output_dim(&q, &oh, &ow);
        if (rc) return rc;
        if (oh < 1 || ow < 1) return failf(NET_E_SHAPE, "layer %s: empty pooling output", name.c_str());
        if (b->q8 && !q8_api()) return FHIP_E_UNSUPPORTED; // (message set by side_api)
        return tops[0]->reshape(b->n, b->c, oh, ow);
    }
    int Forward(hipStream_t s) override
    {
        if (bottoms[0]->q8) return side(q8_api(), [&](const Q8Api* api) { return api->max_pool(&q, bottoms[0]->n, tops[0]->data, bottoms[0]->data, s); });
        return fhip_pooling(&q, bottoms[0]->n, tops[0]->data, bottoms[0]->data, s);
    }
};

struct SoftmaxLayer : Layer
{
    int Forward(hipStream_t s) override
    {
        const Blob* b = bottoms[0];
        return fhip_softmax(tops[0]->data, b->data, b->n, b->c * b->h * b->w, s);
    }
};

// Per-channel affine layers: BatchNorm (batchnorm_layer.h:36-75) and Scale (scale_layer.h:33-98).  Both keep
// (mul, add) on the host until Init so that fusion can compose them: (x*m1 + a1)*m2 + a2.
struct AffineLayer : Layer
{
    int channels = 0;
    std::vector<float> mul, add;
    bool has_add = false, relu = false;
    bool gated = false; // a Scale whose scale is its second bottom (ScaleLayer): no affine map, no fold absorbs it
    DeviceVec d_mul, d_add;
    bool inited = false;

    bool needs_weights() const override { return !gated; }
    AffineLayer* as_affine() override { return this; }
    void compose(const AffineLayer& nx)
    {
        if (!has_add) add.assign(channels, 0.f);
        for (int i = 0; i < channels; ++i)
        {
            mul[i] = mul[i] * nx.mul[i];
            add[i] = add[i] * nx.mul[i] + (nx.has_add ? nx.add[i] : 0.f);
        }
        has_add = has_add || nx.has_add;
    }
    int Reshape() override
    {
        if (bottoms[0]->c != channels)
            return failf(NET_E_SHAPE, "Mismatch channel in layer %s, expected %d but the bottom %s has %d channels.", name.c_str(), channels,
                         bottoms[0]->name.c_str(), bottoms[0]->c);
        return Layer::Reshape();
    }
    int Init(hipStream_t s) override
    {
        if (inited) return 0;
        int rc = d_mul.upload(mul.data(), mul.size(), s);
        if (rc) return rc;
        if (has_add) rc = d_add.upload(add.data(), add.size(), s);
        if (rc) return rc;
        FHIP_CHECK_HIP(hipStreamSynchronize(s));
        inited = true;
        return 0;
    }
    int Forward(hipStream_t s) override
    {
        const Blob* b = bottoms[0];
        return fhip_affine(tops[0]->data, b->data, d_mul.d, has_add ? d_add.d : nullptr, b->n, b->c, b->h * b->w, relu, s);
    }
    int Fuse(Layer* next, int) override
    {
        if (is_plain_relu(next))
        {
            relu = true;
            return 1;
        }
        if (!relu && type == "BatchNorm" && next->type == "Scale") // BN-Scale(-ReLU), batchnorm_layer.h:107-131
        {
            AffineLayer* nx = next->as_affine(); // the order BatchNorm, then Scale is the rule here: the two types by name
            if (nx->gated || nx->channels != channels) return 0;
            compose(*nx);
            return 1;
        }
        return 0;
    }
    size_t weight_bytes() const override { return d_mul.bytes + d_add.bytes; }
};

bool AffineFold::absorb(const AffineLayer& nx, int K)
{
    if (nx.gated || nx.channels != K || nx.relu) return false;
    if (mul.empty())
    {
        mul.assign(K, 1.f);
        add.assign(K, 0.f);
    }
    for (int k = 0; k < K; ++k)
    {
        mul[k] *= nx.mul[k];
        add[k] = add[k] * nx.mul[k] + (nx.has_add ? nx.add[k] : 0.f);
    }
    return true;
}

int ConvLayer::Fuse(Layer* next, int level)
{
    if (ep.pw) return ep.pw->Fuse(next, level) == 1 ? 1 : 0; // behind the absorbed 1x1 convolution: its own fusions
    if (ep.fuse_pool) return 0; // nothing is absorbed behind the pooling
    if (side_epilogues_only() && !is_plain_relu(next) && !next->as_affine()) return 0;
    if (level >= 2 && unclaimed() && next->type == "Convolution" && p.group == p.input_channels && p.group > 1 && p.group <= 256 && p.kernel_h == 3 &&
        p.kernel_w == 3 && p.stride_h == p.stride_w && (p.stride_h == 1 || p.stride_h == 2) && p.pad_left == 1 && p.pad_top == 1)
    {
        // depthwise 3x3 (at most 256 channels: fhip_conv_can_fuse_dw_pw's structural conditions) -> 1x1 convolution: the pair becomes one
        // layer -- one kernel where the shapes qualify too, else the two kernels one after the other inside this layer
        // (a layer typed "Convolution" only, never "ConvolutionDepthWise": kept as found, the code gives no reason -- the group test below
        // would turn every real depthwise layer away anyway)
        const fhip_conv_param& q = next->as_conv()->p;
        if (next->as_conv()->route != ROUTE_MAIN) return 0; // (a grouped one would fail the group test below anyway)
        if (q.group != 1 || q.kernel_h != 1 || q.kernel_w != 1 || q.stride_h != 1 || q.stride_w != 1 || q.pad_left || q.pad_right || q.pad_top || q.pad_bottom)
            return 0;
        // fhip_conv_can_fuse_dw_pw's profitable range -- or the band-staged kernel's pair (32 channels, stride 1, a multiple of 64 output channels:
        // MobileNet's first pair); the row width is only known at Reshape, where the pair falls back to its two kernels if it does not qualify
        const bool band_pair = p.input_channels == 32 && p.stride_h == 1 && q.output_channels % 64 == 0 && q.output_channels <= 128; // = dwpw_band_applicable's bound
        if (!band_pair && (q.output_channels <= 64 || q.output_channels >= (p.stride_h == 1 ? 160 : 400))) return 0;
        return 2; // the pass hands `next` over (fuse_layers)
    }
    if (ep.residual && !is_plain_relu(next)) return 0; // behind the residual add only its ReLU
    if (level >= 2 && next->as_pooling())
    {
        const fhip_pool_param& q = next->as_pooling()->q;
        if (q.pooling_type != 0 || q.global_pooling || q.kernel_h != 2 || q.kernel_w != 2 || q.stride_h != 2 || q.stride_w != 2 || q.pad_left ||
            q.pad_right || q.pad_top || q.pad_bottom)
            return 0;
        ep.poolq = q;
        ep.fuse_pool = true;
        return 1;
    }
    if (is_plain_relu(next))
    {
        p.activation = FHIP_ACT_RELU;
        return 1;
    }
    // level 2 (beyond the reference): fold a following BatchNorm / Scale into the weights and bias
    if (level >= 2 && p.activation == FHIP_ACT_NONE && next->as_affine()) return fold.absorb(*next->as_affine(), bias_channels()) ? 1 : 0;
    return 0;
}

struct BatchNormLayer : AffineLayer
{
    float eps = 0.f;
    int LoadParam(const ParamDict& pd) override
    {
        channels = pd.get(0, 0);
        eps = pd.get(1, 0.f);
        if (channels < 0) return failf(NET_E_SHAPE, "layer %s: negative channel count", name.c_str());
        return 0;
    }
    int LoadWeights(ModelBin& mb) override // slope, mean, var, bias -> alpha/beta (batchnorm_layer.h:43-75)
    {
        std::vector<float> slope, mean, var, bias;
        int rc;
        if ((rc = mb.load(channels, 1, slope)) || (rc = mb.load(channels, 1, mean)) || (rc = mb.load(channels, 1, var)) || (rc = mb.load(channels, 1, bias))) return rc;
        mul.resize(channels);
        add.resize(channels);
        for (int i = 0; i < channels; ++i)
        {
            const float sqrt_var = sqrtf(var[i] + eps);
            add[i] = bias[i] - slope[i] * mean[i] / sqrt_var; // alpha
            mul[i] = slope[i] / sqrt_var;                     // beta
        }
        has_add = true;
        return 0;
    }
};

// y[n][c][:] = x[n][c][:] * g[n][c] for a gate blob g of shape [n][c][1][1]: what a two-bottom `BinaryOp 0=2` and a two-bottom
// `Scale 0=-233` both say (include/feather_hip/feather_gate.h).  Shared by the two layers; route code FHIP_NET_ROUTE_GATE.
static int gate_reshape(const Layer* l, const Blob* x, const Blob* g)
{
    if (g->n != x->n || g->c != x->c || g->h != 1 || g->w != 1)
        return failf(NET_E_SHAPE, "layer %s: a channel gate needs bottoms of shapes [n][c][h][w] and [n][c][1][1], got %s [%d][%d][%d][%d] and %s [%d][%d][%d][%d]",
                     l->name.c_str(), x->name.c_str(), x->n, x->c, x->h, x->w, g->name.c_str(), g->n, g->c, g->h, g->w);
    if (!gate_api()) return FHIP_E_UNSUPPORTED; // message set by gate_api
    return l->tops[0]->reshape(x->n, x->c, x->h, x->w);
}

static int gate_forward(const Layer* l, const Blob* x, const Blob* g, hipStream_t s)
{
    return l->side(gate_api(), [&](const GateApi* api) {
        return api->apply(x->n, x->c, x->h, x->w, l->tops[0]->data, x->data, g->data, nullptr, FHIP_GATE_ACT_NONE, s);
    });
}

// Scale, scale_layer.h:33-98.  ncnn's `0=-233` with two bottoms takes the scale from the second bottom: the channel gate above (`gated`);
// such a layer is no per-channel affine map to any fusion.
struct ScaleLayer : AffineLayer
{
    int bias_term = 0, scale_data_size = 0;
    int LoadParam(const ParamDict& pd) override
    {
        scale_data_size = pd.get(0, 0);
        bias_term = pd.get(1, 0);
        if (scale_data_size == -233 && bottoms.size() == 2)
        {
            if (bias_term) return failf(NET_E_SHAPE, "layer %s: a Scale that takes its scale from a second bottom (0=-233) cannot have a bias term", name.c_str());
            if (tops.size() != 1) return failf(NET_E_SHAPE, "layer %s: a two-bottom Scale has one top", name.c_str());
            gated = true;
            return 0;
        }
        if (scale_data_size < 0) return failf(NET_E_SHAPE, "layer %s: negative scale data size is not accepted (scale_layer.h:37-41)", name.c_str());
        channels = scale_data_size;
        return 0;
    }
    int LoadWeights(ModelBin& mb) override
    {
        if (gated) return 0;
        int rc = mb.load(scale_data_size, 1, mul);
        if (rc) return rc;
        if (bias_term)
        {
            rc = mb.load(scale_data_size, 1, add);
            has_add = true;
        }
        return rc;
    }
    int Reshape() override { return gated ? gate_reshape(this, bottoms[0], bottoms[1]) : AffineLayer::Reshape(); }
    int Init(hipStream_t s) override { return gated ? 0 : AffineLayer::Init(s); }
    int Forward(hipStream_t s) override { return gated ? gate_forward(this, bottoms[0], bottoms[1], s) : AffineLayer::Forward(s); }
    int Fuse(Layer* next, int level) override { return gated ? 0 : AffineLayer::Fuse(next, level); }
    int algo() const override { return gated ? FHIP_NET_ROUTE_GATE : -1; }
};

// ncnn's BinaryOp: only 0=2 (mul) of a tensor and a per-plane scalar, in either order -- the multiply of a squeeze-and-excitation block
// as ncnn's converters write it.
struct BinaryOpLayer : Layer
{
    int LoadParam(const ParamDict& pd) override
    {
        if (pd.get(0, 0) != 2) return failf(NET_E_SHAPE, "layer %s: only BinaryOp mul (0=2) is supported", name.c_str());
        if (pd.get(1, 0)) return failf(NET_E_SHAPE, "layer %s: BinaryOp with a scalar operand is not supported", name.c_str());
        if (bottoms.size() != 2 || tops.size() != 1) return failf(NET_E_SHAPE, "layer %s: BinaryOp needs two bottoms and one top", name.c_str());
        return 0;
    }
    // whether the layer is a multiply of two blobs: what collapse_gate_blocks may take for an SE block's gate (always, here; the layer of a
    // net with fhip_net_set_transformer knows other ops)
    virtual bool multiplies() const { return true; }
    // the gate is the bottom with the 1 x 1 plane; two such bottoms: the second is the gate
    bool gate_first() const { return bottoms[0]->h == 1 && bottoms[0]->w == 1 && !(bottoms[1]->h == 1 && bottoms[1]->w == 1); }
    int Reshape() override { return gate_first() ? gate_reshape(this, bottoms[1], bottoms[0]) : gate_reshape(this, bottoms[0], bottoms[1]); }
    int Forward(hipStream_t s) override { return gate_first() ? gate_forward(this, bottoms[1], bottoms[0], s) : gate_forward(this, bottoms[0], bottoms[1], s); }
    int algo() const override { return FHIP_NET_ROUTE_GATE; }
};

// ncnn's Swish (no params) and HardSigmoid (0=alpha, 1=beta; defaults 0.2 and 0.5): one element-wise launch of libfeather_gate.so each.
struct GateActivationLayer : Layer
{
    int kind = FHIP_GATE_SWISH;
    float alpha = 0.2f, beta = 0.5f;
    int LoadParam(const ParamDict& pd) override
    {
        if (type == "Swish") return 0;
        kind = FHIP_GATE_HARDSIGMOID;
        alpha = pd.get(0, 0.2f);
        beta = pd.get(1, 0.5f);
        if (!std::isfinite(alpha) || !std::isfinite(beta)) return failf(NET_E_SHAPE, "layer %s: HardSigmoid needs finite alpha and beta", name.c_str());
        return 0;
    }
    int Reshape() override { return reshape_with(gate_api()); }
    int Forward(hipStream_t s) override
    {
        const Blob* b = bottoms[0];
        return side(gate_api(), [&](const GateApi* api) { return api->activation(kind, tops[0]->data, b->data, b->n, b->c, b->h * b->w, alpha, beta, s); });
    }
    int algo() const override { return FHIP_NET_ROUTE_GATE; }
};

// Fusion level 2 (collapse_gate_blocks): a whole squeeze-and-excitation block as one layer -- squeeze, excite, and the apply with the
// residual add and its ReLU folded in: at most three launches (four when the plane is large enough for the squeeze's split route) and
// four tensor-sized passes through HBM where the layers one by one make six.  It keeps the type and name of the block's Pooling layer and
// IS a PoolingLayer (q unchanged: global, average), so that whatever looks at a "Pooling" layer's parameters finds them.
// bottoms: the squeezed blob, the gated blob (two tops of one Split), then the shortcut if an Eltwise SUM was absorbed.
//
// The saving grows with the plane (two passes over n x C x HW floats) and the excite kernel's cost with n x C x R, where the dense layers
// of the block as written run on the GEMM: measured, the collapsed form loses where the hidden width is large against
// the plane (2048 x 7 x 7 with R = 128, 1152 x 7 x 7 with R = 48).  So the layer keeps the block's own layers in `parts` and, where
// 2 R > HW at Reshape, runs them one after the other as they were written (`stepwise`): the parent's pooling, dense layers, add and ReLU
// and the gate's multiply.  The blobs inside the block refuse Extract either way.
struct GateBlockLayer : PoolingLayer
{
    int C = 0, R = 0, mact = FHIP_EXCITE_MACT_NONE, gact = FHIP_EXCITE_GACT_SIGMOID, act = FHIP_GATE_ACT_NONE;
    float alpha = 0.2f, beta = 0.5f;
    bool has_b1 = false, has_b2 = false, inited = false, stepwise = false;
    std::vector<float> w1, b1, w2, b2;
    DeviceVec d_w1, d_b1, d_w2, d_b2, mean, gate;
    size_t scratch_bytes = 0;
    std::vector<std::unique_ptr<Layer>> parts; // the block's layers in the order of the list

    template <class Step>
    int each_part(const Step& step) // the stepwise form of a phase: the block's own layers one after the other, up to the first that fails
    {
        for (auto& l : parts)
            if (const int rc = step(l.get())) return rc;
        return 0;
    }
    int Reshape() override
    {
        const Blob* x = bottoms[0];
        const Blob* y = bottoms[1];
        if (x->c != C) return failf(NET_E_TOPOLOGY, "squeeze-and-excitation block %s has %d channels while bottom blob %s has %d", name.c_str(), C, x->name.c_str(), x->c);
        for (size_t i = 1; i < bottoms.size(); ++i)
            if (bottoms[i]->n != x->n || bottoms[i]->c != x->c || bottoms[i]->h != x->h || bottoms[i]->w != x->w)
                return failf(NET_E_SHAPE, "Shape mismatch among bottoms of layer %s.", name.c_str());
        stepwise = 2ll * R > (long long)x->h * x->w;
        scratch_bytes = 0;
        if (stepwise)
            return each_part([&](Layer* l) {
                const int rc = l->Reshape();
                if (!rc) scratch_bytes = std::max(scratch_bytes, l->arena_bytes());
                return rc;
            });
        int rc = side(gate_api(), [&](const GateApi* api) { return api->squeeze_buffer_size(x->n, x->c, x->h, x->w, &scratch_bytes); });
        if (rc) return rc;
        if ((rc = mean.resize((size_t)x->n * C * sizeof(float))) || (rc = gate.resize((size_t)x->n * C * sizeof(float)))) return rc;
        return tops[0]->reshape(y->n, y->c, y->h, y->w);
    }
    int Init(hipStream_t s) override
    {
        if (stepwise) return each_part([&](Layer* l) { return l->Init(s); });
        if (inited) return 0;
        int rc;
        if ((rc = d_w1.upload(w1.data(), w1.size(), s)) || (rc = d_w2.upload(w2.data(), w2.size(), s))) return rc;
        if (has_b1 && (rc = d_b1.upload(b1.data(), b1.size(), s))) return rc;
        if (has_b2 && (rc = d_b2.upload(b2.data(), b2.size(), s))) return rc;
        FHIP_CHECK_HIP(hipStreamSynchronize(s));
        inited = true;
        return 0;
    }
    int Forward(hipStream_t s) override
    {
        if (stepwise) return each_part([&](Layer* l) { return l->Forward(s); });
        const Blob* x = bottoms[0];
        return side(gate_api(), [&](const GateApi* api) {
            int rc = api->squeeze(x->n, x->c, x->h, x->w, mean.d, x->data, scratch_bytes ? net->arena.d : nullptr, s);
            if (!rc) rc = api->excite(x->n, C, R, gate.d, mean.d, d_w1.d, has_b1 ? d_b1.d : nullptr, d_w2.d, has_b2 ? d_b2.d : nullptr, mact, gact, alpha, beta, s);
            if (!rc) rc = api->apply(x->n, x->c, x->h, x->w, tops[0]->data, bottoms[1]->data, gate.d, bottoms.size() > 2 ? bottoms[2]->data : nullptr, act, s);
            return rc;
        });
    }
    size_t weight_bytes() const override
    {
        size_t b = d_w1.bytes + d_b1.bytes + d_w2.bytes + d_b2.bytes;
        if (stepwise)
            for (auto& l : parts) b += l->weight_bytes();
        return b;
    }
    size_t arena_bytes() const override { return scratch_bytes; }
    int algo() const override { return FHIP_NET_ROUTE_GATE; }
};

// ncnn's Interp in a net with fhip_net_set_extended_layers (feather_resample.h has the definition): 0 = resize_type (1 nearest, 2
// bilinear), 1 / 2 = height / width scale, 3 / 4 = output height / width, 6 = align_corner.  A second bottom gives the output size (its
// height and width) and the params 1 .. 4 are not looked at.  One launch of libfeather_resample.so; nothing is uploaded, so Forward
// only launches.
// Fusion level 2 (collapse_upsample_adds): the layer takes over the two-bottom Eltwise SUM that is the sole consumer of its top, and the
// plain ReLU behind that: `residual_at` is the bottom added after the resize, `relu` the ReLU after the sum -- FPN's upsample-and-add as
// one launch, the up-sampled tensor never written.
struct InterpLayer : Layer
{
    int mode = 0, out_h = 0, out_w = 0, align = 0;
    float hs = 1.f, ws = 1.f;
    size_t sized_by = 0;  // 0: the params; else the index of the bottom whose height and width the output takes
    int residual_at = -1; // index of the absorbed Eltwise operand among the bottoms, or -1
    bool relu = false;
    int LoadParam(const ParamDict& pd) override
    {
        if ((bottoms.size() != 1 && bottoms.size() != 2) || tops.size() != 1)
            return failf(NET_E_SHAPE, "layer %s: Interp needs one or two bottoms and one top, got %zu and %zu", name.c_str(), bottoms.size(), tops.size());
        mode = pd.get(0, 0);
        if (mode == 3) return failf(NET_E_SHAPE, "layer %s: Interp resize_type 3 (bicubic) is not supported", name.c_str());
        if (mode != FHIP_INTERP_NEAREST && mode != FHIP_INTERP_BILINEAR)
            return failf(NET_E_SHAPE, "layer %s: Interp resize_type %d is not supported (1 nearest, 2 bilinear)", name.c_str(), mode);
        if (pd.get(5, 0)) return failf(NET_E_SHAPE, "layer %s: Interp dynamic_target_size %d is not supported", name.c_str(), pd.get(5, 0));
        align = pd.get(6, 0) != 0;
        if (bottoms.size() == 2)
        {
            sized_by = 1;
            return 0;
        }
        hs = pd.get(1, 1.f);
        ws = pd.get(2, 1.f);
        out_h = pd.get(3, 0);
        out_w = pd.get(4, 0);
        if (out_h < 0 || out_w < 0) return failf(NET_E_SHAPE, "layer %s: Interp output size %d x %d: every dimension must be at least 1", name.c_str(), out_h, out_w);
        if ((long long)out_h * out_w >= (1ll << 31))
            return failf(NET_E_SHAPE, "layer %s: Interp output size %d x %d: tensors of 2^31 elements or more are not supported", name.c_str(), out_h, out_w);
        const float scale[2] = {hs, ws};
        const int given[2] = {out_h, out_w};
        for (int a = 0; a < 2; ++a)
        {
            if (given[a]) continue;
            if (!std::isfinite(scale[a]) || !(scale[a] > 0.f))
                return failf(NET_E_SHAPE, "layer %s: Interp %s scale %g must be finite and positive", name.c_str(), a ? "width" : "height", (double)scale[a]);
            if (!(scale[a] < 2147483648.f))
                return failf(NET_E_SHAPE, "layer %s: Interp %s scale %g gives an output dimension of 2^31 or more", name.c_str(), a ? "width" : "height", (double)scale[a]);
        }
        return 0;
    }
    int Reshape() override
    {
        const ResampleApi* api = resample_api();
        if (!api) return FHIP_E_UNSUPPORTED; // message set by resample_api
        const Blob* x = bottoms[0];
        int oh = 0, ow = 0;
        if (sized_by)
            oh = bottoms[sized_by]->h, ow = bottoms[sized_by]->w;
        else if (api->output_dim(x->h, x->w, hs, ws, out_h, out_w, &oh, &ow))
            return failf(NET_E_SHAPE, "layer %s: %s", name.c_str(), api->last_error());
        if (x->n < 1 || x->c < 1 || x->h < 1 || x->w < 1 || oh < 1 || ow < 1)
            return failf(NET_E_SHAPE, "layer %s: Interp %d x %d -> %d x %d: every dimension must be at least 1", name.c_str(), x->h, x->w, oh, ow);
        if ((long long)x->n * x->c * oh * ow >= (1ll << 31) || x->count() >= ((size_t)1 << 31))
            return failf(NET_E_SHAPE, "layer %s: Interp to %d x %d: tensors of 2^31 elements or more are not supported", name.c_str(), oh, ow);
        if (residual_at >= 0)
        {
            const Blob* r = bottoms[residual_at];
            if (r->n != x->n || r->c != x->c || r->h != oh || r->w != ow) return failf(NET_E_SHAPE, "Shape mismatch among bottoms of layer %s.", name.c_str());
        }
        return tops[0]->reshape(x->n, x->c, oh, ow);
    }
    int Forward(hipStream_t s) override
    {
        const Blob* x = bottoms[0];
        const Blob* t = tops[0];
        // a scale is handed on only where it decided the size
        return side(resample_api(), [&](const ResampleApi* api) {
            return api->interp(mode, align, x->n, x->c, x->h, x->w, t->h, t->w, sized_by || out_h ? 0.f : hs, sized_by || out_w ? 0.f : ws, t->data, x->data,
                               residual_at >= 0 ? bottoms[residual_at]->data : nullptr, relu, s);
        });
    }
    InterpLayer* as_interp() override { return this; }
    int algo() const override { return FHIP_NET_ROUTE_RESAMPLE; }
};

// ncnn's HardSwish in a net with fhip_net_set_extended_layers: 0 = alpha, 1 = beta (defaults 0.2 and 0.5; MobileNet-V3 writes 1/6 and
// 0.5).  One element-wise launch of libfeather_resample.so.
struct HardSwishLayer : Layer
{
    float alpha = 0.2f, beta = 0.5f;
    int LoadParam(const ParamDict& pd) override
    {
        if (bottoms.size() != 1 || tops.size() != 1)
            return failf(NET_E_SHAPE, "layer %s: HardSwish needs one bottom and one top, got %zu and %zu", name.c_str(), bottoms.size(), tops.size());
        alpha = pd.get(0, 0.2f);
        beta = pd.get(1, 0.5f);
        if (!std::isfinite(alpha) || !std::isfinite(beta) || alpha == 0.f)
            return failf(NET_E_SHAPE, "layer %s: HardSwish needs finite alpha and beta and alpha != 0, got %g and %g", name.c_str(), (double)alpha, (double)beta);
        return 0;
    }
    int Reshape() override { return reshape_with(resample_api()); }
    int Forward(hipStream_t s) override
    {
        const Blob* b = bottoms[0];
        return side(resample_api(), [&](const ResampleApi* api) { return api->hardswish(tops[0]->data, b->data, b->n, b->c, b->h * b->w, alpha, beta, s); });
    }
    int algo() const override { return FHIP_NET_ROUTE_RESAMPLE; }
};

// ncnn's LRN in a net with fhip_net_set_extended_layers (feather_lrn.h has the definition): 0 = region_type (0 across channels, 1 within
// channel), 1 = local_size (5), 2 = alpha (1), 3 = beta (0.75), 4 = bias (1).  One launch of libfeather_lrn.so; nothing is uploaded, so
// Forward only launches.
// Fusion level 2 (Fuse): the layer takes over the non-global Pooling layer that alone reads its top -- AlexNet's and GoogLeNet's norm -> pool
// -- and its top becomes the pooled tensor; the normalised one has no blob.  Up to kLrnOneLaunchMax elements it runs fhip_lrn_pool_forward:
// one launch, the normalised tensor never written.  Above, where that kernel measured slower than the two, and where the
// pooling window covers the whole unpadded plane (fhip_pooling's plane-reduce route, which the one launch does not restate), it runs
// fhip_lrn_forward into the net's scratch arena and fhip_pooling from there.  Both are bit for bit the two layers.
// GoogLeNet's conv2/norm2 at batch 4, the largest of the six measured tensors (0.19 M .. 2.4 M elements) at which one launch was faster than
// the pair; the next larger one measured (6.0 M, AlexNet's norm2 at batch 32) was slower
constexpr size_t kLrnOneLaunchMax = 4 * 192 * 56 * 56;
struct LRNLayer : Layer
{
    int region = 0, local_size = 5;
    float alpha = 1.f, beta = 0.75f, bias = 1.f;
    bool pooled = false; // q is the absorbed Pooling layer's
    size_t scratch_bytes = 0; // pooled, and too large for one launch to pay: the normalised tensor goes through the arena
    fhip_pool_param q;
    LRNLayer() { memset(&q, 0, sizeof(q)); }
    int LoadParam(const ParamDict& pd) override
    {
        if (bottoms.size() != 1 || tops.size() != 1)
            return failf(NET_E_SHAPE, "layer %s: LRN needs one bottom and one top, got %zu and %zu", name.c_str(), bottoms.size(), tops.size());
        region = pd.get(0, 0);
        local_size = pd.get(1, 5);
        alpha = pd.get(2, 1.f);
        beta = pd.get(3, 0.75f);
        bias = pd.get(4, 1.f);
        if (region != FHIP_LRN_ACROSS_CHANNELS && region != FHIP_LRN_WITHIN_CHANNEL)
            return failf(NET_E_SHAPE, "layer %s: LRN region_type %d is not supported (0 across channels, 1 within channel)", name.c_str(), region);
        if (local_size < 1 || local_size % 2 == 0)
            return failf(NET_E_SHAPE, "layer %s: LRN local_size %d must be odd and at least 1", name.c_str(), local_size);
        if (!std::isfinite(alpha) || !std::isfinite(beta) || !std::isfinite(bias))
            return failf(NET_E_SHAPE, "layer %s: LRN needs finite alpha, beta and bias, got %g, %g and %g", name.c_str(), (double)alpha, (double)beta, (double)bias);
        if (!(bias > 0.f) || alpha < 0.f)
            return failf(NET_E_SHAPE, "layer %s: LRN needs bias > 0 and alpha >= 0 (else bias + alpha * sum could be 0 or negative), got %g and %g", name.c_str(),
                         (double)bias, (double)alpha);
        return 0;
    }
    int Reshape() override
    {
        if (!lrn_api()) return FHIP_E_UNSUPPORTED; // message set by lrn_api
        const Blob* b = bottoms[0];
        if (b->n < 1 || b->c < 1 || b->h < 1 || b->w < 1) return failf(NET_E_SHAPE, "layer %s: LRN of an empty blob", name.c_str());
        if (b->count() >= ((size_t)1 << 31)) return failf(NET_E_SHAPE, "layer %s: LRN: tensors of 2^31 elements or more are not supported", name.c_str());
        scratch_bytes = 0;
        if (!pooled) return tops[0]->reshape(b->n, b->c, b->h, b->w);
        q.channels = b->c;
        q.input_h = b->h;
        q.input_w = b->w;
        int oh, ow;
        const int rc = fhip_pooling_output_dim(&q, &oh, &ow);
        if (rc) return rc;
        if (oh < 1 || ow < 1) return failf(NET_E_SHAPE, "layer %s: empty pooling output", name.c_str());
        // a window that covers the unpadded plane: fhip_pooling sums it in its plane-reduce order, which fhip_lrn_pool_forward does not restate
        // (and refuses): the pair, so that the layer keeps the bits of levels 0 and 1
        const bool whole_plane = oh == 1 && ow == 1 && q.pad_top + q.pad_bottom == 0 && q.pad_left + q.pad_right == 0 && q.kernel_h >= b->h && q.kernel_w >= b->w;
        if (b->count() > kLrnOneLaunchMax || whole_plane) scratch_bytes = b->count() * sizeof(float);
        return tops[0]->reshape(b->n, b->c, oh, ow);
    }
    int Forward(hipStream_t s) override
    {
        const Blob* b = bottoms[0];
        float* normalised = scratch_bytes ? net->arena.d : tops[0]->data;
        const int rc = side(lrn_api(), [&](const LrnApi* api) {
            return pooled && !scratch_bytes ? api->pool_forward(region, local_size, alpha, beta, bias, b->n, b->c, b->h, b->w, &q, tops[0]->data, b->data, s)
                                            : api->forward(region, local_size, alpha, beta, bias, b->n, b->c, b->h, b->w, normalised, b->data, s);
        });
        if (rc) return rc;
        return scratch_bytes ? fhip_pooling(&q, b->n, tops[0]->data, normalised, s) : 0;
    }
    size_t arena_bytes() const override { return scratch_bytes; }
    int Fuse(Layer* next, int level) override
    {
        if (level < 2 || pooled || !next->as_pooling()) return 0;
        const fhip_pool_param& p = next->as_pooling()->q;
        if (p.global_pooling || p.kernel_h < 1 || p.kernel_w < 1 || p.stride_h < 1 || p.stride_w < 1) return 0;
        if (p.pad_left < 0 || p.pad_right < 0 || p.pad_top < 0 || p.pad_bottom < 0) return 0;
        q = p;
        pooled = true;
        return 1;
    }
    int algo() const override { return FHIP_NET_ROUTE_LRN; }
};

// ncnn's Deconvolution / DeconvolutionDepthWise (no reference counterpart; the definition is include/feather_hip/feather_deconv.h).
// Runs through libfeather_deconv.so (deconv_api) with route code FHIP_NET_ROUTE_DECONV.  Fuses a following ReLU and, at level 2,
// BatchNorm / Scale (weights are [K][C/group][kh][kw], so the fold is the convolution's); it is no "Convolution" to any other fusion
// (residual add, pooling, depthwise + pointwise, siblings, Winograd chains, first layer, the side stream), which therefore decline it.
struct DeconvLayer : Layer
{
    typedef SideConv<DeconvApi, fhip_deconv_param> Route;
    fhip_deconv_param p;
    int weight_data_size = 0;
    std::vector<float> w_host, b_host;
    AffineFold fold; // folded BatchNorm/Scale (fusion level 2)
    DeviceVec packed, bias;
    size_t buffer_bytes = 0, packed_bytes = 0;
    BuiltFor built;

    DeconvLayer() { memset(&p, 0, sizeof(p)); }

    int LoadParam(const ParamDict& pd) override
    {
        const int dilation_w = pd.get(2, 1), dilation_h = pd.get(12, dilation_w);
        if (dilation_w > 1 || dilation_h > 1) return failf(NET_E_UNKNOWN_LAYER, "layer %s: dilated deconvolution is not supported", name.c_str());
        if (dilation_w < 1 || dilation_h < 1) return failf(NET_E_SHAPE, "layer %s: dilation must be >= 1", name.c_str());
        if (pd.get(8, 0)) return failf(NET_E_UNKNOWN_LAYER, "layer %s: int8 deconvolution is not supported", name.c_str());
        if (pd.get(20, 0) || pd.get(21, 0)) return failf(NET_E_UNKNOWN_LAYER, "layer %s: an explicit deconvolution output size is not supported", name.c_str());
        if (pd.get(9, 0)) return failf(NET_E_UNKNOWN_LAYER, "layer %s: a built-in activation (param 9) is not supported; use a ReLU layer", name.c_str());
        p.kernel_w = pd.get(1, 0);
        p.kernel_h = pd.get(11, p.kernel_w);
        p.stride_w = pd.get(3, 1);
        p.stride_h = pd.get(13, p.stride_w);
        p.pad_left = pd.get(4, 0);
        p.pad_right = pd.get(15, p.pad_left);
        p.pad_top = pd.get(14, p.pad_left);
        p.pad_bottom = pd.get(16, p.pad_top);
        p.output_pad_right = pd.get(18, 0);
        p.output_pad_bottom = pd.get(19, 0);
        p.group = pd.get(7, 1);
        p.output_channels = pd.get(0, 0);
        p.bias_term = pd.get(5, 0);
        p.activation = FHIP_ACT_NONE;
        weight_data_size = pd.get(6, 0);
        if (p.group < 1 || p.output_channels < 1 || p.output_channels % p.group)
            return failf(NET_E_SHAPE, "layer %s: output_channels is not divisible by its group", name.c_str());
        if (p.kernel_h <= 0 || p.kernel_w <= 0 || p.stride_h <= 0 || p.stride_w <= 0) return failf(NET_E_SHAPE, "layer %s: bad deconvolution geometry", name.c_str());
        long long per = (long long)p.output_channels * p.kernel_h; // three ints: the product is taken in two steps, each below 2^62
        if (per <= INT_MAX) per *= p.kernel_w;
        if (weight_data_size <= 0 || per > INT_MAX || ((long long)weight_data_size * p.group) % per)
            return failf(NET_E_SHAPE, "layer %s: weight_data_size does not fit the deconvolution geometry", name.c_str());
        p.input_channels = (int)((long long)weight_data_size * p.group / per);
        if (p.input_channels % p.group) return failf(NET_E_SHAPE, "layer %s: input_channels is not divisible by its group", name.c_str());
        if (p.pad_left < 0 || p.pad_right < 0 || p.pad_top < 0 || p.pad_bottom < 0)
            return failf(NET_E_SHAPE, "layer %s: negative (automatic) padding is not supported", name.c_str());
        if (p.output_pad_right < 0 || p.output_pad_bottom < 0 || p.output_pad_right >= p.stride_w || p.output_pad_bottom >= p.stride_h)
            return failf(NET_E_SHAPE, "layer %s: output padding must be smaller than the stride", name.c_str());
        if (p.output_pad_right > p.pad_right || p.output_pad_bottom > p.pad_bottom)
            return failf(NET_E_SHAPE, "layer %s: output padding larger than the padding of that side is not supported", name.c_str());
        return 0;
    }
    int LoadWeights(ModelBin& mb) override
    {
        built = BuiltFor(); // new weights: the packed form is rebuilt at the next Init
        int rc = mb.load((size_t)weight_data_size, 0, w_host);
        if (rc) return rc;
        if (p.bias_term) rc = mb.load(p.output_channels, 1, b_host);
        return rc;
    }
    int Reshape() override
    {
        const Blob* b = bottoms[0];
        if (p.input_channels != b->c)
            return failf(NET_E_TOPOLOGY, "deconvolution layer %s has %d input channels while bottom blob has %d channels", name.c_str(), p.input_channels, b->c);
        p.input_w = b->w;
        p.input_h = b->h;
        return Route::reshape<true>(this, deconv_api(), p, "deconvolution refused: ", &buffer_bytes, &packed_bytes);
    }
    int Init(hipStream_t s) override
    {
        const BuiltFor want{FHIP_NET_ROUTE_DECONV, 0, packed_bytes};
        if (built == want) return 0;
        std::vector<float> w = w_host, b = b_host;
        fold.apply(w, b, p.output_channels);
        if (!fold.empty()) p.bias_term = 1;
        const int rc = Route::init(this, deconv_api(), p, w, b, packed, packed_bytes, bias, s);
        if (!rc) built = want;
        return rc;
    }
    int Forward(hipStream_t s) override { return Route::forward(this, deconv_api(), p, packed, bias, s); }
    bool needs_weights() const override { return true; }
    int Fuse(Layer* next, int level) override;
    size_t weight_bytes() const override { return packed.bytes + bias.bytes; }
    int algo() const override { return FHIP_NET_ROUTE_DECONV; }
};

int DeconvLayer::Fuse(Layer* next, int level)
{
    if (is_plain_relu(next))
    {
        p.activation = FHIP_ACT_RELU;
        return 1;
    }
    if (level >= 2 && p.activation == FHIP_ACT_NONE && next->as_affine()) return fold.absorb(*next->as_affine(), p.output_channels) ? 1 : 0;
    return 0;
}

struct EltwiseLayer : Layer
{
    bool relu = false;
    EltwiseLayer* as_eltwise() override { return this; }
    int LoadParam(const ParamDict& pd) override // eltwise_layer.h:53-68
    {
        if (pd.has_array(1)) return failf(NET_E_SHAPE, "layer %s: coeffs in eltwise layer are not supported", name.c_str());
        if (pd.get(0, 0) != 1) return failf(NET_E_SHAPE, "layer %s: only eltwise SUM is supported", name.c_str());
        if (bottoms.size() < 2) return failf(NET_E_TOPOLOGY, "layer %s: eltwise needs two bottoms", name.c_str());
        return 0;
    }
    int Reshape() override
    {
        if (bottoms.size() < 2) return failf(NET_E_TOPOLOGY, "layer %s: eltwise needs two bottoms", name.c_str());
        const Blob* a = bottoms[0];
        for (size_t i = 1; i < bottoms.size(); ++i)
            if (bottoms[i]->n != a->n || bottoms[i]->c != a->c || bottoms[i]->h != a->h || bottoms[i]->w != a->w)
                return failf(NET_E_SHAPE, "Shape mismatch among bottoms of layer %s.", name.c_str());
        for (Blob* t : tops)
        {
            int rc = t->reshape(a->n, a->c, a->h, a->w);
            if (rc) return rc;
        }
        return 0;
    }
    int Forward(hipStream_t s) override // the reference adds bottoms 0 and 1 only (eltwise_layer.h:71-79)
    {
        return fhip_add(tops[0]->data, bottoms[0]->data, bottoms[1]->data, bottoms[0]->count(), relu, s);
    }
    int Fuse(Layer* next, int) override
    {
        if (!is_plain_relu(next)) return 0;
        relu = true;
        return 1;
    }
};

struct ConcatLayer : Layer
{
    int axis = 0;
    int LoadParam(const ParamDict& pd) override
    {
        axis = pd.get(0, 0);
        if (axis != 0) return failf(NET_E_SHAPE, "layer %s: only concat at axis = 0 (channels) is supported", name.c_str()); // concat_layer.h:70-73, at Reshape there
        return 0;
    }
    int Reshape() override // concat_layer.h:50-80
    {
        if (axis != 0) return failf(NET_E_SHAPE, "layer %s: only concat at axis = 0 (channels) is supported", name.c_str());
        const Blob* a = bottoms[0];
        int channels = a->c;
        for (size_t i = 1; i < bottoms.size(); ++i)
        {
            if (bottoms[i]->w != a->w || bottoms[i]->h != a->h || bottoms[i]->n != a->n)
                return failf(NET_E_SHAPE, "layer %s: images of different shapes cannot be concatenated together", name.c_str());
            channels += bottoms[i]->c;
        }
        return tops[0]->reshape(a->n, channels, a->h, a->w);
    }
    int Forward(hipStream_t s) override
    {
        Blob* t = tops[0];
        const size_t hw = (size_t)t->h * t->w;
        size_t c_off = 0;
        for (Blob* b : bottoms)
        {
            const size_t row = (size_t)b->c * hw * sizeof(float);
            FHIP_CHECK_HIP(hipMemcpy2DAsync(t->data + c_off * hw, (size_t)t->c * hw * sizeof(float), b->data, row, row, b->n, hipMemcpyDeviceToDevice, s));
            c_off += b->c;
        }
        return 0;
    }
};

// ncnn's ShuffleChannel (0=group, 1=reverse) and Slice (-23300=count,sizes..., 1=axis; channels only): no reference counterpart, the
// definitions are include/feather_hip/feather_shuffle.h.  Both are channel maps -- every output channel is one channel of one bottom -- and so
// is every chain of them with Concat: at fusion level 2 collapse_channel_maps() folds such a run into ONE layer of this type whose `steps`
// are the run in order, whose bottoms are the run's outside inputs and whose tops are the blobs that leave it.  Reshape evaluates the
// steps symbolically into the (source, source channel) table of every top and hands it to libfeather_shuffle.so, which keeps it on the
// device; Forward is one launch whatever the number of steps, bottoms and tops.  Route code FHIP_NET_ROUTE_SHUFFLE.
struct MapStep
{
    enum Kind
    {
        CONCAT,
        SHUFFLE,
        SLICE
    } kind = SHUFFLE;
    std::string name;
    int group = 1, reverse = 0;
    std::vector<int> sizes;
    std::vector<Blob*> bottoms, tops;
};

struct ChannelMapLayer : Layer
{
    std::vector<MapStep> steps;
    fhip_channel_map* map = nullptr;
    std::vector<int> built_src, built_entries; // what `map` was created from

    ~ChannelMapLayer() override { drop_map(); }
    void drop_map()
    {
        if (map)
            if (const ShuffleApi* api = shuffle_api()) api->destroy(map);
        map = nullptr;
    }
    int LoadParam(const ParamDict& pd) override
    {
        MapStep st;
        st.name = name;
        st.bottoms = bottoms;
        st.tops = tops;
        if (bottoms.size() != 1) return failf(NET_E_TOPOLOGY, "layer %s: a %s layer has one bottom", name.c_str(), type.c_str());
        if (type == "ShuffleChannel")
        {
            st.kind = MapStep::SHUFFLE;
            st.group = pd.get(0, 1);
            st.reverse = pd.get(1, 0);
            if (st.group < 1) return failf(NET_E_SHAPE, "layer %s: ShuffleChannel needs group >= 1", name.c_str());
            if (tops.size() != 1) return failf(NET_E_TOPOLOGY, "layer %s: a ShuffleChannel layer has one top", name.c_str());
        }
        else
        {
            st.kind = MapStep::SLICE;
            if (pd.get(1, 0) != 0) return failf(NET_E_SHAPE, "layer %s: only slice at axis = 0 (channels) is supported", name.c_str());
            if (!pd.has_array(0)) return failf(NET_E_SHAPE, "layer %s: Slice needs its sizes (-23300=count,...)", name.c_str());
            for (float v : pd.e[0].array)
            {
                if (v != (float)FHIP_SLICE_SHARE && !(v >= 1.f && v <= 16777216.f)) // the floats that hold every integer: no cast of inf or 1e30 to int
                    return failf(NET_E_SHAPE, "layer %s: a slice size must be positive or -233", name.c_str());
                st.sizes.push_back((int)v);
            }
            if (st.sizes.size() != tops.size())
                return failf(NET_E_TOPOLOGY, "layer %s: Slice has %d sizes and %d tops", name.c_str(), (int)st.sizes.size(), (int)tops.size());
            if (tops.size() > FHIP_CHANNEL_MAP_MAX_BLOBS)
                return failf(NET_E_SHAPE, "layer %s: a Slice into more than %d tops is not supported", name.c_str(), FHIP_CHANNEL_MAP_MAX_BLOBS);
        }
        steps.assign(1, st);
        return 0;
    }
    int Reshape() override
    {
        const ShuffleApi* api = shuffle_api();
        if (!api) return FHIP_E_UNSUPPORTED; // message set by shuffle_api
        const Blob* a = bottoms[0];
        typedef std::vector<std::pair<int, int>> Rows; // (bottom index, channel) per channel of a blob
        std::map<const Blob*, Rows> rows;
        for (size_t i = 0; i < bottoms.size(); ++i)
        {
            const Blob* b = bottoms[i];
            if (b->w != a->w || b->h != a->h || b->n != a->n)
                return failf(NET_E_SHAPE, "layer %s: images of different shapes cannot be concatenated together", name.c_str());
            Rows& r = rows[b];
            r.clear();
            for (int ch = 0; ch < b->c; ++ch) r.emplace_back((int)i, ch);
        }
        for (const MapStep& st : steps)
        {
            if (st.kind == MapStep::CONCAT)
            {
                Rows out;
                for (const Blob* b : st.bottoms) out.insert(out.end(), rows[b].begin(), rows[b].end());
                rows[st.tops[0]] = out;
                continue;
            }
            const Rows in = rows[st.bottoms[0]];
            const int c = (int)in.size();
            if (st.kind == MapStep::SHUFFLE)
            {
                if (c % st.group) return failf(NET_E_SHAPE, "layer %s: group %d does not divide the %d channels of its bottom", st.name.c_str(), st.group, c);
                const int g = st.reverse ? c / st.group : st.group, per = c / g; // the inverse of a shuffle by g is the shuffle by c / g
                Rows out(c);
                for (int i = 0; i < per; ++i)
                    for (int k = 0; k < g; ++k) out[i * g + k] = in[k * per + i];
                rows[st.tops[0]] = out;
                continue;
            }
            std::vector<int> resolved(st.sizes.size());
            if (api->resolve(c, st.sizes.data(), (int)st.sizes.size(), resolved.data()))
                return failf(NET_E_SHAPE, "layer %s (%d channels): %s", st.name.c_str(), c, api->last_error());
            int at = 0;
            for (size_t j = 0; j < resolved.size(); ++j)
            {
                rows[st.tops[j]] = Rows(in.begin() + at, in.begin() + at + resolved[j]);
                at += resolved[j];
            }
        }
        std::vector<int> src, out_c, entries;
        for (const Blob* b : bottoms) src.push_back(b->c);
        for (Blob* t : tops)
        {
            const Rows& r = rows[t];
            out_c.push_back((int)r.size());
            for (const auto& e : r)
            {
                entries.push_back(e.first);
                entries.push_back(e.second);
            }
            const int rc = t->reshape(a->n, (int)r.size(), a->h, a->w);
            if (rc) return rc;
        }
        if (map && src == built_src && entries == built_entries) return 0;
        drop_map();
        if (api->create(&map, src.data(), (int)src.size(), out_c.data(), (int)out_c.size(), entries.data()))
            return failf(FHIP_E_BADARG, "layer %s: %s", name.c_str(), api->last_error());
        built_src = src;
        built_entries = entries;
        return 0;
    }
    int Forward(hipStream_t s) override
    {
        float* outs[FHIP_CHANNEL_MAP_MAX_BLOBS];
        const float* srcs[FHIP_CHANNEL_MAP_MAX_BLOBS];
        for (size_t j = 0; j < tops.size(); ++j) outs[j] = tops[j]->data;
        for (size_t i = 0; i < bottoms.size(); ++i) srcs[i] = bottoms[i]->data;
        const Blob* a = bottoms[0];
        return side(shuffle_api(), [&](const ShuffleApi* api) { return api->forward(map, outs, srcs, a->n, a->h, a->w, s); });
    }
    int algo() const override { return FHIP_NET_ROUTE_SHUFFLE; }
};

struct SplitLayer : Layer
{
    bool reads_q8() const override { return true; } // the tops share the blob, whatever it holds
    bool writes_q8() const override { return bottoms[0]->q8; }
    int Reshape() override
    {
        for (Blob* t : tops) t->share(bottoms[0]);
        return 0;
    }
    int Forward(hipStream_t) override { return 0; } // tops alias the bottom (the reference memcpy's, split_layer.h:43-52)
};

struct DropoutLayer : Layer
{
    float scale = 1.f;
    DeviceVec d_scale;
    int LoadParam(const ParamDict& pd) override
    {
        scale = pd.get(0, 1.f);
        return 0;
    }
    int Reshape() override
    {
        if (scale == 1.f)
        {
            tops[0]->share(bottoms[0]);
            return 0;
        }
        return Layer::Reshape();
    }
    int Init(hipStream_t s) override
    {
        if (scale == 1.f || d_scale.d) return 0;
        std::vector<float> v(bottoms[0]->c, scale);
        int rc = d_scale.upload(v.data(), v.size(), s);
        if (rc) return rc;
        FHIP_CHECK_HIP(hipStreamSynchronize(s));
        return 0;
    }
    int Forward(hipStream_t s) override
    {
        if (scale == 1.f) return 0;
        const Blob* b = bottoms[0];
        return fhip_affine(tops[0]->data, b->data, d_scale.d, nullptr, b->n, b->c, b->h * b->w, 0, s);
    }
};

} // namespace fhip::net
