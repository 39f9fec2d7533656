// net_attn.h -- the layers of a net with fhip_net_set_transformer (Net::transformer): ncnn's MemoryData, LayerNorm, GELU, MultiHeadAttention, the
// element-wise BinaryOp and the InnerProduct that runs once per token -- a Vision Transformer encoder.  include/feather_hip/feather_attn.h
// defines the kernels, libfeather_attn.so holds them (attn_api); every GEMM is the main library's (fhip_conv_forward, IM2COL: a 1x1
// convolution over a 1x1 image whose batch is the number of tokens).  The new layers report the route FHIP_ATTN_NET_ROUTE.  A blob of tokens
// is a blob of rank 2, [n][1][T][E] (Blob::dims, which fhip_net_set_detection maintains: the switch needs it).  One fusion (level >= 2,
// collapse_add_norms): the residual add in front of a Split one of whose tops a LayerNorm alone reads runs with that LayerNorm in one launch,
// bit for bit.  A default net never creates one of these classes.
#pragma once
#include "feather_hip/feather_attn.h" // declarations only: the library is opened at run time (attn_api)
#include "net_detect.h"

namespace fhip::net
{

// libfeather_attn.so, the layers of a net with fhip_net_set_transformer
struct AttnApi
{
    decltype(&fhip_attention_forward) attention = nullptr;
    decltype(&fhip_layer_norm_forward) layer_norm = nullptr;
    decltype(&fhip_add_layer_norm_forward) add_layer_norm = nullptr;
    decltype(&fhip_gelu_forward) gelu = nullptr;
    decltype(&fhip_binary_forward) binary = nullptr;
    decltype(&fhip_attn_last_error) last_error = nullptr;
    SideLibrary library()
    {
        return {"libfeather_attn.so", "a transformer layer (MultiHeadAttention, LayerNorm, GELU, BinaryOp)", "feather_attn.h",
                {{&attention, "fhip_attention_forward"}, {&layer_norm, "fhip_layer_norm_forward"}, {&add_layer_norm, "fhip_add_layer_norm_forward"},
                 {&gelu, "fhip_gelu_forward"}, {&binary, "fhip_binary_forward"}, {&last_error, "fhip_attn_last_error"}}};
    }
};
static const AttnApi* attn_api() { return side_api<AttnApi>(); }

static int attn_too_large(const Layer* l, const Blob* b)
{
    if (b->count() < ((size_t)1 << 31)) return 0;
    return failf(NET_E_SHAPE, "layer %s: %s: tensors of 2^31 elements or more are not supported", l->name.c_str(), l->type.c_str());
}

// top takes b's shape and rank, with storage of its own
static int reshape_like(Blob* top, const Blob* b)
{
    const int dims = b->dims;
    const int rc = top->reshape(b->n, b->c, b->h, b->w);
    top->dims = dims;
    return rc;
}

// ncnn's MemoryData: 0=w 1=h 2=c, w * h * c raw floats: a constant (the class token, the position embedding).  The top holds one copy per
// image of the net's input batch, written when the shapes are planned -- at Init, which runs outside a captured graph -- and never again.
struct MemoryDataLayer : Layer
{
    int w = 0, h = 0, c = 0;
    std::vector<float> host;
    const float* written_to = nullptr;
    int written_n = 0;
    int algo() const override { return FHIP_ATTN_NET_ROUTE; }
    size_t elements() const { return (size_t)w * std::max(h, 1) * std::max(c, 1); }
    int LoadParam(const ParamDict& pd) override
    {
        if (!bottoms.empty() || tops.size() != 1) return failf(NET_E_SHAPE, "layer %s: MemoryData has no bottom and one top, got %zu and %zu", name.c_str(), bottoms.size(), tops.size());
        w = pd.get(0, 0), h = pd.get(1, 0), c = pd.get(2, 0);
        if (w < 1 || h < 0 || c < 0 || (c > 0 && h == 0)) return failf(NET_E_SHAPE, "layer %s: MemoryData needs w (0=%d) >= 1, and h (1=%d) where it has c (2=%d)", name.c_str(), w, h, c);
        if ((long long)w * std::max(h, 1) >= (1ll << 31) || (long long)w * std::max(h, 1) * std::max(c, 1) >= (1ll << 31))
            return failf(NET_E_SHAPE, "layer %s: MemoryData of 2^31 elements or more is not supported", name.c_str());
        return 0;
    }
    bool needs_weights() const override { return true; }
    int LoadWeights(ModelBin& mb) override
    {
        written_to = nullptr;
        return mb.load(elements(), 1, host);
    }
    int Reshape() override
    {
        int n = 0;
        for (auto& l : net->layers)
            if (l->type == "Input" && !l->tops.empty() && n == 0) n = l->tops[0]->n;
        if (n < 1) return failf(NET_E_SHAPE, "layer %s: MemoryData takes its batch from the net's first Input, which has not been fed", name.c_str());
        if ((size_t)n * elements() >= ((size_t)1 << 31)) return failf(NET_E_SHAPE, "layer %s: MemoryData: tensors of 2^31 elements or more are not supported", name.c_str());
        const int rc = tops[0]->reshape(n, std::max(c, 1), std::max(h, 1), w);
        tops[0]->dims = c ? 3 : (h ? 2 : 1);
        return rc;
    }
    int Init(hipStream_t s) override
    {
        Blob* t = tops[0];
        if (written_to == t->data && written_n == t->n) return 0;
        std::vector<float> all((size_t)t->n * host.size());
        for (int i = 0; i < t->n; ++i) memcpy(all.data() + (size_t)i * host.size(), host.data(), host.size() * sizeof(float));
        FHIP_CHECK_HIP(hipMemcpyAsync(t->data, all.data(), all.size() * sizeof(float), hipMemcpyHostToDevice, s));
        FHIP_CHECK_HIP(hipStreamSynchronize(s)); // `all` goes with this call
        written_to = t->data, written_n = t->n;
        return 0;
    }
    int Forward(hipStream_t) override { return 0; }
    size_t weight_bytes() const override { return 0; } // the top is a blob
};

// ncnn's LayerNorm: 0=affine_size 1=eps (0.001) 2=affine (1); gamma then beta, raw, when affine.  The rows are the bottom's last dimension
// (affine_size == w) or, on a blob of rank 3, its planes (affine_size == h * w).
struct LayerNormLayer : Layer
{
    int affine_size = 0, affine = 1, rows = 0, L = 0;
    float eps = 0.001f;
    std::vector<float> gamma, beta;
    DeviceVec d_gamma, d_beta;
    bool inited = false;
    int algo() const override { return FHIP_ATTN_NET_ROUTE; }
    int LoadParam(const ParamDict& pd) override
    {
        if (const int rc = one_to_one_counts(this)) return rc;
        affine_size = pd.get(0, 0), eps = pd.get(1, 0.001f), affine = pd.get(2, 1);
        if (affine_size < 1) return failf(NET_E_SHAPE, "layer %s: LayerNorm affine_size (0=%d) must be positive", name.c_str(), affine_size);
        if (!(eps >= 0.f) || !isfinite(eps)) return failf(NET_E_SHAPE, "layer %s: LayerNorm eps (1=) must be finite and >= 0", name.c_str());
        if (affine != 0 && affine != 1) return failf(NET_E_SHAPE, "layer %s: LayerNorm affine (2=%d) must be 0 or 1", name.c_str(), affine);
        return 0;
    }
    bool needs_weights() const override { return affine != 0; }
    int LoadWeights(ModelBin& mb) override
    {
        if (!affine) return 0;
        inited = false;
        const int rc = mb.load((size_t)affine_size, 1, gamma);
        return rc ? rc : mb.load((size_t)affine_size, 1, beta);
    }
    // rows and L for a bottom b; the top takes its shape
    int plan(const Blob* b, Blob* top)
    {
        if (!attn_api()) return FHIP_E_UNSUPPORTED; // message set by attn_api
        if (const int rc = attn_too_large(this, b)) return rc;
        if (affine_size == b->w) L = b->w;
        else if (b->dims == 3 && (long long)affine_size == (long long)b->h * b->w) L = affine_size;
        else
            return failf(NET_E_SHAPE, "layer %s: LayerNorm affine_size %d is neither the width %d of blob %s nor, on a blob of rank 3, its plane (%d x %d)", name.c_str(),
                         affine_size, b->w, b->name.c_str(), b->h, b->w);
        rows = (int)(b->count() / (size_t)L);
        return reshape_like(top, b);
    }
    int Reshape() override { return plan(bottoms[0], tops[0]); }
    int Init(hipStream_t s) override
    {
        if (inited || !affine) return 0;
        int rc = d_gamma.upload(gamma.data(), gamma.size(), s);
        if (!rc) rc = d_beta.upload(beta.data(), beta.size(), s);
        if (rc) return rc;
        FHIP_CHECK_HIP(hipStreamSynchronize(s));
        inited = true;
        return 0;
    }
    int Forward(hipStream_t s) override
    {
        return side(attn_api(), [&](const AttnApi* api) { return api->layer_norm(rows, L, d_gamma.d, d_beta.d, eps, tops[0]->data, bottoms[0]->data, s); });
    }
    size_t weight_bytes() const override { return d_gamma.bytes + d_beta.bytes; }
};

// ncnn's GELU: 0=fast_gelu
struct GeluLayer : Layer
{
    int fast = 0;
    int algo() const override { return FHIP_ATTN_NET_ROUTE; }
    int LoadParam(const ParamDict& pd) override
    {
        if (const int rc = one_to_one_counts(this)) return rc;
        fast = pd.get(0, 0);
        if (fast != 0 && fast != 1) return failf(NET_E_SHAPE, "layer %s: GELU fast_gelu (0=%d) must be 0 or 1", name.c_str(), fast);
        return 0;
    }
    int Reshape() override
    {
        if (!attn_api()) return FHIP_E_UNSUPPORTED; // message set by attn_api
        if (const int rc = attn_too_large(this, bottoms[0])) return rc;
        return reshape_like(tops[0], bottoms[0]);
    }
    int Forward(hipStream_t s) override
    {
        return side(attn_api(), [&](const AttnApi* api) { return api->gelu(fast, tops[0]->data, bottoms[0]->data, bottoms[0]->count(), s); });
    }
};

// ncnn's BinaryOp in a net with the switch: 0=op_type (0 add .. 5 min) 1=with_scalar 2=b.  One bottom and a scalar; two bottoms of one shape; or
// two bottoms of which one holds a single image's worth, broadcast over the other's batch.  The multiply of a blob of rank 3 by a
// [n][c][1][1] gate stays what it is without the switch: BinaryOpLayer's code, route and bits.  norm: the LayerNorm this add runs with
// (collapse_add_norms); its top is this layer's second top.
struct ElementwiseLayer : BinaryOpLayer
{
    int op = 0, with_scalar = 0, form = FHIP_BINARY_TENSOR, swap = 0;
    float scalar = 0.f;
    bool gate = false;
    std::unique_ptr<LayerNormLayer> norm;
    int LoadParam(const ParamDict& pd) override
    {
        op = pd.get(0, 0), with_scalar = pd.get(1, 0), scalar = pd.get(2, 0.f);
        if (op < FHIP_BINARY_ADD || op > FHIP_BINARY_MIN)
            return failf(NET_E_SHAPE, "layer %s: BinaryOp op_type (0=%d) must be 0 (add), 1 (sub), 2 (mul), 3 (div), 4 (max) or 5 (min)", name.c_str(), op);
        if (with_scalar != 0 && with_scalar != 1) return failf(NET_E_SHAPE, "layer %s: BinaryOp with_scalar (1=%d) must be 0 or 1", name.c_str(), with_scalar);
        if (tops.size() != 1 || bottoms.size() != (with_scalar ? 1u : 2u))
            return failf(NET_E_SHAPE, "layer %s: BinaryOp needs one top and %s, got %zu and %zu", name.c_str(), with_scalar ? "one bottom beside its scalar" : "two bottoms",
                         tops.size(), bottoms.size());
        return 0;
    }
    bool is_gate() const
    {
        if (op != FHIP_BINARY_MUL || with_scalar || bottoms[0]->dims != 3 || bottoms[1]->dims != 3) return false;
        const Blob *x = gate_first() ? bottoms[1] : bottoms[0], *g = gate_first() ? bottoms[0] : bottoms[1];
        return g->h == 1 && g->w == 1 && g->n == x->n && g->c == x->c;
    }
    int Reshape() override
    {
        gate = is_gate();
        if (gate) return BinaryOpLayer::Reshape();
        if (!attn_api()) return FHIP_E_UNSUPPORTED; // message set by attn_api
        const Blob* a = bottoms[0];
        swap = 0;
        if (with_scalar) form = FHIP_BINARY_SCALAR;
        else
        {
            const Blob* b = bottoms[1];
            if (a->dims != b->dims || a->c != b->c || a->h != b->h || a->w != b->w || (a->n != b->n && a->n != 1 && b->n != 1))
                return failf(NET_E_SHAPE, "layer %s: BinaryOp needs bottoms of one shape (or one of them a single image), got %s [%d][%d][%d][%d] and %s [%d][%d][%d][%d]",
                             name.c_str(), a->name.c_str(), a->n, a->c, a->h, a->w, b->name.c_str(), b->n, b->c, b->h, b->w);
            form = a->n == b->n ? FHIP_BINARY_TENSOR : FHIP_BINARY_BROADCAST;
            swap = form == FHIP_BINARY_BROADCAST && a->n == 1; // the first operand is the one broadcast: y op x
            if (swap) a = b;
            if (const int rc = attn_too_large(this, b)) return rc;
        }
        if (const int rc = attn_too_large(this, a)) return rc;
        if (const int rc = reshape_like(tops[0], a)) return rc;
        return norm ? norm->plan(tops[0], tops[1]) : 0;
    }
    int Init(hipStream_t s) override { return norm ? norm->Init(s) : 0; }
    int Forward(hipStream_t s) override
    {
        if (gate) return BinaryOpLayer::Forward(s);
        const Blob *x = swap ? bottoms[1] : bottoms[0], *y = with_scalar ? nullptr : (swap ? bottoms[0] : bottoms[1]);
        if (norm && form == FHIP_BINARY_TENSOR)
            return side(attn_api(), [&](const AttnApi* api) {
                return api->add_layer_norm(norm->rows, norm->L, norm->d_gamma.d, norm->d_beta.d, norm->eps, tops[0]->data, tops[1]->data, x->data, y->data, s);
            });
        const int rc = side(attn_api(), [&](const AttnApi* api) {
            return api->binary(op, form, swap, tops[0]->data, x->data, y ? y->data : nullptr, scalar, x->count(), y ? y->count() : 0, s);
        });
        if (rc || !norm) return rc;
        return side(attn_api(), [&](const AttnApi* api) { return api->layer_norm(norm->rows, norm->L, norm->d_gamma.d, norm->d_beta.d, norm->eps, tops[1]->data, tops[0]->data, s); });
    }
    bool multiplies() const override { return op == FHIP_BINARY_MUL && !with_scalar; }
    bool plain_add() const { return op == FHIP_BINARY_ADD && !with_scalar && !norm; }
    size_t weight_bytes() const override { return norm ? norm->weight_bytes() : 0; }
    int algo() const override { return gate ? FHIP_NET_ROUTE_GATE : FHIP_ATTN_NET_ROUTE; }
};

// InnerProduct in a net with the switch: a bottom of rank 2 [T][F] with F == input_size gives a top of rank 2 [T][num_output] -- the same
// GEMM with n * T columns, ReLU fusion as ever.  Every other bottom behaves as without the switch.
struct TokenInnerProductLayer : InnerProductLayer
{
    bool tokens = false;
    int Reshape() override
    {
        const Blob* b = bottoms[0];
        tokens = !quant && b->dims == 2 && (size_t)b->w == input_size;
        if (!tokens) return InnerProductLayer::Reshape();
        const long long columns = (long long)b->n * b->h;
        if (b->count() >= ((size_t)1 << 31) || columns * (long long)output_size >= (1ll << 31))
            return failf(NET_E_SHAPE, "layer %s: InnerProduct: tensors of 2^31 elements or more are not supported", name.c_str());
        const int rc = tops[0]->reshape(b->n, 1, b->h, (int)output_size);
        tops[0]->dims = 2;
        if (rc) return rc;
        return fhip_conv_get_buffer_size(&p, FHIP_IM2COL, (int)columns, &buffer_bytes, &packed_bytes);
    }
    int Forward(hipStream_t s) override
    {
        if (!tokens) return InnerProductLayer::Forward(s);
        return fhip_conv_forward(&p, FHIP_IM2COL, bottoms[0]->n * bottoms[0]->h, tops[0]->data, bottoms[0]->data, packed.d, (float*)net->arena.d,
                                 p.bias_term ? bias.d : nullptr, s);
    }
};

// ncnn's MultiHeadAttention: 0=embed_dim 1=num_heads 2=weight_data_size 3=kdim 4=vdim 5=attn_mask 6=scale (1 / sqrt(d)); weights q, k, v, out,
// each a tagged [E][E] matrix and a raw bias.  Bottoms: 1 (self-attention), 2 (q, then k = v) or 3 (q, k, v), each of rank 2 [T][E].  The
// projections of bottoms that are one blob run as ONE GEMM onto the concatenated rows (self-attention: n * T columns onto 3E outputs), the
// scale folded into the q rows and the q bias; then the attention core reads that buffer in place, and the output projection writes the top.
// Every buffer between them lies in the net's arena, behind the GEMMs' own scratch.
struct MultiHeadAttentionLayer : Layer
{
    struct Gemm // outputs [first, first + count) x E of the concatenated q / k / v rows, applied to bottom `from`
    {
        fhip_conv_param p;
        int from = 0, first = 0;
        DeviceVec packed, bias;
        size_t buffer_bytes = 0, packed_bytes = 0, at = 0; // at: floats from the projections' start
        bool built = false;
    };
    int E = 0, heads = 1;
    float scale = 0.f;
    std::vector<float> w_host, b_host, wo_host, bo_host; // [3E][E] and [3E] with the scale folded in; the output projection
    std::vector<std::unique_ptr<Gemm>> proj;
    Gemm out;
    size_t scratch = 0, proj_floats = 0, total = 0; // the arena: GEMM scratch (bytes) | projections | the attention's output
    int algo() const override { return FHIP_ATTN_NET_ROUTE; }
    bool needs_weights() const override { return true; }
    static void as_gemm(Gemm& g, int outputs, int inputs)
    {
        memset(&g.p, 0, sizeof(g.p));
        g.p.input_channels = inputs, g.p.output_channels = outputs, g.p.bias_term = 1;
        g.p.input_h = g.p.input_w = g.p.kernel_h = g.p.kernel_w = g.p.stride_h = g.p.stride_w = g.p.group = 1;
        fhip_conv_assign_output_dim(&g.p);
    }
    int LoadParam(const ParamDict& pd) override
    {
        if (bottoms.empty() || bottoms.size() > 3 || tops.size() != 1)
            return failf(NET_E_SHAPE, "layer %s: MultiHeadAttention needs one to three bottoms and one top, got %zu and %zu", name.c_str(), bottoms.size(), tops.size());
        E = pd.get(0, 0), heads = pd.get(1, 1);
        const int wsize = pd.get(2, 0), kdim = pd.get(3, E), vdim = pd.get(4, E);
        if (E < 1 || heads < 1) return failf(NET_E_SHAPE, "layer %s: MultiHeadAttention embed_dim (0=%d) and num_heads (1=%d) must be positive", name.c_str(), E, heads);
        if (E % heads) return failf(NET_E_SHAPE, "layer %s: MultiHeadAttention embed_dim %d is no multiple of num_heads %d", name.c_str(), E, heads);
        if (pd.get(5, 0)) return failf(NET_E_SHAPE, "layer %s: MultiHeadAttention with an attention mask (5=%d) is not supported", name.c_str(), pd.get(5, 0));
        if (kdim != E || vdim != E) return failf(NET_E_SHAPE, "layer %s: MultiHeadAttention kdim (3=%d) and vdim (4=%d) must equal embed_dim %d", name.c_str(), kdim, vdim, E);
        if ((long long)wsize != (long long)E * E) return failf(NET_E_SHAPE, "layer %s: MultiHeadAttention weight_data_size (2=%d) must be embed_dim^2 (%lld)", name.c_str(), wsize, (long long)E * E);
        if ((long long)E * E * 3 >= (1ll << 31)) return failf(NET_E_SHAPE, "layer %s: MultiHeadAttention: tensors of 2^31 elements or more are not supported", name.c_str());
        scale = pd.get(6, 1.f / sqrtf((float)(E / heads)));
        // which bottoms are one blob decides the GEMMs: q k v of one blob -> one; q and k = v -> two; three blobs -> three
        const Blob *q = bottoms[0], *k = bottoms.size() > 1 ? bottoms[1] : q, *v = bottoms.size() > 2 ? bottoms[2] : k;
        const Blob* src[3] = {q, k, v};
        proj.clear();
        for (int i = 0; i < 3; ++i)
        {
            if (i && src[i] == src[i - 1])
            {
                as_gemm(*proj.back(), proj.back()->p.output_channels + E, E);
                continue;
            }
            proj.emplace_back(new Gemm);
            as_gemm(*proj.back(), E, E);
            proj.back()->from = (int)std::min<size_t>(i, bottoms.size() - 1), proj.back()->first = i;
        }
        as_gemm(out, E, E);
        return 0;
    }
    int LoadWeights(ModelBin& mb) override
    {
        const size_t ee = (size_t)E * E;
        w_host.assign(3 * ee, 0.f), b_host.assign(3 * (size_t)E, 0.f);
        std::vector<float> w, b;
        for (int i = 0; i < 4; ++i)
        {
            int rc = mb.load(ee, 0, w);
            if (!rc) rc = mb.load((size_t)E, 1, b);
            if (rc) return rc;
            if (i == 3)
            {
                wo_host.swap(w), bo_host.swap(b);
                break;
            }
            const float f = i == 0 ? scale : 1.f; // ncnn scales q after its bias: (W x + b) * scale
            for (size_t j = 0; j < ee; ++j) w_host[i * ee + j] = i == 0 ? w[j] * f : w[j];
            for (int j = 0; j < E; ++j) b_host[(size_t)i * E + j] = i == 0 ? b[j] * f : b[j];
        }
        for (auto& g : proj) g->built = false;
        out.built = false;
        return 0;
    }
    int Reshape() override
    {
        if (!attn_api()) return FHIP_E_UNSUPPORTED; // message set by attn_api
        const Blob *q = bottoms[0], *k = bottoms.size() > 1 ? bottoms[1] : q, *v = bottoms.size() > 2 ? bottoms[2] : k;
        for (const Blob* b : {q, k, v})
            if (b->dims != 2 || b->w != E)
                return failf(NET_E_SHAPE, "layer %s: MultiHeadAttention needs blobs of rank 2 [T][%d], blob %s has rank %d and (%d, %d, %d)", name.c_str(), E, b->name.c_str(),
                             b->dims, b->c, b->h, b->w);
        if (k->n != q->n || v->n != q->n || v->h != k->h)
            return failf(NET_E_SHAPE, "layer %s: MultiHeadAttention: q, k and v differ in batch, or k and v in length", name.c_str());
        if ((long long)q->n * std::max(q->h, k->h) * 3 * E >= (1ll << 31))
            return failf(NET_E_SHAPE, "layer %s: MultiHeadAttention: tensors of 2^31 elements or more are not supported", name.c_str());
        scratch = 0, proj_floats = 0;
        for (auto& g : proj)
        {
            const Blob* b = bottoms[g->from];
            if (const int rc = fhip_conv_get_buffer_size(&g->p, FHIP_IM2COL, b->n * b->h, &g->buffer_bytes, &g->packed_bytes)) return rc;
            scratch = std::max(scratch, g->buffer_bytes);
            g->at = proj_floats;
            proj_floats += round_up_sz((size_t)b->n * b->h * g->p.output_channels, 64);
        }
        if (const int rc = fhip_conv_get_buffer_size(&out.p, FHIP_IM2COL, q->n * q->h, &out.buffer_bytes, &out.packed_bytes)) return rc;
        scratch = round_up_sz(std::max(scratch, out.buffer_bytes), 256);
        total = scratch + (proj_floats + (size_t)q->n * q->h * E) * sizeof(float);
        return reshape_like(tops[0], q);
    }
    int Init(hipStream_t s) override
    {
        const size_t ee = (size_t)E * E;
        for (auto& g : proj)
        {
            if (g->built) continue;
            const size_t rows = (size_t)g->p.output_channels;
            const std::vector<float> w(w_host.begin() + g->first * ee, w_host.begin() + g->first * ee + rows * E), b(b_host.begin() + (size_t)g->first * E, b_host.begin() + (size_t)g->first * E + rows);
            if (const int rc = init_main(g->p, FHIP_IM2COL, w, b, g->packed, g->packed_bytes, g->bias, s)) return rc;
            g->built = true;
        }
        if (!out.built)
        {
            if (const int rc = init_main(out.p, FHIP_IM2COL, wo_host, bo_host, out.packed, out.packed_bytes, out.bias, s)) return rc;
            out.built = true;
        }
        return 0;
    }
    int Forward(hipStream_t s) override
    {
        float* gemm_scratch = (float*)net->arena.d;
        float* base = (float*)((char*)net->arena.d + scratch);
        float* core = base + proj_floats;
        const Blob *q = bottoms[0], *k = bottoms.size() > 1 ? bottoms[1] : q;
        const float* at[3] = {nullptr, nullptr, nullptr};
        int stride[3] = {0, 0, 0};
        for (auto& g : proj)
        {
            const Blob* b = bottoms[g->from];
            if (const int rc = fhip_conv_forward(&g->p, FHIP_IM2COL, b->n * b->h, base + g->at, b->data, g->packed.d, gemm_scratch, g->bias.d, s)) return rc;
            for (int i = g->first; i < g->first + g->p.output_channels / E; ++i) at[i] = base + g->at + (size_t)(i - g->first) * E, stride[i] = g->p.output_channels;
        }
        const int rc = side(attn_api(), [&](const AttnApi* api) {
            return api->attention(q->n, heads, q->h, k->h, E, at[0], stride[0], at[1], stride[1], at[2], stride[2], core, s);
        });
        if (rc) return rc;
        return fhip_conv_forward(&out.p, FHIP_IM2COL, q->n * q->h, tops[0]->data, core, out.packed.d, gemm_scratch, out.bias.d, s);
    }
    size_t weight_bytes() const override
    {
        size_t b = out.packed.bytes + out.bias.bytes;
        for (auto& g : proj) b += g->packed.bytes + g->bias.bytes;
        return b;
    }
    size_t arena_bytes() const override { return total; }
};

// The layer types of a net with fhip_net_set_transformer (Net::transformer).  load_param_text asks here before create_layer, and only when the
// switch is on: BinaryOp and InnerProduct are types a default net knows too.
static Layer* create_transformer_layer(const std::string& type)
{
    if (type == "MemoryData") return new MemoryDataLayer;
    if (type == "LayerNorm") return new LayerNormLayer;
    if (type == "GELU") return new GeluLayer;
    if (type == "MultiHeadAttention") return new MultiHeadAttentionLayer;
    if (type == "BinaryOp") return new ElementwiseLayer;
    if (type == "InnerProduct") return new TokenInnerProductLayer;
    return nullptr;
}

// Fusion level >= 2: BinaryOp add (two bottoms) -> Split -> {LayerNorm, others}, the residual of an encoder block.  The LayerNorm that alone
// reads one of the Split's tops moves into the add (ElementwiseLayer::norm): one launch writes the sum and its normalisation, bit for bit the
// two.  The Split stays -- its tops alias the sum and launch nothing -- and every blob stays extractable.
static void collapse_add_norms(Net& net)
{
    for (size_t i = 0; i < net.layers.size(); ++i)
    {
        ElementwiseLayer* add = dynamic_cast<ElementwiseLayer*>(net.layers[i].get());
        if (!add || !add->plain_add()) continue;
        const int split = readers(net, add->tops[0], i + 1).sole();
        if (split < 0 || net.layers[split]->type != "Split") continue;
        for (Blob* t : net.layers[split]->tops)
        {
            const int reader = readers(net, t, split + 1).sole();
            LayerNormLayer* ln = reader < 0 ? nullptr : dynamic_cast<LayerNormLayer*>(net.layers[reader].get());
            if (!ln) continue;
            add->tops.push_back(ln->tops[0]);
            add->norm.reset(static_cast<LayerNormLayer*>(net.layers[reader].release()));
            net.layers.erase(net.layers.begin() + reader);
            break;
        }
    }
}

} // namespace fhip::net
