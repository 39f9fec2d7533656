// net_decoder.h -- the layers of a net with fhip_net_set_decoder (Net::decoder): ncnn's SDPA, RMSNorm, RotaryEmbed and Embed -- a decoder-only
// language model.  include/feather_hip/feather_decoder.h defines the kernels, libfeather_decoder.so holds them (decoder_api); the layers
// report the route FHIP_DECODER_NET_ROUTE.  Blobs carry ranks (Blob::dims, which fhip_net_set_detection maintains: the switch needs it):
// tokens are rank 2 [T][E], heads rank 3 [heads][T][d].  The rest of a LLaMA block is existing layers (the token-wise InnerProduct and the
// element-wise BinaryOp of fhip_net_set_transformer, Reshape, Permute, Split); Swish under this switch keeps its bottom's rank, which the
// default net's does not.  Nothing fuses into these layers.  A default net never creates one of these classes.
#pragma once
#include "feather_hip/feather_decoder.h" // declarations only: the library is opened at run time (decoder_api)
#include "net_stft.h"

namespace fhip::net
{

struct DecoderApi
{
    decltype(&fhip_sdpa_get_buffer_size) sdpa_size = nullptr;
    decltype(&fhip_sdpa_forward) sdpa = nullptr;
    decltype(&fhip_kv_concat_forward) kv_concat = nullptr;
    decltype(&fhip_rms_norm_forward) rms_norm = nullptr;
    decltype(&fhip_rotary_forward) rotary = nullptr;
    decltype(&fhip_embed_forward) embed = nullptr;
    decltype(&fhip_decoder_last_error) last_error = nullptr;
    SideLibrary library()
    {
        return {"libfeather_decoder.so", "a decoder layer (SDPA, RMSNorm, RotaryEmbed, Embed)", "feather_decoder.h",
                {{&sdpa_size, "fhip_sdpa_get_buffer_size"}, {&sdpa, "fhip_sdpa_forward"}, {&kv_concat, "fhip_kv_concat_forward"}, {&rms_norm, "fhip_rms_norm_forward"},
                 {&rotary, "fhip_rotary_forward"}, {&embed, "fhip_embed_forward"}, {&last_error, "fhip_decoder_last_error"}}};
    }
};
static const DecoderApi* decoder_api() { return side_api<DecoderApi>(); }

static size_t per_image(const Blob* b) { return (size_t)b->c * b->d * b->h * b->w; }

// ncnn's RMSNorm: 0=affine_size 1=eps (1e-6 here where absent) 2=affine (1); gamma raw when affine.  The rows are the bottom's last dimension.
struct RMSNormLayer : Layer
{
    int affine_size = 0, affine = 1, rows = 0;
    float eps = 1e-6f;
    std::vector<float> gamma;
    DeviceVec d_gamma;
    bool inited = false;
    int algo() const override { return FHIP_DECODER_NET_ROUTE; }
    int LoadParam(const ParamDict& pd) override
    {
        if (const int rc = one_to_one_counts(this)) return rc;
        affine_size = pd.get(0, 0), eps = pd.get(1, 1e-6f), affine = pd.get(2, 1);
        if (affine_size < 1) return failf(NET_E_SHAPE, "layer %s: RMSNorm affine_size (0=%d) must be positive", name.c_str(), affine_size);
        if (!(eps >= 0.f) || !isfinite(eps)) return failf(NET_E_SHAPE, "layer %s: RMSNorm eps (1=) must be finite and >= 0", name.c_str());
        if (affine != 0 && affine != 1) return failf(NET_E_SHAPE, "layer %s: RMSNorm affine (2=%d) must be 0 or 1", name.c_str(), affine);
        return 0;
    }
    bool needs_weights() const override { return affine != 0; }
    int LoadWeights(ModelBin& mb) override
    {
        inited = false;
        return affine ? mb.load((size_t)affine_size, 1, gamma) : 0;
    }
    int Reshape() override
    {
        if (!decoder_api()) return FHIP_E_UNSUPPORTED; // message set by decoder_api
        const Blob* b = bottoms[0];
        if (const int rc = attn_too_large(this, b)) return rc;
        if (b->w != affine_size)
            return failf(NET_E_SHAPE, "layer %s: RMSNorm affine_size %d is not the width %d of blob %s", name.c_str(), affine_size, b->w, b->name.c_str());
        rows = (int)(b->count() / (size_t)b->w);
        return reshape_like(tops[0], b);
    }
    int Init(hipStream_t s) override
    {
        if (inited || !affine) return 0;
        if (const int rc = d_gamma.upload(gamma.data(), gamma.size(), s)) return rc;
        FHIP_CHECK_HIP(hipStreamSynchronize(s));
        inited = true;
        return 0;
    }
    int Forward(hipStream_t s) override
    {
        return side(decoder_api(), [&](const DecoderApi* api) { return api->rms_norm(rows, affine_size, d_gamma.d, eps, tops[0]->data, bottoms[0]->data, s); });
    }
    size_t weight_bytes() const override { return d_gamma.bytes; }
};

// ncnn's RotaryEmbed: 0=interleaved; bottoms x (rank 3 [heads][T][d]), cos and sin ([T][d / 2] of any rank, one per image or one for the batch)
struct RotaryEmbedLayer : Layer
{
    int interleaved = 0, cs_stride = 0;
    int algo() const override { return FHIP_DECODER_NET_ROUTE; }
    int LoadParam(const ParamDict& pd) override
    {
        if (bottoms.size() != 3 || tops.size() != 1)
            return failf(NET_E_SHAPE, "layer %s: RotaryEmbed needs three bottoms (x, cos, sin) and one top, got %zu and %zu", name.c_str(), bottoms.size(), tops.size());
        interleaved = pd.get(0, 0);
        if (interleaved != 0 && interleaved != 1) return failf(NET_E_SHAPE, "layer %s: RotaryEmbed interleaved (0=%d) must be 0 or 1", name.c_str(), interleaved);
        return 0;
    }
    int Reshape() override
    {
        if (!decoder_api()) return FHIP_E_UNSUPPORTED;
        const Blob *x = bottoms[0], *c = bottoms[1], *sn = bottoms[2];
        if (const int rc = attn_too_large(this, x)) return rc;
        if (x->dims != 3 || x->w % 2)
            return failf(NET_E_SHAPE, "layer %s: RotaryEmbed needs a blob of rank 3 [heads][T][d] with d even, blob %s has rank %d and (%d, %d, %d)", name.c_str(), x->name.c_str(),
                         x->dims, x->c, x->h, x->w);
        const size_t want = (size_t)x->h * (x->w / 2);
        for (const Blob* b : {c, sn})
            if (per_image(b) != want || (b->n != 1 && b->n != x->n))
                return failf(NET_E_SHAPE, "layer %s: RotaryEmbed needs cos and sin of T * d / 2 = %zu floats, for the batch or per image; blob %s has %zu and batch %d", name.c_str(),
                             want, b->name.c_str(), per_image(b), b->n);
        if (c->n != sn->n) return failf(NET_E_SHAPE, "layer %s: RotaryEmbed: cos and sin differ in batch", name.c_str());
        cs_stride = c->n == 1 ? 0 : (int)want;
        return reshape_like(tops[0], x);
    }
    int Forward(hipStream_t s) override
    {
        const Blob* x = bottoms[0];
        return side(decoder_api(), [&](const DecoderApi* api) {
            return api->rotary(x->n, x->c, x->h, x->w, interleaved, bottoms[1]->data, bottoms[2]->data, cs_stride, tops[0]->data, x->data, s);
        });
    }
};

// ncnn's Embed: 0=num_output 1=input_dim 2=bias_term 3=weight_data_size; the weight tagged [input_dim][num_output], the bias raw.  The bottom
// holds int32 bit patterns in the float blob, T of them an image (any rank); the top is rank 2 [T][num_output].
struct EmbedLayer : Layer
{
    int E = 0, vocab = 0, bias_term = 0;
    std::vector<float> w_host, b_host;
    DeviceVec d_w, d_b;
    bool inited = false;
    int algo() const override { return FHIP_DECODER_NET_ROUTE; }
    bool needs_weights() const override { return true; }
    int LoadParam(const ParamDict& pd) override
    {
        if (const int rc = one_to_one_counts(this)) return rc;
        E = pd.get(0, 0), vocab = pd.get(1, 0), bias_term = pd.get(2, 0);
        if (E < 1 || vocab < 1) return failf(NET_E_SHAPE, "layer %s: Embed num_output (0=%d) and input_dim (1=%d) must be positive", name.c_str(), E, vocab);
        if (bias_term != 0 && bias_term != 1) return failf(NET_E_SHAPE, "layer %s: Embed bias_term (2=%d) must be 0 or 1", name.c_str(), bias_term);
        if ((long long)E * vocab >= (1ll << 31)) return failf(NET_E_SHAPE, "layer %s: Embed: tensors of 2^31 elements or more are not supported", name.c_str());
        if ((long long)pd.get(3, 0) != (long long)E * vocab)
            return failf(NET_E_SHAPE, "layer %s: Embed weight_data_size (3=%d) must be num_output * input_dim (%lld)", name.c_str(), pd.get(3, 0), (long long)E * vocab);
        return 0;
    }
    int LoadWeights(ModelBin& mb) override
    {
        inited = false;
        const int rc = mb.load((size_t)E * vocab, 0, w_host);
        return rc || !bias_term ? rc : mb.load((size_t)E, 1, b_host);
    }
    int Reshape() override
    {
        if (!decoder_api()) return FHIP_E_UNSUPPORTED;
        const Blob* b = bottoms[0];
        const size_t T = per_image(b);
        if (T < 1 || T * (size_t)b->n * E >= ((size_t)1 << 31)) return failf(NET_E_SHAPE, "layer %s: Embed: tensors of 2^31 elements or more are not supported", name.c_str());
        const int rc = tops[0]->reshape(b->n, 1, (int)T, E);
        tops[0]->dims = 2;
        return rc;
    }
    int Init(hipStream_t s) override
    {
        if (inited) return 0;
        int rc = d_w.upload(w_host.data(), w_host.size(), s);
        if (!rc && bias_term) rc = d_b.upload(b_host.data(), b_host.size(), s);
        if (rc) return rc;
        FHIP_CHECK_HIP(hipStreamSynchronize(s));
        inited = true;
        return 0;
    }
    int Forward(hipStream_t s) override
    {
        const Blob* t = tops[0];
        return side(decoder_api(), [&](const DecoderApi* api) { return api->embed(t->n * t->h, E, vocab, (const int*)bottoms[0]->data, d_w.d, d_b.d, t->data, s); });
    }
    size_t weight_bytes() const override { return d_w.bytes + d_b.bytes; }
};

// ncnn's SDPA: 5=attn_mask 6=scale (0: 1 / sqrt(d)) 7=kv_cache.  Bottoms: q [heads][Tq][d], k and v [kv_heads][Tn][d] (rank 3), then the mask
// if 5=1 (rank 2 [Tq][Tk], or rank 3 [heads or 1][Tq][Tk]; batch n or 1), then past_k and past_v [kv_heads][Tp][d] if 7=1.  Tops: out
// [heads][Tq][d], and with 7=1 present_k and present_v [kv_heads][Tp + Tn][d]: one concat launch per cache, then the core over the present
// blobs.  Causal attention is a mask here, as in ncnn.  The split route's scratch lies in the net's arena.
struct SdpaLayer : Layer
{
    int with_mask = 0, cache = 0, tp = 0;
    float scale = 0.f;
    fhip_sdpa_desc desc;
    size_t scratch = 0;
    int algo() const override { return FHIP_DECODER_NET_ROUTE; }
    int LoadParam(const ParamDict& pd) override
    {
        with_mask = pd.get(5, 0), scale = pd.get(6, 0.f), cache = pd.get(7, 0);
        if ((with_mask != 0 && with_mask != 1) || (cache != 0 && cache != 1))
            return failf(NET_E_SHAPE, "layer %s: SDPA attn_mask (5=%d) and kv_cache (7=%d) must be 0 or 1", name.c_str(), with_mask, cache);
        if (!isfinite(scale)) return failf(NET_E_SHAPE, "layer %s: SDPA scale (6=) must be finite", name.c_str());
        const size_t nb = 3 + (size_t)with_mask + 2 * (size_t)cache, nt = 1 + 2 * (size_t)cache;
        if (bottoms.size() != nb || tops.size() != nt)
            return failf(NET_E_SHAPE, "layer %s: SDPA with 5=%d 7=%d needs %zu bottoms (q, k, v%s%s) and %zu tops, got %zu and %zu", name.c_str(), with_mask, cache, nb,
                         with_mask ? ", mask" : "", cache ? ", past_k, past_v" : "", nt, bottoms.size(), tops.size());
        return 0;
    }
    int Reshape() override
    {
        const DecoderApi* api = decoder_api();
        if (!api) return FHIP_E_UNSUPPORTED;
        const Blob *q = bottoms[0], *k = bottoms[1], *v = bottoms[2];
        const char* ln = name.c_str();
        for (size_t i = 0; i < bottoms.size(); ++i)
        {
            const Blob* b = bottoms[i];
            if (const int rc = attn_too_large(this, b)) return rc;
            if (with_mask && i == 3) continue;
            if (b->dims != 3) return failf(NET_E_SHAPE, "layer %s: SDPA needs blobs of rank 3 [heads][T][d], blob %s has rank %d and (%d, %d, %d)", ln, b->name.c_str(), b->dims, b->c, b->h, b->w);
            if (b->n != q->n) return failf(NET_E_SHAPE, "layer %s: SDPA: blob %s has batch %d, q has %d", ln, b->name.c_str(), b->n, q->n);
        }
        if (v->w != q->w || k->w != q->w) return failf(NET_E_SHAPE, "layer %s: SDPA needs one head width for q, k and v (a dv other than d is not supported), got %d, %d and %d", ln, q->w, k->w, v->w);
        if (v->c != k->c || v->h != k->h) return failf(NET_E_SHAPE, "layer %s: SDPA: k and v differ in heads or length", ln);
        if (q->c % k->c) return failf(NET_E_SHAPE, "layer %s: SDPA: %d heads are no multiple of %d kv heads", ln, q->c, k->c);
        tp = 0;
        if (cache)
        {
            const Blob *pk = bottoms[3 + with_mask], *pv = bottoms[4 + with_mask];
            if (pk->c != k->c || pk->w != k->w || pv->c != k->c || pv->w != k->w || pv->h != pk->h)
                return failf(NET_E_SHAPE, "layer %s: SDPA: the past blobs %s and %s do not fit k [%d][T][%d]", ln, pk->name.c_str(), pv->name.c_str(), k->c, k->w);
            tp = pk->h;
        }
        const long long tk = (long long)tp + k->h;
        if ((long long)q->n * k->c * tk * k->w >= (1ll << 31)) return failf(NET_E_SHAPE, "layer %s: SDPA: tensors of 2^31 elements or more are not supported", ln);
        memset(&desc, 0, sizeof(desc));
        desc.n = q->n, desc.heads = q->c, desc.kv_heads = k->c, desc.tq = q->h, desc.tk = (int)tk, desc.d = q->w;
        desc.q_row_stride = desc.k_row_stride = desc.v_row_stride = desc.out_row_stride = q->w;
        desc.q_head_stride = desc.out_head_stride = q->h * q->w, desc.q_image_stride = desc.out_image_stride = q->c * q->h * q->w;
        desc.k_head_stride = desc.v_head_stride = (int)tk * k->w, desc.k_image_stride = desc.v_image_stride = k->c * (int)tk * k->w;
        desc.scale = scale != 0.f ? scale : 1.f / sqrtf((float)q->w);
        if (with_mask)
        {
            const Blob* m = bottoms[3];
            const bool fits = (m->dims == 2 || m->dims == 3) && m->h == q->h && m->w == tk && (m->c == 1 || (m->dims == 3 && m->c == q->c)) && (m->n == 1 || m->n == q->n);
            if (!fits)
                return failf(NET_E_SHAPE, "layer %s: SDPA: the mask %s (rank %d, batch %d, (%d, %d, %d)) is not [%d][%lld] of rank 2, or [%d or 1][%d][%lld] of rank 3, for the batch or per image",
                             ln, m->name.c_str(), m->dims, m->n, m->c, m->h, m->w, q->h, tk, q->c, q->h, tk);
            desc.mask_head_stride = m->c == 1 ? 0 : m->h * m->w;
            desc.mask_image_stride = m->n == 1 ? 0 : m->c * m->h * m->w;
        }
        if (api->sdpa_size(&desc, &scratch, nullptr)) return failf(NET_E_SHAPE, "layer %s: SDPA: %s", ln, api->last_error());
        if (const int rc = reshape_like(tops[0], q)) return rc;
        for (int i = 1; i <= 2 * cache; ++i)
        {
            if (const int rc = tops[i]->reshape(q->n, k->c, (int)tk, k->w)) return rc;
            tops[i]->dims = 3;
        }
        return 0;
    }
    int Forward(hipStream_t s) override
    {
        const Blob *q = bottoms[0], *k = bottoms[1], *v = bottoms[2];
        const float *keys = k->data, *values = v->data;
        if (cache)
        {
            for (int i = 0; i < 2; ++i)
                if (const int rc = side(decoder_api(), [&](const DecoderApi* api) {
                        return api->kv_concat(q->n, k->c, tp, k->h, k->w, tp ? bottoms[3 + with_mask + i]->data : nullptr, bottoms[1 + i]->data, tops[1 + i]->data, s);
                    }))
                    return rc;
            keys = tops[1]->data, values = tops[2]->data;
        }
        return side(decoder_api(), [&](const DecoderApi* api) {
            return api->sdpa(&desc, q->data, keys, values, with_mask ? bottoms[3]->data : nullptr, tops[0]->data, scratch ? net->arena.d : nullptr, s);
        });
    }
    size_t arena_bytes() const override { return scratch; }
};

// Swish on a blob of any rank: the default net's layer with the bottom's rank kept
struct RankedSwishLayer : GateActivationLayer
{
    int Reshape() override
    {
        const int dims = bottoms[0]->dims;
        const int rc = GateActivationLayer::Reshape();
        tops[0]->dims = dims;
        return rc;
    }
};

// The layer types of a net with fhip_net_set_decoder (Net::decoder).  load_param_text asks here before create_layer, and only when the switch
// is on: Swish is a type a default net knows too.
static Layer* create_decoder_layer(const std::string& type)
{
    if (type == "SDPA") return new SdpaLayer;
    if (type == "RMSNorm") return new RMSNormLayer;
    if (type == "RotaryEmbed") return new RotaryEmbedLayer;
    if (type == "Embed") return new EmbedLayer;
    if (type == "Swish") return new RankedSwishLayer;
    return nullptr;
}

} // namespace fhip::net
