// net_gemm.h -- the layers of a net with fhip_net_set_gemm (Net::gemm): ncnn's Gemm and MatMul, the product of two run-time matrices -- what
// pnnx writes for torch.matmul, bmm, einsum, F.linear with a computed weight and un-fused attention, and what ONNX graphs are full of.
// include/feather_hip/feather_gemm.h defines the kernels, libfeather_gemm.so holds them (gemm_api); the layers report the route
// FHIP_GEMM_NET_ROUTE.  Blobs carry ranks (Blob::dims, which fhip_net_set_detection maintains: the switch needs it).  Every call is one launch
// into the net's blobs, no scratch; nothing fuses into or out of the two layers.  A default net never creates one of these classes.
#pragma once
#include "feather_hip/feather_gemm.h" // declarations only: the library is opened at run time (gemm_api)
#include "net_decoder.h"

namespace fhip::net
{

struct GemmApi
{
    decltype(&fhip_gemm_forward) forward = nullptr;
    decltype(&fhip_gemm_route) route = nullptr;
    decltype(&fhip_gemm_last_error) last_error = nullptr;
    SideLibrary library()
    {
        return {"libfeather_gemm.so", "a matrix product layer (Gemm, MatMul)", "feather_gemm.h",
                {{&forward, "fhip_gemm_forward"}, {&route, "fhip_gemm_route"}, {&last_error, "fhip_gemm_last_error"}}};
    }
};
static const GemmApi* gemm_api() { return side_api<GemmApi>(); }

// the library's own checks, at Reshape: a description it refuses never reaches Forward
static int gemm_accepts(const Layer* l, const GemmApi* api, const fhip_gemm_desc& desc)
{
    char route[96];
    return api->route(&desc, route, (int)sizeof(route)) ? failf(NET_E_SHAPE, "layer %s: %s: %s", l->name.c_str(), l->type.c_str(), api->last_error()) : 0;
}

// ncnn's MatMul: 0=transB; two bottoms, numpy's rules per image of the net's batch.  rank 1 . rank 1: a dot product, the top of rank 1 with
// w = 1; rank 2 . rank 2: [M][K] [K][N]; rank 1 . rank 2: A is a row, the top [N] of rank 1; rank 2 . rank 1: B is a column, the top [M] of
// rank 1; rank 3 on either side: a batch over c, an operand of rank 2 (or of c = 1) broadcast to it with batch stride 0, the top of rank 3.
// transB reads B's last two dimensions as [N][K] and has no effect on a B of rank 1.  One launch where one batch stride per operand
// describes the net's batch and the batch over c together, else one launch per image.
struct MatMulLayer : Layer
{
    int transB = 0, images = 1;
    size_t a_image = 0, b_image = 0, d_image = 0;
    fhip_gemm_desc desc;
    int algo() const override { return FHIP_GEMM_NET_ROUTE; }
    int LoadParam(const ParamDict& pd) override
    {
        if (bottoms.size() != 2 || tops.size() != 1)
            return failf(NET_E_SHAPE, "layer %s: MatMul needs two bottoms and one top, got %zu and %zu", name.c_str(), bottoms.size(), tops.size());
        transB = pd.get(0, 0);
        if (transB != 0 && transB != 1) return failf(NET_E_SHAPE, "layer %s: MatMul transB (0=%d) must be 0 or 1", name.c_str(), transB);
        return 0;
    }
    int Reshape() override
    {
        const GemmApi* api = gemm_api();
        if (!api) return FHIP_E_UNSUPPORTED; // message set by gemm_api
        const Blob *a = bottoms[0], *b = bottoms[1];
        const char* ln = name.c_str();
        for (const Blob* x : {a, b})
        {
            if (const int rc = attn_too_large(this, x)) return rc;
            if (x->dims < 1 || x->dims > 3) return failf(NET_E_SHAPE, "layer %s: MatMul takes blobs of rank 1 to 3, blob %s has rank %d", ln, x->name.c_str(), x->dims);
        }
        if (a->n != b->n) return failf(NET_E_SHAPE, "layer %s: MatMul: blob %s has batch %d, blob %s has %d", ln, a->name.c_str(), a->n, b->name.c_str(), b->n);
        const int ra = a->dims, rb = b->dims, M = ra == 1 ? 1 : a->h, K = a->w, ca = ra == 3 ? a->c : 1, cb = rb == 3 ? b->c : 1;
        const bool b_rows_are_n = rb == 1 || transB; // a column of K floats is [1][K] read as [N][K]
        const int N = rb == 1 ? 1 : (transB ? b->h : b->w), Kb = rb == 1 || transB ? b->w : b->h;
        if (K != Kb) return failf(NET_E_SHAPE, "layer %s: MatMul: K differs, blob %s gives %d and blob %s gives %d", ln, a->name.c_str(), K, b->name.c_str(), Kb);
        const bool batched = ra == 3 || rb == 3;
        if (batched && (ra == 1 || rb == 1)) return failf(NET_E_SHAPE, "layer %s: MatMul of a blob of rank 1 with a blob of rank 3 is not supported", ln);
        if (ca != cb && ca != 1 && cb != 1) return failf(NET_E_SHAPE, "layer %s: MatMul: the batch extents %d and %d are neither equal nor 1", ln, ca, cb);
        const int bc = std::max(ca, cb);
        if ((size_t)a->n * bc * M * N >= ((size_t)1 << 31)) return failf(NET_E_SHAPE, "layer %s: MatMul: tensors of 2^31 elements or more are not supported", ln);
        memset(&desc, 0, sizeof(desc));
        desc.m = M, desc.n = N, desc.k = K, desc.trans_b = b_rows_are_n, desc.c_broadcast = -1, desc.alpha = 1.f;
        desc.lda = K, desc.ldb = b_rows_are_n ? K : N, desc.ldd = N;
        a_image = (size_t)ca * M * K, b_image = (size_t)cb * K * N, d_image = (size_t)bc * M * N;
        if ((ca == bc && cb == bc) || a->n == 1)
            images = 1, desc.batch = a->n * bc;
        else
            images = a->n, desc.batch = bc;
        desc.a_batch_stride = ca == bc ? M * K : 0, desc.b_batch_stride = cb == bc ? K * N : 0, desc.d_batch_stride = M * N;
        if (const int rc = gemm_accepts(this, api, desc)) return rc;
        Blob* t = tops[0];
        const int rc = batched ? t->reshape(a->n, bc, M, N) : (ra == 2 && rb == 2 ? t->reshape(a->n, 1, M, N) : t->reshape(a->n, 1, 1, ra == 2 ? M : N));
        t->dims = batched ? 3 : (ra == 2 && rb == 2 ? 2 : 1);
        return rc;
    }
    int Forward(hipStream_t s) override
    {
        for (int i = 0; i < images; ++i)
            if (const int rc = side(gemm_api(), [&](const GemmApi* api) {
                    return api->forward(&desc, bottoms[0]->data + i * a_image, bottoms[1]->data + i * b_image, nullptr, tops[0]->data + i * d_image, s);
                }))
                return rc;
        return 0;
    }
};

// ncnn's Gemm: 0=alpha 1=beta 2=transA 3=transB 4=constantA 5=constantB 6=constantC 7=M 8=N 9=K 10=constant_broadcast_type_C
// 14=output_transpose.  The bottoms are the non-constant ones among A, B, C in that order (a C bottom is optional); constant operands come
// from the .bin in the order A, B, C, each tagged, fp32 only, uploaded once and broadcast to the net's batch with stride 0.  Bottoms are of
// rank 2, a bottom of rank 1 is a row; a C bottom takes its broadcast type from its shape as ncnn does.  The top is [M][N], or [N][M] with
// 14=1, of rank 2.
struct GemmLayer : Layer
{
    float alpha = 1.f, beta = 1.f;
    int transA = 0, transB = 0, constA = 0, constB = 0, constC = 0, cM = 0, cN = 0, cK = 0, c_type = 0, out_t = 0;
    bool c_bottom = false, inited = false;
    std::vector<float> host[3];
    DeviceVec dev[3];
    fhip_gemm_desc desc;
    int algo() const override { return FHIP_GEMM_NET_ROUTE; }
    size_t const_count(int which) const
    {
        if (which == 0) return constA ? (size_t)cM * cK : 0;
        if (which == 1) return constB ? (size_t)cN * cK : 0;
        if (!constC || c_type < 0) return 0;
        return c_type == 0 ? 1 : (c_type == 3 ? (size_t)cM * cN : (size_t)(c_type == 4 ? cN : cM));
    }
    int LoadParam(const ParamDict& pd) override
    {
        const char* ln = name.c_str();
        alpha = pd.get(0, 1.f), beta = pd.get(1, 1.f), transA = pd.get(2, 0), transB = pd.get(3, 0);
        constA = pd.get(4, 0), constB = pd.get(5, 0), constC = pd.get(6, 0), cM = pd.get(7, 0), cN = pd.get(8, 0), cK = pd.get(9, 0);
        c_type = pd.get(10, 0), out_t = pd.get(14, 0);
        if (pd.get(11, 0)) return failf(NET_E_SHAPE, "layer %s: Gemm output_N1M (11=%d) is not supported", ln, pd.get(11, 0));
        if (pd.get(12, 0) || pd.get(13, 0)) return failf(NET_E_SHAPE, "layer %s: Gemm output_elempack and output_elemtype (12=%d 13=%d) must be 0", ln, pd.get(12, 0), pd.get(13, 0));
        if (pd.get(18, 0)) return failf(FHIP_E_UNSUPPORTED, "layer %s: Gemm with int8 weights (18=int8_scale_term %d) is not supported", ln, pd.get(18, 0));
        for (const int flag : {transA, transB, constA, constB, constC, out_t})
            if (flag != 0 && flag != 1) return failf(NET_E_SHAPE, "layer %s: Gemm transA, transB, constantA, constantB, constantC and output_transpose (2= 3= 4= 5= 6= 14=) must be 0 or 1", ln);
        if (!isfinite(alpha) || !isfinite(beta)) return failf(NET_E_SHAPE, "layer %s: Gemm alpha and beta (0= 1=) must be finite", ln);
        if (constC && (c_type < -1 || c_type > 4)) return failf(NET_E_SHAPE, "layer %s: Gemm constant_broadcast_type_C (10=%d) must be -1 .. 4", ln, c_type);
        const bool need_m = constA || (constC && (c_type == 1 || c_type == 2 || c_type == 3)), need_n = constB || (constC && (c_type == 3 || c_type == 4));
        if ((need_m && cM < 1) || (need_n && cN < 1) || ((constA || constB) && cK < 1) || (long long)std::max(cM, 1) * std::max(cK, 1) >= (1ll << 31) ||
            (long long)std::max(cN, 1) * std::max(cK, 1) >= (1ll << 31) || (long long)std::max(cM, 1) * std::max(cN, 1) >= (1ll << 31))
            return failf(NET_E_SHAPE, "layer %s: Gemm constant operands need M, N, K (7=%d 8=%d 9=%d) positive, each matrix below 2^31 elements", ln, cM, cN, cK);
        const size_t need = (size_t)!constA + (size_t)!constB;
        c_bottom = !constC && bottoms.size() == need + 1;
        if (tops.size() != 1 || bottoms.empty() || (bottoms.size() != need && !c_bottom))
            return failf(NET_E_SHAPE, "layer %s: Gemm with 4=%d 5=%d 6=%d needs %zu bottom(s)%s and one top, got %zu and %zu", ln, constA, constB, constC, need,
                         constC ? "" : " (one more for C)", bottoms.size(), tops.size());
        return 0;
    }
    bool needs_weights() const override { return const_count(0) + const_count(1) + const_count(2) > 0; }
    int LoadWeights(ModelBin& mb) override
    {
        inited = false;
        for (int i = 0; i < 3; ++i)
        {
            host[i].clear();
            if (!const_count(i)) continue;
            uint32_t tag = 0;
            if ((size_t)(mb.end - mb.p) >= 4) memcpy(&tag, mb.p, 4);
            if (tag == 0x01306B47u) return failf(FHIP_E_UNSUPPORTED, "layer %s: Gemm: fp16-tagged weights are not supported (fp32 only)", name.c_str());
            if (const int rc = mb.load(const_count(i), 0, host[i])) return rc;
        }
        return 0;
    }
    int Reshape() override
    {
        const GemmApi* api = gemm_api();
        if (!api) return FHIP_E_UNSUPPORTED;
        const char* ln = name.c_str();
        size_t next = 0;
        const Blob *a = constA ? nullptr : bottoms[next++], *b = constB ? nullptr : bottoms[next++], *c = c_bottom ? bottoms[next++] : nullptr;
        const int n = bottoms[0]->n;
        for (const Blob* x : bottoms)
        {
            if (const int rc = attn_too_large(this, x)) return rc;
            if (x->dims != 1 && x->dims != 2) return failf(NET_E_SHAPE, "layer %s: Gemm takes bottoms of rank 1 or 2, blob %s has rank %d", ln, x->name.c_str(), x->dims);
            if (x->n != n) return failf(NET_E_SHAPE, "layer %s: Gemm: blob %s has batch %d, blob %s has %d", ln, x->name.c_str(), x->n, bottoms[0]->name.c_str(), n);
        }
        const int M = a ? (transA ? a->w : a->h) : cM, Ka = a ? (transA ? a->h : a->w) : cK;
        const int N = b ? (transB ? b->h : b->w) : cN, Kb = b ? (transB ? b->w : b->h) : cK;
        if (Ka != Kb) return failf(NET_E_SHAPE, "layer %s: Gemm: K differs, A gives %d and B gives %d", ln, Ka, Kb);
        if ((constC && c_type >= 0 && ((c_type >= 1 && c_type <= 3 && cM != M) || (c_type >= 3 && cN != N))))
            return failf(NET_E_SHAPE, "layer %s: Gemm: the constant C was written for M %d, N %d, the product is %d x %d", ln, cM, cN, M, N);
        int type = constC ? c_type : -1;
        if (c) // ncnn's rule: the shape says how C broadcasts
        {
            if (c->dims == 1 && c->w == 1) type = 0;
            else if (c->dims == 1 && c->w == M) type = 1;
            else if (c->dims == 1 && c->w == N) type = 4;
            else if (c->dims == 2 && c->w == 1 && c->h == M) type = 2;
            else if (c->dims == 2 && c->w == N && c->h == M) type = 3;
            else if (c->dims == 2 && c->w == N && c->h == 1) type = 4;
            else return failf(NET_E_SHAPE, "layer %s: Gemm: blob %s (rank %d, %d x %d) broadcasts to no %d x %d product", ln, c->name.c_str(), c->dims, c->h, c->w, M, N);
        }
        if ((size_t)n * M * N >= ((size_t)1 << 31)) return failf(NET_E_SHAPE, "layer %s: Gemm: tensors of 2^31 elements or more are not supported", ln);
        memset(&desc, 0, sizeof(desc));
        desc.m = M, desc.n = N, desc.k = Ka, desc.batch = n, desc.trans_a = transA, desc.trans_b = transB, desc.out_transpose = out_t, desc.c_broadcast = type;
        desc.lda = transA ? M : Ka, desc.ldb = transB ? Ka : N, desc.ldc = N, desc.ldd = out_t ? M : N;
        desc.a_batch_stride = a ? M * Ka : 0, desc.b_batch_stride = b ? Ka * N : 0, desc.c_batch_stride = c ? c->h * c->w : 0, desc.d_batch_stride = M * N;
        desc.alpha = alpha, desc.beta = beta;
        if (const int rc = gemm_accepts(this, api, desc)) return rc;
        const int rc = out_t ? tops[0]->reshape(n, 1, N, M) : tops[0]->reshape(n, 1, M, N);
        tops[0]->dims = 2;
        return rc;
    }
    int Init(hipStream_t s) override
    {
        if (inited) return 0;
        for (int i = 0; i < 3; ++i)
            if (!host[i].empty())
                if (const int rc = dev[i].upload(host[i].data(), host[i].size(), s)) return rc;
        FHIP_CHECK_HIP(hipStreamSynchronize(s));
        inited = true;
        return 0;
    }
    int Forward(hipStream_t s) override
    {
        size_t next = 0;
        const float* a = constA ? dev[0].d : bottoms[next++]->data;
        const float* b = constB ? dev[1].d : bottoms[next++]->data;
        const float* c = c_bottom ? bottoms[next++]->data : dev[2].d;
        return side(gemm_api(), [&](const GemmApi* api) { return api->forward(&desc, a, b, desc.c_broadcast >= 0 ? c : nullptr, tops[0]->data, s); });
    }
    size_t weight_bytes() const override { return dev[0].bytes + dev[1].bytes + dev[2].bytes; }
};

// The layer types of a net with fhip_net_set_gemm (Net::gemm).  load_param_text asks here after create_layer: no default net knows them.
static Layer* create_gemm_layer(const std::string& type)
{
    if (type == "Gemm") return new GemmLayer;
    if (type == "MatMul") return new MatMulLayer;
    return nullptr;
}

} // namespace fhip::net
