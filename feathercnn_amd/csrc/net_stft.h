// net_stft.h -- the layers of a net with fhip_net_set_audio (Net::audio): ncnn's Spectrogram and UnaryOp, the front of a speech model that
// takes a waveform.  include/feather_hip/feather_stft.h defines them, libfeather_stft.so holds them (stft_api); the layers report the route
// FHIP_STFT_NET_ROUTE.  A waveform is a blob of rank 1, [n][1][1][L] (what an Input `0=L` yields); the spectrogram is a 1-D blob of rank 2,
// [n][1][freqs][frames], Convolution1D's [C][L], or with power 0 a blob of rank 3, [n][freqs][frames][2].  Blob::dims is what
// fhip_net_set_detection maintains: the switch needs it.  Nothing fuses into these layers.  A default net never creates one of these classes.
#pragma once
#include "feather_hip/feather_stft.h" // declarations only: the library is opened at run time (stft_api)
#include "net_istft.h" // InverseSpectrogramLayer, which create_audio_layer creates

namespace fhip::net
{

// libfeather_stft.so, the layers of a net with fhip_net_set_audio
struct StftApi
{
    decltype(&fhip_stft_output_dim) output_dim = nullptr;
    decltype(&fhip_stft_basis) basis = nullptr;
    decltype(&fhip_stft_forward) forward = nullptr;
    decltype(&fhip_unary_forward) unary = nullptr;
    decltype(&fhip_stft_last_error) last_error = nullptr;
    SideLibrary library()
    {
        return {"libfeather_stft.so", "an audio layer (Spectrogram, UnaryOp)", "feather_stft.h",
                {{&output_dim, "fhip_stft_output_dim"}, {&basis, "fhip_stft_basis"}, {&forward, "fhip_stft_forward"}, {&unary, "fhip_unary_forward"},
                 {&last_error, "fhip_stft_last_error"}}};
    }
};
static const StftApi* stft_api() { return side_api<StftApi>(); }

// ncnn's Spectrogram: 0=n_fft 1=power 2=hoplen 3=winlen 4=window_type 5=center 6=pad_type 7=normalized 8=onesided (feather_stft.h has the
// table).  The basis -- window and normalisation folded in -- is made on the host and uploaded at Init, outside a captured graph.
struct SpectrogramLayer : Layer
{
    int n_fft = 0, power = 0, hop = 0, winlen = 0, window_type = 0, center = 1, pad_type = 2, normalized = 0, onesided = 1;
    int freqs = 0, frames = 0;
    DeviceVec d_basis;
    bool built = false;
    int algo() const override { return FHIP_STFT_NET_ROUTE; }
    int LoadParam(const ParamDict& pd) override
    {
        const char* ln = name.c_str();
        if (bottoms.size() != 1 || tops.size() != 1)
            return failf(NET_E_SHAPE, "layer %s: Spectrogram needs one bottom (a second bottom is not supported) and one top, got %zu and %zu", ln, bottoms.size(), tops.size());
        n_fft = pd.get(0, 0), power = pd.get(1, 0), hop = pd.get(2, n_fft / 4), winlen = pd.get(3, n_fft), window_type = pd.get(4, 0), center = pd.get(5, 1);
        pad_type = pd.get(6, 2), normalized = pd.get(7, 0), onesided = pd.get(8, 1);
        if (n_fft < 2 || n_fft > FHIP_STFT_MAX_NFFT) return failf(NET_E_SHAPE, "layer %s: Spectrogram n_fft (0=%d) must be 2 .. %d", ln, n_fft, FHIP_STFT_MAX_NFFT);
        if (power < 0 || power > 2) return failf(NET_E_SHAPE, "layer %s: Spectrogram power (1=%d) must be 0 (complex), 1 (magnitude) or 2 (squared magnitude)", ln, power);
        if (hop < 1) return failf(NET_E_SHAPE, "layer %s: Spectrogram hoplen (2=%d) must be positive", ln, hop);
        if (winlen < 1 || winlen > n_fft) return failf(NET_E_SHAPE, "layer %s: Spectrogram winlen (3=%d) must be 1 .. n_fft", ln, winlen);
        if (window_type < 0 || window_type > 2) return failf(NET_E_SHAPE, "layer %s: Spectrogram window_type (4=%d) must be 0 (ones), 1 (Hann) or 2 (Hamming)", ln, window_type);
        if (center != 0 && center != 1) return failf(NET_E_SHAPE, "layer %s: Spectrogram center (5=%d) must be 0 or 1", ln, center);
        if (pad_type < 0 || pad_type > 2) return failf(NET_E_SHAPE, "layer %s: Spectrogram pad_type (6=%d) must be 0 (zeros), 1 (replicate) or 2 (reflect)", ln, pad_type);
        if (normalized < 0 || normalized > 2) return failf(NET_E_SHAPE, "layer %s: Spectrogram normalized (7=%d) must be 0, 1 or 2", ln, normalized);
        if (onesided != 0 && onesided != 1) return failf(NET_E_SHAPE, "layer %s: Spectrogram onesided (8=%d) must be 0 or 1", ln, onesided);
        return 0;
    }
    int Reshape() override
    {
        const StftApi* api = stft_api();
        if (!api) return FHIP_E_UNSUPPORTED; // message set by stft_api
        const Blob* b = bottoms[0];
        if (b->c != 1 || b->h != 1)
            return failf(NET_E_SHAPE, "layer %s: Spectrogram needs a blob of rank 1 [L], blob %s has rank %d and (%d, %d, %d)", name.c_str(), b->name.c_str(), b->dims, b->c, b->h, b->w);
        if (api->output_dim(b->w, n_fft, hop, center, pad_type, onesided, &freqs, &frames))
            return failf(NET_E_SHAPE, "layer %s: Spectrogram of blob %s, a row of %d: %s", name.c_str(), b->name.c_str(), b->w, api->last_error());
        if (b->count() >= ((size_t)1 << 31) || (long long)b->n * freqs * frames * (power == 0 ? 2 : 1) >= (1ll << 31))
            return failf(NET_E_SHAPE, "layer %s: Spectrogram: tensors of 2^31 elements or more are not supported", name.c_str());
        const int rc = power == 0 ? tops[0]->reshape(b->n, freqs, frames, 2) : tops[0]->reshape(b->n, 1, freqs, frames);
        tops[0]->dims = power == 0 ? 3 : 2;
        return rc;
    }
    int Init(hipStream_t st) override
    {
        if (built) return 0;
        const StftApi* api = stft_api();
        if (!api) return FHIP_E_UNSUPPORTED;
        std::vector<float> basis((size_t)2 * (onesided ? n_fft / 2 + 1 : n_fft) * n_fft);
        if (api->basis(n_fft, winlen, window_type, normalized, onesided, basis.data(), (long long)basis.size()))
            return failf(NET_E_SHAPE, "layer %s: Spectrogram: %s", name.c_str(), api->last_error());
        if (const int rc = d_basis.upload(basis.data(), basis.size(), st)) return rc;
        FHIP_CHECK_HIP(hipStreamSynchronize(st)); // `basis` goes with this call
        built = true;
        return 0;
    }
    int Forward(hipStream_t st) override
    {
        const Blob* b = bottoms[0];
        return side(stft_api(), [&](const StftApi* api) {
            return api->forward(b->n, b->w, n_fft, power, hop, center, pad_type, onesided, b->data, d_basis.d, tops[0]->data, frames, st);
        });
    }
    size_t weight_bytes() const override { return d_basis.bytes; }
};

// ncnn's UnaryOp: 0=op_type, the ids feather_stft.h lists.  Any rank; the top takes the bottom's shape.
struct UnaryOpLayer : Layer
{
    int op = 0;
    int algo() const override { return FHIP_STFT_NET_ROUTE; }
    int LoadParam(const ParamDict& pd) override
    {
        if (const int rc = one_to_one_counts(this)) return rc;
        op = pd.get(0, 0);
        switch (op)
        {
        case FHIP_UNARY_ABS: case FHIP_UNARY_NEG: case FHIP_UNARY_SQUARE: case FHIP_UNARY_SQRT: case FHIP_UNARY_RSQRT: case FHIP_UNARY_EXP: case FHIP_UNARY_LOG:
        case FHIP_UNARY_RECIPROCAL: case FHIP_UNARY_LOG10: return 0;
        default:
            return failf(NET_E_SHAPE, "layer %s: UnaryOp op_type (0=%d) must be 0 (abs), 1 (neg), 4 (square), 5 (sqrt), 6 (rsqrt), 7 (exp), 8 (log), 15 (reciprocal) or 17 (log10)",
                         name.c_str(), op);
        }
    }
    int Reshape() override
    {
        if (!stft_api()) return FHIP_E_UNSUPPORTED; // message set by stft_api
        if (const int rc = attn_too_large(this, bottoms[0])) return rc;
        return reshape_like(tops[0], bottoms[0]);
    }
    int Forward(hipStream_t st) override
    {
        return side(stft_api(), [&](const StftApi* api) { return api->unary(op, tops[0]->data, bottoms[0]->data, (long long)bottoms[0]->count(), st); });
    }
};

// The layer types of a net with fhip_net_set_audio (Net::audio).
static Layer* create_audio_layer(const std::string& type)
{
    if (type == "Spectrogram") return new SpectrogramLayer;
    if (type == "UnaryOp") return new UnaryOpLayer;
    if (type == "InverseSpectrogram") return new InverseSpectrogramLayer; // net_istft.h, libfeather_istft.so
    return nullptr;
}

} // namespace fhip::net
