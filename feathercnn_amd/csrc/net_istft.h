// net_istft.h -- ncnn's InverseSpectrogram in a net with fhip_net_set_audio (Net::audio): the layer that gives a waveform back, the twin
// of net_stft.h's Spectrogram (whose factory, create_audio_layer, creates it).  include/feather_hip/feather_istft.h defines it,
// libfeather_istft.so holds it (istft_api); the layer reports the route FHIP_ISTFT_NET_ROUTE.  The bottom is a blob of rank 3,
// [n][freqs][frames][2] -- Spectrogram's power-0 top -- and the top a waveform, a blob of rank 1, [n][1][1][out_len].  Nothing fuses into
// the layer.  A default net never creates this class.
#pragma once
#include "feather_hip/feather_istft.h" // declarations only: the library is opened at run time (istft_api)
#include "net_conv3d.h"

namespace fhip::net
{

// libfeather_istft.so, the InverseSpectrogram of a net with fhip_net_set_audio
struct IstftApi
{
    decltype(&fhip_istft_output_dim) output_dim = nullptr;
    decltype(&fhip_istft_basis) basis = nullptr;
    decltype(&fhip_istft_envelope) envelope = nullptr;
    decltype(&fhip_istft_forward) forward = nullptr;
    decltype(&fhip_istft_last_error) last_error = nullptr;
    SideLibrary library()
    {
        return {"libfeather_istft.so", "an audio layer (InverseSpectrogram)", "feather_istft.h",
                {{&output_dim, "fhip_istft_output_dim"}, {&basis, "fhip_istft_basis"}, {&envelope, "fhip_istft_envelope"}, {&forward, "fhip_istft_forward"},
                 {&last_error, "fhip_istft_last_error"}}};
    }
};
static const IstftApi* istft_api() { return side_api<IstftApi>(); }

// ncnn's InverseSpectrogram: 0=n_fft 1=returns 2=hoplen 3=winlen 4=window_type 5=center 7=normalized (feather_istft.h has the table).
// One-sided or two-sided is read off the bottom: freqs == n_fft / 2 + 1 or n_fft.  The basis -- window, 1 / n_fft and normalisation folded
// in -- and the inverse window envelope are made on the host and uploaded at Init, outside a captured graph: the basis once (again if the
// bottom changes sides), the envelope whenever the number of frames has changed since the last upload.
struct InverseSpectrogramLayer : Layer
{
    int n_fft = 0, returns = 1, hop = 0, winlen = 0, window_type = 0, center = 1, normalized = 0;
    int onesided = 1, frames = 0, out_len = 0;
    int basis_sides = -1, envelope_frames = 0; // what the device copies were made for
    DeviceVec d_basis, d_inv_env;
    int algo() const override { return FHIP_ISTFT_NET_ROUTE; }
    int LoadParam(const ParamDict& pd) override
    {
        const char* ln = name.c_str();
        if (bottoms.size() != 1 || tops.size() != 1)
            return failf(NET_E_SHAPE, "layer %s: InverseSpectrogram needs one bottom (a second bottom is not supported) and one top, got %zu and %zu", ln, bottoms.size(), tops.size());
        n_fft = pd.get(0, 0), returns = pd.get(1, 1), hop = pd.get(2, n_fft / 4), winlen = pd.get(3, n_fft), window_type = pd.get(4, 0), center = pd.get(5, 1);
        normalized = pd.get(7, 0);
        if (n_fft < 2 || n_fft > FHIP_ISTFT_MAX_NFFT) return failf(NET_E_SHAPE, "layer %s: InverseSpectrogram n_fft (0=%d) must be 2 .. %d", ln, n_fft, FHIP_ISTFT_MAX_NFFT);
        if (returns != 1) return failf(NET_E_SHAPE, "layer %s: InverseSpectrogram returns (1=%d) must be 1 (real): 0 (complex) and 2 (imaginary) are not supported", ln, returns);
        if (hop < 1) return failf(NET_E_SHAPE, "layer %s: InverseSpectrogram hoplen (2=%d) must be positive", ln, hop);
        if (winlen < 1 || winlen > n_fft) return failf(NET_E_SHAPE, "layer %s: InverseSpectrogram winlen (3=%d) must be 1 .. n_fft", ln, winlen);
        if (window_type < 0 || window_type > 2) return failf(NET_E_SHAPE, "layer %s: InverseSpectrogram window_type (4=%d) must be 0 (ones), 1 (Hann) or 2 (Hamming)", ln, window_type);
        if (center != 0 && center != 1) return failf(NET_E_SHAPE, "layer %s: InverseSpectrogram center (5=%d) must be 0 or 1", ln, center);
        if (normalized < 0 || normalized > 2) return failf(NET_E_SHAPE, "layer %s: InverseSpectrogram normalized (7=%d) must be 0, 1 or 2", ln, normalized);
        return 0;
    }
    int Reshape() override
    {
        const IstftApi* api = istft_api();
        if (!api) return FHIP_E_UNSUPPORTED; // message set by istft_api
        const Blob* b = bottoms[0];
        if (b->dims != 3 || b->w != 2)
            return failf(NET_E_SHAPE, "layer %s: InverseSpectrogram needs a blob of rank 3 [freqs][frames][2], blob %s has rank %d and (%d, %d, %d)", name.c_str(), b->name.c_str(),
                         b->dims, b->c, b->h, b->w);
        if (b->c != n_fft / 2 + 1 && b->c != n_fft)
            return failf(NET_E_SHAPE, "layer %s: InverseSpectrogram of n_fft %d needs %d (one-sided) or %d (two-sided) frequencies, blob %s has %d", name.c_str(), n_fft, n_fft / 2 + 1,
                         n_fft, b->name.c_str(), b->c);
        onesided = b->c == n_fft / 2 + 1 ? 1 : 0;
        frames = b->h;
        if (api->output_dim(frames, n_fft, hop, center, &out_len))
            return failf(NET_E_SHAPE, "layer %s: InverseSpectrogram of blob %s, %d frames: %s", name.c_str(), b->name.c_str(), frames, api->last_error());
        if (b->count() >= ((size_t)1 << 31) || (long long)b->n * out_len >= (1ll << 31))
            return failf(NET_E_SHAPE, "layer %s: InverseSpectrogram: tensors of 2^31 elements or more are not supported", name.c_str());
        const int rc = tops[0]->reshape(b->n, 1, 1, out_len);
        tops[0]->dims = 1;
        return rc;
    }
    int Init(hipStream_t st) override
    {
        const IstftApi* api = istft_api();
        if (!api) return FHIP_E_UNSUPPORTED;
        if (basis_sides == onesided && envelope_frames == frames) return 0;
        std::vector<float> basis, inv_env;
        if (basis_sides != onesided)
        {
            basis.resize((size_t)2 * (onesided ? n_fft / 2 + 1 : n_fft) * n_fft);
            if (api->basis(n_fft, winlen, window_type, normalized, onesided, basis.data(), (long long)basis.size()))
                return failf(NET_E_SHAPE, "layer %s: InverseSpectrogram: %s", name.c_str(), api->last_error());
            if (const int rc = d_basis.upload(basis.data(), basis.size(), st)) return rc;
        }
        if (envelope_frames != frames)
        {
            inv_env.resize((size_t)out_len);
            if (api->envelope(frames, n_fft, hop, winlen, window_type, center, inv_env.data(), (long long)inv_env.size()))
                return failf(NET_E_SHAPE, "layer %s: InverseSpectrogram of %d frames: %s", name.c_str(), frames, api->last_error());
            if (const int rc = d_inv_env.upload(inv_env.data(), inv_env.size(), st)) return rc;
        }
        FHIP_CHECK_HIP(hipStreamSynchronize(st)); // the host arrays go with this call
        basis_sides = onesided, envelope_frames = frames;
        return 0;
    }
    int Forward(hipStream_t st) override
    {
        const Blob* b = bottoms[0];
        return side(istft_api(), [&](const IstftApi* api) {
            return api->forward(b->n, frames, n_fft, hop, center, onesided, b->data, d_basis.d, d_inv_env.d, tops[0]->data, out_len, st);
        });
    }
    size_t weight_bytes() const override { return d_basis.bytes + d_inv_env.bytes; }
};

} // namespace fhip::net
