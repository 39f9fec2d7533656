// net_rnn.h -- the layers of a net with fhip_net_set_recurrent (Net::recurrent): ncnn's LSTM, GRU and RNN.  include/feather_hip/feather_rnn.h
// defines the recurrence, libfeather_rnn.so holds it (rnn_api); the input projections of all steps and both directions are ONE GEMM of the
// main library (fhip_conv_forward, IM2COL: a 1x1 convolution over a 1x1 image whose batch is n * T) onto nd * G * H outputs with the bias,
// written into the net's arena, where the recurrence reads them and keeps its cell scratch.  The layers report the route FHIP_RNN_NET_ROUTE.
// A sequence is a blob of rank 2, [n][1][T][F] (Blob::dims, which fhip_net_set_detection maintains: the switch needs it).  Nothing fuses
// into these layers.  A default net never creates one of these classes.
#pragma once
#include "feather_hip/feather_rnn.h" // declarations only: the library is opened at run time (rnn_api)
#include "net_attn.h"

namespace fhip::net
{

// libfeather_rnn.so, the layers of a net with fhip_net_set_recurrent
struct RnnApi
{
    decltype(&fhip_rnn_forward) forward = nullptr;
    decltype(&fhip_rnn_last_error) last_error = nullptr;
    SideLibrary library()
    {
        return {"libfeather_rnn.so", "a recurrent layer (LSTM, GRU, RNN)", "feather_rnn.h", {{&forward, "fhip_rnn_forward"}, {&last_error, "fhip_rnn_last_error"}}};
    }
};
static const RnnApi* rnn_api() { return side_api<RnnApi>(); }

// ncnn's LSTM (0=num_output 1=weight_data_size 2=direction 3=hidden_size), GRU and RNN (0=num_output 1=weight_data_size 2=direction); weights
// weight_xc [nd][G * H][size], bias_c ([nd][4][H] for LSTM and GRU -- the GRU's rows are R, U, WN, BN -- and [nd][H] for RNN) and weight_hc
// [nd][G * H][H], each tagged.  Bottoms: the sequence [T][size] of rank 2 and, optionally, the initial hidden state [nd][H] (then the cell
// state, LSTM); tops: [T][nd * H] and, optionally, the final states.  A state bottom may also be the rank-3 blob [1][nd][H] an Input yields,
// which has no rank of its own.
struct RecurrentLayer : Layer
{
    int cell = FHIP_RNN_RNN, G = 1, H = 0, direction = 0, nd = 1, size = 0;
    long long wsize = 0;
    std::vector<float> wx, bias, wh, bn; // the GEMM's weights and bias [nd * G * H]; Wh; the GRU's BN rows [nd][H]
    fhip_conv_param p;
    DeviceVec packed, d_bias, d_wh, d_bn;
    size_t buffer_bytes = 0, packed_bytes = 0, scratch = 0, xp_floats = 0, total = 0; // the arena: GEMM scratch (bytes) | xp | the cell scratch
    bool built = false;
    explicit RecurrentLayer(int cell_) : cell(cell_), G(cell_ == FHIP_RNN_LSTM ? 4 : (cell_ == FHIP_RNN_GRU ? 3 : 1)) {}
    int algo() const override { return FHIP_RNN_NET_ROUTE; }
    bool needs_weights() const override { return true; }
    size_t states() const { return cell == FHIP_RNN_LSTM ? 2 : 1; }
    int LoadParam(const ParamDict& pd) override
    {
        const size_t full = 1 + states();
        if ((bottoms.size() != 1 && bottoms.size() != full) || (tops.size() != 1 && tops.size() != full))
            return failf(NET_E_SHAPE, "layer %s: %s needs 1 or %zu bottoms and 1 or %zu tops (the sequence, then the state%s), got %zu and %zu", name.c_str(), type.c_str(), full, full,
                         full == 3 ? "s: hidden, cell" : "", bottoms.size(), tops.size());
        H = pd.get(0, 0), wsize = pd.get(1, 0), direction = pd.get(2, 0);
        if (H < 1) return failf(NET_E_SHAPE, "layer %s: %s num_output (0=%d) must be positive", name.c_str(), type.c_str(), H);
        if (direction < 0 || direction > 2) return failf(NET_E_SHAPE, "layer %s: %s direction (2=%d) must be 0 (forward), 1 (reverse) or 2 (bidirectional)", name.c_str(), type.c_str(), direction);
        nd = direction == 2 ? 2 : 1;
        if (cell == FHIP_RNN_LSTM && pd.get(3, H) != H)
            return failf(NET_E_SHAPE, "layer %s: LSTM with a projection (hidden_size 3=%d other than num_output %d) is not supported", name.c_str(), pd.get(3, H), H);
        if (pd.get(8, 0) != 0) return failf(NET_E_SHAPE, "layer %s: %s with int8 weights (8=%d) is not supported", name.c_str(), type.c_str(), pd.get(8, 0));
        const long long rows = (long long)nd * G * H;
        if (rows > ((1ll << 31) - 1) / H) /* rows * H >= 2^31, without forming the product */ return failf(NET_E_SHAPE, "layer %s: %s num_output (0=%d): tensors of 2^31 elements or more are not supported", name.c_str(), type.c_str(), H);
        if (wsize < 1 || wsize % rows)
            return failf(NET_E_SHAPE, "layer %s: %s weight_data_size (1=%lld) must be a positive multiple of directions * gates * num_output (%lld)", name.c_str(), type.c_str(), wsize, rows);
        size = (int)(wsize / rows);
        memset(&p, 0, sizeof(p));
        p.input_channels = size, p.output_channels = (int)rows, p.bias_term = 1;
        p.input_h = p.input_w = p.kernel_h = p.kernel_w = p.stride_h = p.stride_w = p.group = 1;
        p.output_h = p.output_w = 1; // (not fhip_conv_assign_output_dim: it takes size == 1 == group for a depthwise layer with one output)
        return 0;
    }
    int LoadWeights(ModelBin& mb) override
    {
        built = false;
        std::vector<float> b;
        int rc = mb.load((size_t)wsize, 0, wx);
        if (!rc) rc = mb.load((size_t)nd * (cell == FHIP_RNN_RNN ? 1 : 4) * H, 0, b);
        if (!rc) rc = mb.load((size_t)nd * G * H * H, 0, wh);
        if (rc) return rc;
        if (cell != FHIP_RNN_GRU)
        {
            bias.swap(b); // [nd][G][H] as stored
            return 0;
        }
        bias.assign((size_t)nd * 3 * H, 0.f), bn.assign((size_t)nd * H, 0.f);
        for (int d = 0; d < nd; ++d)
        {
            std::copy(b.begin() + (size_t)d * 4 * H, b.begin() + (size_t)d * 4 * H + 3 * (size_t)H, bias.begin() + (size_t)d * 3 * H); // R, U, WN: into the GEMM
            std::copy(b.begin() + (size_t)d * 4 * H + 3 * (size_t)H, b.begin() + (size_t)(d + 1) * 4 * H, bn.begin() + (size_t)d * H);  // BN: inside the reset gate's product
        }
        return 0;
    }
    int Reshape() override
    {
        if (!rnn_api()) return FHIP_E_UNSUPPORTED; // message set by rnn_api
        const Blob* b = bottoms[0];
        if (b->dims != 2 || b->w != size)
            return failf(NET_E_SHAPE, "layer %s: %s needs a blob of rank 2 [T][%d], blob %s has rank %d and (%d, %d, %d)", name.c_str(), type.c_str(), size, b->name.c_str(), b->dims,
                         b->c, b->h, b->w);
        for (size_t i = 1; i < bottoms.size(); ++i)
        {
            const Blob* s = bottoms[i];
            if (s->n != b->n || s->c != 1 || s->h != nd || s->w != H)
                return failf(NET_E_SHAPE, "layer %s: %s needs a state blob [%d][%d] for each of the %d sequences, blob %s holds (%d, %d, %d) for %d", name.c_str(), type.c_str(), nd, H,
                             b->n, s->name.c_str(), s->c, s->h, s->w, s->n);
        }
        const long long columns = (long long)b->n * b->h;
        if (b->count() >= ((size_t)1 << 31) || columns * p.output_channels >= (1ll << 31))
            return failf(NET_E_SHAPE, "layer %s: %s: tensors of 2^31 elements or more are not supported", name.c_str(), type.c_str());
        int rc = tops[0]->reshape(b->n, 1, b->h, nd * H);
        tops[0]->dims = 2;
        for (size_t i = 1; i < tops.size() && !rc; ++i)
        {
            rc = tops[i]->reshape(b->n, 1, nd, H);
            tops[i]->dims = 2;
        }
        if (rc) return rc;
        if ((rc = fhip_conv_get_buffer_size(&p, FHIP_IM2COL, (int)columns, &buffer_bytes, &packed_bytes))) return rc;
        scratch = round_up_sz(buffer_bytes, 256);
        xp_floats = round_up_sz((size_t)columns * p.output_channels, 64);
        total = scratch + (xp_floats + (cell == FHIP_RNN_LSTM ? (size_t)nd * b->n * H : 0)) * sizeof(float);
        return 0;
    }
    int Init(hipStream_t s) override
    {
        if (built) return 0;
        if (const int rc = init_main(p, FHIP_IM2COL, wx, bias, packed, packed_bytes, d_bias, s)) return rc;
        int rc = d_wh.upload(wh.data(), wh.size(), s);
        if (!rc && cell == FHIP_RNN_GRU) rc = d_bn.upload(bn.data(), bn.size(), s);
        if (rc) return rc;
        FHIP_CHECK_HIP(hipStreamSynchronize(s));
        built = true;
        return 0;
    }
    int Forward(hipStream_t s) override
    {
        const Blob* b = bottoms[0];
        float* xp = (float*)((char*)net->arena.d + scratch);
        if (const int rc = fhip_conv_forward(&p, FHIP_IM2COL, b->n * b->h, xp, b->data, packed.d, (float*)net->arena.d, d_bias.d, s)) return rc;
        const float *h0 = bottoms.size() > 1 ? bottoms[1]->data : nullptr, *c0 = bottoms.size() > 2 ? bottoms[2]->data : nullptr;
        float *hn = tops.size() > 1 ? tops[1]->data : nullptr, *cn = tops.size() > 2 ? tops[2]->data : nullptr;
        return side(rnn_api(), [&](const RnnApi* api) {
            return api->forward(cell, direction, b->n, b->h, H, xp, p.output_channels, d_wh.d, d_bn.d, h0, c0, tops[0]->data, nd * H, hn, cn,
                                cell == FHIP_RNN_LSTM ? xp + xp_floats : nullptr, s);
        });
    }
    size_t weight_bytes() const override { return packed.bytes + d_bias.bytes + d_wh.bytes + d_bn.bytes; }
    size_t arena_bytes() const override { return total; }
};

// The layer types of a net with fhip_net_set_recurrent (Net::recurrent).
static Layer* create_recurrent_layer(const std::string& type)
{
    if (type == "LSTM") return new RecurrentLayer(FHIP_RNN_LSTM);
    if (type == "GRU") return new RecurrentLayer(FHIP_RNN_GRU);
    if (type == "RNN") return new RecurrentLayer(FHIP_RNN_RNN);
    return nullptr;
}

} // namespace fhip::net
