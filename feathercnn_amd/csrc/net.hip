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
#include <ctype.h>
#include <dlfcn.h>
#include <errno.h>
#include <float.h>
#include <limits.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "common.h"
#include "feather_hip/feather_canvas.h" // declarations only: the library is opened at run time (canvas_api)
#include "feather_hip/feather_atrous.h" // declarations only: the library is opened at run time (atrous_api)
#include "feather_hip/feather_deconv.h" // declarations only: the library is opened at run time (deconv_api)
#include "feather_hip/feather_gate.h" // declarations only: the library is opened at run time (gate_api)
#include "feather_hip/feather_gconv.h" // declarations only: the library is opened at run time (gconv_api)
#include "feather_hip/feather_inorm.h" // declarations only: the library is opened at run time (inorm_api)
#include "feather_hip/feather_lrn.h" // declarations only: the library is opened at run time (lrn_api)
#include "feather_hip/feather_net.h"
#include "feather_hip/feather_resample.h" // declarations only: the library is opened at run time (resample_api)
#include "feather_hip/feather_shuffle.h" // declarations only: the library is opened at run time (shuffle_api)

namespace fhip
{
namespace net
{

static int failf(int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    return fail(code, buf);
}

// Error codes of the Net level follow the reference where it has one (net.cpp:111,134,276; layers return -100).
enum
{
    NET_E_IO = -1,
    NET_E_SHAPE = -100,
    NET_E_UNKNOWN_LAYER = -200,
    NET_E_TOPOLOGY = -300,
    NET_E_BASE_RESHAPE = -400
};

// ---- the side libraries: libfeather_<x>.so next to libfeather_hip.so, one per layer family added after the first release ----------------
// Each is opened lazily from the directory this library was loaded from (then by its bare name, the loader's search path), so that
// libfeather_hip.so keeps linking and loading without it; a net that needs one and cannot find it fails at Reshape (canvas: at
// plan_chains).  A typed struct per library holds its entry points and describes itself once (library()); side_api<X>() opens and
// caches it.
struct SideSymbol
{
    void* slot; // the function pointer of the Api struct that receives the address
    const char* name;
};

struct SideLibrary
{
    const char *file, *needs, *header; // libfeather_<x>.so, what needs it (for the message), feather_<x>.h
    std::vector<SideSymbol> symbols;
};

// Opens the library and fills every slot; false, with the message set and nothing left open, if the file or one entry point is missing.
static bool open_side_library(const SideLibrary& lib)
{
    std::string tried;
    Dl_info self;
    if (dladdr((void*)&open_side_library, &self) && self.dli_fname)
    {
        tried = self.dli_fname;
        const size_t slash = tried.rfind('/');
        tried = (slash == std::string::npos ? std::string() : tried.substr(0, slash + 1)) + lib.file;
    }
    void* h = nullptr;
    for (const char* path : {tried.c_str(), lib.file})
        if (*path && (h = dlopen(path, RTLD_NOW | RTLD_LOCAL))) break;
    if (!h)
    {
        failf(FHIP_E_UNSUPPORTED, "%s needs %s next to libfeather_hip.so (%s): %s", lib.needs, lib.file, tried.c_str(), dlerror());
        return false;
    }
    bool all = true;
    for (const SideSymbol& s : lib.symbols)
    {
        void* f = dlsym(h, s.name);
        memcpy(s.slot, &f, sizeof(f));
        all = all && f;
    }
    if (!all)
    {
        failf(FHIP_E_UNSUPPORTED, "%s (%s) does not export the entry points of %s", lib.file, tried.c_str(), lib.header);
        dlclose(h);
    }
    return all;
}

// One table, mutex and `loaded` flag per library; a failed open leaves them untouched and is tried again at the next call.
template <class Api>
static const Api* side_api()
{
    static std::mutex mu;
    static Api api;
    static bool loaded = false;
    std::lock_guard<std::mutex> lk(mu);
    if (loaded) return &api;
    Api a;
    if (!open_side_library(a.library())) return nullptr;
    api = a;
    loaded = true;
    return &api;
}

// libfeather_gconv.so, the route of a Convolution layer with 1 < group < C
struct GconvApi
{
    decltype(&fhip_gconv_supported) supported = nullptr;
    decltype(&fhip_gconv_get_buffer_size) get_buffer_size = nullptr;
    decltype(&fhip_gconv_init) init = nullptr;
    decltype(&fhip_gconv_forward) forward = nullptr;
    decltype(&fhip_gconv_last_error) last_error = nullptr;
    SideLibrary library()
    {
        return {"libfeather_gconv.so", "a convolution with 1 < group < input_channels", "feather_gconv.h",
                {{&supported, "fhip_gconv_supported"}, {&get_buffer_size, "fhip_gconv_get_buffer_size"}, {&init, "fhip_gconv_init"},
                 {&forward, "fhip_gconv_forward"}, {&last_error, "fhip_gconv_last_error"}}};
    }
};
static const GconvApi* gconv_api() { return side_api<GconvApi>(); }

// libfeather_atrous.so, the route of a Convolution layer with dilation > 1 (fhip_net_set_dilated)
struct AtrousApi
{
    decltype(&fhip_atrous_assign_output_dim) assign_output_dim = nullptr;
    decltype(&fhip_atrous_supported) supported = nullptr;
    decltype(&fhip_atrous_get_buffer_size) get_buffer_size = nullptr;
    decltype(&fhip_atrous_init) init = nullptr;
    decltype(&fhip_atrous_forward) forward = nullptr;
    decltype(&fhip_atrous_last_error) last_error = nullptr;
    SideLibrary library()
    {
        return {"libfeather_atrous.so", "a dilated convolution", "feather_atrous.h",
                {{&assign_output_dim, "fhip_atrous_assign_output_dim"}, {&supported, "fhip_atrous_supported"},
                 {&get_buffer_size, "fhip_atrous_get_buffer_size"}, {&init, "fhip_atrous_init"}, {&forward, "fhip_atrous_forward"},
                 {&last_error, "fhip_atrous_last_error"}}};
    }
};
static const AtrousApi* atrous_api() { return side_api<AtrousApi>(); }

// libfeather_deconv.so, the route of Deconvolution / DeconvolutionDepthWise layers
struct DeconvApi
{
    decltype(&fhip_deconv_assign_output_dim) assign_output_dim = nullptr;
    decltype(&fhip_deconv_supported) supported = nullptr;
    decltype(&fhip_deconv_get_buffer_size) get_buffer_size = nullptr;
    decltype(&fhip_deconv_init) init = nullptr;
    decltype(&fhip_deconv_forward) forward = nullptr;
    decltype(&fhip_deconv_last_error) last_error = nullptr;
    SideLibrary library()
    {
        return {"libfeather_deconv.so", "a Deconvolution layer", "feather_deconv.h",
                {{&assign_output_dim, "fhip_deconv_assign_output_dim"}, {&supported, "fhip_deconv_supported"},
                 {&get_buffer_size, "fhip_deconv_get_buffer_size"}, {&init, "fhip_deconv_init"}, {&forward, "fhip_deconv_forward"},
                 {&last_error, "fhip_deconv_last_error"}}};
    }
};
static const DeconvApi* deconv_api() { return side_api<DeconvApi>(); }

// libfeather_inorm.so, the route of InstanceNorm, PReLU / Sigmoid / TanH / Clip layers and of a ReLU with a slope
struct InormApi
{
    decltype(&fhip_instance_norm_get_buffer_size) get_buffer_size = nullptr;
    decltype(&fhip_instance_norm_forward) forward = nullptr;
    decltype(&fhip_activation_forward) activation = nullptr;
    decltype(&fhip_inorm_last_error) last_error = nullptr;
    SideLibrary library()
    {
        return {"libfeather_inorm.so", "an InstanceNorm / activation layer", "feather_inorm.h",
                {{&get_buffer_size, "fhip_instance_norm_get_buffer_size"}, {&forward, "fhip_instance_norm_forward"},
                 {&activation, "fhip_activation_forward"}, {&last_error, "fhip_inorm_last_error"}}};
    }
};
static const InormApi* inorm_api() { return side_api<InormApi>(); }

// libfeather_shuffle.so, the route of ShuffleChannel and Slice layers and of the Concat / ShuffleChannel / Slice runs collapsed at
// fusion level 2
struct ShuffleApi
{
    decltype(&fhip_channel_slice_resolve) resolve = nullptr;
    decltype(&fhip_channel_map_create) create = nullptr;
    decltype(&fhip_channel_map_destroy) destroy = nullptr;
    decltype(&fhip_channel_map_forward) forward = nullptr;
    decltype(&fhip_shuffle_last_error) last_error = nullptr;
    SideLibrary library()
    {
        return {"libfeather_shuffle.so", "a ShuffleChannel / Slice layer", "feather_shuffle.h",
                {{&resolve, "fhip_channel_slice_resolve"}, {&create, "fhip_channel_map_create"}, {&destroy, "fhip_channel_map_destroy"},
                 {&forward, "fhip_channel_map_forward"}, {&last_error, "fhip_shuffle_last_error"}}};
    }
};
static const ShuffleApi* shuffle_api() { return side_api<ShuffleApi>(); }

// libfeather_gate.so, the route of the squeeze-and-excitation layers: a two-bottom BinaryOp (mul) or Scale, Swish, HardSigmoid, and the
// whole SE block collapsed at fusion level 2 (collapse_gate_blocks)
struct GateApi
{
    decltype(&fhip_channel_gate_forward) apply = nullptr;
    decltype(&fhip_squeeze_get_buffer_size) squeeze_buffer_size = nullptr;
    decltype(&fhip_squeeze_forward) squeeze = nullptr;
    decltype(&fhip_excite_forward) excite = nullptr;
    decltype(&fhip_gate_activation_forward) activation = nullptr;
    decltype(&fhip_gate_last_error) last_error = nullptr;
    SideLibrary library()
    {
        return {"libfeather_gate.so", "a channel-gate / Swish / HardSigmoid layer", "feather_gate.h",
                {{&apply, "fhip_channel_gate_forward"}, {&squeeze_buffer_size, "fhip_squeeze_get_buffer_size"}, {&squeeze, "fhip_squeeze_forward"},
                 {&excite, "fhip_excite_forward"}, {&activation, "fhip_gate_activation_forward"}, {&last_error, "fhip_gate_last_error"}}};
    }
};
static const GateApi* gate_api() { return side_api<GateApi>(); }

// libfeather_resample.so, the route of the Interp and HardSwish layers of a net with fhip_net_set_extended_layers, and of an Interp
// collapsed with the Eltwise SUM (and ReLU) behind it at fusion level 2 (collapse_upsample_adds)
struct ResampleApi
{
    decltype(&fhip_interp_output_dim) output_dim = nullptr;
    decltype(&fhip_interp_forward) interp = nullptr;
    decltype(&fhip_hardswish_forward) hardswish = nullptr;
    decltype(&fhip_resample_last_error) last_error = nullptr;
    SideLibrary library()
    {
        return {"libfeather_resample.so", "an Interp / HardSwish layer", "feather_resample.h",
                {{&output_dim, "fhip_interp_output_dim"}, {&interp, "fhip_interp_forward"}, {&hardswish, "fhip_hardswish_forward"},
                 {&last_error, "fhip_resample_last_error"}}};
    }
};
static const ResampleApi* resample_api() { return side_api<ResampleApi>(); }

// libfeather_lrn.so, the route of the LRN layers of a net with fhip_net_set_extended_layers, alone or with the Pooling layer behind them
// (LRNLayer::Fuse at fusion level 2)
struct LrnApi
{
    decltype(&fhip_lrn_forward) forward = nullptr;
    decltype(&fhip_lrn_pool_forward) pool_forward = nullptr;
    decltype(&fhip_lrn_last_error) last_error = nullptr;
    SideLibrary library()
    {
        return {"libfeather_lrn.so", "an LRN layer", "feather_lrn.h",
                {{&forward, "fhip_lrn_forward"}, {&pool_forward, "fhip_lrn_pool_forward"}, {&last_error, "fhip_lrn_last_error"}}};
    }
};
static const LrnApi* lrn_api() { return side_api<LrnApi>(); }

// libfeather_canvas.so, the chained Winograd transforms of layers that run on 2x2 image canvases (plan_chains).  The canvas form is a
// faster way to run the same run of layers, not a layer type: a net that qualifies and cannot find the library fails at plan_chains.
struct CanvasApi
{
    decltype(&fhip_canvas_output_to_next_input) chain = nullptr;
    decltype(&fhip_canvas_output_transform) output = nullptr;
    decltype(&fhip_canvas_last_error) last_error = nullptr;
    SideLibrary library()
    {
        return {"libfeather_canvas.so", "a chained Winograd run on 2x2 image canvases", "feather_canvas.h",
                {{&chain, "fhip_canvas_output_to_next_input"}, {&output, "fhip_canvas_output_transform"}, {&last_error, "fhip_canvas_last_error"}}};
    }
};
static const CanvasApi* canvas_api() { return side_api<CanvasApi>(); }

// ---- ncnn ParamDict (ncnn/paramdict.cpp:92-174): "id=value" pairs, value is float iff it contains '.' or 'e' -----
struct ParamDict
{
    static const int kMax = 32; // NCNN_MAX_PARAM_COUNT is 20
    struct Entry
    {
        bool loaded = false;
        uint32_t bits = 0; // union { int i; float f; } exactly like the reference
        std::vector<float> array;
    } e[kMax];

    void clear()
    {
        for (auto& x : e) x = Entry();
    }
    int get(int id, int def) const
    {
        if (id < 0 || id >= kMax || !e[id].loaded) return def;
        int v;
        memcpy(&v, &e[id].bits, 4);
        return v;
    }
    float get(int id, float def) const
    {
        if (id < 0 || id >= kMax || !e[id].loaded) return def;
        float v;
        memcpy(&v, &e[id].bits, 4);
        return v;
    }
    bool has_array(int id) const { return id >= 0 && id < kMax && e[id].loaded && !e[id].array.empty(); }

    static bool is_float(const std::string& s)
    {
        for (char ch : s)
            if (ch == '.' || ch == 'e' || ch == 'E') return true;
        return false;
    }
    // `tok` is one whitespace-delimited token "id=value" or "-233xx=len,v0,v1,..."; returns false if it is not a pair.
    static bool looks_like_pair(const std::string& tok)
    {
        size_t i = 0;
        if (i < tok.size() && tok[i] == '-') ++i;
        const size_t d0 = i;
        while (i < tok.size() && isdigit((unsigned char)tok[i])) ++i;
        return i > d0 && i < tok.size() && tok[i] == '=';
    }
    int parse(const std::string& tok)
    {
        const size_t eq = tok.find('=');
        // a file may hold any digits: the id is read wide, and its range is checked before any arithmetic on it
        errno = 0;
        const long long raw_id = strtoll(tok.substr(0, eq).c_str(), nullptr, 10);
        const std::string val = tok.substr(eq + 1);
        const bool is_array = raw_id <= -23300;
        if (errno == ERANGE || raw_id <= -23300 - kMax || raw_id >= kMax || (raw_id < 0 && !is_array))
            return failf(FHIP_E_BADARG, "param id %.24s out of range", tok.c_str());
        const long long wide_id = is_array ? -raw_id - 23300 : raw_id;
        const int id = (int)wide_id;
        if (is_array)
        {
            std::vector<std::string> parts;
            size_t a = 0;
            while (a <= val.size())
            {
                const size_t b = val.find(',', a);
                parts.push_back(val.substr(a, b == std::string::npos ? std::string::npos : b - a));
                if (b == std::string::npos) break;
                a = b + 1;
            }
            const int len = atoi(parts[0].c_str());
            if (len < 0 || parts.size() != (size_t)len + 1) return failf(NET_E_IO, "ParamDict read array element fail"); // paramdict.cpp:124-128
            e[id].array.resize(len);
            for (int j = 0; j < len; ++j) e[id].array[j] = (float)atof(parts[j + 1].c_str());
        }
        else
        {
            if (val.empty()) return failf(NET_E_IO, "ParamDict read value fail"); // paramdict.cpp:153-157
            if (is_float(val))
            {
                const float f = (float)atof(val.c_str());
                memcpy(&e[id].bits, &f, 4);
            }
            else
            {
                const int i = atoi(val.c_str());
                memcpy(&e[id].bits, &i, 4);
            }
        }
        e[id].loaded = true;
        return 0;
    }
};

// ---- ncnn ModelBin (ncnn/modelbin.cpp:47-197) over a memory image of the .bin ---------------------------------
struct ModelBin
{
    const unsigned char* p;
    const unsigned char* end;

    static float half_to_float(uint16_t h)
    {
        const uint32_t sign = (uint32_t)(h >> 15) << 31;
        int exp = (h >> 10) & 0x1f;
        uint32_t man = h & 0x3ff;
        uint32_t bits;
        if (exp == 0)
        {
            if (man == 0)
                bits = sign;
            else
            {
                exp = 1;
                while (!(man & 0x400))
                {
                    man <<= 1;
                    --exp;
                }
                man &= 0x3ff;
                bits = sign | ((uint32_t)(exp + 112) << 23) | (man << 13);
            }
        }
        else if (exp == 31)
            bits = sign | 0x7f800000u | (man << 13);
        else
            bits = sign | ((uint32_t)(exp + 112) << 23) | (man << 13);
        float f;
        memcpy(&f, &bits, 4);
        return f;
    }
    bool take(void* dst, size_t bytes)
    {
        if ((size_t)(end - p) < bytes) return false;
        if (dst) memcpy(dst, p, bytes);
        p += bytes;
        return true;
    }
    // type 0: 4-byte tag then payload (raw fp32 / fp16 / 256-entry table); type 1: raw fp32 (modelbin.cpp:52-189)
    int load(size_t w, int type, std::vector<float>& out)
    {
        // every payload form holds at least one byte per weight: a count the rest of the file cannot hold is refused before anything of
        // that size is allocated (counts are products of file values: negative ones arrive here as huge ones)
        if (w > (size_t)(end - p))
        {
            out.clear();
            return failf(NET_E_SHAPE, "ModelBin read weight_data failed (file too short for %zu weights)", w);
        }
        out.assign(w, 0.f);
        if (type == 1)
        {
            if (!take(out.data(), w * 4)) return failf(NET_E_SHAPE, "ModelBin read weight_data failed (file too short)");
            return 0;
        }
        if (type != 0) return failf(NET_E_SHAPE, "ModelBin load type %d not implemented", type);
        unsigned char f[4];
        if (!take(f, 4)) return failf(NET_E_SHAPE, "ModelBin read flag_struct failed");
        uint32_t tag;
        memcpy(&tag, f, 4);
        const unsigned flag = f[0] + f[1] + f[2] + f[3];
        if (tag == 0x01306B47u) // fp16 payload, padded to 4 bytes
        {
            const size_t bytes = (w * 2 + 3) / 4 * 4;
            if ((size_t)(end - p) < bytes) return failf(NET_E_SHAPE, "ModelBin read float16_weights failed");
            for (size_t i = 0; i < w; ++i)
            {
                uint16_t h;
                memcpy(&h, p + 2 * i, 2);
                out[i] = half_to_float(h);
            }
            p += bytes;
            return 0;
        }
        if (tag == 0x000D4B38u) return failf(FHIP_E_UNSUPPORTED, "int8 weights are not supported (conv_layer.h:50-55 rejects them too)");
        if (tag == 0x0002C056u)
        {
            if (!take(out.data(), w * 4)) return failf(NET_E_SHAPE, "ModelBin read weight_data failed");
            return 0;
        }
        if (flag != 0) // 256-entry codebook + one byte per weight, padded to 4 bytes
        {
            float table[256];
            if (!take(table, sizeof(table))) return failf(NET_E_SHAPE, "ModelBin read quantization_value failed");
            const size_t bytes = (w + 3) / 4 * 4;
            if ((size_t)(end - p) < bytes) return failf(NET_E_SHAPE, "ModelBin read index_array failed");
            for (size_t i = 0; i < w; ++i) out[i] = table[p[i]];
            p += bytes;
            return 0;
        }
        if (!take(out.data(), w * 4)) return failf(NET_E_SHAPE, "ModelBin read weight_data failed (file too short)");
        return 0;
    }
};

// ---- blobs ---------------------------------------------------------------------------------------------------
struct Blob
{
    std::string name;
    int n = 0, c = 0, h = 0, w = 0;
    float* data = nullptr;
    size_t capacity = 0;   // floats owned
    Blob* alias = nullptr; // data is another blob's
    bool fused_away = false;
    bool chained = false; // fusion level 3: lives only as the next layer's Winograd-domain input (plan_chains); shape kept, no storage

    size_t count() const { return (size_t)n * c * h * w; }
    int reshape(int n_, int c_, int h_, int w_)
    {
        n = n_;
        c = c_;
        h = h_;
        w = w_;
        alias = nullptr;
        // a blob the previous plan chained away has no storage and, as a rule, will have none after this Reshape either: plan_chains
        // allocates it afterwards if the new shapes un-chain it (no device malloc + free per chained blob and shape change)
        if (chained && !data) return 0;
        if (count() > capacity)
        {
            if (data && capacity) (void)hipFree(data);
            data = nullptr;
            capacity = 0;
            FHIP_CHECK_HIP(hipMalloc((void**)&data, count() * sizeof(float)));
            capacity = count();
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

// ---- layers (reference layer.h:28-86) -------------------------------------------------------------------------
struct Layer
{
    std::string type, name;
    std::vector<Blob*> bottoms, tops;
    Net* net = nullptr;

    virtual ~Layer() {}
    virtual int LoadParam(const ParamDict&) { return 0; }
    virtual int LoadWeights(ModelBin&) { return 0; }
    // default (layer.cpp:103-114): one bottom, one top of the same shape
    virtual int Reshape()
    {
        if (tops.size() != 1 || bottoms.size() != 1) return failf(NET_E_BASE_RESHAPE, "layer %s: base Reshape needs 1 bottom and 1 top", name.c_str());
        return tops[0]->reshape(bottoms[0]->n, bottoms[0]->c, bottoms[0]->h, bottoms[0]->w);
    }
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
    virtual int sibling_state() const { return 0; } // 1: launches the GEMM that also computes the NEXT layer; 2: computed by the layer before
    virtual int residual_state() const { return 0; } // 1: an Eltwise SUM operand is added in this layer's GEMM epilogue; 2: absorbed, added by a separate launch
};

// A ReLU layer without a slope: the only ReLU the fused epilogues of the convolution, deconvolution, InnerProduct, affine and Eltwise
// layers compute.  A leaky one (ncnn's `ReLU 0=slope`) stays a layer of its own behind them.
static bool is_plain_relu(const Layer* l);

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

struct InputLayer : Layer
{
    int Reshape() override { return 0; } // shape comes from FeedInput (input_layer.h:33-46)
    int Forward(hipStream_t) override { return 0; }
};

// A BatchNorm / Scale folded into the convolution or deconvolution before it (fusion level 2): y = y * mul[k] + add[k] per output
// channel k, applied to the filters and the bias at Init.  K is the caller's business: the layers count their channels differently.
struct AffineLayer;
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

// feather::ConvLayer, layers/conv_layer.h:26-193 (also registered as ConvolutionDepthWise, layer_factory.cpp)
struct ConvLayer : Layer
{
    fhip_conv_param p;
    int algo_ = -1, inited_algo = -2;
    // what the packed weights' content depends on besides the route and the byte count (fhip_conv_packed_layout): a new input size packs
    // again when it changes -- a 1x1 layer's streamed image and its InnerProduct image have the same size
    int layout = 0, inited_layout = -1;
    // 1 < group < input_channels: the layer runs through libfeather_gconv.so (gconv_api) with route code FHIP_NET_ROUTE_GCONV.
    // p.output_channels then holds the WHOLE layer's K (the library's convention), not K / group as conv_layer.h:69-75 leaves it.
    // Such a layer fuses a following ReLU and, at level 2, BatchNorm / Scale; every other fusion declines it.
    bool gconv = false;
    // dilation > 1 in a net with fhip_net_set_dilated: the layer runs through libfeather_atrous.so (atrous_api) with route code
    // FHIP_NET_ROUTE_ATROUS, whatever its group.  p.output_channels holds the WHOLE layer's K here too; ap() is the library's param.
    // Fusions as on the grouped route: a following ReLU, at level 2 BatchNorm / Scale, nothing else.
    bool atrous = false;
    int dilation_h = 1, dilation_w = 1;
    fhip_atrous_param ap() const
    {
        fhip_atrous_param a;
        a.output_channels = p.output_channels, a.input_channels = p.input_channels, a.input_h = p.input_h, a.input_w = p.input_w;
        a.kernel_h = p.kernel_h, a.kernel_w = p.kernel_w, a.output_h = p.output_h, a.output_w = p.output_w;
        a.stride_h = p.stride_h, a.stride_w = p.stride_w, a.pad_left = p.pad_left, a.pad_bottom = p.pad_bottom, a.pad_right = p.pad_right, a.pad_top = p.pad_top;
        a.group = p.group, a.bias_term = p.bias_term, a.activation = p.activation, a.dilation_h = dilation_h, a.dilation_w = dilation_w;
        return a;
    }
    std::vector<float> w_host, b_host;
    AffineFold fold; // folded BatchNorm/Scale (fusion level 2)
    DeviceVec packed, bias;
    size_t buffer_bytes = 0, packed_bytes = 0;
    // fusion level 2: a following 2x2 / stride-2 max pooling is absorbed (fhip_conv_forward_maxpool2 when the route can,
    // else this layer runs conv -> pre_pool -> fhip_pooling itself)
    bool fuse_pool = false, pool_fast = false;
    fhip_pool_param poolq;
    DeviceVec pre_pool;
    // fusion level 2: a following Eltwise SUM (+ReLU) with an earlier blob is absorbed: top = act(conv + bias + residual)
    Blob* residual = nullptr;
    bool res_fast = false;
    // fusion level 2: this is a 3x3 depthwise layer and the 1x1 convolution that is its only consumer was absorbed (`pw` owns its
    // parameters, weights and further fusions); when the pair qualifies at the current shape the two run as ONE kernel
    // (fhip_conv_forward_dw_pw) and the depthwise output never exists, else dw -> `mid` -> pw one after the other
    std::unique_ptr<ConvLayer> pw;
    bool pair_fast = false;
    DeviceVec mid;
    // fusion level 3 (plan_chains, after Reshape): this Winograd layer's input arrives already transformed (chain_in) and / or its
    // output leaves as the next layer's transformed input (chain_next); chain_pos = position in the run (picks the V slot)
    ConvLayer* chain_next = nullptr;
    bool chain_in = false;
    int chain_pos = 0;
    size_t chain_bytes = 0; // arena the run needs (reported instead of buffer_bytes)
    // fusion level 3 (plan_chains): this chained layer's V and M hold 2x2 image canvases (feather_canvas.h): its tile GEMM runs on
    // canvas_p -- the layer as one (2H + 2)-pixel image -- at a quarter of the batch, its boundaries through libfeather_canvas.so
    bool canvas = false;
    fhip_conv_param canvas_p;
    fhip_winograd_plan run_plan; // the plan this chained layer runs with (plain or canvas), set by plan_chains
    // fusion level 3 (plan_chains): a first layer (3x3 / s1 / p1, 2 .. 4 input channels) whose only consumer is a Winograd layer is computed
    // inside that layer's input transform (fhip_winograd_f63_input_from_first): `head_of` = the consumer (this layer then launches nothing,
    // its top has no storage), `head` = the absorbed first layer (on the consumer); first_raw = this layer's filters as loaded
    ConvLayer* head_of = nullptr;
    ConvLayer* head = nullptr;
    DeviceVec first_raw;
    // fusion level 2 (plan_siblings, after Reshape): this 1x1 layer and the NEXT layer of the list -- a 1x1 layer on the same bottom with
    // the same stride: ResNet's projection shortcut and the first layer of the main branch -- run as ONE GEMM over the stacked filters
    // (fhip_conv_forward_siblings).  `sib` (on the first layer) = the second; `sib_of` (on the second, which launches nothing) = the first.
    ConvLayer* sib = nullptr;
    ConvLayer* sib_of = nullptr;
    ConvLayer* sib_packed_for = nullptr; // the partner sib_packed / sib_bias were built with
    DeviceVec sib_packed, sib_bias;
    bool sib_has_bias = false;
    bool first_candidate() const
    {
        return p.kernel_h == 3 && p.kernel_w == 3 && p.stride_h == 1 && p.stride_w == 1 && p.group == 1 && p.input_channels >= 2 && p.input_channels <= 4 && p.pad_left == 1 &&
               p.pad_right == 1 && p.pad_top == 1 && p.pad_bottom == 1;
    }

    ConvLayer()
    {
        memset(&p, 0, sizeof(p));
        memset(&poolq, 0, sizeof(poolq));
    }

    int LoadParam(const ParamDict& pd) override
    {
        dilation_w = pd.get(2, 1);
        dilation_h = pd.get(12, dilation_w);
        atrous = dilation_w > 1 || dilation_h > 1;
        if (atrous && !(net && net->dilated))
            return failf(NET_E_UNKNOWN_LAYER, "layer %s: dilated convolution is not supported (fhip_net_set_dilated lifts this)", name.c_str());
        if (dilation_w < 1 || dilation_h < 1) return failf(NET_E_SHAPE, "layer %s: dilation must be >= 1", name.c_str());
        if (pd.get(8, 0)) return failf(NET_E_UNKNOWN_LAYER, "layer %s: int8 convolution is not supported", name.c_str());
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
        gconv = !atrous && p.group > 1 && p.group < p.input_channels;
        if (gconv || atrous) p.output_channels *= p.group;
        if (atrous)
        {
            if (p.pad_left < 0 || p.pad_top < 0) return failf(NET_E_UNKNOWN_LAYER, "layer %s: automatic padding is not supported", name.c_str());
            if (p.input_channels < 1 || p.input_channels % p.group) return failf(NET_E_SHAPE, "layer %s: weight_data_size does not fit the convolution geometry", name.c_str());
            algo_ = FHIP_NET_ROUTE_ATROUS;
        }
        return 0;
    }
    int LoadWeights(ModelBin& mb) override
    {
        const size_t wsize = (size_t)p.input_channels * p.output_channels * p.kernel_h * p.kernel_w / (gconv || atrous ? p.group : 1);
        inited_algo = -2; // new weights: every packed form is rebuilt at the next Init
        sib_packed_for = nullptr;
        int rc = mb.load(wsize, 0, w_host);
        if (rc) return rc;
        if (p.bias_term)
        {
            const int k = atrous ? p.output_channels : p.group == p.input_channels ? p.input_channels : p.output_channels;
            rc = mb.load(k, 1, b_host);
        }
        return rc;
    }
    int Reshape() override
    {
        const Blob* b = bottoms[0];
        p.input_w = b->w;
        p.input_h = b->h;
        if (p.input_channels != b->c)
            return failf(NET_E_TOPOLOGY, "convolution layer %s has %d input channels while bottom blob has %d channels", name.c_str(), p.input_channels, b->c);
        if (atrous)
        {
            const AtrousApi* api = atrous_api();
            if (!api) return FHIP_E_UNSUPPORTED; // message set by atrous_api
            fhip_atrous_param a = ap();
            if (api->assign_output_dim(&a)) return failf(NET_E_SHAPE, "layer %s: %s", name.c_str(), api->last_error());
            p.output_h = a.output_h;
            p.output_w = a.output_w;
            if (api->supported(&a) != 1) return failf(FHIP_E_UNSUPPORTED, "layer %s: dilated convolution refused: %s", name.c_str(), api->last_error());
            algo_ = FHIP_NET_ROUTE_ATROUS;
            int rc = tops[0]->reshape(b->n, p.output_channels, p.output_h, p.output_w);
            if (rc) return rc;
            if ((rc = api->get_buffer_size(&a, b->n, &buffer_bytes, &packed_bytes))) return failf(rc, "layer %s: %s", name.c_str(), api->last_error());
            return 0;
        }
        fhip_conv_assign_output_dim(&p);
        if (p.output_h < 1 || p.output_w < 1) return failf(NET_E_SHAPE, "layer %s: empty output", name.c_str());
        if (gconv)
        {
            const GconvApi* api = gconv_api();
            if (!api) return FHIP_E_UNSUPPORTED; // message set by gconv_api
            if (api->supported(&p) != 1) return failf(FHIP_E_UNSUPPORTED, "layer %s: grouped convolution refused: %s", name.c_str(), api->last_error());
            algo_ = FHIP_NET_ROUTE_GCONV;
            int rc = tops[0]->reshape(b->n, p.output_channels, p.output_h, p.output_w);
            if (rc) return rc;
            if ((rc = api->get_buffer_size(&p, b->n, &buffer_bytes, &packed_bytes))) return failf(rc, "layer %s: %s", name.c_str(), api->last_error());
            return 0;
        }
        int rc = net->tuned_selection ? fhip_conv_select_algo_tuned(&p, &algo_) : fhip_conv_select_algo(&p, &algo_);
        if (rc) return rc;
        if (pw)
        {
            // the absorbed 1x1 convolution reshapes against a stand-in for the depthwise output, then takes over this layer's top
            Blob dwout;
            dwout.n = b->n;
            dwout.c = p.output_channels;
            dwout.h = p.output_h;
            dwout.w = p.output_w;
            pw->bottoms.assign(1, &dwout);
            pw->tops = tops;
            pw->net = net;
            rc = pw->Reshape();
            pw->bottoms.clear();
            if (rc) return rc;
            pair_fast = fhip_conv_can_fuse_dw_pw(&p, &pw->p, b->n) != 0 && !pw->fuse_pool && !pw->residual && pw->algo_ == FHIP_IM2COL;
            if (!pair_fast && (rc = mid.resize((size_t)b->n * p.output_channels * p.output_h * p.output_w * sizeof(float)))) return rc;
            size_t bb = 0;
            if ((rc = fhip_conv_get_buffer_size(&p, algo_, b->n, &bb, &packed_bytes))) return rc;
            buffer_bytes = std::max(bb, pw->buffer_bytes);
            return fhip_conv_packed_layout(&p, algo_, &layout);
        }
        res_fast = residual && fhip_conv_can_fuse_residual(&p, algo_) != 0;
        if (residual && (residual->n != b->n || residual->c != p.output_channels || residual->h != p.output_h || residual->w != p.output_w))
            return failf(NET_E_SHAPE, "Shape mismatch among bottoms of layer %s.", name.c_str());
        if (fuse_pool)
        {
            poolq.channels = p.output_channels;
            poolq.input_h = p.output_h;
            poolq.input_w = p.output_w;
            int ph, pw;
            if ((rc = fhip_pooling_output_dim(&poolq, &ph, &pw))) return rc;
            pool_fast = fhip_conv_can_fuse_maxpool2(&p, algo_) != 0;
            if (!pool_fast && (rc = pre_pool.resize((size_t)b->n * p.output_channels * p.output_h * p.output_w * sizeof(float)))) return rc;
            rc = tops[0]->reshape(b->n, p.output_channels, ph, pw);
        }
        else
            rc = tops[0]->reshape(b->n, p.output_channels, p.output_h, p.output_w);
        if (rc) return rc;
        if ((rc = fhip_conv_get_buffer_size(&p, algo_, b->n, &buffer_bytes, &packed_bytes))) return rc;
        return fhip_conv_packed_layout(&p, algo_, &layout);
    }
    // filters and bias with the folded BatchNorm / Scale (fusion level 2) applied
    void folded(std::vector<float>& w, std::vector<float>& b) const
    {
        w = w_host;
        b = b_host;
        fold.apply(w, b, p.output_channels);
    }
    int init_siblings(hipStream_t s)
    {
        std::vector<float> wa, ba, wb, bb;
        folded(wa, ba);
        sib->folded(wb, bb);
        fhip_conv_param pa = p, pb = sib->p, both;
        pa.bias_term = ba.empty() ? 0 : 1;
        pb.bias_term = bb.empty() ? 0 : 1;
        int rc = fhip_conv_siblings_geometry(&pa, &pb, &both);
        if (rc) return rc;
        wa.insert(wa.end(), wb.begin(), wb.end());
        sib_has_bias = both.bias_term != 0;
        if (sib_has_bias)
        {
            if (ba.empty()) ba.assign(p.output_channels, 0.f);
            if (bb.empty()) bb.assign(sib->p.output_channels, 0.f);
            ba.insert(ba.end(), bb.begin(), bb.end());
            if ((rc = sib_bias.upload(ba.data(), ba.size(), s))) return rc;
        }
        size_t bytes = 0, pk = 0;
        if ((rc = fhip_conv_get_buffer_size(&both, FHIP_IM2COL, bottoms[0]->n, &bytes, &pk))) return rc;
        DeviceVec raw;
        if ((rc = raw.upload(wa.data(), wa.size(), s))) return rc;
        if ((rc = sib_packed.resize(pk))) return rc;
        if ((rc = fhip_conv_init(&both, FHIP_IM2COL, sib_packed.d, raw.d, s))) return rc;
        FHIP_CHECK_HIP(hipStreamSynchronize(s)); // `raw` goes out of scope
        sib_packed_for = sib;
        return 0;
    }
    int Init(hipStream_t s) override
    {
        if (pw)
        {
            const int rc = pw->Init(s);
            if (rc) return rc;
        }
        if (sib && sib_packed_for != sib)
        {
            const int rc = init_siblings(s);
            if (rc) return rc;
        }
        if (inited_algo == algo_ && packed.bytes == packed_bytes && inited_layout == layout) return 0;
        std::vector<float> w, b;
        folded(w, b);
        if (!fold.empty()) p.bias_term = 1;
        DeviceVec raw;
        int rc = raw.upload(w.data(), w.size(), s);
        if (rc) return rc;
        if (first_candidate() && (rc = first_raw.upload(w.data(), w.size(), s))) return rc; // 27 floats per output channel
        rc = packed.resize(packed_bytes);
        if (rc) return rc;
        if (atrous)
        {
            const AtrousApi* api = atrous_api();
            if (!api) return FHIP_E_UNSUPPORTED;
            const fhip_atrous_param a = ap();
            if ((rc = api->init(&a, (float*)packed.d, (const float*)raw.d, s))) return failf(rc, "layer %s: %s", name.c_str(), api->last_error());
        }
        else if (gconv)
        {
            const GconvApi* api = gconv_api();
            if (!api) return FHIP_E_UNSUPPORTED;
            if ((rc = api->init(&p, (float*)packed.d, (const float*)raw.d, s))) return failf(rc, "layer %s: %s", name.c_str(), api->last_error());
        }
        else
            rc = fhip_conv_init(&p, algo_, packed.d, raw.d, s);
        if (rc) return rc;
        if (p.bias_term)
        {
            rc = bias.upload(b.data(), b.size(), s);
            if (rc) return rc;
        }
        FHIP_CHECK_HIP(hipStreamSynchronize(s)); // `raw` and the host copies go out of scope
        inited_algo = algo_;
        inited_layout = layout;
        return 0;
    }
    int Forward(hipStream_t s) override
    {
        const float* b = p.bias_term ? bias.d : nullptr;
        if (atrous)
        {
            const AtrousApi* api = atrous_api();
            if (!api) return FHIP_E_UNSUPPORTED;
            const fhip_atrous_param a = ap();
            const int rc = api->forward(&a, bottoms[0]->n, tops[0]->data, bottoms[0]->data, (const float*)packed.d, nullptr, b, s);
            return rc ? failf(rc, "layer %s: %s", name.c_str(), api->last_error()) : 0;
        }
        if (gconv)
        {
            const GconvApi* api = gconv_api();
            if (!api) return FHIP_E_UNSUPPORTED;
            const int rc = api->forward(&p, bottoms[0]->n, tops[0]->data, bottoms[0]->data, (const float*)packed.d, nullptr, b, s);
            return rc ? failf(rc, "layer %s: %s", name.c_str(), api->last_error()) : 0;
        }
        if (head_of) return 0; // computed inside head_of's input transform
        if (sib_of) return 0;  // computed by the layer before, in the same GEMM
        if (sib)
            return fhip_conv_forward_siblings(&p, &sib->p, bottoms[0]->n, tops[0]->data, sib->tops[0]->data, bottoms[0]->data, sib_packed.d,
                                              sib_has_bias ? sib_bias.d : nullptr, s);
        if (pw)
        {
            const float* pb = pw->p.bias_term ? pw->bias.d : nullptr;
            if (pair_fast)
                return fhip_conv_forward_dw_pw(&p, &pw->p, bottoms[0]->n, tops[0]->data, bottoms[0]->data, packed.d, b, pw->packed.d, pb, s);
            int rc = fhip_conv_forward(&p, algo_, bottoms[0]->n, mid.d, bottoms[0]->data, packed.d, (float*)net->arena.d, b, s);
            if (rc) return rc;
            Blob dwout; // stand-in for the depthwise output the pair no longer has a blob for
            dwout.n = bottoms[0]->n;
            dwout.c = p.output_channels;
            dwout.h = p.output_h;
            dwout.w = p.output_w;
            dwout.data = mid.d;
            pw->bottoms.assign(1, &dwout);
            pw->tops = tops;
            rc = pw->Forward(s);
            pw->bottoms.clear();
            dwout.data = nullptr;
            return rc;
        }
        if (chain_in || chain_next || head)
        {
            char* base = reinterpret_cast<char*>(net->arena.d);
            float* v = reinterpret_cast<float*>(base + net->chain_slot[chain_pos & 1]);
            float* vn = reinterpret_cast<float*>(base + net->chain_slot[(chain_pos + 1) & 1]);
            float* m = reinterpret_cast<float*>(base + net->chain_m);
            const float* in = chain_in || head ? nullptr : bottoms[0]->data;
            const int n = bottoms[0]->n;
            if (head)
            {
                const int rc = fhip_winograd_f63_input_from_first(&head->p, &p, n, v, head->bottoms[0]->data, head->first_raw.d,
                                                                  head->p.bias_term ? head->bias.d : nullptr, s);
                if (rc) return rc;
            }
            if (canvas || (chain_next && chain_next->canvas)) return forward_canvas(n, in, v, m, vn, b, s);
            if (chain_next) return fhip_conv_forward_chained(&p, n, nullptr, in, packed.d, v, m, b, &chain_next->p, vn, fuse_pool ? 1 : 0, s);
            if (!fuse_pool || pool_fast) return fhip_conv_forward_chained(&p, n, tops[0]->data, in, packed.d, v, m, b, nullptr, nullptr, fuse_pool ? 1 : 0, s);
            const int rc = fhip_conv_forward_chained(&p, n, pre_pool.d, in, packed.d, v, m, b, nullptr, nullptr, 0, s);
            if (rc) return rc;
            return fhip_pooling(&poolq, n, tops[0]->data, pre_pool.d, s);
        }
        if (residual)
        {
            if (residual->alias) residual->data = residual->alias->data;
            if (res_fast)
                return fhip_conv_forward_residual(&p, algo_, bottoms[0]->n, tops[0]->data, bottoms[0]->data, packed.d, (float*)net->arena.d, b,
                                                  residual->data, s);
            fhip_conv_param q = p; // route without the fused epilogue: conv, then the add (+ReLU) in place on the top
            q.activation = FHIP_ACT_NONE;
            const int rc = fhip_conv_forward(&q, algo_, bottoms[0]->n, tops[0]->data, bottoms[0]->data, packed.d, (float*)net->arena.d, b, s);
            if (rc) return rc;
            return fhip_add(tops[0]->data, tops[0]->data, residual->data, tops[0]->count(), p.activation == FHIP_ACT_RELU, s);
        }
        if (!fuse_pool) return fhip_conv_forward(&p, algo_, bottoms[0]->n, tops[0]->data, bottoms[0]->data, packed.d, (float*)net->arena.d, b, s);
        if (pool_fast)
            return fhip_conv_forward_maxpool2(&p, algo_, bottoms[0]->n, tops[0]->data, bottoms[0]->data, packed.d, (float*)net->arena.d, b, s);
        const int rc = fhip_conv_forward(&p, algo_, bottoms[0]->n, pre_pool.d, bottoms[0]->data, packed.d, (float*)net->arena.d, b, s);
        if (rc) return rc;
        return fhip_pooling(&poolq, bottoms[0]->n, tops[0]->data, pre_pool.d, s);
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
            if (canvas) return failf(FHIP_E_UNSUPPORTED, "layer %s: a canvas layer takes its input from the chained transform before it", name.c_str());
            if ((rc = fhip_winograd_f63_input_transform(&p, n, v, in, s))) return rc;
        }
        rc = canvas ? fhip_winograd_f63_tile_gemm(&canvas_p, n / 4, m, packed.d, v, s) : fhip_winograd_f63_tile_gemm(&p, n, m, packed.d, v, s);
        if (rc) return rc;
        if (chain_next)
        {
            const int form = !canvas ? FHIP_CANVAS_ENTRY : chain_next->canvas ? FHIP_CANVAS_INSIDE : FHIP_CANVAS_EXIT;
            rc = api->chain(form, &p, &chain_next->p, n, &run_plan, &chain_next->run_plan, vn, m, b, s);
        }
        else
            rc = api->output(&p, n, &run_plan, tops[0]->data, m, b, fuse_pool ? 1 : 0, s);
        return rc ? failf(rc, "layer %s: %s", name.c_str(), api->last_error()) : 0;
    }
    int Fuse(Layer* next, int level) override;
    // absorb `elt` = Eltwise SUM of this layer's top and `other` (a blob produced earlier in the layer list)
    bool FuseResidual(Blob* other)
    {
        if (pw)
        {
            // behind an absorbed 1x1 convolution (MobileNet-V2 style dw -> pw(linear) -> add): the add goes into the POINTWISE layer's
            // epilogue; the pair then runs its two kernels one after the other (Reshape: pair_fast needs a pointwise layer without residual)
            if (fuse_pool || residual || !pw->FuseResidual(other)) return false;
            pw->bottoms.pop_back();   // the pointwise layer's bottoms are set per call (a stand-in for the depthwise output)
            bottoms.push_back(other); // dependency scans look at THIS layer
            return true;
        }
        if (gconv || atrous || fuse_pool || residual || p.activation != FHIP_ACT_NONE) return false;
        residual = other;
        bottoms.push_back(other); // so that dependency scans (fusion, branch concurrency) see the second input
        return true;
    }
    size_t weight_bytes() const override
    {
        return packed.bytes + bias.bytes + pre_pool.bytes + mid.bytes + first_raw.bytes + sib_packed.bytes + sib_bias.bytes + (pw ? pw->weight_bytes() : 0);
    }
    const fhip_conv_param* fused_pointwise(int* one_kernel) const override
    {
        if (one_kernel) *one_kernel = pair_fast ? 1 : 0;
        return pw ? &pw->p : nullptr;
    }
    size_t arena_bytes() const override { return std::max(buffer_bytes, chain_bytes); }
    const fhip_conv_param* conv_param() const override { return &p; }
    int algo() const override { return atrous ? FHIP_NET_ROUTE_ATROUS : gconv ? FHIP_NET_ROUTE_GCONV : algo_; }
    int sibling_state() const override { return sib ? 1 : sib_of ? 2 : 0; }
    int residual_state() const override { return !residual ? 0 : res_fast ? 1 : 2; }
    void chain_state(int* v_from_previous, int* writes_next_v) const override
    {
        *v_from_previous = head ? 2 : chain_in ? 1 : 0;
        *writes_next_v = head_of ? 2 : chain_next ? 1 : 0;
    }
    int canvas_state() const override { return canvas ? 1 : 0; }
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
    bool inited = false;

    InnerProductLayer() { memset(&p, 0, sizeof(p)); }
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
        return 0;
    }
    int LoadWeights(ModelBin& mb) override
    {
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
        int rc = tops[0]->reshape(b->n, (int)output_size, 1, 1);
        if (rc) return rc;
        return fhip_conv_get_buffer_size(&p, FHIP_IM2COL, b->n, &buffer_bytes, &packed_bytes);
    }
    int Init(hipStream_t s) override
    {
        if (inited) return 0;
        DeviceVec raw;
        int rc = raw.upload(w_host.data(), w_host.size(), s);
        if (rc) return rc;
        rc = packed.resize(packed_bytes);
        if (rc) return rc;
        rc = fhip_conv_init(&p, FHIP_IM2COL, packed.d, raw.d, s);
        if (rc) return rc;
        if (p.bias_term)
        {
            rc = bias.upload(b_host.data(), b_host.size(), s);
            if (rc) return rc;
        }
        FHIP_CHECK_HIP(hipStreamSynchronize(s));
        std::vector<float>().swap(w_host); // the packed copy is shape independent: the raw weights are not needed again
        inited = true;
        return 0;
    }
    int Forward(hipStream_t s) override
    {
        return fhip_conv_forward(&p, FHIP_IM2COL, bottoms[0]->n, tops[0]->data, bottoms[0]->data, packed.d, (float*)net->arena.d,
                                 p.bias_term ? bias.d : nullptr, s);
    }
    int Fuse(Layer* next, int) override
    {
        if (is_plain_relu(next))
        {
            p.activation = FHIP_ACT_RELU;
            return 1;
        }
        return 0;
    }
    size_t weight_bytes() const override { return packed.bytes + bias.bytes; }
    size_t arena_bytes() const override { return buffer_bytes; }
    int algo() const override { return FHIP_IM2COL; }
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
    int Reshape() override
    {
        if (slope != 0.f && !inorm_api()) return FHIP_E_UNSUPPORTED; // message set by inorm_api
        return Layer::Reshape();
    }
    int Forward(hipStream_t s) override
    {
        if (slope == 0.f) return fhip_relu(tops[0]->data, bottoms[0]->data, bottoms[0]->count(), s);
        const InormApi* api = inorm_api();
        if (!api) return FHIP_E_UNSUPPORTED;
        const Blob* b = bottoms[0];
        const int rc = api->activation(FHIP_ACTIVATION_LEAKY_RELU, tops[0]->data, b->data, b->n, b->c, b->h * b->w, slope, 0.f, nullptr, s);
        return rc ? failf(rc, "layer %s: %s", name.c_str(), api->last_error()) : 0;
    }
};

static bool is_plain_relu(const Layer* l) { return l->type == "ReLU" && static_cast<const ReluLayer*>(l)->slope == 0.f; }

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
        const InormApi* api = inorm_api();
        if (!api) return FHIP_E_UNSUPPORTED; // message set by inorm_api
        int rc = api->get_buffer_size(b->n, b->c, b->h, b->w, &scratch_bytes);
        if (rc) return failf(rc, "layer %s: %s", name.c_str(), api->last_error());
        return Layer::Reshape();
    }
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
        const InormApi* api = inorm_api();
        if (!api) return FHIP_E_UNSUPPORTED;
        const Blob* b = bottoms[0];
        const int rc = api->forward(b->n, b->c, b->h, b->w, tops[0]->data, b->data, affine ? d_gamma.d : nullptr, affine ? d_beta.d : nullptr, eps, act,
                                    slope, scratch_bytes ? net->arena.d : nullptr, s);
        return rc ? failf(rc, "layer %s: %s", name.c_str(), api->last_error()) : 0;
    }
    int Fuse(Layer* next, int) override
    {
        if (next->type != "ReLU" || act != FHIP_INORM_ACT_NONE) return 0;
        slope = static_cast<ReluLayer*>(next)->slope;
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
        if (!inorm_api()) return FHIP_E_UNSUPPORTED; // message set by inorm_api
        return Layer::Reshape();
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
        const InormApi* api = inorm_api();
        if (!api) return FHIP_E_UNSUPPORTED;
        const Blob* b = bottoms[0];
        const int rc = api->activation(kind, tops[0]->data, b->data, b->n, b->c, b->h * b->w, p0, p1, num_slope > 1 ? d_slopes.d : nullptr, s);
        return rc ? failf(rc, "layer %s: %s", name.c_str(), api->last_error()) : 0;
    }
    size_t weight_bytes() const override { return d_slopes.bytes; }
};

struct PoolingLayer : Layer
{
    fhip_pool_param q;
    PoolingLayer() { memset(&q, 0, sizeof(q)); }
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
        return tops[0]->reshape(b->n, b->c, oh, ow);
    }
    int Forward(hipStream_t s) override { return fhip_pooling(&q, bottoms[0]->n, tops[0]->data, bottoms[0]->data, s); }
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
            AffineLayer* nx = static_cast<AffineLayer*>(next);
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
    const GateApi* api = gate_api();
    if (!api) return FHIP_E_UNSUPPORTED;
    const int rc = api->apply(x->n, x->c, x->h, x->w, l->tops[0]->data, x->data, g->data, nullptr, FHIP_GATE_ACT_NONE, s);
    return rc ? failf(rc, "layer %s: %s", l->name.c_str(), api->last_error()) : 0;
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
    int Reshape() override
    {
        if (!gate_api()) return FHIP_E_UNSUPPORTED; // message set by gate_api
        return Layer::Reshape();
    }
    int Forward(hipStream_t s) override
    {
        const GateApi* api = gate_api();
        if (!api) return FHIP_E_UNSUPPORTED;
        const Blob* b = bottoms[0];
        const int rc = api->activation(kind, tops[0]->data, b->data, b->n, b->c, b->h * b->w, alpha, beta, s);
        return rc ? failf(rc, "layer %s: %s", name.c_str(), api->last_error()) : 0;
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

    int Reshape() override
    {
        const Blob* x = bottoms[0];
        const Blob* y = bottoms[1];
        if (x->c != C) return failf(NET_E_TOPOLOGY, "squeeze-and-excitation block %s has %d channels while bottom blob %s has %d", name.c_str(), C, x->name.c_str(), x->c);
        for (size_t i = 1; i < bottoms.size(); ++i)
            if (bottoms[i]->n != x->n || bottoms[i]->c != x->c || bottoms[i]->h != x->h || bottoms[i]->w != x->w)
                return failf(NET_E_SHAPE, "Shape mismatch among bottoms of layer %s.", name.c_str());
        stepwise = 2ll * R > (long long)x->h * x->w;
        if (stepwise)
        {
            scratch_bytes = 0;
            for (auto& l : parts)
            {
                const int rc = l->Reshape();
                if (rc) return rc;
                scratch_bytes = std::max(scratch_bytes, l->arena_bytes());
            }
            return 0;
        }
        const GateApi* api = gate_api();
        if (!api) return FHIP_E_UNSUPPORTED; // message set by gate_api
        int rc = api->squeeze_buffer_size(x->n, x->c, x->h, x->w, &scratch_bytes);
        if (rc) return failf(rc, "layer %s: %s", name.c_str(), api->last_error());
        if ((rc = mean.resize((size_t)x->n * C * sizeof(float))) || (rc = gate.resize((size_t)x->n * C * sizeof(float)))) return rc;
        return tops[0]->reshape(y->n, y->c, y->h, y->w);
    }
    int Init(hipStream_t s) override
    {
        if (stepwise)
        {
            for (auto& l : parts)
            {
                const int rc = l->Init(s);
                if (rc) return rc;
            }
            return 0;
        }
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
        if (stepwise)
        {
            for (auto& l : parts)
            {
                const int rc = l->Forward(s);
                if (rc) return rc;
            }
            return 0;
        }
        const GateApi* api = gate_api();
        if (!api) return FHIP_E_UNSUPPORTED;
        const Blob* x = bottoms[0];
        int rc = api->squeeze(x->n, x->c, x->h, x->w, mean.d, x->data, scratch_bytes ? net->arena.d : nullptr, s);
        if (!rc) rc = api->excite(x->n, C, R, gate.d, mean.d, d_w1.d, has_b1 ? d_b1.d : nullptr, d_w2.d, has_b2 ? d_b2.d : nullptr, mact, gact, alpha, beta, s);
        if (!rc) rc = api->apply(x->n, x->c, x->h, x->w, tops[0]->data, bottoms[1]->data, gate.d, bottoms.size() > 2 ? bottoms[2]->data : nullptr, act, s);
        return rc ? failf(rc, "layer %s: %s", name.c_str(), api->last_error()) : 0;
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
        const ResampleApi* api = resample_api();
        if (!api) return FHIP_E_UNSUPPORTED;
        const Blob* x = bottoms[0];
        const Blob* t = tops[0];
        // a scale is handed on only where it decided the size
        const int rc = api->interp(mode, align, x->n, x->c, x->h, x->w, t->h, t->w, sized_by || out_h ? 0.f : hs, sized_by || out_w ? 0.f : ws, t->data, x->data,
                                   residual_at >= 0 ? bottoms[residual_at]->data : nullptr, relu, s);
        return rc ? failf(rc, "layer %s: %s", name.c_str(), api->last_error()) : 0;
    }
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
    int Reshape() override
    {
        if (!resample_api()) return FHIP_E_UNSUPPORTED; // message set by resample_api
        return Layer::Reshape();
    }
    int Forward(hipStream_t s) override
    {
        const ResampleApi* api = resample_api();
        if (!api) return FHIP_E_UNSUPPORTED;
        const Blob* b = bottoms[0];
        const int rc = api->hardswish(tops[0]->data, b->data, b->n, b->c, b->h * b->w, alpha, beta, s);
        return rc ? failf(rc, "layer %s: %s", name.c_str(), api->last_error()) : 0;
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
        const LrnApi* api = lrn_api();
        if (!api) return FHIP_E_UNSUPPORTED;
        const Blob* b = bottoms[0];
        float* normalised = scratch_bytes ? net->arena.d : tops[0]->data;
        const int rc = pooled && !scratch_bytes ? api->pool_forward(region, local_size, alpha, beta, bias, b->n, b->c, b->h, b->w, &q, tops[0]->data, b->data, s)
                                                : api->forward(region, local_size, alpha, beta, bias, b->n, b->c, b->h, b->w, normalised, b->data, s);
        if (rc) return failf(rc, "layer %s: %s", name.c_str(), api->last_error());
        return scratch_bytes ? fhip_pooling(&q, b->n, tops[0]->data, normalised, s) : 0;
    }
    size_t arena_bytes() const override { return scratch_bytes; }
    int Fuse(Layer* next, int level) override
    {
        if (level < 2 || pooled || next->type != "Pooling") return 0;
        const fhip_pool_param& p = static_cast<PoolingLayer*>(next)->q;
        if (p.global_pooling || p.kernel_h < 1 || p.kernel_w < 1 || p.stride_h < 1 || p.stride_w < 1) return 0;
        if (p.pad_left < 0 || p.pad_right < 0 || p.pad_top < 0 || p.pad_bottom < 0) return 0;
        q = p;
        pooled = true;
        return 1;
    }
    int algo() const override { return FHIP_NET_ROUTE_LRN; }
};

int ConvLayer::Fuse(Layer* next, int level)
{
    if (pw) return pw->Fuse(next, level) == 1 ? 1 : 0; // behind the absorbed 1x1 convolution: its own fusions
    if (fuse_pool) return 0; // nothing is absorbed behind the pooling
    if ((gconv || atrous) && !is_plain_relu(next) && next->type != "BatchNorm" && next->type != "Scale") return 0; // the grouped and dilated routes have these epilogues only
    if (level >= 2 && !residual && next->type == "Convolution" && p.group == p.input_channels && p.group > 1 && p.group <= 256 && p.kernel_h == 3 &&
        p.kernel_w == 3 && p.stride_h == p.stride_w && (p.stride_h == 1 || p.stride_h == 2) && p.pad_left == 1 && p.pad_top == 1)
    {
        // depthwise 3x3 (at most 256 channels: fhip_conv_can_fuse_dw_pw's structural conditions) -> 1x1 convolution: the pair becomes one
        // layer -- one kernel where the shapes qualify too, else the two kernels one after the other inside this layer
        const fhip_conv_param& q = static_cast<ConvLayer*>(next)->p;
        if (static_cast<ConvLayer*>(next)->atrous) return 0;
        if (q.group != 1 || q.kernel_h != 1 || q.kernel_w != 1 || q.stride_h != 1 || q.stride_w != 1 || q.pad_left || q.pad_right || q.pad_top || q.pad_bottom)
            return 0;
        // fhip_conv_can_fuse_dw_pw's profitable range -- or the band-staged kernel's pair (32 channels, stride 1, a multiple of 64 output channels:
        // MobileNet's first pair); the row width is only known at Reshape, where the pair falls back to its two kernels if it does not qualify
        const bool band_pair = p.input_channels == 32 && p.stride_h == 1 && q.output_channels % 64 == 0 && q.output_channels <= 128; // = dwpw_band_applicable's bound
        if (!band_pair && (q.output_channels <= 64 || q.output_channels >= (p.stride_h == 1 ? 160 : 400))) return 0;
        return 2; // the pass hands `next` over (fuse_layers)
    }
    if (residual && !is_plain_relu(next)) return 0; // behind the residual add only its ReLU
    if (level >= 2 && next->type == "Pooling")
    {
        const fhip_pool_param& q = static_cast<PoolingLayer*>(next)->q;
        if (q.pooling_type != 0 || q.global_pooling || q.kernel_h != 2 || q.kernel_w != 2 || q.stride_h != 2 || q.stride_w != 2 || q.pad_left ||
            q.pad_right || q.pad_top || q.pad_bottom)
            return 0;
        poolq = q;
        fuse_pool = true;
        return 1;
    }
    if (is_plain_relu(next))
    {
        p.activation = FHIP_ACT_RELU;
        return 1;
    }
    // level 2 (beyond the reference): fold a following BatchNorm / Scale into the weights and bias
    if (level >= 2 && p.activation == FHIP_ACT_NONE && (next->type == "BatchNorm" || next->type == "Scale"))
    {
        const int K = atrous ? p.output_channels : p.group == p.input_channels ? p.input_channels : p.output_channels;
        return fold.absorb(*static_cast<AffineLayer*>(next), K) ? 1 : 0;
    }
    return 0;
}

// ncnn's Deconvolution / DeconvolutionDepthWise (no reference counterpart; the definition is include/feather_hip/feather_deconv.h).
// Runs through libfeather_deconv.so (deconv_api) with route code FHIP_NET_ROUTE_DECONV.  Fuses a following ReLU and, at level 2,
// BatchNorm / Scale (weights are [K][C/group][kh][kw], so the fold is the convolution's); it is no "Convolution" to any other fusion
// (residual add, pooling, depthwise + pointwise, siblings, Winograd chains, first layer, the side stream), which therefore decline it.
struct DeconvLayer : Layer
{
    fhip_deconv_param p;
    int weight_data_size = 0;
    std::vector<float> w_host, b_host;
    AffineFold fold; // folded BatchNorm/Scale (fusion level 2)
    DeviceVec packed, bias;
    size_t buffer_bytes = 0, packed_bytes = 0;
    bool inited = false;

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
        inited = false; // new weights: the packed form is rebuilt at the next Init
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
        const DeconvApi* api = deconv_api();
        if (!api) return FHIP_E_UNSUPPORTED; // message set by deconv_api
        p.input_w = b->w;
        p.input_h = b->h;
        if (api->assign_output_dim(&p)) return failf(NET_E_SHAPE, "layer %s: %s", name.c_str(), api->last_error());
        if (api->supported(&p) != 1) return failf(FHIP_E_UNSUPPORTED, "layer %s: deconvolution refused: %s", name.c_str(), api->last_error());
        int rc = tops[0]->reshape(b->n, p.output_channels, p.output_h, p.output_w);
        if (rc) return rc;
        if ((rc = api->get_buffer_size(&p, b->n, &buffer_bytes, &packed_bytes))) return failf(rc, "layer %s: %s", name.c_str(), api->last_error());
        return 0;
    }
    int Init(hipStream_t s) override
    {
        if (inited && packed.bytes == packed_bytes) return 0;
        const DeconvApi* api = deconv_api();
        if (!api) return FHIP_E_UNSUPPORTED;
        std::vector<float> w = w_host, b = b_host;
        fold.apply(w, b, p.output_channels);
        if (!fold.empty()) p.bias_term = 1;
        DeviceVec raw;
        int rc = raw.upload(w.data(), w.size(), s);
        if (rc) return rc;
        if ((rc = packed.resize(packed_bytes))) return rc;
        if ((rc = api->init(&p, packed.d, raw.d, s))) return failf(rc, "layer %s: %s", name.c_str(), api->last_error());
        if (p.bias_term && (rc = bias.upload(b.data(), b.size(), s))) return rc;
        FHIP_CHECK_HIP(hipStreamSynchronize(s)); // `raw` and the host copies go out of scope
        inited = true;
        return 0;
    }
    int Forward(hipStream_t s) override
    {
        const DeconvApi* api = deconv_api();
        if (!api) return FHIP_E_UNSUPPORTED;
        const int rc = api->forward(&p, bottoms[0]->n, tops[0]->data, bottoms[0]->data, packed.d, nullptr, p.bias_term ? bias.d : nullptr, s);
        return rc ? failf(rc, "layer %s: %s", name.c_str(), api->last_error()) : 0;
    }
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
    if (level >= 2 && p.activation == FHIP_ACT_NONE && (next->type == "BatchNorm" || next->type == "Scale"))
        return fold.absorb(*static_cast<AffineLayer*>(next), p.output_channels) ? 1 : 0;
    return 0;
}

struct EltwiseLayer : Layer
{
    bool relu = false;
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
        if (is_plain_relu(next))
        {
            relu = true;
            return 1;
        }
        return 0;
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
        const ShuffleApi* api = shuffle_api();
        if (!api) return FHIP_E_UNSUPPORTED;
        float* outs[FHIP_CHANNEL_MAP_MAX_BLOBS];
        const float* srcs[FHIP_CHANNEL_MAP_MAX_BLOBS];
        for (size_t j = 0; j < tops.size(); ++j) outs[j] = tops[j]->data;
        for (size_t i = 0; i < bottoms.size(); ++i) srcs[i] = bottoms[i]->data;
        const Blob* a = bottoms[0];
        const int rc = api->forward(map, outs, srcs, a->n, a->h, a->w, s);
        return rc ? failf(rc, "layer %s: %s", name.c_str(), api->last_error()) : 0;
    }
    int algo() const override { return FHIP_NET_ROUTE_SHUFFLE; }
};

static bool is_channel_map_type(const Layer* l)
{
    return l->type == "ShuffleChannel" || l->type == "Slice" || (l->type == "Concat" && static_cast<const ConcatLayer*>(l)->axis == 0);
}

// Fusion level 2: a run of Concat / ShuffleChannel / Slice layers, in any order, that follow each other in the layer list and are linked
// by blobs with exactly one consumer becomes one ChannelMapLayer (ShuffleNet v2's Concat -> ShuffleChannel -> Slice: two bottoms, two
// tops, one launch).  The layer keeps the type and name of the run's first layer; the linking blobs are fused away.  A run of Concat
// layers alone is left as it is (their copies are not this route's); a run with more bottoms or tops than one map takes is cut
// back to its longest prefix that fits.
static void collapse_channel_maps(Net& net)
{
    auto uses = [&](const Blob* b) {
        int u = 0;
        for (auto& l : net.layers)
            for (const Blob* x : l->bottoms) u += x == b;
        return u;
    };
    auto holds = [](const std::vector<Blob*>& v, const Blob* b) { return std::find(v.begin(), v.end(), b) != v.end(); };
    for (size_t i = 0; i < net.layers.size(); ++i)
    {
        if (!is_channel_map_type(net.layers[i].get())) continue;
        std::vector<Blob*> made = net.layers[i]->tops;
        size_t end = i + 1;
        for (; end < net.layers.size(); ++end)
        {
            const Layer* l = net.layers[end].get();
            if (!is_channel_map_type(l)) break;
            bool reads = false, sole = true;
            for (const Blob* b : l->bottoms)
                if (holds(made, b))
                {
                    reads = true;
                    sole = sole && uses(b) == 1;
                }
            if (!reads || !sole) break;
            made.insert(made.end(), l->tops.begin(), l->tops.end());
        }
        // the longest prefix of the run that moves channels and fits one map
        std::vector<Blob*> sources, inner, finals;
        for (; end - i >= 2; --end)
        {
            sources.clear();
            inner.clear();
            finals.clear();
            bool moves = false;
            for (size_t k = i; k < end; ++k)
            {
                moves = moves || net.layers[k]->type != "Concat";
                for (Blob* b : net.layers[k]->bottoms)
                {
                    if (holds(made, b))
                        inner.push_back(b);
                    else if (!holds(sources, b))
                        sources.push_back(b);
                }
            }
            for (size_t k = i; k < end; ++k)
                for (Blob* t : net.layers[k]->tops)
                    if (!holds(inner, t)) finals.push_back(t);
            if (moves && sources.size() <= FHIP_CHANNEL_MAP_MAX_BLOBS && finals.size() <= FHIP_CHANNEL_MAP_MAX_BLOBS) break;
        }
        if (end - i < 2) continue;
        std::unique_ptr<ChannelMapLayer> run(new ChannelMapLayer);
        run->type = net.layers[i]->type;
        run->name = net.layers[i]->name;
        run->net = &net;
        run->bottoms = sources;
        run->tops = finals;
        for (size_t k = i; k < end; ++k)
        {
            Layer* l = net.layers[k].get();
            if (l->type == "Concat")
            {
                MapStep st;
                st.kind = MapStep::CONCAT;
                st.name = l->name;
                st.bottoms = l->bottoms;
                st.tops = l->tops;
                run->steps.push_back(st);
            }
            else
                run->steps.push_back(static_cast<ChannelMapLayer*>(l)->steps[0]);
        }
        for (Blob* b : inner) b->fused_away = true;
        net.layers[i] = std::move(run);
        net.layers.erase(net.layers.begin() + i + 1, net.layers.begin() + end);
    }
}

struct SplitLayer : Layer
{
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

// Fusion level 2: a squeeze-and-excitation block,
//
//   Split(x) -> Pooling(global, average) -> {InnerProduct | Convolution 1x1, group 1} -> [ReLU | Swish]
//            -> {InnerProduct | Convolution 1x1, group 1} -> {Sigmoid | HardSigmoid}
//            -> {BinaryOp mul | Scale -233}(x, gate)   [-> Eltwise SUM with another blob [-> plain ReLU]]
//
// where every linking blob has exactly one consumer, becomes one GateBlockLayer.  The pass runs BEFORE the pairwise Fuse pass of
// fuse_layers: afterwards the first excite layer would already have absorbed its ReLU and the block would no longer read as written.
// The layer keeps the Pooling layer's type and name and takes the place of the block's LAST layer in the list: the shortcut of a residual
// block may be produced between the Pooling layer and the Eltwise layer, and everything the block reads is ready where its last layer
// stood.  A block that does not match (a linking blob with a second consumer, a grouped, strided or padded excite convolution, a pooling
// that is not global average, operands that are not two tops of one Split) stays layer by layer.
static void collapse_gate_blocks(Net& net)
{
    auto sole_consumer = [&](const Blob* b) -> int { // index of the only layer that reads b (once), or -1
        int uses = 0, at = -1;
        for (size_t j = 0; j < net.layers.size(); ++j)
            for (const Blob* x : net.layers[j]->bottoms)
                if (x == b)
                {
                    ++uses;
                    at = (int)j;
                }
        return uses == 1 ? at : -1;
    };
    auto one_to_one = [](const Layer* l) { return l->bottoms.size() == 1 && l->tops.size() == 1; };
    // W [out][in] and bias of an InnerProduct or of a plain 1x1 convolution
    auto dense = [&](Layer* l, int& in, int& out, std::vector<float>& w, std::vector<float>& b, bool& has_b) {
        if (!one_to_one(l)) return false;
        if (l->type == "InnerProduct")
        {
            InnerProductLayer* ip = static_cast<InnerProductLayer*>(l);
            if (ip->p.activation != FHIP_ACT_NONE || ip->w_host.size() != ip->input_size * ip->output_size) return false;
            in = (int)ip->input_size, out = (int)ip->output_size, w = ip->w_host, b = ip->b_host, has_b = ip->p.bias_term != 0;
            return true;
        }
        if (l->type != "Convolution") return false;
        ConvLayer* cv = static_cast<ConvLayer*>(l);
        const fhip_conv_param& p = cv->p;
        if (cv->gconv || cv->atrous || p.group != 1 || p.kernel_h != 1 || p.kernel_w != 1 || p.stride_h != 1 || p.stride_w != 1 || p.pad_left || p.pad_right ||
            p.pad_top || p.pad_bottom || p.activation != FHIP_ACT_NONE || !cv->fold.empty() || cv->w_host.size() != (size_t)p.input_channels * p.output_channels)
            return false;
        in = p.input_channels, out = p.output_channels, w = cv->w_host, b = cv->b_host, has_b = p.bias_term != 0;
        return true;
    };
    for (size_t i = 0; i < net.layers.size(); ++i)
    {
        Layer* pool = net.layers[i].get();
        if (pool->type != "Pooling" || !one_to_one(pool)) continue;
        const fhip_pool_param& q = static_cast<PoolingLayer*>(pool)->q;
        if (!q.global_pooling || q.pooling_type == 0) continue;
        std::vector<int> gone(1, (int)i);
        std::vector<Blob*> inner;
        std::unique_ptr<GateBlockLayer> blk(new GateBlockLayer);
        auto step = [&](Blob* top) -> Layer* { // the layer behind a linking blob
            const int j = sole_consumer(top);
            if (j < 0) return nullptr;
            gone.push_back(j);
            inner.push_back(top);
            return net.layers[j].get();
        };
        Layer* l = step(pool->tops[0]);
        int in2 = 0, out2 = 0;
        if (!l || !dense(l, blk->C, blk->R, blk->w1, blk->b1, blk->has_b1)) continue;
        if (!(l = step(l->tops[0]))) continue;
        if (one_to_one(l) && (is_plain_relu(l) || l->type == "Swish"))
        {
            blk->mact = l->type == "Swish" ? FHIP_EXCITE_MACT_SWISH : FHIP_EXCITE_MACT_RELU;
            if (!(l = step(l->tops[0]))) continue;
        }
        if (!dense(l, in2, out2, blk->w2, blk->b2, blk->has_b2) || in2 != blk->R || out2 != blk->C) continue;
        if (!(l = step(l->tops[0])) || !one_to_one(l)) continue;
        if (l->type == "HardSigmoid")
        {
            blk->gact = FHIP_EXCITE_GACT_HARDSIGMOID;
            blk->alpha = static_cast<GateActivationLayer*>(l)->alpha;
            blk->beta = static_cast<GateActivationLayer*>(l)->beta;
        }
        else if (l->type != "Sigmoid")
            continue;
        Blob* g = l->tops[0];
        if (!(l = step(g)) || l->bottoms.size() != 2 || l->tops.size() != 1) continue;
        Blob* x = nullptr;
        if (l->type == "BinaryOp")
            x = l->bottoms[0] == g ? l->bottoms[1] : l->bottoms[0];
        else if (l->type == "Scale" && static_cast<ScaleLayer*>(l)->gated && l->bottoms[1] == g)
            x = l->bottoms[0];
        if (!x || x == g || x == pool->bottoms[0]) continue;
        bool siblings = false; // the squeezed and the gated blob are two tops of one Split: the same tensor
        for (auto& s : net.layers)
            if (s->type == "Split")
            {
                bool a = false, b = false;
                for (const Blob* t : s->tops) a = a || t == pool->bottoms[0], b = b || t == x;
                siblings = siblings || (a && b);
            }
        if (!siblings) continue;
        blk->bottoms.push_back(pool->bottoms[0]);
        blk->bottoms.push_back(x);
        Blob* out = l->tops[0];
        const int jsum = sole_consumer(out);
        if (jsum >= 0)
        {
            Layer* sum = net.layers[jsum].get();
            if (sum->type == "Eltwise" && sum->bottoms.size() == 2 && sum->tops.size() == 1 && sum->bottoms[0] != sum->bottoms[1])
            {
                blk->bottoms.push_back(sum->bottoms[0] == out ? sum->bottoms[1] : sum->bottoms[0]);
                gone.push_back(jsum);
                inner.push_back(out);
                out = sum->tops[0];
                const int jrelu = sole_consumer(out);
                if (static_cast<EltwiseLayer*>(sum)->relu)
                    blk->act = FHIP_GATE_ACT_RELU;
                else if (jrelu >= 0 && one_to_one(net.layers[jrelu].get()) && is_plain_relu(net.layers[jrelu].get()))
                {
                    blk->act = FHIP_GATE_ACT_RELU;
                    gone.push_back(jrelu);
                    inner.push_back(out);
                    out = net.layers[jrelu]->tops[0];
                }
            }
        }
        bool forward = true; // the chain runs down the list
        for (size_t k = 1; k < gone.size(); ++k) forward = forward && gone[k] > gone[k - 1];
        if (!forward) continue;
        blk->type = pool->type;
        blk->name = pool->name;
        blk->net = &net;
        blk->q = q;
        blk->tops.assign(1, out);
        for (Blob* b : inner) b->fused_away = true;
        for (int j : gone) blk->parts.push_back(std::move(net.layers[j])); // kept for the shapes that run stepwise
        net.layers[gone.back()] = std::move(blk);
        for (size_t k = gone.size() - 1; k-- > 0;) net.layers.erase(net.layers.begin() + gone[k]);
        --i; // the layer that moved into slot i has not been looked at
    }
}

// Fusion level 2: FPN's upsample-and-add,
//
//   Interp(x [, size]) -> Eltwise SUM (two bottoms, no coefficients) with another blob [-> plain ReLU]
//
// where the Interp's top -- and the sum's, if a ReLU follows -- has exactly one consumer, becomes the InterpLayer alone: the other operand is
// its last bottom (residual_at) and the whole chain is one launch that never writes the up-sampled tensor.  Like collapse_gate_blocks the
// pass runs before the pairwise Fuse pass and the layer takes the place of the chain's LAST layer in the list: the other operand (FPN's
// lateral convolution) may be produced between the Interp and the Eltwise layer.  The layer keeps its type and name; the blobs inside the
// chain refuse Extract.  An Interp whose top has a second consumer stays as written.
static void collapse_upsample_adds(Net& net)
{
    auto sole_consumer = [&](const Blob* b) -> int { // index of the only layer that reads b (once), or -1
        int uses = 0, at = -1;
        for (size_t j = 0; j < net.layers.size(); ++j)
            for (const Blob* x : net.layers[j]->bottoms)
                if (x == b)
                {
                    ++uses;
                    at = (int)j;
                }
        return uses == 1 ? at : -1;
    };
    for (size_t i = 0; i < net.layers.size(); ++i)
    {
        if (net.layers[i]->type != "Interp") continue;
        InterpLayer* up = static_cast<InterpLayer*>(net.layers[i].get());
        if (up->residual_at >= 0 || up->tops.size() != 1) continue;
        Blob* top = up->tops[0];
        const int jsum = sole_consumer(top);
        if (jsum <= (int)i) continue;
        Layer* sum = net.layers[jsum].get();
        if (sum->type != "Eltwise" || sum->bottoms.size() != 2 || sum->tops.size() != 1 || sum->bottoms[0] == sum->bottoms[1]) continue;
        Blob* other = sum->bottoms[0] == top ? sum->bottoms[1] : sum->bottoms[0];
        Blob* out = sum->tops[0];
        int last = jsum;
        bool relu = static_cast<EltwiseLayer*>(sum)->relu;
        std::vector<Blob*> inner(1, top);
        if (!relu)
        {
            const int jrelu = sole_consumer(out);
            if (jrelu > jsum && net.layers[jrelu]->bottoms.size() == 1 && net.layers[jrelu]->tops.size() == 1 && is_plain_relu(net.layers[jrelu].get()))
            {
                relu = true;
                inner.push_back(out);
                out = net.layers[jrelu]->tops[0];
                last = jrelu;
            }
        }
        up->bottoms.push_back(other);
        up->residual_at = (int)up->bottoms.size() - 1;
        up->relu = relu;
        up->tops[0] = out;
        for (Blob* b : inner) b->fused_away = true;
        std::unique_ptr<Layer> moved = std::move(net.layers[i]);
        net.layers[last] = std::move(moved); // the ReLU (or the Eltwise) is dropped, the Interp stands in its place
        if (last != jsum) net.layers.erase(net.layers.begin() + jsum);
        net.layers.erase(net.layers.begin() + i);
        --i; // the layer that moved into slot i has not been looked at
    }
}

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
        std::unique_ptr<Layer> layer(create_layer(type));
        if (!layer && net.extended) layer.reset(create_extended_layer(type));
        if (!layer)
        {
            std::unique_ptr<Layer> opt_in(create_extended_layer(type));
            return failf(NET_E_UNKNOWN_LAYER, "layer %s not exists or registered%s", type.c_str(), opt_in ? " (fhip_net_set_extended_layers lifts this)" : "");
        }
        layer->type = type;
        layer->name = name;
        layer->net = &net;
        const int bottom_count = atoi(nb.c_str()), top_count = atoi(nt.c_str());
        // the reference uses both counts as read (net.cpp:98-137) and a layer without bottoms or tops faults at its first Reshape
        if (bottom_count < 0 || top_count < 1 || (bottom_count == 0 && type != "Input"))
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

// The fusion pass of layer.cpp:82-101 (TryFuse): a layer absorbs the single consumer of its single top.
static void fuse_layers(Net& net)
{
    if (net.fused) return;
    net.fused = true;
    if (net.fusion <= 0) return;
    if (net.fusion >= 2) collapse_channel_maps(net);
    if (net.fusion >= 2) collapse_gate_blocks(net);
    if (net.fusion >= 2) collapse_upsample_adds(net);
    for (size_t i = 0; i < net.layers.size(); ++i)
    {
        for (;;)
        {
            Layer* cur = net.layers[i].get();
            if (cur->tops.size() != 1) break;
            Blob* top = cur->tops[0];
            size_t consumer = 0;
            int uses = 0;
            for (size_t j = i + 1; j < net.layers.size(); ++j)
                for (Blob* b : net.layers[j]->bottoms)
                    if (b == top)
                    {
                        ++uses;
                        consumer = j;
                    }
            if (uses != 1) break;
            Layer* nx = net.layers[consumer].get();
            if (net.fusion >= 2 && nx->type == "Eltwise" && nx->bottoms.size() == 2 && nx->tops.size() == 1 && nx->bottoms[0] != nx->bottoms[1] &&
                (cur->type == "Convolution" || cur->type == "ConvolutionDepthWise"))
            {
                // conv -> Eltwise(sum with an EARLIER blob) [-> ReLU]: the add moves into the conv's epilogue
                Blob* other = nx->bottoms[0] == top ? nx->bottoms[1] : nx->bottoms[0];
                bool earlier = false;
                for (size_t j = 0; j < i; ++j)
                    for (Blob* t : net.layers[j]->tops) earlier = earlier || t == other;
                if (!earlier || !static_cast<ConvLayer*>(cur)->FuseResidual(other)) break;
                top->fused_away = true;
                cur->tops[0] = nx->tops[0];
                net.layers.erase(net.layers.begin() + consumer);
                continue;
            }
            if (nx->bottoms.size() != 1 || nx->tops.size() != 1) break;
            const int fr = cur->Fuse(nx, net.fusion);
            if (fr != 1 && fr != 2) break;
            if (fr == 2) static_cast<ConvLayer*>(cur)->pw.reset(static_cast<ConvLayer*>(net.layers[consumer].release())); // adopted, not dropped
            top->fused_away = true;
            cur->tops[0] = nx->tops[0];
            net.layers.erase(net.layers.begin() + consumer);
        }
    }
}

// Which layers may leave the main stream (see Net::concurrency).  Needs the algorithms chosen by Reshape: only layers without
// scratch (the arena is shared) qualify.
static int plan_concurrency(Net& net)
{
    const size_t L = net.layers.size();
    net.side.assign(L, -1);
    net.waits.assign(L, std::vector<int>());
    if (!net.concurrency) return 0;
    int pairs = 0;
    for (size_t i = 0; i < L; ++i)
    {
        Layer* l = net.layers[i].get();
        if ((l->type != "Convolution" && l->type != "ConvolutionDepthWise") || l->arena_bytes() != 0 || l->tops.size() != 1) continue;
        if (l->sibling_state()) continue; // writes (or is written with) the top of its neighbour: stays on the net's stream
        size_t consumer = 0;
        int uses = 0;
        for (size_t j = i + 1; j < L; ++j)
            for (Blob* b : net.layers[j]->bottoms)
                if (b == l->tops[0] || b->alias == l->tops[0])
                {
                    ++uses;
                    consumer = j;
                }
        if (uses != 1 || consumer <= i + 1) continue;
        bool work_between = false; // something worth overlapping with
        for (size_t j = i + 1; j < consumer; ++j) work_between = work_between || net.layers[j]->algo() >= 0;
        if (!work_between) continue;
        net.side[i] = pairs;
        net.waits[consumer].push_back(pairs);
        ++pairs;
    }
    if (pairs && !net.side_stream) FHIP_CHECK_HIP(hipStreamCreateWithFlags(&net.side_stream, hipStreamNonBlocking));
    while (net.events.size() < (size_t)2 * pairs)
    {
        hipEvent_t e;
        FHIP_CHECK_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        net.events.push_back(e);
    }
    return 0;
}

// Fusion level 3, after Reshape (needs the routes and shapes): a Winograd layer directly followed by the 3x3 / stride-1 / pad-1 Winograd
// layer that is the only consumer of its top hands over its output already transformed (fhip_conv_forward_chained); the blob between
// them gets no storage.  VGG-16: conv1_2 ... conv5_3 become one run.
static int plan_chains(Net& net)
{
    const size_t L = net.layers.size();
    std::vector<ConvLayer*> conv(L, nullptr);
    for (size_t i = 0; i < L; ++i)
        if (net.layers[i]->type == "Convolution" || net.layers[i]->type == "ConvolutionDepthWise")
        {
            conv[i] = static_cast<ConvLayer*>(net.layers[i].get());
            conv[i]->chain_next = nullptr;
            conv[i]->chain_in = false;
            conv[i]->chain_pos = 0;
            conv[i]->chain_bytes = 0;
            conv[i]->canvas = false;
            conv[i]->head = conv[i]->head_of = nullptr;
        }
    for (auto& kv : net.blobs) kv.second->chained = false;
    for (auto& b : net.shadowed) b->chained = false; // blobs whose name a later top re-used (in-place style .param files) re-plan too
    net.chain_slot[0] = net.chain_slot[1] = net.chain_m = 0;
    if (net.fusion < 3) return 0;
    auto plain = [](const ConvLayer* c) { return c && !c->pw && !c->residual && c->algo_ == FHIP_WINOGRADF63 && c->tops.size() == 1 && c->bottoms.size() == 1; };
    for (size_t i = 0; i + 1 < L; ++i)
    {
        ConvLayer *a = conv[i], *b = conv[i + 1];
        if (!plain(a) || !plain(b) || b->bottoms[0] != a->tops[0]) continue;
        if (a->fuse_pool && !a->pool_fast) continue;
        int uses = 0;
        for (size_t j = 0; j < L; ++j)
            for (Blob* x : net.layers[j]->bottoms) uses += (x == a->tops[0] || x->alias == a->tops[0]) ? 1 : 0;
        if (uses != 1) continue;
        if (!fhip_conv_can_chain_winograd(&a->p, a->algo_, &b->p, b->algo_, a->fuse_pool ? 1 : 0)) continue;
        a->chain_next = b;
        b->chain_in = true;
        b->chain_pos = a->chain_pos + 1;
        a->tops[0]->chained = true;
        a->tops[0]->drop_storage();
    }
    // 2x2 image canvases (feather_canvas.h): a maximal sub-run of chained layers on one plane size, entered through a pooled boundary, whose
    // planes are whole tiles as canvases (14 and 56 pixels: 0.69 x and 0.90 x the tiles) runs with four images of a channel per "image".
    // It ends in a pooled boundary to a plain layer, or with the run (the canvas output transform; a pooling that is not fused stays plain).
    for (size_t i = 0; i < L; ++i)
    {
        ConvLayer* c = conv[i];
        if (!c || !c->chain_in || c->canvas) continue;
        ConvLayer* prev = nullptr;
        for (size_t j = 0; j < i; ++j)
            if (conv[j] && conv[j]->chain_next == c) prev = conv[j];
        if (!prev || prev->canvas || !prev->fuse_pool || prev->head) continue; // a sub-run starts behind a plain layer's pooled boundary
        const int n = c->bottoms[0]->n;
        fhip_conv_param q;
        if (fhip_winograd_f63_canvas_param(&prev->p, n, &q) == FHIP_OK) continue; // (never: a pooled consumer of a canvas plane is not one)
        if (prev->p.kernel_h != 3 || prev->p.pad_left != 1 || prev->p.pad_right != 1 || prev->p.pad_top != 1 || prev->p.pad_bottom != 1 ||
            prev->p.output_h != prev->p.output_w || prev->p.output_h != prev->p.input_h)
            continue;
        std::vector<ConvLayer*> run;
        for (ConvLayer* x = c; x; x = x->chain_next)
        {
            if (x->p.input_h != c->p.input_h || x->p.input_w != c->p.input_w || fhip_winograd_f63_canvas_param(&x->p, n, &q) != FHIP_OK) break;
            if (x->p.activation != FHIP_ACT_NONE && x->p.activation != FHIP_ACT_RELU) break;
            run.push_back(x);
            if (x->fuse_pool) break; // the plane size changes behind it
        }
        if (run.empty()) continue;
        ConvLayer* last = run.back();
        // the sub-run must be the whole stretch on this plane size, and leave through a form that exists: EXIT (pooled), or the end of the run
        if (last->chain_next && !last->fuse_pool) continue;
        if (!last->chain_next && last->fuse_pool && !last->pool_fast) continue;
        if (!canvas_api()) return FHIP_E_UNSUPPORTED; // message set by canvas_api
        for (ConvLayer* x : run)
        {
            x->canvas = true;
            (void)fhip_winograd_f63_canvas_param(&x->p, n, &x->canvas_p);
        }
    }
    // a first layer in front of a Winograd layer (VGG-16: conv1_1 -> conv1_2) is computed inside that layer's input transform
    for (size_t i = 0; i + 1 < L; ++i)
    {
        ConvLayer *a = conv[i], *b = conv[i + 1];
        if (!a || a->atrous || a->pw || a->residual || a->fuse_pool || a->chain_in || a->chain_next || a->tops.size() != 1 || a->bottoms.size() != 1) continue;
        if (!a->first_candidate() || !plain(b) || b->chain_in || b->bottoms[0] != a->tops[0]) continue;
        int uses = 0;
        for (size_t j = 0; j < L; ++j)
            for (Blob* x : net.layers[j]->bottoms) uses += (x == a->tops[0] || x->alias == a->tops[0]) ? 1 : 0;
        if (uses != 1) continue;
        if (!fhip_conv_can_fuse_first_winograd(&a->p, &b->p, b->algo_, a->bottoms[0]->n)) continue;
        a->head_of = b;
        b->head = a;
        a->tops[0]->chained = true;
        a->tops[0]->drop_storage();
    }
    // blobs the previous plan had chained and this one did not: Reshape left them without storage
    auto restore = [](Blob* b) -> int {
        if (b->chained || b->data || b->alias || b->fused_away || b->count() == 0) return 0;
        FHIP_CHECK_HIP(hipMalloc((void**)&b->data, b->count() * sizeof(float)));
        b->capacity = b->count();
        return 0;
    };
    for (auto& kv : net.blobs)
        if (const int rc = restore(kv.second.get())) return rc;
    for (auto& b : net.shadowed)
        if (const int rc = restore(b.get())) return rc;
    auto up = [](size_t x) { return (x + 255) / 256 * 256; };
    size_t slot[2] = {0, 0}, msz = 0;
    for (size_t i = 0; i < L; ++i)
    {
        ConvLayer* c = conv[i];
        if (!c || (!c->chain_in && !c->chain_next && !c->head)) continue;
        fhip_winograd_plan pl;
        const int rc = fhip_winograd_f63_plan_canvas(&c->p, c->bottoms[0]->n, c->canvas ? 2 : 1, &pl);
        if (rc) return rc;
        c->run_plan = pl;
        slot[c->chain_pos & 1] = std::max(slot[c->chain_pos & 1], up(pl.v_bytes));
        msz = std::max(msz, up(pl.m_bytes));
    }
    net.chain_slot[0] = 0;
    net.chain_slot[1] = slot[0];
    net.chain_m = slot[0] + slot[1];
    for (size_t i = 0; i < L; ++i)
        if (conv[i] && (conv[i]->chain_in || conv[i]->chain_next || conv[i]->head)) conv[i]->chain_bytes = slot[0] + slot[1] + msz;
    return 0;
}

// Fusion level 2, after Reshape (needs routes, shapes and the batch): two 1x1 convolutions that follow each other in the layer list and
// read the same blob with the same stride run as one GEMM (fhip_conv_forward_siblings).  ResNet-50: res3a / res4a / res5a branch1 + branch2a.
static int plan_siblings(Net& net)
{
    const size_t L = net.layers.size();
    std::vector<ConvLayer*> conv(L, nullptr);
    for (size_t i = 0; i < L; ++i)
        if (net.layers[i]->type == "Convolution")
        {
            conv[i] = static_cast<ConvLayer*>(net.layers[i].get());
            conv[i]->sib = conv[i]->sib_of = nullptr;
        }
    if (net.fusion < 2) return 0;
    auto root = [](const Blob* b) { return b->alias ? b->alias : b; };
    auto plain = [](const ConvLayer* c) {
        return c && !c->pw && !c->residual && !c->fuse_pool && !c->chain_in && !c->chain_next && !c->head && !c->head_of && !c->sib && !c->sib_of &&
               c->algo_ == FHIP_IM2COL && c->tops.size() == 1 && c->bottoms.size() == 1;
    };
    for (size_t i = 0; i + 1 < L; ++i)
    {
        ConvLayer *a = conv[i], *b = conv[i + 1];
        if (!plain(a) || !plain(b) || root(a->bottoms[0]) != root(b->bottoms[0]) || a->tops[0] == b->tops[0]) continue;
        // both layers on the 128-row tile when alone (a 64-row layer -- ResNet's res2a_branch2a -- is faster on its own 64 x 128 tile:
        // tools/sibling_bench.py 116 vs 126 us for the pair)
        if (a->p.output_channels <= 64 || b->p.output_channels <= 64) continue;
        if (!fhip_conv_can_fuse_siblings(&a->p, a->algo_, &b->p, b->algo_, a->bottoms[0]->n)) continue;
        a->sib = b;
        b->sib_of = a;
    }
    // a pair that a new shape un-planned keeps no stacked copy of its filters (the layers' own packed weights stay -- they are what
    // the pair falls back to, and what Extract-driven level changes run)
    for (size_t i = 0; i < L; ++i)
        if (conv[i] && !conv[i]->sib && conv[i]->sib_packed.bytes)
        {
            conv[i]->sib_packed.release();
            conv[i]->sib_bias.release();
            conv[i]->sib_packed_for = nullptr;
        }
    return 0;
}

static int reshape_all(Net& net)
{
    net.drop_graph();
    size_t need = 0;
    for (auto& l : net.layers)
    {
        const int rc = l->Reshape();
        if (rc) return rc;
    }
    {
        int rc = plan_chains(net);
        if (rc) return rc;
        if ((rc = plan_siblings(net))) return rc;
    }
    for (auto& l : net.layers) need = std::max(need, l->arena_bytes());
    // one scratch arena shared by every layer = max over layers (mempool.cpp:88-92)
    if (need > net.arena.bytes)
    {
        const int rc = net.arena.resize(need);
        if (rc) return rc;
    }
    net.shapes_dirty = false;
    return plan_concurrency(net);
}

static int prepare(Net& net)
{
    if (!net.param_loaded) return failf(NET_E_IO, "Network has not been loaded. Please load the param file first.");
    if (!net.weights_loaded)
    {
        bool needs = false;
        for (auto& l : net.layers) needs = needs || (l->type != "Input" && l->type != "ReLU" && l->type != "Pooling" && l->type != "Softmax" &&
                                                     l->type != "Split" && l->type != "Eltwise" && l->type != "Concat" && l->type != "Dropout" &&
                                                     l->type != "Sigmoid" && l->type != "TanH" && l->type != "Clip" && l->type != "ShuffleChannel" &&
                                                     l->type != "Slice" && l->type != "BinaryOp" && l->type != "Swish" && l->type != "HardSigmoid" &&
                                                     l->type != "Interp" && l->type != "HardSwish" && l->type != "LRN" &&
                                                     !(l->type == "Scale" && static_cast<ScaleLayer*>(l.get())->gated));
        if (needs) return failf(NET_E_IO, "weights have not been loaded");
    }
    fuse_layers(net);
    for (auto& kv : net.blobs)
        if (!kv.second->fused_away && kv.second->count() == 0)
        {
            bool is_input = false;
            for (auto& l : net.layers)
                if (l->type == "Input")
                    for (Blob* tb : l->tops) is_input = is_input || tb == kv.second.get();
            if (is_input) return failf(NET_E_SHAPE, "input blob %s has not been fed", kv.first.c_str());
        }
    if (net.shapes_dirty)
    {
        const int rc = reshape_all(net);
        if (rc) return rc;
    }
    for (auto& l : net.layers) // Init is a no-op for a layer whose packed weights are still valid
    {
        const int rc = l->Init(net.stream);
        if (rc) return rc;
    }
    net.initialized = true;
    return 0;
}

static int run_layers(Net& net)
{
    for (size_t i = 0; i < net.layers.size(); ++i)
    {
        Layer* l = net.layers[i].get();
        if (i < net.side.size() && net.side[i] >= 0)
        {
            hipEvent_t fork = net.events[2 * net.side[i]], join = net.events[2 * net.side[i] + 1];
            FHIP_CHECK_HIP(hipEventRecord(fork, net.stream)); // everything this layer reads is produced earlier on the main stream
            FHIP_CHECK_HIP(hipStreamWaitEvent(net.side_stream, fork, 0));
            const int rc = l->Forward(net.side_stream);
            if (rc) return rc;
            FHIP_CHECK_HIP(hipEventRecord(join, net.side_stream));
            continue;
        }
        if (i < net.waits.size())
            for (int pair : net.waits[i]) FHIP_CHECK_HIP(hipStreamWaitEvent(net.stream, net.events[2 * pair + 1], 0));
        const int rc = l->Forward(net.stream);
        if (rc) return rc;
    }
    return 0;
}

static int forward(Net& net)
{
    int rc = prepare(net);
    if (rc) return rc;
    if (!net.use_graph) return run_layers(net);
    if (!net.graph_exec)
    {
        hipGraph_t graph = nullptr;
        FHIP_CHECK_HIP(hipStreamBeginCapture(net.stream, hipStreamCaptureModeThreadLocal));
        rc = run_layers(net);
        const hipError_t e = hipStreamEndCapture(net.stream, &graph);
        if (rc)
        {
            if (graph) (void)hipGraphDestroy(graph);
            return rc;
        }
        FHIP_CHECK_HIP(e);
        const hipError_t ei = hipGraphInstantiate(&net.graph_exec, graph, nullptr, nullptr, 0);
        (void)hipGraphDestroy(graph);
        FHIP_CHECK_HIP(ei);
    }
    FHIP_CHECK_HIP(hipGraphLaunch(net.graph_exec, net.stream));
    return 0;
}

} // namespace net
} // namespace fhip

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
        m->impl.concurrency = n->impl.concurrency;
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

int fhip_net_set_concurrency(fhip_net* n, int on)
{
    NET_GUARD(n);
    n->impl.concurrency = on != 0;
    n->impl.shapes_dirty = true; // re-plan (and drop a captured graph) at the next Forward
    for (auto& m : n->more) (void)fhip_net_set_concurrency(m.get(), on);
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
