// net_side.h -- the Net runtime's errors and its side libraries: the table of each libfeather_<x>.so and side_api<X>(), which opens it.
// First of the headers of net.hip (net_side.h, net_model.h, net_core.h, net_conv.h, net_layers.h, net_detect.h, net_yolo.h, net_roi.h, net_frame.h, net_attn.h, net_rnn.h, net_plan.h): none includes a later one.
#pragma once
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
#include "feather_hip/feather_colpass.h" // declarations only: the library is opened at run time (colpass_api)
#include "feather_hip/feather_atrous.h" // declarations only: the library is opened at run time (atrous_api)
#include "feather_hip/feather_deconv.h" // declarations only: the library is opened at run time (deconv_api)
#include "feather_hip/feather_detect.h" // declarations only: the library is opened at run time (detect_api)
#include "feather_hip/feather_gate.h" // declarations only: the library is opened at run time (gate_api)
#include "feather_hip/feather_gconv.h" // declarations only: the library is opened at run time (gconv_api)
#include "feather_hip/feather_inorm.h" // declarations only: the library is opened at run time (inorm_api)
#include "feather_hip/feather_lrn.h" // declarations only: the library is opened at run time (lrn_api)
#include "feather_hip/feather_net.h"
#include "feather_hip/feather_q8.h" // declarations only: the library is opened at run time (q8_api)
#include "feather_hip/feather_qconv.h" // declarations only: the library is opened at run time (qconv_api)
#include "feather_hip/feather_resample.h" // declarations only: the library is opened at run time (resample_api)
#include "feather_hip/feather_shuffle.h" // declarations only: the library is opened at run time (shuffle_api)

namespace fhip::net
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

// libfeather_qconv.so, the route of the Convolution / InnerProduct layers with int8 weights of a net with fhip_net_set_quantized
struct QconvApi
{
    decltype(&fhip_qconv_assign_output_dim) assign_output_dim = nullptr;
    decltype(&fhip_qconv_supported) supported = nullptr;
    decltype(&fhip_qconv_get_buffer_size) get_buffer_size = nullptr;
    decltype(&fhip_qconv_init) init = nullptr;
    decltype(&fhip_qconv_dequant_scales) dequant_scales = nullptr;
    decltype(&fhip_qconv_forward) forward = nullptr;
    decltype(&fhip_qconv_last_error) last_error = nullptr;
    SideLibrary library()
    {
        return {"libfeather_qconv.so", "an int8 convolution / InnerProduct layer", "feather_qconv.h",
                {{&assign_output_dim, "fhip_qconv_assign_output_dim"}, {&supported, "fhip_qconv_supported"},
                 {&get_buffer_size, "fhip_qconv_get_buffer_size"}, {&init, "fhip_qconv_init"}, {&dequant_scales, "fhip_qconv_dequant_scales"},
                 {&forward, "fhip_qconv_forward"}, {&last_error, "fhip_qconv_last_error"}}};
    }
};
static const QconvApi* qconv_api() { return side_api<QconvApi>(); }

// libfeather_q8.so, the int8 layers of a net with fhip_net_set_requantized whose input, output or both are q8 blobs, and the ReLU and max
// Pooling layers between them
struct Q8Api
{
    decltype(&fhip_q8_assign_output_dim) assign_output_dim = nullptr;
    decltype(&fhip_q8_supported) supported = nullptr;
    decltype(&fhip_q8_get_buffer_size) get_buffer_size = nullptr;
    decltype(&fhip_q8_init) init = nullptr;
    decltype(&fhip_q8_dequant_scales) dequant_scales = nullptr;
    decltype(&fhip_q8_forward) forward = nullptr;
    decltype(&fhip_q8_relu_forward) relu = nullptr;
    decltype(&fhip_q8_max_pool_forward) max_pool = nullptr;
    decltype(&fhip_q8_last_error) last_error = nullptr;
    SideLibrary library()
    {
        return {"libfeather_q8.so", "an int8 layer with int8 input or output", "feather_q8.h",
                {{&assign_output_dim, "fhip_q8_assign_output_dim"}, {&supported, "fhip_q8_supported"}, {&get_buffer_size, "fhip_q8_get_buffer_size"},
                 {&init, "fhip_q8_init"}, {&dequant_scales, "fhip_q8_dequant_scales"}, {&forward, "fhip_q8_forward"}, {&relu, "fhip_q8_relu_forward"},
                 {&max_pool, "fhip_q8_max_pool_forward"}, {&last_error, "fhip_q8_last_error"}}};
    }
};
static const Q8Api* q8_api() { return side_api<Q8Api>(); }

// libfeather_detect.so, the layers of a net with fhip_net_set_detection: Permute, Normalize, PriorBox, DetectionOutput, the strided softmax
// and the Concat of permuted heads collapsed at fusion level 2 (net_detect.h)
struct DetectApi
{
    decltype(&fhip_permute_output_dim) permute_output_dim = nullptr;
    decltype(&fhip_permute_forward) permute = nullptr;
    decltype(&fhip_permute_concat_forward) permute_concat = nullptr;
    decltype(&fhip_normalize_forward) normalize = nullptr;
    decltype(&fhip_axis_softmax_forward) axis_softmax = nullptr;
    decltype(&fhip_priorbox_fill) priorbox = nullptr;
    decltype(&fhip_detection_output_get_buffer_size) detection_buffer_size = nullptr;
    decltype(&fhip_detection_output_forward) detection_output = nullptr;
    decltype(&fhip_detect_last_error) last_error = nullptr;
    SideLibrary library()
    {
        return {"libfeather_detect.so", "a detection-head layer (Permute, Normalize, PriorBox, DetectionOutput, Softmax along an axis)", "feather_detect.h",
                {{&permute_output_dim, "fhip_permute_output_dim"}, {&permute, "fhip_permute_forward"}, {&permute_concat, "fhip_permute_concat_forward"},
                 {&normalize, "fhip_normalize_forward"}, {&axis_softmax, "fhip_axis_softmax_forward"}, {&priorbox, "fhip_priorbox_fill"},
                 {&detection_buffer_size, "fhip_detection_output_get_buffer_size"}, {&detection_output, "fhip_detection_output_forward"},
                 {&last_error, "fhip_detect_last_error"}}};
    }
};
static const DetectApi* detect_api() { return side_api<DetectApi>(); }

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

// libfeather_colpass.so, the tile GEMM of chained 64-input-channel Winograd layers that writes the column-passed M and the chained transform
// that reads it (plan_chains, fhip_net_set_colpass).  Like the canvas form a faster way to run the same layers, not a layer type: at mode
// 1 a tree without the library keeps the main route (colpass_api_quiet), at mode 2 the net fails at plan_chains.
struct ColpassApi
{
    decltype(&fhip_colpass_supported) supported = nullptr;
    decltype(&fhip_colpass_tile_gemm) tile_gemm = nullptr;
    decltype(&fhip_colpass_output_to_next_input) chain = nullptr;
    decltype(&fhip_colpass_last_error) last_error = nullptr;
    SideLibrary library()
    {
        return {"libfeather_colpass.so", "a chained Winograd layer on the column-passed tile GEMM (fhip_net_set_colpass 2)", "feather_colpass.h",
                {{&supported, "fhip_colpass_supported"}, {&tile_gemm, "fhip_colpass_tile_gemm"}, {&chain, "fhip_colpass_output_to_next_input"},
                 {&last_error, "fhip_colpass_last_error"}}};
    }
};
static const ColpassApi* colpass_api() { return side_api<ColpassApi>(); }
// the default mode: a tree without the library is no error, and the thread's last error stays what it was
static const ColpassApi* colpass_api_quiet()
{
    const std::string kept = fhip_last_error();
    const ColpassApi* api = colpass_api();
    if (!api) fail(FHIP_OK, kept.c_str());
    return api;
}

} // namespace fhip::net
