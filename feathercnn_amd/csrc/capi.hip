// capi.hip -- the extern "C" surface declared in include/feather_hip/feather_hip.h: algorithm selection,
// buffer sizing, Init and Forward dispatch (the GPU counterpart of reference src/booster/avx/booster.cpp),
// error reporting and per-stage event timing.
#include <string.h>
#include <stdlib.h>

#include <algorithm>
#include <mutex>
#include <string>
#include <vector>

#include "common.h"
#include "feather_hip/feather_net.h"

namespace fhip
{
// kernels (winograd_f63.hip, implicit_gemm.hip, depthwise.hip)
int winograd_plan(const fhip_conv_param& p, int batch, fhip_winograd_plan* plan);
int winograd_transform_kernel(const fhip_conv_param& p, float* u, const float* kernel, hipStream_t s);
int winograd_input_transform(const fhip_conv_param& p, int batch, float* v, const float* input, hipStream_t s);
int winograd_tile_gemm(const fhip_conv_param& p, int batch, float* m, const float* u, const float* v, hipStream_t s);
int winograd_output_transform(const fhip_conv_param& p, int batch, float* output, const float* m, const float* bias,
                              hipStream_t s, int pool = 0);
bool winograd_can_pool(const fhip_conv_param& p);
bool winograd_can_chain(const fhip_conv_param& p, const fhip_conv_param& next, int pool);
bool winograd_can_fuse_first(const fhip_conv_param& first, const fhip_conv_param& next, int batch);
fhip_conv_param igemm_twin_geometry(const fhip_conv_param& a, const fhip_conv_param& b);
bool igemm_twin_applicable(const fhip_conv_param& a, const fhip_conv_param& b, int batch);
int igemm_twin_forward(const fhip_conv_param& a, const fhip_conv_param& b, int batch, float* out_a, float* out_b, const float* in, const float* packed,
                       const float* bias, hipStream_t s);
int winograd_input_from_first(const fhip_conv_param& first, const fhip_conv_param& next, int batch, float* v, const float* input,
                              const float* first_kernel, const float* first_bias, hipStream_t s);
int winograd_output_to_next_input(const fhip_conv_param& p, const fhip_conv_param& next, int batch, float* vn, const float* m, const float* bias,
                                  hipStream_t s, int pool);
void igemm_packed_dims(const fhip_conv_param& p, int* kd_padded, int* k_padded);
int igemm_init(const fhip_conv_param& p, float* packed, const float* kernel, hipStream_t s);
int igemm_forward(const fhip_conv_param& p, int batch, float* out, const float* in, const float* packed, const float* bias,
                  float* buffer, bool force_no_act, hipStream_t s, const float* residual = nullptr);
size_t igemm_buffer_bytes(const fhip_conv_param& p, int batch);
int igemm_check_columns(const fhip_conv_param& p, int batch);
size_t igemm_packed_floats(const fhip_conv_param& p);
int igemm_packed_layout(const fhip_conv_param& p);
bool igemm_streams(const fhip_conv_param& p, int batch);
int depthwise_forward(const fhip_conv_param& p, int batch, float* out, const float* in, const float* kernel, const float* bias,
                      hipStream_t s);
int depthwise_init(const fhip_conv_param& p, float* packed, const float* kernel, hipStream_t s);
size_t depthwise_packed_floats(const fhip_conv_param& p, size_t* w12_offset);
bool dwpw_applicable(const fhip_conv_param& dw, const fhip_conv_param& pw, int batch);
int dwpw_forward(const fhip_conv_param& dw, const fhip_conv_param& pw, int batch, float* out, const float* in, const float* dw_packed,
                 const float* dw_bias, const float* pw_packed, const float* pw_bias, hipStream_t s);

// ---- errors -----------------------------------------------------------------------------------------
static thread_local std::string g_last_error;

int fail(int code, const char* msg)
{
    g_last_error = msg ? msg : "";
    return code;
}

int fail_hip(hipError_t e, const char* what)
{
    g_last_error = std::string(what) + ": " + hipGetErrorString(e);
    return FHIP_E_HIP;
}

int device_compute_units()
{
    static int cached[64] = {0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
    if (cached[dev] == 0)
    {
        int cu = 0;
        if (hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cu <= 0) cu = 256;
        cached[dev] = cu;
    }
    return cached[dev];
}

// LDS bytes of one CU of the current device (cached per device; 160 KiB on MI355X) -- what the persistent grids' residency estimates divide by
size_t device_lds_bytes()
{
    static size_t cached[64] = {0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 160 * 1024;
    if (cached[dev] == 0)
    {
        // gfx950: 160 KiB by the architecture (MI355X_MICROARCH.md; some ROCm versions report the 64 KiB per-block default here).  Any other part: what the
        // runtime says, at least the 64 KiB every CDNA CU has -- the estimates then err on the side of fewer resident blocks, never more
        hipDeviceProp_t prop;
        int b = 0;
        if (hipGetDeviceProperties(&prop, dev) == hipSuccess && strncmp(prop.gcnArchName, "gfx950", 6) == 0)
            b = 160 * 1024;
        else if (hipDeviceGetAttribute(&b, hipDeviceAttributeMaxSharedMemoryPerMultiprocessor, dev) != hipSuccess || b < 64 * 1024)
            b = 64 * 1024;
        cached[dev] = (size_t)b;
    }
    return cached[dev];
}

// ---- stage timing -----------------------------------------------------------------------------------
struct TimedLaunch
{
    int stage;
    hipEvent_t a, b;
};
static std::mutex g_tm_mu;
static bool g_tm_on = false;
static std::vector<TimedLaunch> g_tm_pending;
static std::vector<std::pair<hipEvent_t, hipEvent_t>> g_tm_pool;

StageTimer::StageTimer(int st, hipStream_t s) : stage(st), stream(s), slot(-1)
{
    if (!g_tm_on) return;
    std::lock_guard<std::mutex> lk(g_tm_mu);
    TimedLaunch t;
    t.stage = st;
    if (!g_tm_pool.empty())
    {
        t.a = g_tm_pool.back().first;
        t.b = g_tm_pool.back().second;
        g_tm_pool.pop_back();
    }
    else if (hipEventCreate(&t.a) != hipSuccess || hipEventCreate(&t.b) != hipSuccess)
        return;
    (void)hipEventRecord(t.a, s);
    g_tm_pending.push_back(t);
    slot = (int)g_tm_pending.size() - 1;
}

StageTimer::~StageTimer()
{
    if (slot < 0) return;
    std::lock_guard<std::mutex> lk(g_tm_mu);
    if (slot < (int)g_tm_pending.size()) (void)hipEventRecord(g_tm_pending[slot].b, stream);
}

static bool valid_param(const fhip_conv_param* p)
{
    return p && p->input_channels > 0 && p->output_channels > 0 && p->input_h > 0 && p->input_w > 0 && p->kernel_h > 0 &&
           p->kernel_w > 0 && p->output_h > 0 && p->output_w > 0;
}

} // namespace fhip

using namespace fhip;

extern "C"
{

int fhip_conv_assign_output_dim(fhip_conv_param* p)
{
    if (!p) return fail(FHIP_E_BADARG, "null param");
    if (p->group == 0) p->group = 1;
    if (p->stride_h == 0) p->stride_h = 1;
    if (p->stride_w == 0) p->stride_w = 1;
    p->output_h = (p->input_h + p->pad_top + p->pad_bottom - p->kernel_h) / p->stride_h + 1;
    p->output_w = (p->input_w + p->pad_left + p->pad_right - p->kernel_w) / p->stride_w + 1;
    if (p->group == p->input_channels) p->output_channels = p->input_channels;
    return FHIP_OK;
}

int fhip_conv_select_algo_tuned(const fhip_conv_param* p, int* algo)
{
    const int rc = fhip_conv_select_algo(p, algo);
    if (rc) return rc;
    if (*algo == FHIP_IM2COL && p->group == 1 && p->kernel_h == 3 && p->kernel_w == 3 && p->stride_h == 1 && p->stride_w == 1 && p->input_h >= 4 &&
        p->input_w >= 4 && p->output_channels % 4 == 0 && p->input_channels % 4 == 0 && p->input_channels >= 16 && p->input_channels <= 1024)
        *algo = FHIP_WINOGRADF63;
    return FHIP_OK;
}

double fhip_conv_flops(const fhip_conv_param* p)
{
    if (!p || p->group == 0) return 0.0;
    return 2.0 * p->output_channels * p->input_channels * p->output_h * p->output_w * p->kernel_h * p->kernel_w / p->group;
}

int fhip_conv_select_algo(const fhip_conv_param* p, int* algo)
{
    if (!p || !algo) return fail(FHIP_E_BADARG, "null argument");
    if (p->group == p->input_channels)
        *algo = FHIP_DEPTHWISE;
    else if (p->group == 1 && p->kernel_h == 3 && p->kernel_w == 3 && p->stride_h == 1 && p->stride_w == 1 && p->input_h > 8 &&
             p->input_w > 8 && p->output_channels % 4 == 0 && p->input_channels % 4 == 0)
        *algo = FHIP_WINOGRADF63;
    else if (p->group == 1)
        *algo = FHIP_IM2COL;
    else
    {
        *algo = -1;
        return fail(FHIP_E_UNSUPPORTED, "Partial group conv is not supported (same as the reference, avx/booster.cpp:304-308)");
    }
    return FHIP_OK;
}

int fhip_winograd_f63_plan(const fhip_conv_param* p, int batch, fhip_winograd_plan* plan)
{
    if (!valid_param(p) || !plan) return fail(FHIP_E_BADARG, "bad param");
    return winograd_plan(*p, batch, plan);
}

int fhip_conv_get_buffer_size(const fhip_conv_param* p, int algo, int batch, size_t* buffer_bytes, size_t* packed_bytes)
{
    if (!valid_param(p) || !buffer_bytes || !packed_bytes || batch < 1) return fail(FHIP_E_BADARG, "bad argument");
    switch (algo)
    {
        case FHIP_NAIVE:
        case FHIP_IM2COL:
        {
            if (p->group > 1) return fail(FHIP_E_UNSUPPORTED, "implicit GEMM handles group == 1 only");
            if (const int rc = igemm_check_columns(*p, batch)) return rc; // what igemm_forward refuses
            *buffer_bytes = igemm_buffer_bytes(*p, batch); // no column matrix; split-K partial sums for under-filled grids only
            *packed_bytes = igemm_packed_floats(*p) * sizeof(float);
            return FHIP_OK;
        }
        case FHIP_DEPTHWISE:
            if ((long long)batch * p->input_channels > 0x7fffffffLL) return fail(FHIP_E_BADARG, "N*C too large: 2^31 planes or more"); // as depthwise_forward
            *buffer_bytes = 0; // no padded copy
            *packed_bytes = depthwise_packed_floats(*p, nullptr) * sizeof(float);
            return FHIP_OK;
        case FHIP_WINOGRADF63:
        {
            fhip_winograd_plan pl;
            int rc = winograd_plan(*p, batch, &pl);
            if (rc) return rc;
            *buffer_bytes = pl.v_bytes + pl.m_bytes; // V | M
            *packed_bytes = pl.u_bytes;
            return FHIP_OK;
        }
        default: return fail(FHIP_E_UNSUPPORTED, "This algo is not supported on gfx950 (nor on AVX2, avx/booster.cpp:348-354)");
    }
}

int fhip_conv_packed_layout(const fhip_conv_param* p, int algo, int* layout)
{
    if (!valid_param(p) || !layout) return fail(FHIP_E_BADARG, "bad argument");
    switch (algo)
    {
        case FHIP_NAIVE:
        case FHIP_IM2COL: *layout = igemm_packed_layout(*p); return FHIP_OK; // which weight images follow the panels
        case FHIP_DEPTHWISE: *layout = 0; return FHIP_OK;                      // the filters and their 12-float copies: no plane in it
        case FHIP_WINOGRADF63:
        {
            fhip_winograd_plan pl;
            const int rc = winograd_plan(*p, 1, &pl);
            if (rc) return rc;
            *layout = pl.frequency_points; // U of F(6,3) or of F(4,3)
            return FHIP_OK;
        }
        default: return fail(FHIP_E_UNSUPPORTED, "This algo is not supported on gfx950");
    }
}

int fhip_conv_init(const fhip_conv_param* p, int algo, float* packed, const float* kernel, void* stream)
{
    if (!valid_param(p) || !packed || !kernel) return fail(FHIP_E_BADARG, "bad argument");
    hipStream_t s = (hipStream_t)stream;
    switch (algo)
    {
        case FHIP_NAIVE:
        case FHIP_IM2COL: return igemm_init(*p, packed, kernel, s);
        case FHIP_DEPTHWISE: return depthwise_init(*p, packed, kernel, s);
        case FHIP_WINOGRADF63: return winograd_transform_kernel(*p, packed, kernel, s);
        default: return fail(FHIP_E_UNSUPPORTED, "This algo is not supported on gfx950");
    }
}

static int conv_forward_impl(const fhip_conv_param* p, int algo, int batch, float* output, const float* input, const float* packed,
                             float* buffer, const float* bias, void* stream, int pool, const float* residual = nullptr)
{
    if (!valid_param(p) || !output || !input || !packed || batch < 1) return fail(FHIP_E_BADARG, "bad argument");
    hipStream_t s = (hipStream_t)stream;
    if (pool && (algo != FHIP_WINOGRADF63 || !winograd_can_pool(*p)))
        return fail(FHIP_E_UNSUPPORTED, "fused max pooling is available on the Winograd route with even output dims only");
    if (residual && algo != FHIP_IM2COL) return fail(FHIP_E_UNSUPPORTED, "the fused residual add is available on the IM2COL route only");
    switch (algo)
    {
        case FHIP_NAIVE: return igemm_forward(*p, batch, output, input, packed, bias, buffer, true, s);
        case FHIP_IM2COL: return igemm_forward(*p, batch, output, input, packed, bias, buffer, false, s, residual);
        case FHIP_DEPTHWISE: return depthwise_forward(*p, batch, output, input, packed, bias, s);
        case FHIP_WINOGRADF63:
        {
            if (!buffer) return fail(FHIP_E_BADARG, "Winograd needs the scratch buffer");
            // K2 -> K3 -> K4 back to back on the caller's stream; V and M live in the caller's scratch arena (winograd_plan)
            fhip_winograd_plan pl;
            int rc = winograd_plan(*p, batch, &pl);
            if (rc) return rc;
            float* v = reinterpret_cast<float*>(reinterpret_cast<char*>(buffer) + pl.v_offset_bytes);
            float* m = reinterpret_cast<float*>(reinterpret_cast<char*>(buffer) + pl.m_offset_bytes);
            if ((rc = winograd_input_transform(*p, batch, v, input, s))) return rc;
            if ((rc = winograd_tile_gemm(*p, batch, m, packed, v, s))) return rc;
            return winograd_output_transform(*p, batch, output, m, bias, s, pool);
        }
        default: return fail(FHIP_E_UNSUPPORTED, "This algo is not supported on gfx950");
    }
}

int fhip_conv_forward(const fhip_conv_param* p, int algo, int batch, float* output, const float* input, const float* packed,
                      float* buffer, const float* bias, void* stream)
{
    return conv_forward_impl(p, algo, batch, output, input, packed, buffer, bias, stream, 0);
}

int fhip_conv_forward_maxpool2(const fhip_conv_param* p, int algo, int batch, float* pooled_output, const float* input, const float* packed,
                               float* buffer, const float* bias, void* stream)
{
    return conv_forward_impl(p, algo, batch, pooled_output, input, packed, buffer, bias, stream, 1);
}

int fhip_conv_forward_residual(const fhip_conv_param* p, int algo, int batch, float* output, const float* input, const float* packed,
                               float* buffer, const float* bias, const float* residual, void* stream)
{
    if (!residual) return fail(FHIP_E_BADARG, "null residual");
    return conv_forward_impl(p, algo, batch, output, input, packed, buffer, bias, stream, 0, residual);
}

int fhip_conv_streams_1x1(const fhip_conv_param* p, int algo, int batch)
{
    return valid_param(p) && (algo == FHIP_IM2COL || algo == FHIP_NAIVE) && batch >= 1 && igemm_streams(*p, batch) ? 1 : 0;
}

int fhip_conv_can_fuse_residual(const fhip_conv_param* p, int algo) { return valid_param(p) && algo == FHIP_IM2COL ? 1 : 0; }

int fhip_conv_can_fuse_maxpool2(const fhip_conv_param* p, int algo)
{
    return valid_param(p) && algo == FHIP_WINOGRADF63 && winograd_can_pool(*p) ? 1 : 0;
}

int fhip_conv_can_fuse_dw_pw(const fhip_conv_param* dw, const fhip_conv_param* pw, int batch)
{
    return valid_param(dw) && valid_param(pw) && dwpw_applicable(*dw, *pw, batch) ? 1 : 0;
}

int fhip_conv_forward_dw_pw(const fhip_conv_param* dw, const fhip_conv_param* pw, int batch, float* output, const float* input,
                            const float* dw_packed, const float* dw_bias, const float* pw_packed, const float* pw_bias, void* stream)
{
    if (!valid_param(dw) || !valid_param(pw) || !output || !input || !dw_packed || !pw_packed || batch < 1) return fail(FHIP_E_BADARG, "bad argument");
    return dwpw_forward(*dw, *pw, batch, output, input, dw_packed, dw_bias, pw_packed, pw_bias, (hipStream_t)stream);
}

int fhip_conv_can_fuse_siblings(const fhip_conv_param* a, int algo_a, const fhip_conv_param* b, int algo_b, int batch)
{
    return valid_param(a) && valid_param(b) && algo_a == FHIP_IM2COL && algo_b == FHIP_IM2COL && igemm_twin_applicable(*a, *b, batch) ? 1 : 0;
}

int fhip_conv_siblings_geometry(const fhip_conv_param* a, const fhip_conv_param* b, fhip_conv_param* both)
{
    if (!valid_param(a) || !valid_param(b) || !both) return fail(FHIP_E_BADARG, "bad argument");
    *both = igemm_twin_geometry(*a, *b);
    return FHIP_OK;
}

int fhip_conv_forward_siblings(const fhip_conv_param* a, const fhip_conv_param* b, int batch, float* output_a, float* output_b, const float* input,
                               const float* packed_both, const float* bias_both, void* stream)
{
    if (!valid_param(a) || !valid_param(b) || !output_a || !output_b || !input || !packed_both || batch < 1) return fail(FHIP_E_BADARG, "bad argument");
    return igemm_twin_forward(*a, *b, batch, output_a, output_b, input, packed_both, bias_both, (hipStream_t)stream);
}

int fhip_conv_can_chain_winograd(const fhip_conv_param* p, int algo, const fhip_conv_param* next, int next_algo, int pool)
{
    return valid_param(p) && valid_param(next) && algo == FHIP_WINOGRADF63 && next_algo == FHIP_WINOGRADF63 && winograd_can_chain(*p, *next, pool) ? 1 : 0;
}

int fhip_conv_forward_chained(const fhip_conv_param* p, int batch, float* output, const float* input, const float* packed, float* v, float* m,
                              const float* bias, const fhip_conv_param* next, float* v_next, int pool, void* stream)
{
    if (!valid_param(p) || !packed || !v || !m || batch < 1) return fail(FHIP_E_BADARG, "bad argument");
    if (next ? (!valid_param(next) || !v_next) : !output) return fail(FHIP_E_BADARG, "a chained layer needs `next` and `v_next`, the last one `output`");
    hipStream_t s = (hipStream_t)stream;
    int rc;
    if (input && (rc = winograd_input_transform(*p, batch, v, input, s))) return rc; // else V was written by the layer before
    if ((rc = winograd_tile_gemm(*p, batch, m, packed, v, s))) return rc;
    if (next) return winograd_output_to_next_input(*p, *next, batch, v_next, m, bias, s, pool);
    if (pool && !winograd_can_pool(*p)) return fail(FHIP_E_UNSUPPORTED, "fused max pooling needs even output dims");
    return winograd_output_transform(*p, batch, output, m, bias, s, pool);
}

// 2x2 image canvases (feather_canvas.h): the layer as ONE pad-1 image of 2H + 2 pixels per side, four images of a channel with a two-pixel
// zero seam between them.  14- and 56-pixel planes (square, even, the canvas whole tiles: (2H + 2) % 6 == 0, within a block's LDS with a
// lane per tile), batches that are a multiple of 4, layers the F(6,3) transforms take.
#ifndef FHIP_CANVAS_PLANES
#define FHIP_CANVAS_PLANES 3
#endif
static bool winograd_canvas_param(const fhip_conv_param& p, int batch, fhip_conv_param* canvas)
{
    if (p.kernel_h != 3 || p.kernel_w != 3 || p.stride_h > 1 || p.stride_w > 1 || p.group > 1) return false;
    if (p.pad_left != 1 || p.pad_right != 1 || p.pad_top != 1 || p.pad_bottom != 1) return false;
    const int h = p.input_h;
    if (batch < 4 || (batch & 3) || h != p.input_w || h < 2 || (h & 1) || (2 * h + 2) % 6 != 0) return false;
    // The rule is on for the two plane sizes it was measured on: other sides with (2H + 2) % 6 == 0 (26, 38, 50) would leave
    // through boundaries (26 -> pool -> 13) nobody has measured or tested.  FHIP_CANVAS_PLANES (build-time, per-stage A/B runs) is a mask:
    // bit 0 = 14-pixel planes, bit 1 = 56-pixel planes.
    if (!((h == 14 && (FHIP_CANVAS_PLANES & 1)) || (h == 56 && (FHIP_CANVAS_PLANES & 2)))) return false;
    const int side = 2 * h + 2, tiles = side / 6;
    if (tiles * tiles > 512 || (size_t)(side + 2) * (side + 4) * sizeof(float) > 64 * 1024) return false;
    fhip_conv_param q = p;
    q.input_h = q.input_w = q.output_h = q.output_w = side;
    fhip_winograd_plan own;
    if (winograd_plan(p, batch, &own) != FHIP_OK || own.frequency_points != 64) return false; // planes the F(4x4,3x3) route takes stay plain
    if (canvas) *canvas = q;
    return true;
}

int fhip_winograd_f63_canvas_param(const fhip_conv_param* p, int batch, fhip_conv_param* canvas)
{
    if (!valid_param(p) || !canvas) return fail(FHIP_E_BADARG, "bad argument");
    if (!winograd_canvas_param(*p, batch, canvas)) return fail(FHIP_E_UNSUPPORTED, "this layer and batch do not run on 2x2 image canvases");
    return FHIP_OK;
}

int fhip_winograd_f63_plan_canvas(const fhip_conv_param* p, int batch, int canvas, fhip_winograd_plan* plan)
{
    if (!valid_param(p) || !plan || (canvas != 1 && canvas != 2)) return fail(FHIP_E_BADARG, "bad argument");
    if (canvas == 1) return winograd_plan(*p, batch, plan);
    fhip_conv_param q;
    if (!winograd_canvas_param(*p, batch, &q)) return fail(FHIP_E_UNSUPPORTED, "this layer and batch do not run on 2x2 image canvases");
    return winograd_plan(q, batch / 4, plan);
}

int fhip_winograd_f63_output_to_next_input(const fhip_conv_param* p, const fhip_conv_param* next, int batch, float* v_next, const float* m,
                                           const float* bias, int pool, void* stream)
{
    if (!valid_param(p) || !valid_param(next) || !v_next || !m || batch < 1) return fail(FHIP_E_BADARG, "bad argument");
    return winograd_output_to_next_input(*p, *next, batch, v_next, m, bias, (hipStream_t)stream, pool);
}

int fhip_conv_can_fuse_first_winograd(const fhip_conv_param* first, const fhip_conv_param* next, int next_algo, int batch)
{
    return valid_param(first) && valid_param(next) && next_algo == FHIP_WINOGRADF63 && winograd_can_fuse_first(*first, *next, batch) ? 1 : 0;
}

int fhip_winograd_f63_input_from_first(const fhip_conv_param* first, const fhip_conv_param* next, int batch, float* v_next, const float* input,
                                       const float* first_kernel, const float* first_bias, void* stream)
{
    if (!valid_param(first) || !valid_param(next) || !v_next || !input || !first_kernel || batch < 1) return fail(FHIP_E_BADARG, "bad argument");
    return winograd_input_from_first(*first, *next, batch, v_next, input, first_kernel, first_bias, (hipStream_t)stream);
}

int fhip_winograd_f63_transform_kernel(const fhip_conv_param* p, float* u, const float* kernel, void* stream)
{
    if (!valid_param(p) || !u || !kernel) return fail(FHIP_E_BADARG, "bad argument");
    return winograd_transform_kernel(*p, u, kernel, (hipStream_t)stream);
}

int fhip_winograd_f63_input_transform(const fhip_conv_param* p, int batch, float* v, const float* input, void* stream)
{
    if (!valid_param(p) || !v || !input) return fail(FHIP_E_BADARG, "bad argument");
    return winograd_input_transform(*p, batch, v, input, (hipStream_t)stream);
}

int fhip_winograd_f63_tile_gemm(const fhip_conv_param* p, int batch, float* m, const float* u, const float* v, void* stream)
{
    if (!valid_param(p) || !m || !u || !v) return fail(FHIP_E_BADARG, "bad argument");
    return winograd_tile_gemm(*p, batch, m, u, v, (hipStream_t)stream);
}

int fhip_winograd_f63_output_transform(const fhip_conv_param* p, int batch, float* output, const float* m, const float* bias,
                                       void* stream)
{
    if (!valid_param(p) || !output || !m) return fail(FHIP_E_BADARG, "bad argument");
    return winograd_output_transform(*p, batch, output, m, bias, (hipStream_t)stream);
}

int fhip_stage_timing_enable(int on)
{
    std::lock_guard<std::mutex> lk(g_tm_mu);
    g_tm_on = on != 0;
    return FHIP_OK;
}

int fhip_stage_timing_collect(double* ms, long long* launches)
{
    if (!ms || !launches) return fail(FHIP_E_BADARG, "null argument");
    std::lock_guard<std::mutex> lk(g_tm_mu);
    for (int i = 0; i < FHIP_STAGE_COUNT; ++i)
    {
        ms[i] = 0.0;
        launches[i] = 0;
    }
    int rc = FHIP_OK;
    for (auto& t : g_tm_pending)
    {
        float dt = 0.f;
        hipError_t e = hipEventSynchronize(t.b);
        if (e == hipSuccess) e = hipEventElapsedTime(&dt, t.a, t.b);
        if (e != hipSuccess)
            rc = fail_hip(e, "stage timing");
        else if (t.stage >= 0 && t.stage < FHIP_STAGE_COUNT)
        {
            ms[t.stage] += dt;
            launches[t.stage] += 1;
        }
        g_tm_pool.emplace_back(t.a, t.b);
    }
    g_tm_pending.clear();
    return rc;
}

const char* fhip_last_error(void) { return g_last_error.c_str(); }

const char* fhip_version(void) { return "feather_hip 0.1 (gfx950)"; }

int fhip_device_info(char* name, int name_len, int* cus, int* lds_bytes)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n < 1) return fail(FHIP_E_NODEVICE, "no HIP device");
    int dev = 0;
    FHIP_CHECK_HIP(hipGetDevice(&dev));
    hipDeviceProp_t prop;
    FHIP_CHECK_HIP(hipGetDeviceProperties(&prop, dev));
    if (name && name_len > 0)
    {
        snprintf(name, name_len, "%s (%s)", prop.name, prop.gcnArchName);
    }
    if (cus) *cus = prop.multiProcessorCount;
    if (lds_bytes) *lds_bytes = (int)prop.maxSharedMemoryPerMultiProcessor;
    return FHIP_OK;
}

// ---- calibration: what the fp32 matrix pipe sustains on THIS device, at the clock the chip really runs it at -------------------
namespace
{
typedef float cal_f32x16 __attribute__((ext_vector_type(16)));
__device__ unsigned long long g_cal_ticks[2]; // shader-clock ticks, 100 MHz wall-clock ticks (sampled blocks)

// Nothing but v_mfma_f32_32x32x2_f32: four independent accumulator chains per wave, 3 waves per SIMD (the residency of the product's
// GEMM kernels), operands in registers.  Whatever this kernel reaches is the ceiling every MFMA-bound kernel of the library lives under.
// The operands are eight random values per lane that rotate from MFMA to MFMA: dynamic power follows the toggling of the operand
// bits, constant operands run 10 % faster than anything a real GEMM can reach on this part.
__global__ __launch_bounds__(256) void mfma_calibration_kernel(float* sink, const float* noise, int steps)
{
    const long long c0 = clock64(), w0 = wall_clock64();
    cal_f32x16 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    float a[8], b[8];
#pragma unroll
    for (int u = 0; u < 8; ++u)
    {
        a[u] = noise[(threadIdx.x * 16 + u + blockIdx.x) & 4095];
        b[u] = noise[(threadIdx.x * 16 + 8 + u + 3 * blockIdx.x) & 4095];
    }
    for (int s = 0; s < steps; ++s)
    {
#pragma unroll
        for (int u = 0; u < 8; ++u)
        {
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u], b[u], acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[(u + 3) & 7], b[(u + 5) & 7], acc[1], 0, 0, 0);
            acc[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[(u + 1) & 7], b[(u + 2) & 7], acc[2], 0, 0, 0);
            acc[3] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[(u + 6) & 7], b[(u + 7) & 7], acc[3], 0, 0, 0);
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) asm volatile("" : "+v"(a[u]), "+v"(b[u]));
    }
    float sum = 0.f;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) sum += acc[t][r];
    if (sum == 123.456f) sink[0] = sum; // keeps the chains alive
    if (threadIdx.x == 0 && (blockIdx.x & 15) == 0)
    {
        atomicAdd(&g_cal_ticks[0], (unsigned long long)(clock64() - c0));
        atomicAdd(&g_cal_ticks[1], (unsigned long long)(wall_clock64() - w0));
    }
}
} // namespace

// the measurement proper; the caller owns (and always frees) the buffers and events
static int calibrate_mfma_f32_run(float* sink, float* noise, hipEvent_t e0, hipEvent_t e1, int blocks, int steps, hipStream_t s, double* tflops,
                                  double* shader_mhz)
{
    {
        std::vector<float> h(4096);
        unsigned x = 2463534242u;
        for (auto& v : h)
        {
            x ^= x << 13;
            x ^= x >> 17;
            x ^= x << 5;
            v = (float)(int)x * (1.0f / 2147483648.0f); // U(-1, 1): what the nets' activations and weights look like
        }
        FHIP_CHECK_HIP(hipMemcpyAsync(noise, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice, s));
        FHIP_CHECK_HIP(hipStreamSynchronize(s));
    }
    const unsigned long long zero[2] = {0, 0};
    double best_tf = 0, best_mhz = 0;
    for (int rep = 0; rep < 12; ++rep) // the first repetition warms up; the power manager takes a few ms to settle: best of the rest
    {
        FHIP_CHECK_HIP(hipMemcpyToSymbolAsync(HIP_SYMBOL(g_cal_ticks), zero, sizeof zero, 0, hipMemcpyHostToDevice, s));
        FHIP_CHECK_HIP(hipEventRecord(e0, s));
        hipLaunchKernelGGL(mfma_calibration_kernel, dim3(blocks), dim3(256), 0, s, sink, noise, steps);
        FHIP_CHECK_HIP(hipEventRecord(e1, s));
        FHIP_CHECK_HIP(hipEventSynchronize(e1));
        float ms = 0;
        FHIP_CHECK_HIP(hipEventElapsedTime(&ms, e0, e1));
        unsigned long long ticks[2] = {0, 0};
        FHIP_CHECK_HIP(hipMemcpyFromSymbol(ticks, HIP_SYMBOL(g_cal_ticks), sizeof ticks));
        const double flops = 2.0 * 32 * 32 * 2 * 32.0 * steps * 4.0 * blocks; // per MFMA x 32 MFMAs per step x waves
        const double tf = flops / (ms * 1e-3) / 1e12, mhz = ticks[1] ? (double)ticks[0] / (double)ticks[1] * 100.0 : 0.0;
        if (rep > 0 && tf > best_tf)
        {
            best_tf = tf;
            best_mhz = mhz;
        }
    }
    *tflops = best_tf;
    *shader_mhz = best_mhz;
    return FHIP_OK;
}

int fhip_calibrate_mfma_f32(double* tflops, double* shader_mhz, void* stream)
{
    if (!tflops || !shader_mhz) return fail(FHIP_E_BADARG, "null argument");
    int dev = 0;
    FHIP_CHECK_HIP(hipGetDevice(&dev));
    hipDeviceProp_t prop;
    FHIP_CHECK_HIP(hipGetDeviceProperties(&prop, dev));
    const int blocks = prop.multiProcessorCount * 3, steps = 256; // 3 blocks of 4 waves per CU, 8192 MFMAs per wave: ~0.8 ms
    float *sink = nullptr, *noise = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    int rc = FHIP_OK;
    // every resource is released on every path
    if (hipMalloc((void**)&sink, 4) != hipSuccess || hipMalloc((void**)&noise, 4096 * sizeof(float)) != hipSuccess || hipEventCreate(&e0) != hipSuccess ||
        hipEventCreate(&e1) != hipSuccess)
        rc = fail(FHIP_E_HIP, "fhip_calibrate_mfma_f32: could not allocate its buffers / events");
    else
        rc = calibrate_mfma_f32_run(sink, noise, e0, e1, blocks, steps, (hipStream_t)stream, tflops, shader_mhz);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (sink) (void)hipFree(sink);
    if (noise) (void)hipFree(noise);
    return rc;
}

} // extern "C"
