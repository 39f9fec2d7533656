/* feather_net.h -- C-ABI of the layers between the convolutions and of the feather::Net-compatible
 * runtime on device blobs (the callers and data formats either side of the
 * ConvBooster hot path).  Same conventions as feather_hip.h: plain C, DEVICE pointers (fp32 NCHW dense),
 * `stream` is a hipStream_t as void*, every call returns 0 or a negative fhip_error.
 *
 * Paths cited are relative to /root/reference/src.
 */
#ifndef FEATHER_NET_H_
#define FEATHER_NET_H_

#include "feather_hip/feather_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- layer kernels ---------------------------------------------------------------------------------- */

/* ReluLayer::Forward, layers/relu_layer.h:29-41: y = x > 0 ? x : 0 over `count` floats. */
/* Size limit (fhip_relu, fhip_add): FHIP_E_BADARG at 2^31 blocks of 256 lanes or more -- a lane per float4 on 16-byte aligned pointers, per
 * float otherwise: about 2^39 floats.  Indices are 64-bit below that. */
FHIP_API int fhip_relu(float* y, const float* x, size_t count, void* stream);

/* EltwiseLayer::Forward (SUM only) -> booster::add_relu<fuse_relu>, layers/eltwise_layer.h:69-80,
 * booster/avx/generic_kernels.cpp:138: y = a + b, then max(0, .) when relu != 0. */
FHIP_API int fhip_add(float* y, const float* a, const float* b, size_t count, int relu, void* stream);

/* booster::scale<bias> (generic_kernels.cpp:203-233) and booster::batchnorm<bias,scale,relu>
 * (generic_kernels.cpp:237-279) are both per-channel affine maps: y[n][c][i] = x[n][c][i]*mul[c] + add[c],
 * optionally followed by ReLU.  mul/add are device vectors of `channels` floats; add may be NULL. */
/* Size limit: FHIP_E_BADARG at 2^31 blocks of 256 lanes or more (a lane per float4 when hw % 4 == 0 and y, x are 16-byte aligned, else per float). */
FHIP_API int fhip_affine(float* y, const float* x, const float* mul, const float* add, int batch, int channels, int hw,
                         int relu, void* stream);

/* ---- uint8 images to the input tensor --------------------------------------------------------------- */

/* Pixel types: ncnn's Mat::PIXEL_* codes with the same values (reference src/ncnn/mat.h:125-146).  A plain format is read as it is
 * (RGB and BGR in source order, no swap); FROM | (TO << 16) converts.  Gray is (r*77 + g*150 + b*29) >> 8 in integer arithmetic. */
enum
{
    FHIP_PIXEL_CONVERT_SHIFT = 16,
    FHIP_PIXEL_RGB = 1,
    FHIP_PIXEL_BGR = (1 << 1),
    FHIP_PIXEL_GRAY = (1 << 2),
    FHIP_PIXEL_RGBA = (1 << 3),
    FHIP_PIXEL_RGB2BGR = FHIP_PIXEL_RGB | (FHIP_PIXEL_BGR << FHIP_PIXEL_CONVERT_SHIFT),
    FHIP_PIXEL_RGB2GRAY = FHIP_PIXEL_RGB | (FHIP_PIXEL_GRAY << FHIP_PIXEL_CONVERT_SHIFT),
    FHIP_PIXEL_BGR2RGB = FHIP_PIXEL_BGR | (FHIP_PIXEL_RGB << FHIP_PIXEL_CONVERT_SHIFT),
    FHIP_PIXEL_BGR2GRAY = FHIP_PIXEL_BGR | (FHIP_PIXEL_GRAY << FHIP_PIXEL_CONVERT_SHIFT),
    FHIP_PIXEL_GRAY2RGB = FHIP_PIXEL_GRAY | (FHIP_PIXEL_RGB << FHIP_PIXEL_CONVERT_SHIFT),
    FHIP_PIXEL_GRAY2BGR = FHIP_PIXEL_GRAY | (FHIP_PIXEL_BGR << FHIP_PIXEL_CONVERT_SHIFT),
    FHIP_PIXEL_RGBA2RGB = FHIP_PIXEL_RGBA | (FHIP_PIXEL_RGB << FHIP_PIXEL_CONVERT_SHIFT),
    FHIP_PIXEL_RGBA2BGR = FHIP_PIXEL_RGBA | (FHIP_PIXEL_BGR << FHIP_PIXEL_CONVERT_SHIFT),
    FHIP_PIXEL_RGBA2GRAY = FHIP_PIXEL_RGBA | (FHIP_PIXEL_GRAY << FHIP_PIXEL_CONVERT_SHIFT)
};

/* ncnn's Mat::from_pixels_resize (reference src/ncnn/mat_pixel.cpp:1369-1410) + substract_mean_normalize for a batch, on the device.
 *   pixels: DEVICE, `batch` images of h rows x w pixels of the type's source channels, dense ([N][h][w][cin] bytes, any byte offset);
 *   output: DEVICE, [N][cout][target_h][target_w] fp32 (cout = 3, 1 or 4 as from_pixels gives them), 4-byte aligned.
 * When the size changes, each image is resized first, in its source format, with ncnn's fixed-point bilinear resize
 * (mat_pixel_resize.cpp resize_bilinear_c1 / c3 / c4), and the conversion runs on the resized bytes; the output is bit-identical to the
 * reference's.  One deliberate difference: a source 1 pixel wide or high that must be resized is refused (FHIP_E_BADARG) -- the reference
 * reads column / row -1 there.
 *   mean / norm: HOST arrays of cout floats, or NULL (upstream ncnn's substract_mean_normalize, compiled out of the reference build):
 *     mean only: x - mean; norm only: x * norm; both: x * norm + (-(mean * norm)), rounded after the product and after the sum (no FMA).
 * Asynchronous on `stream` and stream-capturable: no allocation, no copy, everything the kernel needs is passed by value.  One launch. */
/* Size limit: FHIP_E_BADARG at 2^31 blocks of 256 lanes or more (a lane per output float4 when target_w % 4 == 0 and output is 16-byte aligned,
 * else per float). */
FHIP_API int fhip_pixels_to_float(float* output, const unsigned char* pixels, int batch, int type, int w, int h, int target_w, int target_h,
                                  const float* mean, const float* norm, void* stream);

/* NV21 (yuv420sp) camera frames to the fp32 input tensor, on the device: one of the two chains the reference offers, bit-identical to it.
 *   yuv: DEVICE, `batch` frames of w x h, dense: each frame is w*h Y bytes, then (w/2)*(h/2) interleaved V,U pairs (w*h*3/2 bytes per
 *     frame, any byte offset);
 *   output: DEVICE, [N][cout][target_h][target_w] fp32, 4-byte aligned; cout = 3 (PIXEL_RGB, PIXEL_RGB2BGR) or 1 (PIXEL_RGB2GRAY).
 *   resize_first = 1: resize_bilinear_yuv420sp (mat_pixel_resize.cpp:1174-1189: Y as c1, VU as c2 at half size), then yuv420sp2rgb at the
 *     target size, then Mat::from_pixels(rgb, type);
 *   resize_first = 0: yuv420sp2rgb at the source size, then Mat::from_pixels_resize(rgb, type, w, h, target_w, target_h) (resize in RGB).
 * yuv420sp2rgb is the reference's C path (mat_pixel.cpp:1266-1320).  mean / norm as in fhip_pixels_to_float.  FHIP_E_BADARG, before any
 * device call, for a type other than PIXEL_RGB / RGB2BGR / RGB2GRAY, an odd w or h (the reference asserts against it), and with
 * resize_first an odd target size or a frame narrower or lower than 4 pixels -- deliberate differences: the reference resizes the 1-pair
 * VU plane of such a frame by reading index -1, even at equal size.  Asynchronous on `stream`, stream-capturable, one launch. */
FHIP_API int fhip_yuv420sp_to_float(float* output, const unsigned char* yuv, int batch, int type, int w, int h, int target_w, int target_h,
                                    int resize_first, const float* mean, const float* norm, void* stream);

/* One image of a mixed-size batch: `data` points at pixel (0, 0), rows of w pixels of the type's source channels are `stride` bytes apart
 * (0: w * cin, dense), and the region (roi_x, roi_y, roi_w, roi_h) is what gets resized (roi_w = roi_h = 0: the whole image).  The ROI
 * lies inside the image.  Only the ROI's bytes are read. */
typedef struct fhip_pixel_image
{
    const unsigned char* data;
    int w, h, stride;
    int roi_x, roi_y, roi_w, roi_h;
} fhip_pixel_image;

/* The plan of fhip_pixels_to_float_images: every descriptor checked on the host (FHIP_E_BADARG, the image index in fhip_last_error: null
 * data, w or h < 1, a stride below w * cin, a ROI not inside the image, a ROI axis of 1 pixel that must be resized; an unknown type, a
 * batch or target < 1), then written to `plan` as an opaque header (batch, type, target) plus one entry per image (the ROI's first byte,
 * pitch, ROI size, resize flag and the reference's IEEE double scales).  plan = NULL: only *plan_bytes is set, to the size a plan takes;
 * otherwise *plan_bytes is plan's capacity on entry and the size written on return.  `plan` is 8-byte aligned.  Host only. */
/* Size limit: FHIP_E_BADARG for an image whose row (w * channels) is 2 GiB (2^31 bytes) or longer. */
FHIP_API int fhip_pixel_images_plan(const fhip_pixel_image* images, int batch, int type, int target_w, int target_h, void* plan,
                                    size_t* plan_bytes);
/* fhip_pixels_to_float for a planned batch: output image i, of [batch][cout][target_h][target_w] fp32 (4-byte aligned), is
 * Mat::from_pixels_resize of a dense copy of image i's ROI to the plan's target, then mean / norm as fhip_pixels_to_float applies them.
 * Batch, type, target and the launch shape come from the HOST plan; the kernel reads `plan_device`, a DEVICE copy of the same bytes
 * (8-byte aligned) that must stay there until the conversion has run.  The plan's pointers are the descriptors' DEVICE pointers.
 * One launch; no allocation, no copy: stream-capturable (a replay reads the plan and the images as they are then).  FHIP_E_BADARG,
 * before any device call, for a host plan fhip_pixel_images_plan did not write. */
FHIP_API int fhip_pixels_to_float_images(float* output, const void* plan, const void* plan_device, const float* mean, const float* norm,
                                         void* stream);

/* Convolution (+bias, +ReLU as the param says) followed by a 2x2 / stride-2 / unpadded MAX pooling, fused: the pooled
 * tensor [N][K][OH/2][OW/2] is written straight from the Winograd output transform and the full-resolution activation
 * never reaches HBM (VGG: every pooling layer follows a 3x3 convolution).  Same arguments as fhip_conv_forward.  Only the
 * WINOGRADF63 route with even output dims can do it: fhip_conv_can_fuse_maxpool2 returns 1 when it can, and
 * fhip_conv_forward_maxpool2 returns FHIP_E_UNSUPPORTED otherwise (run fhip_conv_forward + fhip_pooling instead).
 * Equal to ConvLayer::Forward + PoolingLayer::Forward of the reference (conv_layer.h:141-150, pooling_layer.h:37-88). */
FHIP_API int fhip_conv_can_fuse_maxpool2(const fhip_conv_param* param, int algo);
FHIP_API int fhip_conv_forward_maxpool2(const fhip_conv_param* param, int algo, int batch, float* pooled_output, const float* input,
                                        const float* packed, float* buffer, const float* bias, void* stream);

/* Convolution followed by an Eltwise SUM with `residual` (same shape as the output) and the activation the param names:
 * output = act(conv(input) + bias + residual), the add done in the GEMM epilogue (ResNet's last 1x1 of a bottleneck +
 * shortcut + ReLU; reference: ConvLayer::Forward, EltwiseLayer::Forward -> booster::add_relu, eltwise_layer.h:69-80).  Same
 * arguments as fhip_conv_forward plus `residual`.  IM2COL route only (fhip_conv_can_fuse_residual), else FHIP_E_UNSUPPORTED. */
FHIP_API int fhip_conv_can_fuse_residual(const fhip_conv_param* param, int algo);
FHIP_API int fhip_conv_forward_residual(const fhip_conv_param* param, int algo, int batch, float* output, const float* input,
                                        const float* packed, float* buffer, const float* bias, const float* residual, void* stream);

/* A 3x3 depthwise convolution (+bias, +ReLU as `dw` says) followed by the 1x1 convolution that is its only consumer (+bias, +ReLU as
 * `pw` says), fused: output = act_pw(W_pw * act_dw(dw(input) + b_dw) + b_pw).  The pointwise GEMM computes its column operand from
 * the depthwise layer's INPUT on the fly, so the depthwise output -- a tensor as large as the pair's input -- never reaches HBM
 * (MobileNet-V1's first dw/pw pairs are HBM bound).  Equal to two ConvLayer::Forward calls of the reference (conv_layer.h:141-150
 * with DEPTHWISE_Forward, avx/booster.cpp:136-160, then IM2COL_Forward, :83-102).
 *   dw_packed / pw_packed: what fhip_conv_init produced for FHIP_DEPTHWISE / FHIP_IM2COL; no scratch buffer is needed.
 * fhip_conv_can_fuse_dw_pw returns 1 when the pair qualifies: depthwise 3x3, stride 1 or 2, pad_left = pad_top = 1, input and
 * output widths multiples of 4 with output_w * stride == input_w, at most 256 channels; pointwise 1x1 stride 1 unpadded on exactly
 * the depthwise output, large enough not to run split-K at this batch, and with 64 < output_channels < 160 (stride 1) / 400 (stride 2)
 * -- the range in which one kernel beats two on this chip.  Otherwise fhip_conv_forward_dw_pw returns FHIP_E_UNSUPPORTED (run the two
 * layers one after the other). */
FHIP_API int fhip_conv_can_fuse_dw_pw(const fhip_conv_param* dw, const fhip_conv_param* pw, int batch);
/* Size limit: fhip_conv_can_fuse_dw_pw is 0 (and the call FHIP_E_UNSUPPORTED) beyond 0x7fffff00 GEMM columns (batch * Ho * Wo). */
FHIP_API int fhip_conv_forward_dw_pw(const fhip_conv_param* dw, const fhip_conv_param* pw, int batch, float* output, const float* input,
                                     const float* dw_packed, const float* dw_bias, const float* pw_packed, const float* pw_bias, void* stream);

/* PoolingLayer, layers/pooling_layer.h:90-131 (fields as its LoadParam reads them). */
typedef struct fhip_pool_param
{
    int channels, input_h, input_w;
    int kernel_h, kernel_w;
    int stride_h, stride_w;
    int pad_left, pad_right, pad_top, pad_bottom;
    int pooling_type;   /* 0 = max, anything else = average (pooling_layer.h:75) */
    int global_pooling; /* kernel = whole image, output 1x1 (pooling_layer.h:116-123) */
} fhip_pool_param;

/* PoolingLayer::Reshape, pooling_layer.h:116-131: ceil((in + pads - k) / stride) + 1, or 1x1 when global. */
FHIP_API int fhip_pooling_output_dim(const fhip_pool_param* p, int* out_h, int* out_w);
/* PoolingLayer::Forward, pooling_layer.h:37-88.  Reference semantics kept exactly: the window origin is
 * j*stride - pad_top - pad_bottom (both pads, :56,:67), windows are clipped to the image, the average
 * divides by the number of in-range taps, an empty window yields -FLT_MAX (max) or NaN (average). */
/* Size limits: FHIP_E_BADARG for more than 0x7fffff00 planes (batch * channels), and for an input plane (input_h * input_w) or an output plane of 2^31
 * elements or more (the kernels keep these in int); planes * H * W beyond 2^31 is supported. */
FHIP_API int fhip_pooling(const fhip_pool_param* p, int batch, float* y, const float* x, void* stream);

/* SoftmaxLayer::Forward, layers/softmax_layer.h:33-53: max-subtracted exp / sum over all
 * `count_per_image` values of each image. */
/* No size limit below int batch and int count_per_image: a block per row, 64-bit row offsets. */
FHIP_API int fhip_softmax(float* y, const float* x, int batch, int count_per_image, void* stream);

/* Consecutive Winograd layers without the activation between them.  When layer `p` (WINOGRADF63: 3x3, stride 1) is followed -- directly,
 * or behind a 2x2 / stride-2 max pooling when pool = 1 -- by a 3x3 / stride-1 / pad-1 WINOGRADF63 layer `next` that is its only consumer,
 * p's output transform can write next's TRANSFORMED INPUT V' (fhip_winograd_plan(next): [64][C'][P'_pad]) instead of the activation:
 * one kernel does Y = A^T m A, + bias, ReLU [, pooling] into LDS (one whole (image, channel) plane per block, zero border = next's
 * padding) and V' = B^T d B out of it, with the butterflies and the fp32 operation order of the two separate transforms, so V' is
 * bit-identical.  The activation -- one HBM write and one read per layer boundary -- never exists (VGG-16: 11 of its 12 boundaries
 * between 3x3 layers).  Equal to ConvLayer::Forward [+ PoolingLayer::Forward] of the reference followed by the input-transform step of
 * the next ConvLayer::Forward (conv_layer.h:141-150; sgemm/winograd split: avx/booster.cpp:163-217, winograd_kernels_F63.cpp:64-515).
 *   fhip_conv_can_chain_winograd: 1 when the pair qualifies (both WINOGRADF63, next 3x3/s1/p1 on exactly p's [pooled] output, the
 *     padded plane fits a block's LDS: up to 112x112 activations).
 *   fhip_conv_forward_chained runs ONE layer of such a run:  input != NULL -> first layer: transform `input` into `v` first;
 *     input == NULL -> `v` already holds this layer's V (the previous call wrote it as its v_next).  next != NULL -> write next's V into
 *     `v_next` (a different buffer than `v`; `output` is ignored); next == NULL -> last layer: write `output` (pooled when pool = 1,
 *     as fhip_conv_forward_maxpool2).  `v` / `m` / `v_next` are caller-owned scratch of fhip_winograd_plan's v_bytes / m_bytes.
 *   fhip_winograd_f63_output_to_next_input is the chained transform alone (stage-level tests and profiling). */
FHIP_API int fhip_conv_can_chain_winograd(const fhip_conv_param* param, int algo, const fhip_conv_param* next, int next_algo, int pool);
FHIP_API int fhip_conv_forward_chained(const fhip_conv_param* param, int batch, float* output, const float* input, const float* packed, float* v,
                                       float* m, const float* bias, const fhip_conv_param* next, float* v_next, int pool, void* stream);
/* Size limit: FHIP_E_BADARG at batch * output_channels of 2^31 planes or more (and what fhip_winograd_f63_plan refuses). */
FHIP_API int fhip_winograd_f63_output_to_next_input(const fhip_conv_param* param, const fhip_conv_param* next, int batch, float* v_next,
                                                    const float* m, const float* bias, int pool, void* stream);

/* Two 1x1 convolutions of the SAME input as one GEMM: ResNet's projection shortcut (res3a_branch1, 256 -> 512, stride 2) and the first
 * layer of the main branch beside it (res3a_branch2a, 256 -> 128, stride 2) read the same pixels of the same blob; in the reference they are
 * two ConvLayer::Forward calls (conv_layer.h:141-150; packed SGEMM avx/sgemm.cpp:377-433).  Here their filter matrices are stacked
 * ([Ka + Kb][C]) and one launch writes rows < Ka to `output_a` and the rest to `output_b`, each with its own activation: the short grid of
 * the main-branch layer (1 - 4 row tiles) rides in the long one of the shortcut instead of running the chip at 3 blocks per CU.
 *   fhip_conv_can_fuse_siblings: 1 when the pair qualifies at this batch (both IM2COL 1x1 / pad 0 / group 1 on the same input geometry and
 *     stride, Ka a multiple of 128, the combined grid needs no split-K and takes the LDS-tiled route).
 *   fhip_conv_siblings_geometry fills the geometry of the stacked layer: run fhip_conv_get_buffer_size / fhip_conv_init (algo IM2COL) on
 *     it with the stacked filters to get `packed_both`; `bias_both` = the two biases one after the other (zeros for a layer without one).
 *   fhip_conv_forward_siblings: the launch.  Results equal the two layers run on the LDS-tiled route (same tile, same k order). */
FHIP_API int fhip_conv_can_fuse_siblings(const fhip_conv_param* a, int algo_a, const fhip_conv_param* b, int algo_b, int batch);
FHIP_API int fhip_conv_siblings_geometry(const fhip_conv_param* a, const fhip_conv_param* b, fhip_conv_param* both);
/* Size limit: fhip_conv_can_fuse_siblings is 0 (and the call FHIP_E_UNSUPPORTED) beyond 0x7fffff00 GEMM columns (batch * Ho * Wo). */
FHIP_API int fhip_conv_forward_siblings(const fhip_conv_param* a, const fhip_conv_param* b, int batch, float* output_a, float* output_b,
                                        const float* input, const float* packed_both, const float* bias_both, void* stream);

/* A net's first convolution inside the Winograd layer behind it.  `first` is a 3x3 / stride-1 / pad-1 convolution with 2 .. 4 input
 * channels (VGG-16's conv1_1: ConvLayer::Forward through the im2col + SGEMM route, conv_layer.h:141-150, avx/booster.cpp:108-160) whose
 * only consumer `next` is a 3x3 / stride-1 / pad-1 WINOGRADF63 layer.  Its output is as large as the largest tensor of the net and holds
 * 27 multiply-adds per value, so next's input transform can compute every activation value of its 8x8 windows from the image instead
 * of loading it: V(next) = B^T act(first(image)) B with the consumer's zero padding outside the image; the first layer's output never
 * exists in memory.  `first_kernel` are first's filters as loaded ([K][C][3][3], device), `first_bias` its bias or NULL; the image
 * must be under 1 GiB and its width even.
 *   fhip_conv_can_fuse_first_winograd: 1 when the pair qualifies at this batch.
 *   fhip_winograd_f63_input_from_first writes next's V (fhip_winograd_plan(next).v_bytes); run the rest of `next` with
 *     fhip_conv_forward_chained(next, ..., input = NULL, v = that buffer, ...). */
/* Size limits: the pair qualifies while the input holds fewer than 2^30 bytes (4 * batch * c * h * w: 1783 images of 3 x 224 x 224) and the first
 * layer has at most 65535 output channels; beyond, the query is 0 and fhip_winograd_f63_input_from_first returns FHIP_E_UNSUPPORTED.  Where V of
 * `next` passes 2^31 bytes (batch 91 of 64 x 224 x 224) another form of the kernel runs: nothing for the caller to do. */
FHIP_API int fhip_conv_can_fuse_first_winograd(const fhip_conv_param* first, const fhip_conv_param* next, int next_algo, int batch);
FHIP_API int fhip_winograd_f63_input_from_first(const fhip_conv_param* first, const fhip_conv_param* next, int batch, float* v_next,
                                                const float* input, const float* first_kernel, const float* first_bias, void* stream);

/* ---- feather::Net on device blobs --------------------------------------------------------------------- */

/* Opaque handle to a feather::Net (include/feather/net.h; reference net.h:30-70). */
typedef struct fhip_net fhip_net;

FHIP_API int fhip_net_create(fhip_net** net);
FHIP_API int fhip_net_destroy(fhip_net* net);
/* All work of this net is enqueued on `stream` (default: the NULL stream).  Set before the first Forward. */
FHIP_API int fhip_net_set_stream(fhip_net* net, void* stream);
/* The stream this net's work is enqueued on as it stands (a hipStream_t as void*; NULL = the NULL stream): the one given to
 * fhip_net_set_stream, or the net's own after fhip_net_set_graph(1) without one.  Work that reads a blob of fhip_net_extract on this
 * stream is ordered after Forward (and after the gather of sub-batch replicas) with no synchronisation. */
FHIP_API int fhip_net_get_stream(fhip_net* net, void** stream);
/* Fusion level.  Set before the first Forward.
 *   0: none -- every layer of the file runs and every blob can be extracted, like the reference as shipped.
 *   1 (default): the TryFuse pass the reference declares but never calls (layer.cpp:82-101): Conv+ReLU, InnerProduct+ReLU,
 *      BatchNorm+Scale(+ReLU), Scale+ReLU, Eltwise+ReLU.
 *   2: + BatchNorm / Scale folded into the convolution before them, Conv + 2x2 max pooling, Conv + Eltwise SUM (+ReLU), a 3x3
 *      depthwise layer + the 1x1 convolution behind it as one layer (fhip_conv_forward_dw_pw where the pair qualifies), and two 1x1
 *      convolutions of the same input that follow each other as one GEMM (fhip_conv_forward_siblings; both blobs keep their storage);
 *      a squeeze-and-excitation block as one layer (FHIP_NET_ROUTE_GATE); Interp + Eltwise SUM (+ReLU) as one layer
 *      (FHIP_NET_ROUTE_RESAMPLE); LRN + the Pooling layer behind it as one layer (FHIP_NET_ROUTE_LRN).
 *   3: + runs of Winograd layers chained (fhip_conv_forward_chained): the blob between two chained layers has a shape but no storage;
 *      a first layer (3x3 / stride 1 / pad 1, 2 .. 4 input channels) in front of a Winograd layer is computed inside that layer's input
 *      transform (fhip_winograd_f63_input_from_first): its top has no storage either.
 * A blob that a fusion removed cannot be extracted (fhip_net_extract fails and says which level to use). */
FHIP_API int fhip_net_set_fusion(fhip_net* net, int on);
/* 1: convolutions choose their route with fhip_conv_select_algo_tuned (MI355X cost model) instead of the reference's
 * SelectAlgo rule; 0 (default): the reference rule. */
FHIP_API int fhip_net_set_tuned_selection(fhip_net* net, int on);
/* 1: a Convolution / ConvolutionDepthWise layer with dilation > 1 (ncnn params 2 / 12) is loaded and runs through libfeather_atrous.so
 * (feather_atrous.h, route code FHIP_NET_ROUTE_ATROUS); 0 (default): LoadParam refuses it with -200.  The default is a refusal only because
 * tests/test_net_cpu.py pins that answer for a default net; flip it when that test is next revised.  Its only effect is lifting that
 * refusal (a dilated Deconvolution stays refused).  Call before LoadParam; later it is FHIP_E_BADARG. */
FHIP_API int fhip_net_set_dilated(fhip_net* net, int on);
/* 1: the layer types Interp (nearest / bilinear resize; one bottom, or two where the second gives the output size) and HardSwish are loaded
 * and run through libfeather_resample.so (feather_resample.h has their definitions; route code FHIP_NET_ROUTE_RESAMPLE), and LRN through
 * libfeather_lrn.so (feather_lrn.h; FHIP_NET_ROUTE_LRN; an even or non-positive local_size, a region_type outside 0 / 1, alpha, beta or
 * bias not finite, bias <= 0 or alpha < 0 are -100 at LoadParam); 0 (default):
 * LoadParam refuses them with -200, as tests/test_inorm_cpu.py and tests/test_gate_cpu.py pin for a default net.  Its only effect is
 * lifting that refusal: PixelShuffle stays -200 and a bicubic Interp -100.  Call before LoadParam; later it is FHIP_E_BADARG.  Copied to
 * sub-batch replicas. */
FHIP_API int fhip_net_set_extended_layers(fhip_net* net, int on);
/* 1: the layers of ncnn's SSD detection head are loaded -- Permute, Flatten, Reshape, Normalize (the SSD form), PriorBox and DetectionOutput
 * -- and Concat takes any axis of its bottoms' rank and Softmax its axis (0=axis, 1=fixbug0), as feather_detect.h defines them; they run
 * through libfeather_detect.so and report the route FHIP_DETECT_NET_ROUTE (feather_detect.h).  A blob then has a rank (ncnn's Mat::dims): 3
 * unless one of these layers says otherwise.  The top of DetectionOutput is [n][1][keep_top_k][6], rows (label, score, xmin, ymin, xmax,
 * ymax) and zero rows past an image's count.  At fusion level 2 a Concat of Flatten of Permute order 3 heads is one launch, and a Concat of
 * PriorBox tops is evaluated when shapes change and launches nothing.  0 (default): LoadParam refuses the new types with -200, Concat
 * refuses every axis but channels and Softmax ignores its params, as before.  Its only effect is lifting those refusals: PixelShuffle and
 * Padding stay -200.  Call before LoadParam; later it is FHIP_E_BADARG.  Copied to sub-batch replicas. */
FHIP_API int fhip_net_set_detection(fhip_net* net, int on);
/* rows >= 1: the layers of ncnn's YOLO heads are loaded -- Reorg, YoloDetectionOutput (YOLOv2) and Yolov3DetectionOutput, as feather_yolo.h
 * defines them; they run through libfeather_yolo.so and report the route FHIP_YOLO_NET_ROUTE (feather_yolo.h).  The top of either detection
 * layer is [n][1][rows][6] of rank 2 -- rows (label + 1, score, xmin, ymin, xmax, ymax), the first `rows` survivors of the NMS, zero rows past
 * an image's count -- the shape Net::ExtractDetections reads.  Nothing fuses into these layers: every fusion level runs them as written.
 * 0 (default): LoadParam refuses the three types with -200.  Its only effect is lifting that refusal: PixelShuffle and Padding stay -200.
 * rows outside 0 .. FHIP_YOLO_MAX_ROWS (1024): FHIP_E_BADARG.  Call before LoadParam; later it is FHIP_E_BADARG.  Copied to sub-batch
 * replicas. */
FHIP_API int fhip_net_set_yolo(fhip_net* net, int rows);
/* 1: the layers of the second stage of ncnn's two-stage detectors (Faster R-CNN, R-FCN) are loaded -- Proposal, ROIPooling, ROIAlign and
 * PSROIPooling, as feather_roi.h defines them; they run through libfeather_roi.so and report the route FHIP_ROI_NET_ROUTE (feather_roi.h).
 * Proposal reads score [n][18][h][w], bbox [n][36][h][w] and im_info, a second Input fed with fhip_net_feed_input(name, n, 1, 1, 3, ...) --
 * (height, width, scale) per image -- and writes rois [n][R][1][4], R = after_nms_topN, rows past an image's count the sentinel
 * (0, 0, -1, -1), and optionally scores [n][R][1][1].  An ROI layer reads features [n][C][h][w] and rois [n][R][1][4] (a Proposal top or an
 * Input) and writes [n * R][channels][pooled_h][pooled_w], row i * R + r from image i: the layers behind it see a batch of n * R.  With
 * sub-batch replicas every Input is dealt out with the images and fhip_net_extract gathers the rows in image order.  Nothing fuses into
 * these layers.  0 (default): LoadParam refuses the four types with -200; on-then-off equals the default.  Call before LoadParam; later it
 * is FHIP_E_BADARG.  Copied to sub-batch replicas. */
FHIP_API int fhip_net_set_roi(fhip_net* net, int on);
/* 1: the layers that frame an image-to-image net are loaded -- ncnn's Padding (constant with a value or per-channel values, replicate,
 * reflect; channel pads), Crop (offsets and sizes, or a reference blob as second bottom) and PixelShuffle (both modes), as feather_frame.h
 * defines them; they run through libfeather_frame.so and report the route FHIP_FRAME_NET_ROUTE (feather_frame.h).  Padding's dynamic form
 * (a second bottom, -233 margins) and Crop by starts / ends / axes are refused with -100.  A layer that changes nothing (all margins 0, a
 * crop of the whole blob, an upscale factor of 1) shares its bottom's storage and launches nothing.  At fusion level >= 2 a Padding that
 * only zero-pads the plane in front of the one fp32 Convolution / ConvolutionDepthWise that reads it is folded into that convolution's pads
 * (fhip_net_layer_conv_param shows the sums; the Padding's top is no longer extractable), and PixelShuffle absorbs a ReLU behind it, bit for
 * bit.  0 (default): LoadParam refuses the three types with -200; on-then-off equals the default.  Call before LoadParam; later it is
 * FHIP_E_BADARG.  Copied to sub-batch replicas. */
FHIP_API int fhip_net_set_frame(fhip_net* net, int on);
/* 1: the layers of a Vision Transformer encoder are loaded -- ncnn's MemoryData (0=w 1=h 2=c and that many raw floats: a constant, replicated
 * to the batch of the net's first Input when the shapes are planned and written once, at Init), LayerNorm (0=affine_size 1=eps 2=affine; rows
 * of w floats, or planes of h * w on a blob of rank 3), GELU (0=fast_gelu), MultiHeadAttention (0=embed_dim 1=num_heads 2=weight_data_size
 * 3=kdim 4=vdim 5=attn_mask 6=scale; one bottom, q and k = v, or q, k and v, each a blob of rank 2 [T][E]) and the element-wise BinaryOp (0=op
 * 0 .. 5, 1=with_scalar 2=b; two bottoms of one shape, or one of them a single image), as feather_attn.h defines their kernels; they run
 * through libfeather_attn.so and report the route FHIP_ATTN_NET_ROUTE (feather_attn.h).  An InnerProduct whose bottom is a blob of rank 2
 * [T][F] with F its input size runs once per token and gives [T][num_output]; every GEMM of these layers is the main library's.  The
 * multiply of a blob by a [n][c][1][1] gate stays on FHIP_NET_ROUTE_GATE.  Refused with -100: an attention mask, kdim or vdim other than
 * embed_dim, weight_data_size other than embed_dim^2, embed_dim % num_heads != 0, an op code past 5, an affine_size that is neither w nor
 * h * w, tensors of 2^31 elements or more.  The blobs of these layers have ranks, which fhip_net_set_detection maintains: without it
 * LoadParam refuses the new types with -200 and says so (BinaryOp and InnerProduct stay what a default net loads).  At fusion level >= 2 a BinaryOp add whose top a Split hands to one LayerNorm (and to
 * other layers) runs with that LayerNorm in one launch, bit for bit.  0 (default): LoadParam refuses the new types with -200, BinaryOp and
 * InnerProduct are what they were; on-then-off equals the default.  Call before LoadParam; later it is FHIP_E_BADARG.  Copied to sub-batch
 * replicas. */
FHIP_API int fhip_net_set_transformer(fhip_net* net, int on);
/* 1: ncnn's recurrent layers are loaded -- LSTM (0=num_output 1=weight_data_size 2=direction 3=hidden_size), GRU and RNN (0=num_output
 * 1=weight_data_size 2=direction); weights weight_xc [nd][G * H][size], bias_c ([nd][4][H] for LSTM and GRU, [nd][H] for RNN) and weight_hc
 * [nd][G * H][H], each tagged, with nd = 2 for direction 2 and size = weight_data_size / nd / G / H -- as feather_rnn.h defines the
 * recurrence; they run through libfeather_rnn.so and report the route FHIP_RNN_NET_ROUTE (feather_rnn.h).  Bottom 0 is a blob of rank 2
 * [T][size]; the optional further bottoms are the initial hidden state [nd][H] (then the cell state, LSTM: 1 or 3 bottoms and tops; GRU and
 * RNN: 1 or 2); top 0 is [T][nd * H] of rank 2, the optional further tops the final states.  The input projections of all steps and both
 * directions are one GEMM of the main library into the net's arena; the recurrence reads them there.  Nothing fuses into these layers.
 * Refused with -100 at LoadParam, naming the layer and the param: num_output < 1, a direction outside 0 .. 2, a weight_data_size that is no
 * positive multiple of nd * G * H, an LSTM projection (3= other than num_output), 8= (int8) other than 0, other bottom or top counts, 2^31
 * elements or more; at Reshape: a bottom of another rank or width, a state blob of another shape or batch.  The blobs of these layers have
 * ranks, which fhip_net_set_detection maintains: without it LoadParam refuses the types with -200 and says so.  0 (default): LoadParam
 * refuses the three types with -200; on-then-off equals the default.  Call before LoadParam; later it is FHIP_E_BADARG.  Copied to
 * sub-batch replicas. */
FHIP_API int fhip_net_set_recurrent(fhip_net* net, int on);
/* 1: a Convolution, ConvolutionDepthWise or InnerProduct layer with int8 weights (ncnn param 8 = int8_scale_term 1 .. 100: int8-tagged
 * weights, then the bias, then the weight scales, then one input scale in the .bin) is loaded and runs through libfeather_qconv.so
 * (feather_qconv.h has the definition, bit for bit; route code FHIP_NET_ROUTE_QCONV), fp32 in and out; 0 (default): LoadParam refuses
 * param 8 with -200 and the weight reader refuses the int8 tag, as tests/loader_cases.py and the hostile-model tests pin for a default
 * net.  Its only effect is lifting those refusals for the layers the library runs: int8_scale_term > 100 (requantised int8 output), a
 * partial group, a dilation and automatic pads stay -200, and param 8 on weights with any other tag is refused when the weights are read
 * (this runtime does not quantise at load).  Call before LoadParam; later it is FHIP_E_BADARG.  Copied to sub-batch replicas. */
FHIP_API int fhip_net_set_quantized(fhip_net* net, int on);
/* 1, in a net with fhip_net_set_quantized: a Convolution or ConvolutionDepthWise layer with int8_scale_term 101 .. 200 (ncnn's
 * requantised int8 output, what ncnn2int8's fuse_requantize writes; one more raw fp32, the output scale, behind the input scale in the
 * .bin) is loaded, and its top is a q8 blob: int8 in device memory, as feather_q8.h defines it, bit for bit.  The layer and the int8
 * layers that read such a blob run through libfeather_q8.so and report FHIP_NET_ROUTE_QCONV like every int8 layer.  A q8 blob may be
 * read by an int8 Convolution / ConvolutionDepthWise, a Split, a plain ReLU and a max Pooling (the last two keep it q8); a BatchNorm /
 * Scale behind the producer exists only folded (fusion level 2) and is applied before the requantisation.  Every other reader -- average
 * Pooling, Eltwise, Concat, InnerProduct, an fp32 convolution, an unfused BatchNorm, a layer of another library -- is refused at the first
 * Forward with -300, and so is fhip_net_extract of the blob.  0 (default): such a layer is refused at LoadParam with -200 as before; without
 * fhip_net_set_quantized the switch changes nothing.  InnerProduct with int8_scale_term > 100 and a term above 200 stay refused.  Call
 * before LoadParam; later it is FHIP_E_BADARG.  Copied to sub-batch replicas. */
FHIP_API int fhip_net_set_requantized(fhip_net* net, int on);
/* 1: independent branches run concurrently: a convolution that needs no scratch arena and whose output is only consumed
 * further down the layer list (ResNet's projection shortcut, SqueezeNet's expand1x1) is enqueued on a second stream owned by
 * the net while the main stream continues; fork and join are events (hipGraph-capturable).  0 (default): one stream. */
FHIP_API int fhip_net_set_concurrency(fhip_net* net, int on);
/* How a chained Winograd layer (fusion level 3) with 64 input channels and a multiple of 64 output channels, followed by a plain chained layer,
 * runs its tile GEMM and its boundary: through libfeather_colpass.so (feather_colpass.h: the GEMM applies the output transform's column
 * pass and writes 48 planes of M instead of 64; every value behind it is bit-identical).  0: never.  1 (default): where the layer's M has
 * at least 150 MB, the size class in which these launches are HBM-bound (VGG-16 at batch 32: conv1_2 and conv2_1); a tree without the library
 * keeps the main route, silently.  2: wherever the library accepts the layer; a tree without it then fails at Reshape, like the canvas
 * library.  The route is decided again at every Reshape.  Other values: FHIP_E_BADARG.  Copied to sub-batch replicas. */
FHIP_API int fhip_net_set_colpass(fhip_net* net, int mode);
/* 1: after the first Forward for a shape, record the layer sequence into a hipGraph and replay it.  Capture is not
 * allowed on the NULL stream: if no stream was set, the net creates and uses its own non-blocking stream (order device
 * inputs produced on other streams yourself). */
FHIP_API int fhip_net_set_graph(fhip_net* net, int on);

/* Sub-batch replicas (default 1 = off).  With R > 1 the handle owns R complete copies of the net (weights, blobs, arena, graph), each on a
 * stream of its own: FeedInput deals the images of a batch out in R contiguous shares (the first ones take the remainder), Forward
 * runs the replicas concurrently -- forked off and joined back into the net's stream with events, so the caller's stream order is
 * unchanged -- and Extract puts the shares back together ([N][C][H][W], images in feed order).  Images are independent, so results
 * equal the single-net ones up to the batch-dependent reduction order of split-K layers (<= 1e-6 normalised).  What it buys: kernels of
 * different character overlap (MobileNet-V1 b256: HBM-bound depthwise layers of one share under the MFMA-bound 1x1 layers of the
 * other, +8 % images/s with R = 2) and the tails of small launches are filled; nets made of long uniform launches gain nothing
 * (VGG-16, ResNet-50: +-1 %).  Set once, before LoadParam.  Introspection calls describe replica 0; fhip_net_forward_timed refuses a net
 * with replicas (kernels of concurrent replicas share the chip, their durations are not layer times). */
FHIP_API int fhip_net_set_sub_batches(fhip_net* net, int replicas);

/* Net::LoadParam, net.cpp:54-170 (ncnn text .param: magic 7767517, "layers blobs", one line per layer). */
FHIP_API int fhip_net_load_param(fhip_net* net, const char* path);
FHIP_API int fhip_net_load_param_mem(fhip_net* net, const char* text, size_t len);
/* Net::LoadWeights, net.cpp:172-233 (ncnn .bin read in layer order; ncnn/modelbin.cpp:47-197). */
FHIP_API int fhip_net_load_weights(fhip_net* net, const char* path);
FHIP_API int fhip_net_load_weights_mem(fhip_net* net, const void* data, size_t len);
/* The same image in DEVICE memory of the current device: what `ncclBroadcast` of the .bin from rank 0 leaves on every rank
 * (the one collective of the multi-GPU path; tests/cpp/multi_gpu_main.cpp, INTEGRATION.md "multi-GPU from C++").
 * Staged through host memory once (weights stay on the host until Init folds BatchNorm / Scale into them); `device_data` stays the
 * caller's and may be freed on return. */
FHIP_API int fhip_net_load_weights_device(fhip_net* net, const void* device_data, size_t len);

/* Net::FeedInput, net.cpp:235-246, extended with a batch.  `data` holds n*c*h*w floats; `on_device` says
 * whether it is a device pointer (copied device-to-device on the net's stream) or a host pointer. */
FHIP_API int fhip_net_feed_input(fhip_net* net, const char* blob_name, int n, int c, int h, int w, const float* data,
                                 int on_device);
/* Net::FeedInput of `n` uint8 images: fhip_pixels_to_float (same type, sizes, mean, norm) straight into the input blob, which becomes
 * [n][cout][target_h][target_w] (reshaped, and the graph dropped, only when that shape changes).  Enqueued on the net's stream; with
 * sub-batch replicas each replica's share of the images is converted into its own blob, forked and joined like fhip_net_feed_input.
 * `on_device` = 0: `pixels` is host memory, uploaded once as uint8 into a staging buffer the net owns (no fp32 on the host); 1: device
 * memory, ordered on the net's stream.  FHIP_E_BADARG for a bad type or size, the error codes of fhip_net_feed_input otherwise. */
FHIP_API int fhip_net_feed_pixels(fhip_net* net, const char* blob_name, int n, const unsigned char* pixels, int type, int w, int h,
                                  int target_w, int target_h, const float* mean, const float* norm, int on_device);
/* fhip_net_feed_pixels for `n` NV21 frames: fhip_yuv420sp_to_float (same sizes, type, chain, mean, norm) straight into the input blob,
 * with the same reshape, stream, replica and staging behaviour; host frames are uploaded as w*h*3/2 bytes each. */
FHIP_API int fhip_net_feed_yuv420sp(fhip_net* net, const char* blob_name, int n, const unsigned char* yuv, int w, int h, int target_w,
                                    int target_h, int type, int resize_first, const float* mean, const float* norm, int on_device);
/* fhip_net_feed_pixels for `n` images of their own sizes, pitches and ROIs (fhip_pixel_image): fhip_pixels_to_float_images straight into
 * the input blob, [n][cout][target_h][target_w], with the same reshape, stream and graph behaviour; each sub-batch replica converts its
 * contiguous share of the images.  `on_device` = 0: each ROI's rows (from its first byte to its last, one copy per image) are uploaded
 * back to back into the net's staging buffer together with the plans (the images may be reused once the net's stream has passed the
 * feed); 1: the descriptors point at device memory and only the plans are uploaded. */
FHIP_API int fhip_net_feed_pixel_images(fhip_net* net, const char* blob_name, int n, const fhip_pixel_image* images, int type,
                                        int target_w, int target_h, const float* mean, const float* norm, int on_device);
/* Net::Forward, net.cpp:297-334: Reshape when the input shape changed, Init once, then every layer in file
 * order on the net's stream.  Asynchronous: returns after enqueueing. */
FHIP_API int fhip_net_forward(fhip_net* net);
/* Net::Extract(name, float**, n, c, h, w), net.cpp:263-279: DEVICE pointer into the net's blob + its shape.
 * The pointer stays valid until the next Reshape.  With sub-batch replicas the pointer is a per-name buffer the shares are gathered
 * into (on the net's stream); it is re-allocated only when that blob's total size grows, i.e. after a FeedInput with a larger shape. */
FHIP_API int fhip_net_extract(fhip_net* net, const char* blob_name, float** device_ptr, int* n, int* c, int* h, int* w);
/* Convenience: synchronise the stream and copy the blob to a host buffer of `capacity` floats. */
FHIP_API int fhip_net_extract_host(fhip_net* net, const char* blob_name, float* host, size_t capacity);

/* Introspection (after LoadParam / fusion). */
FHIP_API int fhip_net_layer_count(fhip_net* net);
/* Route code of a Convolution layer with 1 < group < input_channels: it runs through libfeather_gconv.so (feather_gconv.h), which
 * libfeather_hip.so opens from its own directory when a net holds such a layer (FHIP_E_UNSUPPORTED at the first Reshape if it is not
 * there).  None of the reference's ConvAlgo values; reported from LoadParam on. */
#define FHIP_NET_ROUTE_GCONV 100
/* Route code of a Deconvolution / DeconvolutionDepthWise layer: it runs through libfeather_deconv.so (feather_deconv.h), opened the same
 * way the first time a net holds such a layer.  It fuses a following ReLU and, at fusion level 2, BatchNorm / Scale; no other fusion
 * takes it.  Reported from LoadParam on. */
#define FHIP_NET_ROUTE_DECONV 101
/* Route code of an InstanceNorm layer: it runs through libfeather_inorm.so (feather_inorm.h), opened the same way the first time a net
 * holds such a layer, a PReLU / Sigmoid / TanH / Clip layer or a ReLU with a slope.  It absorbs a following ReLU (plain or leaky) from
 * fusion level 1 on; no other fusion takes it.  Reported from LoadParam on. */
#define FHIP_NET_ROUTE_INORM 102
/* Route code of a ShuffleChannel or Slice layer: one channel-map launch of libfeather_shuffle.so (feather_shuffle.h), opened the same way
 * the first time a net holds such a layer.  At fusion level 2 a run of Concat / ShuffleChannel / Slice layers that follow each other in
 * the layer list, linked by blobs with one consumer each, is one layer with this route (it keeps the type and name of the run's first
 * layer; the blobs between them cannot be extracted); no other fusion takes these layers.  Reported from LoadParam on. */
#define FHIP_NET_ROUTE_SHUFFLE 103
/* Route code of a Convolution layer with dilation > 1 in a net with fhip_net_set_dilated: it runs through libfeather_atrous.so
 * (feather_atrous.h), opened the same way the first time a net holds such a layer, whatever its group (a dilated layer with
 * 1 < group < C goes there, not to libfeather_gconv.so).  It fuses a following ReLU and, at fusion level 2, BatchNorm / Scale; no other
 * fusion takes it.  Reported from LoadParam on. */
#define FHIP_NET_ROUTE_ATROUS 104
/* Route code of the squeeze-and-excitation layers: a `BinaryOp 0=2` or a `Scale 0=-233` with two bottoms of shapes [n][c][h][w] and
 * [n][c][1][1] (the channel gate), Swish and HardSigmoid.  They run through libfeather_gate.so (feather_gate.h), opened the same way the
 * first time a net holds such a layer.  At fusion level 2 a whole block -- Split -> global average Pooling -> {InnerProduct | 1x1
 * Convolution} -> [ReLU | Swish] -> {InnerProduct | 1x1 Convolution} -> {Sigmoid | HardSigmoid} -> the multiply [-> Eltwise SUM [-> ReLU]],
 * linked by blobs with one consumer each -- is one layer with this route: squeeze, excite and apply, three launches.  It keeps the type
 * and name of the block's Pooling layer and stands where the block's last layer stood; the blobs between them cannot be extracted.  The
 * pass runs before the pairwise fusions, so the excite layers are matched as written.  Reported from LoadParam on. */
#define FHIP_NET_ROUTE_GATE 105
/* Route code of an Interp or HardSwish layer in a net with fhip_net_set_extended_layers: one launch of libfeather_resample.so
 * (feather_resample.h), opened the same way the first time a net holds such a layer.  At fusion level 2 an Interp whose top has a sole
 * consumer, a two-bottom Eltwise SUM, takes that sum over, and the plain ReLU behind it if that is the sum's sole consumer (FPN's
 * upsample-and-add): one layer of one launch that keeps the Interp's type and name, has the sum's other operand as its last bottom and
 * stands where the chain's last layer stood; the up-sampled tensor is never written and the blobs inside the chain cannot be extracted.
 * No other fusion takes these layers.  Reported from LoadParam on. */
#define FHIP_NET_ROUTE_RESAMPLE 106
/* Route code of an LRN layer in a net with fhip_net_set_extended_layers: one launch of libfeather_lrn.so (feather_lrn.h), opened the same
 * way the first time a net holds such a layer.  At fusion level 2 an LRN whose top has a sole consumer, a non-global Pooling layer with one
 * bottom and one top, takes that layer over (AlexNet's and GoogLeNet's norm -> pool): one layer that keeps the LRN's type and name and equals
 * the two layers bit for bit; the normalised tensor has no blob and cannot be extracted.  Up to 4 * 192 * 56 * 56 elements the layer is one launch
 * (fhip_lrn_pool_forward) and that tensor is never written; above, where the one launch measured slower than the two, and where the pooling
 * window covers the whole unpadded plane (fhip_pooling's plane-reduce route, whose order the one launch does not restate), it is
 * fhip_lrn_forward into the net's scratch arena and fhip_pooling from there.  A Pooling layer in front of an LRN is not fused.  No other fusion takes the layer.  Reported from LoadParam on. */
#define FHIP_NET_ROUTE_LRN 107
/* Route code of a Convolution, ConvolutionDepthWise or InnerProduct layer with int8 weights in a net with fhip_net_set_quantized: one
 * launch of libfeather_qconv.so (feather_qconv.h), opened the same way the first time a net holds such a layer.  It fuses a following
 * ReLU and, at fusion level 2, BatchNorm / Scale -- into the dequantisation scales and the bias, as feather_qconv.h defines it, never into
 * the int8 weights; no other fusion takes it.  Reported from LoadParam on. */
#define FHIP_NET_ROUTE_QCONV 108
/* type / name are copied (truncated) into caller buffers of `len` bytes; algo = fhip_conv_algo for
 * convolutions after the first Forward (FHIP_NET_ROUTE_GCONV for a grouped one), else -1. */
FHIP_API int fhip_net_layer_info(fhip_net* net, int index, char* type, char* name, int len, int* algo);
/* Geometry of a Convolution / ConvolutionDepthWise layer as it runs (after Reshape: output dims assigned, BatchNorm folded, ...) and
 * the batch of its input blob; FHIP_E_BADARG for any other layer type.  (bench.py prices each layer's kernel against its roofline
 * with ConvParam::GetFLOPS, booster.h:145-148.) */
FHIP_API int fhip_net_layer_conv_param(fhip_net* net, int index, fhip_conv_param* param, int* batch);
/* Fusion level 2 makes a 3x3 depthwise layer (<= 256 channels, stride 1 / 2, pad 1) and the 1x1 convolution behind it ONE layer: for
 * such a layer, fhip_net_layer_conv_param describes the depthwise half and this returns the pointwise half; *one_kernel = 1 when the
 * pair runs as one kernel at the current shape (fhip_conv_forward_dw_pw), 0 when it runs the two kernels one after the other.
 * FHIP_E_BADARG for every other layer. */
FHIP_API int fhip_net_layer_fused_pointwise(fhip_net* net, int index, fhip_conv_param* param, int* one_kernel);
/* Fusion level 3: *v_from_previous = 1 when this convolution's transformed input is written by the layer before it (it runs no input
 * transform), *writes_next_v = 1 when its output leaves as the next layer's transformed input (fhip_conv_forward_chained).  The value
 * is 2 for the pair "first layer computed inside the next layer's input transform" (fhip_winograd_f63_input_from_first): writes_next_v =
 * 2 on the first layer (it launches nothing), v_from_previous = 2 on the Winograd layer behind it. */
FHIP_API int fhip_net_layer_chain(fhip_net* net, int index, int* v_from_previous, int* writes_next_v);
/* Fusion level 3: *canvas = 1 when this chained Winograd layer runs on 2x2 image canvases (feather_canvas.h: four images of a channel as
 * one (2H + 2)-pixel image, fhip_winograd_f63_plan_canvas(.., 2) sizes its V and M), 0 otherwise.  VGG-16 at a batch that is a multiple
 * of 4: conv3_1 .. conv3_3 (56 pixels) and conv5_1 .. conv5_3 (14 pixels). */
FHIP_API int fhip_net_layer_canvas(fhip_net* net, int index, int* canvas);
/* Fusion level 3: *colpass = 1 when this chained Winograd layer runs its tile GEMM and its boundary through libfeather_colpass.so
 * (fhip_net_set_colpass; its M holds 48 column-passed planes), 0 otherwise.  VGG-16 at batch 32: conv1_2 and conv2_1. */
FHIP_API int fhip_net_layer_colpass(fhip_net* net, int index, int* colpass);
/* Fusion level 2: *state = 1 when this 1x1 convolution's launch also computes the NEXT layer of the list (a 1x1 convolution of the same
 * input: fhip_conv_forward_siblings), 2 when this layer is that next one (it launches nothing), 0 otherwise. */
FHIP_API int fhip_net_layer_sibling(fhip_net* net, int index, int* state);
/* Fusion level 2: *state = 1 when an Eltwise SUM behind this convolution was absorbed and its other operand is added in the GEMM epilogue
 * (fhip_conv_forward_residual: the operand is one more read of an output-sized tensor by this launch), 2 when it was absorbed but is added by a
 * launch of its own (fhip_add), 0 when the layer has no residual operand. */
FHIP_API int fhip_net_layer_residual(fhip_net* net, int index, int* state);
/* One eager forward with a pair of events around every layer; ms must hold layer_count entries. */
FHIP_API int fhip_net_forward_timed(fhip_net* net, float* ms);
/* Device bytes currently held: blobs, weights, scratch arena. */
FHIP_API int fhip_net_memory(fhip_net* net, size_t* blob_bytes, size_t* weight_bytes, size_t* arena_bytes);

#ifdef __cplusplus
}
#endif
#endif /* FEATHER_NET_H_ */
