/* feather_detect.h -- C-ABI of libfeather_detect.so: the layers of an SSD detection head on the MI355X (gfx950) -- Permute, Normalize,
 * a softmax along any axis, PriorBox and DetectionOutput -- as ncnn defines them, on fp32 blobs with a leading batch.
 *
 * The reference has none of these layers and ncnn's sources were not at hand: this text is the definition, written from what
 * priorbox.cpp, detectionoutput.cpp, permute.cpp, normalize.cpp and softmax.cpp do.  Where it had to decide something, it says "decided
 * here".  tests/detect_ref.py restates it line by line.
 *
 * Blobs and ranks.  ncnn's layers depend on a Mat's `dims`.  A blob of rank 3 (c, h, w) is [n][c][h][w], one of rank 2 (h, w) is
 * [n][1][h][w], one of rank 1 (w) is [n][1][1][w]; the batch index is outermost and every layer works per image.
 *
 * Permute        order_type 0 .. 5.  For a rank-3 input (w, h, c) the output's (w, h, c) are the input's
 *                   0: w h c (a copy)   1: h w c   2: w c h   3: c w h   4: h c w   5: c h w
 *                so order 3 turns [c][h][w] into [h][w][c] (NCHW -> NHWC).  A rank-2 input (w, h) takes 0 (copy) and 1 (h w: the transpose).
 *                Exact: values are moved, never computed.
 *
 * Normalize      the SSD form only (across_spatial = 0, across_channel = 1): per pixel, in fp32, every product and sum rounded on its own,
 *                   s = the sum over c of x[c] * x[c], ascending c, from 0.f;   a = 1.f / sqrtf(s + eps);   y[c] = (x[c] * a) * scale[c]
 *                with scale[0] for every channel when channel_shared.  sqrtf and the division are correctly rounded, so the result is pinned
 *                to the bit.  eps > 0 is required (decided here: with eps <= 0 an all-zero pixel divides by zero).
 *
 * Softmax        along the middle axis of [outer][len][inner]:  m = max over the axis;  e = expf(x - m);  y = e / (the sum of e, ascending,
 *                from 0.f).  expf is the device function; the result is compared at the bound of fhip_softmax's tests.
 *
 * PriorBox       a host function of shapes only.  For a feature map of h x w cells and an image of image_h x image_w pixels:
 *                   step_w = (float)image_w / w and step_h = (float)image_h / h unless given (> 0)
 *                   num_prior = num_min * (1 + num_ratios * (1 + flip)) + num_max      (num_max is 0 or num_min)
 *                   for each cell, rows outer:  cx = (j + offset) * step_w,  cy = (i + offset) * step_h;  for each min_size k:
 *                      the box (min, min);  if max sizes are given the box (sqrtf(min * max[k]), same);  per aspect ratio ar the box
 *                      (min * sqrtf(ar), min / sqrtf(ar)) and, with flip, the box (min / sqrtf(ar), min * sqrtf(ar))
 *                   a box (bw, bh) is  (cx - bw * 0.5f) / image_w, (cy - bh * 0.5f) / image_h, (cx + bw * 0.5f) / image_w, (cy + bh * 0.5f) / image_h
 *                   with clip every coordinate is min(max(v, 0.f), 1.f)
 *                The output is two rows of 4 * h * w * num_prior floats: the boxes, then the four variances repeated per box.  All in fp32,
 *                each operation rounded on its own; sqrtf is correctly rounded, so the host result is pinned to the bit.
 *
 * DetectionOutput  per image, from location [4 * P], confidence [P * num_class] (prior-major: the scores of prior p are consecutive) and the
 *                priorbox rows [2][4 * P] (one set for the batch, or one per image):
 *                1. the box of prior p, from its prior (x0, y0, x1, y1), variances v and location l, in fp32:
 *                      pw = x1 - x0;  ph = y1 - y0;  pcx = (x0 + x1) * 0.5f;  pcy = (y0 + y1) * 0.5f
 *                      cx = (v0 * l0) * pw + pcx;  cy = (v1 * l1) * ph + pcy;  bw = expf(v2 * l2) * pw;  bh = expf(v3 * l3) * ph
 *                      box = (cx - bw * 0.5f, cy - bh * 0.5f, cx + bw * 0.5f, cy + bh * 0.5f).   No clipping.
 *                2. per class 1 .. num_class - 1 (0 is the background): the candidates are the priors with score > confidence_threshold,
 *                   ordered by score descending, then prior index ascending; the first nms_top_k of them go through greedy NMS in that
 *                   order: a candidate is dropped when its IoU with a box already kept is > nms_threshold.
 *                      area = (x1 - x0) * (y1 - y0);  iw = min(ax1, bx1) - max(ax0, bx0), ih likewise;  inter = iw <= 0 || ih <= 0 ? 0 : iw * ih
 *                      iou = inter / (area_a + area_b - inter)      (0 / 0 compares false: such a pair suppresses nothing)
 *                3. all survivors of all classes, ordered by score descending, then class ascending, then prior ascending; the first
 *                   keep_top_k are the result.
 *                The tie rules (prior index, class) are decided here: they make the result a function of the input, which ncnn's unstable
 *                quicksort is not.  A NaN score is no candidate.
 *                The output is [n][keep_top_k][6], rows (label, score, xmin, ymin, xmax, ymax); rows past an image's count are all zero, and
 *                label 0 never occurs in a real row, so the count is the number of rows with label > 0.  This fixed height is the one
 *                deliberate difference from ncnn's Mat of as many rows as there are detections (decided here): it is what lets the layer run
 *                in a captured graph and in sub-batch replicas.
 *                Limits, refused with FHIP_E_BADARG and never truncated: 1 <= P <= FHIP_DETECT_MAX_PRIORS, 2 <= num_class <=
 *                FHIP_DETECT_MAX_CLASSES, 1 <= nms_top_k, keep_top_k <= FHIP_DETECT_MAX_TOP_K, n <= 65535, n * P * num_class < 2^31.  The number
 *                of candidates of a class has no limit: they are selected in chunks of FHIP_DETECT_CHUNK priors.
 *                Results do not depend on thread scheduling: where candidates are compacted with atomics, their order comes from sorting
 *                their keys (score, prior) afterwards, and the keys are distinct.
 *
 * No entry allocates, copies or synchronises: every device entry is hipGraph-capturable.  Pointers need 4-byte alignment only.  No layer is in
 * place.  The library is separate from libfeather_hip.so and needs nothing from it but the enums of feather_hip.h; it keeps its own
 * last-error slot. */
#ifndef FEATHER_HIP_FEATHER_DETECT_H_
#define FEATHER_HIP_FEATHER_DETECT_H_

#include <stddef.h>

#include "feather_hip/feather_hip.h"

#ifdef __cplusplus
extern "C"
{
#endif

#define FHIP_DETECT_API __attribute__((visibility("default")))

/* Route code fhip_net_layer_info reports for the layers of a net with fhip_net_set_detection (feather_net.h) that run through this
 * library or are views it defines: Permute, Flatten, Reshape, Normalize, PriorBox, DetectionOutput and that net's Concat and Softmax. */
#define FHIP_DETECT_NET_ROUTE 109

#define FHIP_DETECT_MAX_PRIORS (1 << 22)
#define FHIP_DETECT_MAX_CLASSES 256
#define FHIP_DETECT_MAX_TOP_K 1024
/* sources of one fhip_permute_concat_forward */
#define FHIP_PERMUTE_CONCAT_MAX 8
/* priors one pass of the selection kernel looks at */
#define FHIP_DETECT_CHUNK 1024

/* `what` of fhip_detect_route */
enum fhip_detect_op
{
    FHIP_DETECT_PERMUTE = 0,   /* a = order_type, b = dims, (c, h, w) */
    FHIP_DETECT_NORMALIZE = 1, /* (c, h, w); the pointers decide the 16-byte form */
    FHIP_DETECT_SOFTMAX = 2,
    FHIP_DETECT_SELECT = 3,    /* DetectionOutput's first launch */
    FHIP_DETECT_MERGE = 4,     /* DetectionOutput's second launch */
    FHIP_DETECT_PERMUTE_CONCAT = 5
};

/* The (c, h, w) of Permute's output for an input of rank `dims` (2 or 3; rank 2: c = 1).  FHIP_E_BADARG: order_type outside 0 .. 5, rank 2
 * with an order above 1, dims outside 2 / 3, a dimension < 1, c != 1 at rank 2, a NULL pointer. */
FHIP_DETECT_API int fhip_permute_output_dim(int order_type, int dims, int c, int h, int w, int* out_c, int* out_h, int* out_w);

/* out = Permute(in[n][c][h][w]): one launch on `stream` (a hipStream_t as void*).  FHIP_E_BADARG: what fhip_permute_output_dim refuses, n < 1,
 * 2^31 elements or more, NULL or unaligned (4 bytes) pointers, out overlapping in. */
FHIP_DETECT_API int fhip_permute_forward(int order_type, int dims, int n, int c, int h, int w, float* out, const float* in, void* stream);

/* Concat(axis 0) of Flatten of Permute(order 3) of `sources` (1 .. FHIP_PERMUTE_CONCAT_MAX) blobs in[i][n][c[i]][hw[i]], in one launch
 * ("fhip::permute_concat_kernel"): out[n][total], total = the sum of c[i] * hw[i], image by image the sources' NHWC forms one after the other;
 * every source is transposed through the LDS tile straight into its slice.  The sources travel as kernel arguments: nothing is uploaded.
 * Exact.  FHIP_E_BADARG: a count outside the range, a dimension < 1, n < 1, 2^31 elements or blocks or more, NULL or unaligned pointers, out
 * overlapping a source. */
FHIP_DETECT_API int fhip_permute_concat_forward(int sources, const int* c, const int* hw, int n, float* out, const float* const* in, void* stream);

/* out[n][c][h][w] = Normalize(in) as defined above; scale holds c floats, or one when channel_shared.  One launch.  FHIP_E_BADARG: a
 * dimension < 1, 2^31 elements or more, eps not finite or <= 0, NULL or unaligned pointers, out overlapping in. */
FHIP_DETECT_API int fhip_normalize_forward(int n, int c, int h, int w, int channel_shared, float eps, float* out, const float* in, const float* scale,
                                           void* stream);

/* out[outer][len][inner] = the softmax of `in` along the middle axis.  One launch.  FHIP_E_BADARG: an extent < 1, 2^31 elements or more, NULL or
 * unaligned pointers, out overlapping in. */
FHIP_DETECT_API int fhip_axis_softmax_forward(int outer, int len, int inner, float* out, const float* in, void* stream);

/* PriorBox on the HOST: needs no device and launches nothing.  variances: four floats.  step_w / step_h <= 0: image extent / feature extent.
 * *num_prior receives the boxes per cell (may be NULL); out receives 2 * 4 * h * w * num_prior floats and may be NULL to ask for
 * num_prior alone (capacity is then ignored).  FHIP_E_BADARG: h, w, image_w or image_h < 1, num_min < 1, num_max neither 0 nor num_min, a
 * negative count or a NULL array with a positive count, a size or ratio that is not finite and > 0, a variance, offset or step that is not
 * finite, 2 * 4 * h * w * num_prior >= 2^31, capacity (floats) too small. */
FHIP_DETECT_API int fhip_priorbox_fill(int h, int w, int image_w, int image_h, const float* min_sizes, int num_min, const float* max_sizes, int num_max,
                                       const float* aspect_ratios, int num_ratios, const float* variances, int flip, int clip, float step_w,
                                       float step_h, float offset, int* num_prior, float* out, size_t capacity);

/* Bytes of device scratch fhip_detection_output_forward needs (the survivors of every class of every image between its two launches).
 * FHIP_E_BADARG: the limits above, NULL bytes. */
FHIP_DETECT_API int fhip_detection_output_get_buffer_size(int n, int num_priors, int num_class, int nms_top_k, int keep_top_k, size_t* bytes);

/* out[n][keep_top_k][6] = DetectionOutput(location[n][4 * P], confidence[n][P * num_class], priorbox[prior_n][2][4 * P]) as defined above;
 * prior_n is 1 (one set of priors for the batch) or n.  Two launches: "fhip::detect_select_kernel", a block per (class, image), selects,
 * decodes the selected boxes and runs the NMS in LDS; "fhip::detect_merge_kernel", a block per image, merges and writes every row.
 * FHIP_E_BADARG: the limits above, thresholds that are not finite, prior_n neither 1 nor n, NULL or unaligned pointers (scratch: 8 bytes). */
FHIP_DETECT_API int fhip_detection_output_forward(int n, int num_priors, int num_class, float nms_threshold, int nms_top_k, int keep_top_k,
                                                  float confidence_threshold, int prior_n, float* out, const float* location, const float* confidence,
                                                  const float* priorbox, void* scratch, void* stream);

/* The kernel instantiation a call would launch, as the demangled name without return type and parameters, copied into name[len]:
 *   FHIP_DETECT_PERMUTE    "fhip::permute_tile_kernel" for order 3 at rank 3 and order 1 at either rank -- transposes of [rows][cols] matrices
 *                          through a 32 x 33 LDS tile, loads and stores both coalesced, ragged tiles guarded -- else
 *                          "fhip::permute_generic_kernel": one output element per lane, coalesced stores
 *   FHIP_DETECT_NORMALIZE  "fhip::normalize_kernel<4>": a lane owns four adjacent pixels, 16-byte accesses, when h * w % 4 == 0 and both
 *                          pointers are 16-byte aligned; else "fhip::normalize_kernel<1>"
 *   FHIP_DETECT_PERMUTE_CONCAT "fhip::permute_concat_kernel"
 *   FHIP_DETECT_SOFTMAX    "fhip::axis_softmax_kernel";  FHIP_DETECT_SELECT "fhip::detect_select_kernel";  FHIP_DETECT_MERGE
 *                          "fhip::detect_merge_kernel"
 * a, b: see fhip_detect_op.  FHIP_E_BADARG: an unknown `what`, NULL name, len < 1, and what the forward refuses of (a, b, c, h, w). */
FHIP_DETECT_API int fhip_detect_route(int what, int a, int b, int c, int h, int w, const float* out, const float* in, char* name, int len);

/* Message of this thread's last failing call of this library ("" if none). */
FHIP_DETECT_API const char* fhip_detect_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* FEATHER_HIP_FEATHER_DETECT_H_ */
