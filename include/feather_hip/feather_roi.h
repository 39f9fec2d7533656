/* feather_roi.h -- C-ABI of libfeather_roi.so: the layers of a two-stage detector (Faster R-CNN, R-FCN) on the MI355X (gfx950) -- Proposal,
 * ROIPooling, ROIAlign and PSROIPooling -- as ncnn defines them, on fp32 blobs with a leading batch.
 *
 * The reference has none of these layers: this text is the definition, written from what ncnn's proposal.cpp, roipooling.cpp, roialign.cpp
 * and psroipooling.cpp do.  Where it had to decide something, it says "decided here".  tests/roi_ref.py restates it line by line.
 * Everything is fp32 and every operation is rounded on its own (no contraction); expf is the device function; roundf rounds halves away
 * from zero; (int) truncates.  No layer is in place.
 *
 * generate_anchors (host)   anchors[num_ratios * num_scales][4] of ncnn's generate_anchors; row ratio_index * num_scales + scale_index:
 *                   r_w = round(base_size / sqrt(ratio)), r_h = round(r_w * ratio), both in double and halves away from zero (decided here:
 *                   ncnn leaves the precision to the compiler);  rs_w = (float)r_w * scale, rs_h = (float)r_h * scale;  c = (float)base_size * 0.5f;
 *                   the row is (c - rs_w * 0.5f, c - rs_h * 0.5f, c + rs_w * 0.5f, c + rs_h * 0.5f).  ncnn's Proposal calls it with ratios 0.5, 1, 2
 *                   and scales 8, 16, 32.  The box is centred on base_size / 2, where py-faster-rcnn centres on (base_size - 1) / 2 and counts
 *                   x2 - x1 + 1 as the width: base 16 gives the nine published anchors with x2 and y2 one larger.
 *
 * Proposal          params 0=feat_stride (16), 1=base_size (16), 2=pre_nms_topN (6000), 3=after_nms_topN (300), 4=nms_thresh (0.7), 5=min_size (16).
 *                   score[n][2A][h][w]: anchor q's foreground score is plane A + q;  bbox[n][4A][h][w]: planes 4q .. 4q + 3 are dx, dy, dw, dh;
 *                   im_info[n][3]: (height, width, scale) of every image;  a[A][4]: the anchor table.  For anchor q, row i, column j:
 *                      ax = a[q][0] + (float)(j * feat_stride);  ay = a[q][1] + (float)(i * feat_stride);  aw = a[q][2] - a[q][0];  ah = a[q][3] - a[q][1]
 *                      cx = ax + aw * 0.5f;  cy = ay + ah * 0.5f;  pcx = cx + aw * dx;  pcy = cy + ah * dy;  pw = aw * expf(dw);  ph = ah * expf(dh)
 *                      x1 = pcx - pw * 0.5f;  y1 = pcy - ph * 0.5f;  x2 = pcx + pw * 0.5f;  y2 = pcy + ph * 0.5f
 *                      clip(v, hi) = v < 0.f ? 0.f : (v > hi ? hi : v)   -- ncnn's max(min(v, hi), 0.f); a NaN stays a NaN
 *                      x1, x2 = clip(., im_w - 1.f);  y1, y2 = clip(., im_h - 1.f)
 *                      the box is a candidate when x2 - x1 + 1.f >= min_size * im_scale and y2 - y1 + 1.f >= min_size * im_scale and its
 *                      score is not a NaN; a NaN extent compares false (decided here: ncnn would sort NaNs in an unspecified order)
 *                   Candidates are ordered by score descending, ties by the index (q * h + i) * w + j ascending (decided here: ncnn's push order
 *                   made deterministic; -0.f equals 0.f).  The first pre_nms_topN of them are kept (<= 0: all).  Greedy NMS runs in that order:
 *                      area = (x2 - x1 + 1.f) * (y2 - y1 + 1.f)
 *                      inter = 0.f when a.x1 > b.x2 || a.x2 < b.x1 || a.y1 > b.y2 || a.y2 < b.y1, else
 *                              (min(a.x2, b.x2) - max(a.x1, b.x1)) * (min(a.y2, b.y2) - max(a.y1, b.y1))       -- without + 1, as ncnn
 *                      a candidate is dropped when inter / (area_a + area_b - inter) > nms_thresh for a box kept before it
 *                   The first after_nms_topN = R survivors are the ROIs: rois[n][R][4] rows (x1, y1, x2, y2) and, where asked, scores[n][R].
 *                   Rows past an image's count hold the sentinel (0, 0, -1, -1) and the score 0 (decided here): a real ROI never has x2 < x1,
 *                   so the count is the number of rows with x2 >= x1 and a legitimate (0, 0, 0, 0) stays distinguishable.  The fixed height is
 *                   the one deliberate difference from ncnn's Mat of as many channels as there are ROIs, as for DetectionOutput.  Greedy NMS
 *                   only looks backwards, so the output is a PREFIX OF NCNN'S LIST whatever R is.  Scores are moved, never computed.
 *                   Results do not depend on thread scheduling: every anchor owns one distinct 64-bit key (score bits, inverted index), 0 when
 *                   it is no candidate; the order comes from sorting keys, and atomics only count.
 *
 * The three ROI layers   features[n][C][h][w] and rois[n][R][4] (R >= 1; a Proposal top or anything else) -> out[n * R][channels][ph][pw]; row
 *                   i * R + r is ROI r = (rx1, ry1, rx2, ry2) of image i, read from image i's features.  ncnn's layer is n = R = 1.  Every ROI
 *                   is pooled by the same text, the sentinel, inverted and outside ones included.  ROI coordinates are meant finite with
 *                   |v * scale| < 2^30: beyond that the (int) conversions leave the result unspecified -- never an access outside the tensors.
 *   ROIPooling      params 0=pooled_width (7), 1=pooled_height (7), 2=spatial_scale (0.0625).
 *                      x1 = (int)roundf(rx1 * scale), y1, x2, y2 likewise;  rw = max(x2 - x1 + 1, 1);  rh = max(y2 - y1 + 1, 1)
 *                      bw = (float)rw / (float)pw;  bh = (float)rh / (float)ph
 *                      bin (p, q):  hs = y1 + (int)floorf((float)p * bh);  he = y1 + (int)ceilf((float)(p + 1) * bh), both clamped to [0, h];
 *                                   ws = x1 + (int)floorf((float)q * bw);  we = x1 + (int)ceilf((float)(q + 1) * bw), both clamped to [0, w]
 *                      out = 0.f when he <= hs || we <= ws, else the maximum of in[c][hs .. he)[ws .. we) (m = the first; m = m < v ? v : m in
 *                      row-major order).  Exact: values are moved.
 *   PSROIPooling    params 0 .. 2 as above, 3=output_dim.  C must be output_dim * ph * pw.
 *                      x1 = roundf(rx1) * scale;  y1 = roundf(ry1) * scale;  x2 = roundf(rx2 + 1.f) * scale;  y2 = roundf(ry2 + 1.f) * scale
 *                      rw = max(x2 - x1, 0.1f);  rh = max(y2 - y1, 0.1f);  bw = rw / (float)pw;  bh = rh / (float)ph
 *                      bin (d, p, q) reads channel (d * ph + p) * pw + q:
 *                         hs = (int)floorf(y1 + (float)p * bh);  he = (int)ceilf(y1 + (float)(p + 1) * bh), clamped to [0, h]; ws, we likewise
 *                      out = 0.f when he <= hs || we <= ws, else sum / (float)((he - hs) * (we - ws)), sum from 0.f in row-major order
 *   ROIAlign        params 0 .. 2 as above, 3=sampling_ratio (0), 4=aligned (0), 5=version (0).
 *                      x1 = rx1 * scale, y1, x2, y2 likewise, each - 0.5f when aligned;  rw = x2 - x1;  rh = y2 - y1, each max(., 1.f) when not aligned
 *                      bw = rw / (float)pw;  bh = rh / (float)ph
 *                   version 0 (ncnn's original), bin (p, q):
 *                      hs = y1 + (float)p * bh;  he = y1 + (float)(p + 1) * bh;  ws, we likewise;  each clamped to [0, (float)h] / [0, (float)w] with
 *                      clip above;  out = 0.f when he <= hs || we <= ws (decided here: without sampling; ncnn samples first and may read past
 *                      the map);  gh = sampling_ratio > 0 ? sampling_ratio : (int)ceilf(he - hs), gw likewise
 *                      sample (by, bx):  y = hs + (((float)by + 0.5f) * bh) / (float)gh;  x = ws + (((float)bx + 0.5f) * bw) / (float)gw
 *                         x0 = (int)x (below 0: 0);  when x0 >= w - 1: x0 = xn = w - 1, a0 = 1.f, a1 = 0.f (decided here for x0 >= w, where ncnn
 *                         reads past the row), else xn = x0 + 1, a0 = (float)xn - x, a1 = x - (float)x0;  y0, yn, b0, b1 likewise with h
 *                         v = (in[y0][x0] * a0 + in[y0][xn] * a1) * b0 + (in[yn][x0] * a0 + in[yn][xn] * a1) * b1
 *                      out = (the sum of v from 0.f, by outer, bx inner) / (float)(gh * gw)
 *                   version 1 (detectron2 / torchvision):
 *                      gh = sampling_ratio > 0 ? sampling_ratio : (int)ceilf(rh / (float)ph), gw likewise;  count = (float)max(gh * gw, 1)
 *                      sample (iy, ix) of bin (p, q):  y = (y1 + (float)p * bh) + (((float)iy + 0.5f) * bh) / (float)gh, x likewise
 *                         the sample is 0.f when y < -1.f || y > (float)h || x < -1.f || x > (float)w;  else y = y <= 0.f ? 0.f : y, x likewise
 *                         yl = (int)y;  when yl >= h - 1: yh = yl = h - 1, y = (float)yl, else yh = yl + 1;  xl, xh likewise
 *                         ly = y - (float)yl;  lx = x - (float)xl;  hy = 1.f - ly;  hx = 1.f - lx
 *                         v = (((hy * hx) * in[yl][xl] + (hy * lx) * in[yl][xh]) + (ly * hx) * in[yh][xl]) + (ly * lx) * in[yh][xh]
 *                      out = (the sum of v from 0.f, iy outer, ix inner) / count
 *                   Either version: a sampling grid extent above FHIP_ROI_MAX_GRID is FHIP_ROI_MAX_GRID (decided here: ncnn loops on; an ROI
 *                   that many cells wide per bin is no ROI of a feature map this library accepts).
 *
 * Limits, refused with FHIP_E_BADARG and never truncated: 1 .. FHIP_ROI_MAX_ANCHORS anchors, at most FHIP_ROI_MAX_CELLS anchors per image
 * (A * h * w), 1 .. FHIP_ROI_MAX_ROIS rows of a Proposal top, n <= 65535, every tensor below 2^31 elements, thresholds, scales and anchors
 * that are not finite, pooled extents outside 1 .. FHIP_ROI_MAX_POOLED.
 *
 * No entry allocates, copies or synchronises: every device entry is hipGraph-capturable.  The anchors travel as kernel arguments: nothing is
 * uploaded.  Pointers need 4-byte alignment (scratch: 8).  The library is separate from libfeather_hip.so and needs nothing from it but the
 * enums of feather_hip.h; it keeps its own last-error slot. */
#ifndef FEATHER_HIP_FEATHER_ROI_H_
#define FEATHER_HIP_FEATHER_ROI_H_

#include <stddef.h>

#include "feather_hip/feather_hip.h"

#ifdef __cplusplus
extern "C"
{
#endif

#define FHIP_ROI_API __attribute__((visibility("default")))

/* Route code fhip_net_layer_info reports for the layers of a net with fhip_net_set_roi (feather_net.h): Proposal, ROIPooling, ROIAlign and
 * PSROIPooling. */
#define FHIP_ROI_NET_ROUTE 111

#define FHIP_ROI_MAX_ANCHORS 32
#define FHIP_ROI_MAX_CELLS (1 << 24)
#define FHIP_ROI_MAX_ROIS 2048
#define FHIP_ROI_MAX_POOLED 64
#define FHIP_ROI_MAX_GRID 4096
/* candidates one selection round takes, and keys one pass of the selection kernel looks at */
#define FHIP_ROI_CHUNK 1024

/* `what` of fhip_roi_route (a and b are ignored but for FHIP_ROI_ALIGN: a = version) */
enum fhip_roi_op
{
    FHIP_ROI_KEYS = 1,   /* the Proposal's first launch */
    FHIP_ROI_SELECT = 2, /* the Proposal's second launch */
    FHIP_ROI_POOL = 3,
    FHIP_ROI_ALIGN = 4, /* a = version (0 or 1) */
    FHIP_ROI_PSROI = 5
};

/* anchors[num_ratios * num_scales][4] as defined above: a host function, no device needed.  FHIP_E_BADARG: base_size < 1, a count < 1, more
 * than FHIP_ROI_MAX_ANCHORS rows, a ratio or scale that is not finite and > 0, NULL pointers. */
FHIP_ROI_API int fhip_roi_generate_anchors(int base_size, const float* ratios, int num_ratios, const float* scales, int num_scales, float* anchors);

/* Bytes of device scratch fhip_proposal_forward needs (one key per anchor of every image between its two launches).  FHIP_E_BADARG: the
 * limits above, a dimension < 1, a NULL pointer. */
FHIP_ROI_API int fhip_proposal_get_buffer_size(int n, int num_anchors, int h, int w, size_t* bytes);

/* rois[n][after_nms_topN][4] (and scores[n][after_nms_topN] unless NULL) = Proposal(score[n][2A][h][w], bbox[n][4A][h][w], im_info[n][3]) as
 * defined above.  anchors[A][4] is a HOST array, read before the call returns.  Two launches on `stream` (a hipStream_t as void*):
 * "fhip::proposal_key_kernel", a lane per anchor, writes every anchor's key; "fhip::proposal_select_kernel", a block per image, selects in
 * score order, decodes the selected boxes, runs the NMS with the kept boxes in LDS and writes every row.  FHIP_E_BADARG: the limits above,
 * feat_stride < 1, nms_thresh, min_size or an anchor not finite, NULL or unaligned pointers (scratch: 8 bytes), an output or the scratch
 * overlapping another tensor. */
FHIP_ROI_API int fhip_proposal_forward(int n, int num_anchors, int h, int w, int feat_stride, int pre_nms_topN, int after_nms_topN, float nms_thresh,
                                       float min_size, const float* anchors, float* rois, float* scores, const float* score, const float* bbox,
                                       const float* im_info, void* scratch, void* stream);

/* out[n * R][c][pooled_h][pooled_w] = ROIPooling(in[n][c][h][w], rois[n][R][4]) as defined above: one launch, "fhip::roi_pool_kernel", an output
 * element per lane.  FHIP_E_BADARG: a dimension < 1, pooled extents outside 1 .. FHIP_ROI_MAX_POOLED, a scale not finite, 2^31 elements or
 * more, NULL or unaligned pointers, out overlapping an input. */
FHIP_ROI_API int fhip_roi_pool_forward(int n, int c, int h, int w, int num_rois, int pooled_w, int pooled_h, float spatial_scale, float* out,
                                       const float* in, const float* rois, void* stream);

/* out[n * R][c][pooled_h][pooled_w] = ROIAlign(in, rois): one launch, "fhip::roi_align_kernel<version>".  FHIP_E_BADARG as above, and a
 * version other than 0 / 1, aligned other than 0 / 1, sampling_ratio < 0 or above FHIP_ROI_MAX_GRID. */
FHIP_ROI_API int fhip_roi_align_forward(int n, int c, int h, int w, int num_rois, int pooled_w, int pooled_h, float spatial_scale, int sampling_ratio,
                                        int aligned, int version, float* out, const float* in, const float* rois, void* stream);

/* out[n * R][output_dim][pooled_h][pooled_w] = PSROIPooling(in[n][c][h][w], rois): one launch, "fhip::psroi_pool_kernel".  FHIP_E_BADARG as
 * above, and c != output_dim * pooled_h * pooled_w. */
FHIP_ROI_API int fhip_psroi_pool_forward(int n, int c, int h, int w, int num_rois, int pooled_w, int pooled_h, float spatial_scale, int output_dim,
                                         float* out, const float* in, const float* rois, void* stream);

/* The kernel a call would launch, as the demangled name without return type and parameters, copied into name[len]:
 *   FHIP_ROI_KEYS "fhip::proposal_key_kernel";  FHIP_ROI_SELECT "fhip::proposal_select_kernel";  FHIP_ROI_POOL "fhip::roi_pool_kernel";
 *   FHIP_ROI_ALIGN "fhip::roi_align_kernel<0>" or "fhip::roi_align_kernel<1>";  FHIP_ROI_PSROI "fhip::psroi_pool_kernel"
 * FHIP_E_BADARG: an unknown `what` (0 is none), NULL name, len < 1, a version other than 0 / 1. */
FHIP_ROI_API int fhip_roi_route(int what, int a, int b, char* name, int len);

/* Message of this thread's last failing call of this library ("" if none). */
FHIP_ROI_API const char* fhip_roi_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* FEATHER_HIP_FEATHER_ROI_H_ */
