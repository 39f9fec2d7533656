/* feather_yolo.h -- C-ABI of libfeather_yolo.so: the layers of a YOLO detection head on the MI355X (gfx950) -- Reorg, YoloDetectionOutput
 * (YOLOv2) and Yolov3DetectionOutput -- as ncnn defines them, on fp32 blobs with a leading batch.
 *
 * The reference has none of these layers: this text is the definition, written from what ncnn's reorg.cpp, yolodetectionoutput.cpp and
 * yolov3detectionoutput.cpp do.  Where it had to decide something, it says "decided here".  tests/yolo_ref.py restates it line by line.
 * Everything is fp32 and every operation is rounded on its own (no contraction); expf is the device function.
 *
 * Reorg          params 0=stride, 1=mode (default 0).  For in[n][c][h][w]: oh = h / stride, ow = w / stride, rounded down as ncnn does; rows
 *                and columns past oh * stride and ow * stride are not read.  The output is [n][c * stride * stride][oh][ow]:
 *                   mode 0:  out[q * s * s + sh * s + sw][i][j] = in[q][i * s + sh][j * s + sw]
 *                   mode 1:  the output channel is (sh * s + sw) * c + q
 *                Exact: values are moved, never computed.
 *
 * YoloDetectionOutput (version 2)   params 0=num_class, 1=num_box, 2=confidence_threshold, 3=nms_threshold, -23304=biases.  1 ..
 *                FHIP_YOLO_MAX_SCALES bottoms of shape [n][num_box * (5 + num_class)][h][w].  For box pp of cell (i, j), base = pp * (5 + num_class):
 *                planes base .. base + 3 are x, y, w, h, plane base + 4 the objectness, the planes behind it the class scores s[c].
 *                   sigmoid(v) = 1.f / (1.f + expf(-v))
 *                   m = the maximum of s (fmaxf, from -FLT_MAX);  e[c] = expf(s[c] - m);  sum = the sum of e in class order, from 0.f;
 *                   p[c] = e[c] / sum;  the class is the FIRST maximum of p;  confidence = sigmoid(objectness) * p[class]
 *                   the box is a candidate when confidence >= confidence_threshold (a NaN is no candidate)
 *                   cx = ((float)j + sigmoid(x)) / (float)w;  cy = ((float)i + sigmoid(y)) / (float)h
 *                   bw = (expf(w_raw) * biases[2 * pp]) / (float)w;  bh = (expf(h_raw) * biases[2 * pp + 1]) / (float)h
 *                   box = (cx - bw * 0.5f, cy - bh * 0.5f, cx + bw * 0.5f, cy + bh * 0.5f)
 *
 * Yolov3DetectionOutput (version 3)   adds -23305=mask and -23306=anchors_scale.  For bottom b, box pp:  a = mask[b * num_box + pp];
 *                   the class is the FIRST maximum of the RAW class scores (s[c] > best, from s[0])
 *                   confidence = 1.f / ((1.f + expf(-objectness)) * (1.f + expf(-s[class])));  the same >= test decides candidates
 *                   cx and cy as above
 *                   bw = (expf(w_raw) * biases[2 * a]) / (anchors_scale[b] * (float)w);  bh = (expf(h_raw) * biases[2 * a + 1]) / (anchors_scale[b] * (float)h)
 *
 * Both versions. All candidates of an image, over all bottoms, are ordered by confidence descending; ties are broken by a global box index
 *                ascending: bottom, then box, then row, then column (index = first[b] + (pp * h + i) * w + j).  The tie rule is decided here:
 *                it makes the result a function of the input, which ncnn's quicksort does not.  Greedy NMS runs in that order and is
 *                class-agnostic, as in ncnn, with the formulas of feather_detect.h:
 *                   area = (x1 - x0) * (y1 - y0);  iw = min(ax1, bx1) - max(ax0, bx0), ih likewise;  inter = iw <= 0 || ih <= 0 ? 0 : iw * ih
 *                   iou = inter / (area_a + area_b - inter)      (0 / 0 compares false: such a pair suppresses nothing)
 *                a candidate is dropped when its IoU with a box already kept is > nms_threshold.
 *                The output is [n][rows][6], rows (label + 1, score, xmin, ymin, xmax, ymax): the first `rows` survivors, the remaining rows
 *                all zero; label 0 never occurs in a real row, so the count is the number of rows with label > 0.
 *                Greedy NMS decides a candidate from better-ordered candidates only, so the output is by definition a PREFIX OF NCNN'S LIST,
 *                whatever `rows` is: rows = 5 gives the first 5 rows of rows = 64.  The fixed height is the one deliberate difference from
 *                ncnn's Mat of as many rows as there are detections (decided here), as for DetectionOutput: it lets the layer run in a
 *                captured graph and in sub-batch replicas.
 *                The number of candidates has no limit: they are selected in score order FHIP_YOLO_CHUNK at a time until `rows` are kept or
 *                the candidates are exhausted.  Results do not depend on thread scheduling: every box owns one distinct 64-bit key
 *                (confidence bits, inverted index, label), the order comes from sorting keys, and atomics only count.
 *
 * Limits, refused with FHIP_E_BADARG and never truncated: 1 .. FHIP_YOLO_MAX_SCALES bottoms, 1 .. FHIP_YOLO_MAX_BOXES boxes per cell, 1 ..
 * FHIP_YOLO_MAX_CLASSES classes, at most FHIP_YOLO_MAX_CELLS boxes per image over all bottoms, 1 .. FHIP_YOLO_MAX_ROWS rows, n <= 65535, and
 * every tensor below 2^31 elements.
 *
 * No entry allocates, copies or synchronises: every device entry is hipGraph-capturable.  Anchors, masks and anchor scales travel as kernel
 * arguments: nothing is uploaded.  Pointers need 4-byte alignment (scratch: 8).  No layer is in place.  The library is separate from
 * libfeather_hip.so and needs nothing from it but the enums of feather_hip.h; it keeps its own last-error slot. */
#ifndef FEATHER_HIP_FEATHER_YOLO_H_
#define FEATHER_HIP_FEATHER_YOLO_H_

#include <stddef.h>

#include "feather_hip/feather_hip.h"

#ifdef __cplusplus
extern "C"
{
#endif

#define FHIP_YOLO_API __attribute__((visibility("default")))

/* Route code fhip_net_layer_info reports for the layers of a net with fhip_net_set_yolo (feather_net.h): Reorg, YoloDetectionOutput and
 * Yolov3DetectionOutput. */
#define FHIP_YOLO_NET_ROUTE 110

#define FHIP_YOLO_MAX_SCALES 4
#define FHIP_YOLO_MAX_BOXES 16
#define FHIP_YOLO_MAX_CLASSES 256
#define FHIP_YOLO_MAX_CELLS (1 << 22)
#define FHIP_YOLO_MAX_ROWS 1024
/* candidates one selection round keeps, and keys one pass of the selection kernel looks at */
#define FHIP_YOLO_CHUNK 1024
/* floats of the LDS tile of the Reorg kernel: planes with stride * w above it take the direct kernel */
#define FHIP_REORG_TILE 4096

/* `what` of fhip_yolo_route */
enum fhip_yolo_op
{
    FHIP_YOLO_REORG = 0, /* a = stride, b = w */
    FHIP_YOLO_SCORE = 1, /* a = version (2 or 3): the detection's first launch */
    FHIP_YOLO_SELECT = 2 /* the detection's second launch */
};

/* The (c, h, w) of Reorg's output.  FHIP_E_BADARG: stride < 1, a dimension < 1, h or w below stride, c * stride * stride >= 2^31, a NULL
 * pointer. */
FHIP_YOLO_API int fhip_reorg_output_dim(int stride, int c, int h, int w, int* out_c, int* out_h, int* out_w);

/* out = Reorg(in[n][c][h][w]) as defined above: one launch on `stream` (a hipStream_t as void*).  FHIP_E_BADARG: what fhip_reorg_output_dim
 * refuses, mode outside 0 / 1, n < 1, 2^31 elements or more, NULL or unaligned (4 bytes) pointers, out overlapping in. */
FHIP_YOLO_API int fhip_reorg_forward(int stride, int mode, int n, int c, int h, int w, float* out, const float* in, void* stream);

/* Bytes of device scratch fhip_yolo_detection_forward needs (one key per box of every image between its two launches); h[i], w[i] are the
 * extents of bottom i.  FHIP_E_BADARG: the limits above, a dimension < 1, NULL pointers. */
FHIP_YOLO_API int fhip_yolo_get_buffer_size(int n, int scales, int num_box, int num_class, const int* h, const int* w, size_t* bytes);

/* out[n][rows][6] = YoloDetectionOutput (version 2) or Yolov3DetectionOutput (version 3) of bottoms[i][n][num_box * (5 + num_class)][h[i]][w[i]]
 * as defined above.  biases: num_biases floats, an even count, at least 2 * num_box of them at version 2; version 3 reads mask[scales * num_box]
 * (every entry in 0 .. num_biases / 2 - 1) and anchors_scale[scales] (finite, > 0), version 2 ignores both.  biases, mask, anchors_scale, h,
 * w and bottoms are HOST arrays, read before the call returns.  Two launches: "fhip::yolo_score_kernel<V>", a lane per box, writes every
 * box's key; "fhip::yolo_select_kernel", a block per image, selects, decodes the selected boxes, runs the NMS in LDS and writes every row.
 * FHIP_E_BADARG: the limits above, a version other than 2 / 3, thresholds, biases or scales that are not finite, a mask entry outside the
 * anchors, NULL or unaligned pointers (scratch: 8 bytes), out or scratch overlapping a bottom or each other. */
FHIP_YOLO_API int fhip_yolo_detection_forward(int version, int n, int scales, int num_box, int num_class, const int* h, const int* w,
                                              float confidence_threshold, float nms_threshold, const float* biases, int num_biases, const int* mask,
                                              const float* anchors_scale, int rows, float* out, const float* const* bottoms, void* scratch, void* stream);

/* The kernel instantiation a call would launch, as the demangled name without return type and parameters, copied into name[len]:
 *   FHIP_YOLO_REORG   "fhip::reorg_tile_kernel" when stride > 1 and stride * w <= FHIP_REORG_TILE: a block loads the contiguous input rows of a
 *                     group of output rows into LDS and writes stride * stride contiguous runs, both sides coalesced; else
 *                     "fhip::reorg_direct_kernel": one output element per lane, coalesced stores
 *   FHIP_YOLO_SCORE   "fhip::yolo_score_kernel<2>" or "fhip::yolo_score_kernel<3>";   FHIP_YOLO_SELECT "fhip::yolo_select_kernel"
 * FHIP_E_BADARG: an unknown `what`, NULL name, len < 1, stride or w < 1, a version other than 2 / 3. */
FHIP_YOLO_API int fhip_yolo_route(int what, int a, int b, char* name, int len);

/* Message of this thread's last failing call of this library ("" if none). */
FHIP_YOLO_API const char* fhip_yolo_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* FEATHER_HIP_FEATHER_YOLO_H_ */
