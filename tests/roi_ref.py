"""include/feather_hip/feather_roi.h restated in numpy, operation for operation, in float32 -- what the device is held to exactly: the three
ROI layers to the bit, the Proposal for rows, order, counts and scores -- and the same text in float64, the yardstick for the Proposal's
coordinates.  Every operation works on values of `dtype`, so numpy rounds each on its own as the header says; sums run in the header's
order, never pairwise."""
import math

import numpy as np

F = np.float32
MAX_GRID = 4096  # FHIP_ROI_MAX_GRID
RATIOS, SCALES = (0.5, 1.0, 2.0), (8.0, 16.0, 32.0)


def _c_round(v):
    """C's round(): halves away from zero."""
    return math.copysign(math.floor(abs(v) + 0.5), v)


def generate_anchors(base_size=16, ratios=RATIOS, scales=SCALES):
    """[len(ratios) * len(scales)][4] float32: r_w and r_h in double, the rest in float32."""
    out = np.empty((len(ratios) * len(scales), 4), F)
    c = F(base_size) * F(0.5)
    for i, ratio in enumerate(ratios):
        ratio = float(F(ratio))
        r_w = _c_round(base_size / math.sqrt(ratio))
        r_h = _c_round(r_w * ratio)
        for j, scale in enumerate(scales):
            rs_w, rs_h = F(r_w) * F(scale), F(r_h) * F(scale)
            out[i * len(scales) + j] = (c - rs_w * F(0.5), c - rs_h * F(0.5), c + rs_w * F(0.5), c + rs_h * F(0.5))
    return out


def _clip(v, hi):
    zero = v.dtype.type(0)
    return np.where(v < zero, zero, np.where(v > hi, hi, v))  # a NaN stays a NaN


def decode(score, bbox, im_info, anchors, feat_stride, min_size, dtype=np.float32):
    """-> (boxes [n][A * h * w][4], scores [n][A * h * w] as fed, candidate mask, the smallest |extent - min_size * im_scale| over all anchors), in the
    index order (q * h + i) * w + j."""
    T = dtype
    n, _, h, w = score.shape
    a = np.asarray(anchors, F).astype(T)
    A = len(a)
    half, one = T(0.5), T(1)
    s = np.asarray(score, F)[:, A:].reshape(n, -1)
    d = np.asarray(bbox, F).astype(T).reshape(n, A, 4, h, w)
    info = np.asarray(im_info, F).astype(T).reshape(n, 3)
    with np.errstate(all="ignore"):
        ax = a[:, 0].reshape(1, A, 1, 1) + (np.arange(w) * feat_stride).astype(T).reshape(1, 1, 1, w)
        ay = a[:, 1].reshape(1, A, 1, 1) + (np.arange(h) * feat_stride).astype(T).reshape(1, 1, h, 1)
        aw = (a[:, 2] - a[:, 0]).reshape(1, A, 1, 1)
        ah = (a[:, 3] - a[:, 1]).reshape(1, A, 1, 1)
        cx, cy = ax + aw * half, ay + ah * half
        pcx, pcy = cx + aw * d[:, :, 0], cy + ah * d[:, :, 1]
        pw, ph = aw * np.exp(d[:, :, 2]), ah * np.exp(d[:, :, 3])
        im_h, im_w = info[:, 0].reshape(n, 1, 1, 1), info[:, 1].reshape(n, 1, 1, 1)
        min_box = (T(F(min_size)) * info[:, 2]).reshape(n, 1, 1, 1)
        x1, y1 = _clip(pcx - pw * half, im_w - one), _clip(pcy - ph * half, im_h - one)
        x2, y2 = _clip(pcx + pw * half, im_w - one), _clip(pcy + ph * half, im_h - one)
        ew, eh = x2 - x1 + one, y2 - y1 + one
        cand = ((ew >= min_box) & (eh >= min_box)).reshape(n, -1) & ~np.isnan(s)
        margin = float(np.nanmin(np.minimum(np.abs(ew.astype(np.float64) - min_box), np.abs(eh.astype(np.float64) - min_box)), initial=np.inf))
    boxes = np.stack([np.broadcast_to(v, (n, A, h, w)).reshape(n, -1) for v in (x1, y1, x2, y2)], axis=2)
    return boxes, s, cand, margin


def ious(kept, box):
    """ncnn's ratio of every row of kept [k][4] with box [4]: the intersection without + 1, the areas with it."""
    one, zero = kept.dtype.type(1), kept.dtype.type(0)
    aa = (kept[:, 2] - kept[:, 0] + one) * (kept[:, 3] - kept[:, 1] + one)
    ab = (box[2] - box[0] + one) * (box[3] - box[1] + one)
    disjoint = (kept[:, 0] > box[2]) | (kept[:, 2] < box[0]) | (kept[:, 1] > box[3]) | (kept[:, 3] < box[1])
    inter = np.where(disjoint, zero, (np.minimum(kept[:, 2], box[2]) - np.maximum(kept[:, 0], box[0])) * (np.minimum(kept[:, 3], box[3]) - np.maximum(kept[:, 1], box[1])))
    return inter / (aa + ab - inter)


def select(boxes, s, cand, pre_nms_topN, after_nms_topN, nms_thresh, margins=None):
    """The ordering, the cut and the greedy NMS of decode()'s result -> (rois [n][R][4], scores [n][R] float32); margins["iou"] receives the
    smallest compared |IoU - nms_thresh|, margins["order"] the smallest difference of two adjacent
    scores among the candidates the loop reached and the one behind them."""
    n, R, dtype = boxes.shape[0], after_nms_topN, boxes.dtype.type
    thr = dtype(F(nms_thresh))
    rois = np.zeros((n, R, 4), boxes.dtype)
    rois[:, :, 2:] = -1
    scores = np.zeros((n, R), F)
    worst = gap = np.inf
    for img in range(n):
        idx = np.nonzero(cand[img])[0]
        order = idx[np.lexsort((idx, -s[img][idx]))]  # score descending (-0.f equals 0.f), then index ascending
        if pre_nms_topN > 0:
            order = order[:pre_nms_topN + 1]  # (one more: the cut itself is a matter of order)
        count = reached = 0
        for r in order[:pre_nms_topN] if pre_nms_topN > 0 else order:
            if count >= R:
                break
            reached += 1
            b = boxes[img, r]
            if count:
                v = ious(rois[img, :count], b)
                worst = min(worst, float(np.abs(v.astype(np.float64) - float(thr)).min()))
                if (v > thr).any():
                    continue
            rois[img, count] = b
            scores[img, count] = s[img, r]
            count += 1
        if len(order) > 1:  # among the candidates the loop took, and the one behind them
            gap = min(gap, float(np.abs(np.diff(s[img][order[:reached + 1]].astype(np.float64))).min(initial=np.inf)))
    if margins is not None:
        margins["iou"] = min(margins.get("iou", np.inf), worst)
        margins["order"] = min(margins.get("order", np.inf), gap)
    return rois, scores


def proposal(score, bbox, im_info, anchors=None, feat_stride=16, pre_nms_topN=6000, after_nms_topN=300, nms_thresh=0.7, min_size=16, dtype=np.float32,
             margins=None):
    """Proposal -> (rois [n][R][4] in `dtype`, scores [n][R] float32).  margins: a dict that receives the smallest |extent - min box size|
    over all anchors ("extent"), the smallest compared |IoU - nms_thresh| ("iou") and the smallest difference of two adjacent candidates' scores
    ("order": 0 where two are equal)."""
    anchors = generate_anchors() if anchors is None else anchors
    boxes, s, cand, margin = decode(score, bbox, im_info, anchors, feat_stride, min_size, dtype)
    m = {}
    out = select(boxes, s, cand, pre_nms_topN, after_nms_topN, nms_thresh, m)
    if margins is not None:
        margins["extent"] = margin
        margins["iou"], margins["order"] = m["iou"], m["order"]
    return out


def counts(rois):
    """The number of real rows of every image of rois [n][R][4]: those with x2 >= x1."""
    return [int((img[:, 2] >= img[:, 0]).sum()) for img in rois]


def trim(rois):
    return [img[:k] for img, k in zip(rois, counts(rois))]


def worst_coordinate_error(got, want64, im_info):
    """The worst |got - want64| over the real rows, relative to the larger extent of the row's image."""
    worst = 0.0
    for g, w, info, k in zip(np.asarray(got, np.float64), np.asarray(want64, np.float64), np.asarray(im_info, np.float64).reshape(-1, 3), counts(want64)):
        if k:
            worst = max(worst, float(np.abs(g[:k] - w[:k]).max() / max(info[0], info[1])))
    return worst


# ---- the three ROI layers: scalar code per ROI and bin, vectors over the channels ----------------------------------------------------------
def _roundf(v):
    """C's roundf on a scalar of v's type."""
    T = type(v)
    a = abs(v)
    f = np.floor(a)
    r = f + (T(1) if a - f >= T(0.5) else T(0))
    return r if v >= 0 else -r


def _clampi(v, hi):
    return min(max(v, 0), hi)


def _rows(x, rois, dtype):
    """features [n][C][h][w] and rois [n][R][4] (or [n][R][1][4]) as `dtype`, and an iterator over (output row, the image's features, the ROI)."""
    f = np.asarray(x, F).astype(dtype)
    r = np.asarray(rois, F).astype(dtype).reshape(f.shape[0], -1, 4)
    return f, r, [(i * r.shape[1] + k, f[i], r[i, k]) for i in range(r.shape[0]) for k in range(r.shape[1])]


def roi_pool(x, rois, pooled_w=7, pooled_h=7, spatial_scale=0.0625, dtype=np.float32):
    T = dtype
    f, r, rows = _rows(x, rois, T)
    n, C, h, w = f.shape
    scale = T(F(spatial_scale))
    out = np.zeros((len(rows), C, pooled_h, pooled_w), T)
    for row, feat, roi in rows:
        x1, y1, x2, y2 = (int(_roundf(v * scale)) for v in roi)
        rw, rh = max(x2 - x1 + 1, 1), max(y2 - y1 + 1, 1)
        bw, bh = T(rw) / T(pooled_w), T(rh) / T(pooled_h)
        for p in range(pooled_h):
            hs, he = _clampi(y1 + int(np.floor(T(p) * bh)), h), _clampi(y1 + int(np.ceil(T(p + 1) * bh)), h)
            for q in range(pooled_w):
                ws, we = _clampi(x1 + int(np.floor(T(q) * bw)), w), _clampi(x1 + int(np.ceil(T(q + 1) * bw)), w)
                if he > hs and we > ws:
                    out[row, :, p, q] = feat[:, hs:he, ws:we].max(axis=(1, 2))  # without NaNs the header's m = m < v ? v : m is the maximum
    return out


def psroi_pool(x, rois, output_dim, pooled_w=7, pooled_h=7, spatial_scale=0.0625, dtype=np.float32):
    T = dtype
    f, r, rows = _rows(x, rois, T)
    n, C, h, w = f.shape
    assert C == output_dim * pooled_h * pooled_w
    scale = T(F(spatial_scale))
    out = np.zeros((len(rows), output_dim, pooled_h, pooled_w), T)
    for row, feat, roi in rows:
        x1, y1 = _roundf(roi[0]) * scale, _roundf(roi[1]) * scale
        x2, y2 = _roundf(roi[2] + T(1)) * scale, _roundf(roi[3] + T(1)) * scale
        rw, rh = max(x2 - x1, T(F(0.1))), max(y2 - y1, T(F(0.1)))
        bw, bh = rw / T(pooled_w), rh / T(pooled_h)
        planes = feat.reshape(output_dim, pooled_h, pooled_w, h, w)
        for p in range(pooled_h):
            hs, he = _clampi(int(np.floor(y1 + T(p) * bh)), h), _clampi(int(np.ceil(y1 + T(p + 1) * bh)), h)
            for q in range(pooled_w):
                ws, we = _clampi(int(np.floor(x1 + T(q) * bw)), w), _clampi(int(np.ceil(x1 + T(q + 1) * bw)), w)
                if he > hs and we > ws:
                    total = np.zeros(output_dim, T)
                    for y in range(hs, he):
                        for xx in range(ws, we):
                            total = total + planes[:, p, q, y, xx]
                    out[row, :, p, q] = total / T((he - hs) * (we - ws))
    return out


def _clip1(v, hi):
    T = type(v)
    return T(0) if v < T(0) else (hi if v > hi else v)


def _grid(sampling, extent):
    return min(sampling if sampling > 0 else int(np.ceil(extent)), MAX_GRID)


def roi_align(x, rois, pooled_w=7, pooled_h=7, spatial_scale=0.0625, sampling_ratio=0, aligned=0, version=0, dtype=np.float32):
    T = dtype
    f, r, rows = _rows(x, rois, T)
    n, C, h, w = f.shape
    scale, half, one, zero = T(F(spatial_scale)), T(0.5), T(1), T(0)
    out = np.zeros((len(rows), C, pooled_h, pooled_w), T)
    for row, feat, roi in rows:
        x1, y1, x2, y2 = (v * scale for v in roi)
        if aligned:
            x1, y1, x2, y2 = x1 - half, y1 - half, x2 - half, y2 - half
        rw, rh = x2 - x1, y2 - y1
        if not aligned:
            rw, rh = max(rw, one), max(rh, one)
        bw, bh = rw / T(pooled_w), rh / T(pooled_h)
        for p in range(pooled_h):
            for q in range(pooled_w):
                total = np.zeros(C, T)
                if version == 0:
                    hs, he = _clip1(y1 + T(p) * bh, T(h)), _clip1(y1 + T(p + 1) * bh, T(h))
                    ws, we = _clip1(x1 + T(q) * bw, T(w)), _clip1(x1 + T(q + 1) * bw, T(w))
                    if he <= hs or we <= ws:
                        continue
                    gh, gw = _grid(sampling_ratio, he - hs), _grid(sampling_ratio, we - ws)
                    for by in range(gh):
                        y = hs + ((T(by) + half) * bh) / T(gh)
                        y0 = max(int(y), 0)
                        if y0 >= h - 1:
                            y0 = yn = h - 1
                            b0, b1 = one, zero
                        else:
                            yn = y0 + 1
                            b0, b1 = T(yn) - y, y - T(y0)
                        for bx in range(gw):
                            xx = ws + ((T(bx) + half) * bw) / T(gw)
                            x0 = max(int(xx), 0)
                            if x0 >= w - 1:
                                x0 = xn = w - 1
                                a0, a1 = one, zero
                            else:
                                xn = x0 + 1
                                a0, a1 = T(xn) - xx, xx - T(x0)
                            r0 = feat[:, y0, x0] * a0 + feat[:, y0, xn] * a1
                            r1 = feat[:, yn, x0] * a0 + feat[:, yn, xn] * a1
                            total = total + (r0 * b0 + r1 * b1)
                    out[row, :, p, q] = total / T(gh * gw)
                else:
                    gh, gw = _grid(sampling_ratio, rh / T(pooled_h)), _grid(sampling_ratio, rw / T(pooled_w))
                    count = T(max(gh * gw, 1))
                    ybase, xbase = y1 + T(p) * bh, x1 + T(q) * bw
                    for iy in range(gh):
                        y = ybase + ((T(iy) + half) * bh) / T(gh)
                        y_out = y < -one or y > T(h)
                        y = zero if y <= zero else y
                        yl = max(int(y), 0)
                        if yl >= h - 1:
                            yh = yl = h - 1
                            y = T(yl)
                        else:
                            yh = yl + 1
                        ly = y - T(yl)
                        hy = one - ly
                        for ix in range(gw):
                            xx = xbase + ((T(ix) + half) * bw) / T(gw)
                            if y_out or xx < -one or xx > T(w):
                                continue
                            xx = zero if xx <= zero else xx
                            xl = max(int(xx), 0)
                            if xl >= w - 1:
                                xh = xl = w - 1
                                xx = T(xl)
                            else:
                                xh = xl + 1
                            lx = xx - T(xl)
                            hx = one - lx
                            v = (((hy * hx) * feat[:, yl, xl] + (hy * lx) * feat[:, yl, xh]) + (ly * hx) * feat[:, yh, xl]) + (ly * lx) * feat[:, yh, xh]
                            total = total + v
                    out[row, :, p, q] = total / count
    return out


# ---- reading a zoo .param ------------------------------------------------------------------------------------------------------------------
def parse_param(text):
    """-> [(type, name, bottoms, tops, {id: value})] of a .param without arrays."""
    out = []
    for line in text.decode().split("\n")[2:]:
        f = line.split()
        if not f:
            continue
        nb, nt = int(f[2]), int(f[3])
        pd = {}
        for kv in f[4 + nb + nt:]:
            k, v = kv.split("=")
            if int(k) > -23300:
                pd[int(k)] = float(v) if any(ch in v for ch in ".eE") else int(v)
        out.append((f[0], f[1], f[4:4 + nb], f[4 + nb:4 + nb + nt], pd))
    return out
