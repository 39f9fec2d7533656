"""include/feather_hip/feather_yolo.h restated in numpy, operation for operation, in float32 -- what the device is held to exactly for rows, labels
and order -- and the same text in float64, the yardstick for scores and coordinates.  Every operation works on arrays of `dtype`, so numpy
rounds each on its own as the header says; sums run in class order, never pairwise."""
import numpy as np

F = np.float32
FLT_MAX = float(np.finfo(np.float32).max)


def reorg(x, stride, mode=0):
    """Reorg of [n][c][h][w]: mode 0 out[q * s * s + sh * s + sw][i][j] = in[q][i * s + sh][j * s + sw]; mode 1 channel (sh * s + sw) * c + q."""
    n, c, h, w = x.shape
    s, oh, ow = stride, h // stride, w // stride
    out = np.empty((n, c * s * s, oh, ow), x.dtype)
    for q in range(c):
        for sh in range(s):
            for sw in range(s):
                ch = q * s * s + sh * s + sw if mode == 0 else (sh * s + sw) * c + q
                out[:, ch] = x[:, q, sh:oh * s:s, sw:ow * s:s]
    return out


def _sigmoid(v):
    one = v.dtype.type(1)
    return one / (one + np.exp(-v))


def scores(bottoms, version, num_class, num_box, dtype=np.float32):
    """-> (confidence [n][boxes per image], label [n][boxes per image], runner-up margin [n][boxes]) in global box order: bottom, box, row, column."""
    conf, label, gap = [], [], []
    with np.errstate(all="ignore"):
        for x in bottoms:
            n, _, h, w = x.shape
            v = np.asarray(x, F).astype(dtype).reshape(n, num_box, 5 + num_class, h, w)
            obj, s = v[:, :, 4], v[:, :, 5:]
            if version == 2:
                m = np.fmax.reduce(s, axis=2, initial=dtype(-FLT_MAX))
                e = np.exp(s - m[:, :, None])
                total = np.zeros_like(m)
                for c in range(num_class):
                    total = total + e[:, :, c]
                ranked = e / total[:, :, None]
                lab = np.argmax(ranked, axis=2)
                best = np.take_along_axis(ranked, lab[:, :, None], axis=2)[:, :, 0]
                cf = _sigmoid(obj) * best
            else:
                ranked = s
                lab = np.argmax(s, axis=2)
                best = np.take_along_axis(s, lab[:, :, None], axis=2)[:, :, 0]
                one = dtype(1)
                cf = one / ((one + np.exp(-obj)) * (one + np.exp(-best)))
            if num_class > 1:
                top2 = np.sort(ranked, axis=2)[:, :, -2:]
                gap.append((top2[:, :, 1] - top2[:, :, 0]).reshape(n, -1))
            else:
                gap.append(np.full((n, num_box * h * w), np.inf))
            conf.append(cf.reshape(n, -1))
            label.append(lab.reshape(n, -1))
    return np.concatenate(conf, axis=1), np.concatenate(label, axis=1), np.concatenate(gap, axis=1)


def _boxes(bottoms, img, index, version, num_class, num_box, biases, mask, anchors_scale, dtype):
    """The decoded boxes [len(index)][4] of the global box indices `index` of image `img`."""
    first = np.cumsum([0] + [num_box * x.shape[2] * x.shape[3] for x in bottoms])
    out = np.empty((len(index), 4), dtype)
    half = dtype(0.5)
    with np.errstate(all="ignore"):
        for k, r in enumerate(index):
            b = int(np.searchsorted(first, r, side="right") - 1)
            x = bottoms[b]
            h, w = x.shape[2], x.shape[3]
            pp, cell = divmod(int(r - first[b]), h * w)
            i, j = divmod(cell, w)
            raw = np.asarray(x[img, pp * (5 + num_class):pp * (5 + num_class) + 4, i, j], F).astype(dtype)
            cx = (dtype(j) + _sigmoid(raw[0:1])[0]) / dtype(w)
            cy = (dtype(i) + _sigmoid(raw[1:2])[0]) / dtype(h)
            if version == 2:
                bw = (np.exp(raw[2]) * dtype(F(biases[2 * pp]))) / dtype(w)
                bh = (np.exp(raw[3]) * dtype(F(biases[2 * pp + 1]))) / dtype(h)
            else:
                a, sc = int(mask[b * num_box + pp]), dtype(F(anchors_scale[b]))
                bw = (np.exp(raw[2]) * dtype(F(biases[2 * a]))) / (sc * dtype(w))
                bh = (np.exp(raw[3]) * dtype(F(biases[2 * a + 1]))) / (sc * dtype(h))
            out[k] = (cx - bw * half, cy - bh * half, cx + bw * half, cy + bh * half)
    return out


def iou(kept, box):
    """IoU of every row of kept [k][4] with box [4], feather_detect.h's formulas; 0 / 0 is NaN."""
    with np.errstate(all="ignore"):
        zero = kept.dtype.type(0)
        iw = np.minimum(kept[:, 2], box[2]) - np.maximum(kept[:, 0], box[0])
        ih = np.minimum(kept[:, 3], box[3]) - np.maximum(kept[:, 1], box[1])
        inter = np.where((iw <= zero) | (ih <= zero), zero, iw * ih)
        aa = (kept[:, 2] - kept[:, 0]) * (kept[:, 3] - kept[:, 1])
        ab = (box[2] - box[0]) * (box[3] - box[1])
        return inter / (aa + ab - inter)


def detection(bottoms, version, num_class, num_box, biases, confidence_threshold, nms_threshold, rows, mask=None, anchors_scale=None, dtype=np.float32,
              margins=None):
    """YoloDetectionOutput (version 2) / Yolov3DetectionOutput (version 3) of the bottoms [n][num_box * (5 + num_class)][h][w] -> [n][rows][6] in
    `dtype`.  margins: a dict that receives the smallest |confidence - threshold| over all boxes ("threshold"), the smallest |IoU - nms_threshold|
    over the compared pairs ("iou"), the smallest difference of two adjacent candidates that are not exactly equal ("order") and the smallest
    lead of a box's class over its runner-up ("class")."""
    thr, nms = dtype(F(confidence_threshold)), dtype(F(nms_threshold))
    conf, label, gap = scores(bottoms, version, num_class, num_box, dtype)
    n = conf.shape[0]
    out = np.zeros((n, rows, 6), dtype)
    m = dict(threshold=np.inf, iou=np.inf, order=np.inf, **{"class": np.inf})
    for img in range(n):
        c = conf[img]
        with np.errstate(all="ignore"):
            cand = np.nonzero(c >= thr)[0]
            m["threshold"] = min(m["threshold"], float(np.nanmin(np.abs(c.astype(np.float64) - float(thr)), initial=np.inf)))
        order = cand[np.lexsort((cand, -c[cand]))]  # confidence descending, then global index ascending
        if len(order):
            m["class"] = min(m["class"], float(gap[img][order].min()))
        d = -np.diff(c[order].astype(np.float64))
        if (d > 0).any():
            m["order"] = min(m["order"], float(d[d > 0].min()))
        kept = np.empty((0, 4), dtype)
        count, at, step = 0, 0, 256
        while at < len(order) and count < rows:  # decode in blocks: most candidates of a large case are never reached
            block = order[at:at + step]
            boxes = _boxes(bottoms, img, block, version, num_class, num_box, biases, mask, anchors_scale, dtype)
            for r, box in zip(block, boxes):
                if count >= rows:
                    break
                v = iou(kept, box)
                if len(v):
                    with np.errstate(all="ignore"):
                        m["iou"] = min(m["iou"], float(np.nanmin(np.abs(v.astype(np.float64) - float(nms)), initial=np.inf)))
                if (v > nms).any():
                    continue
                kept = np.vstack([kept, box[None]])
                out[img, count] = (label[img][r] + 1, c[r], *box)
                count += 1
            at += step
    if margins is not None:
        margins.update(m)
    return out


def trim(out):
    """[n][rows][6] -> one (count, 6) array per image: the rows with a label."""
    return [img[:int((img[:, 0] > 0).sum())] for img in out]


def worst_relative(got, want64):
    """The worst relative deviation of the scores and coordinates of `got` from `want64` (elementwise, relative to |want64|; an exact 0 compares
    absolutely)."""
    a, b = np.asarray(got, np.float64)[..., 1:], np.asarray(want64, np.float64)[..., 1:]
    with np.errstate(all="ignore"):
        return float(np.max(np.abs(a - b) / np.where(b == 0, 1.0, np.abs(b)), initial=0.0))


def parse_param(text):
    """-> [(type, name, bottoms, tops, {id: value or list})] of a .param."""
    tok = text.decode().split("\n")
    out = []
    for line in tok[2:]:
        f = line.split()
        if not f:
            continue
        nb, nt = int(f[2]), int(f[3])
        pd = {}
        for kv in f[4 + nb + nt:]:
            k, v = kv.split("=")
            k = int(k)
            if k <= -23300:
                pd[k] = [float(t) for t in v.split(",")[1:]]
            else:
                pd[k] = float(v) if any(ch in v for ch in ".eE") else int(v)
        out.append((f[0], f[1], f[4:4 + nb], f[4 + nb:4 + nb + nt], pd))
    return out


def shapes(text):
    """{blob: (c, h, w)} of a zoo .param, from the params alone (no weights): the layer types the YOLO nets use."""
    s = {}
    for t, name, bottoms, tops, pd in parse_param(text):
        if t == "Input":
            s[tops[0]] = (pd[2], pd[1], pd[0])
            continue
        c, h, w = s[bottoms[0]]
        if t in ("Convolution", "ConvolutionDepthWise"):
            k, st, p = pd[1], pd.get(3, 1), pd.get(4, 0)
            s[tops[0]] = (pd[0], (h + 2 * p - k) // st + 1, (w + 2 * p - k) // st + 1)
        elif t in ("Deconvolution", "DeconvolutionDepthWise"):
            k, st, p = pd[1], pd.get(3, 1), pd.get(4, 0)
            s[tops[0]] = (pd[0], (h - 1) * st + k - 2 * p + pd.get(18, 0), (w - 1) * st + k - 2 * p + pd.get(19, 0))
        elif t == "Pooling":
            k, st, pl = pd[1], pd.get(2, 1), pd.get(3, 0)
            pr, pt = pd.get(14, pl), pd.get(13, pl)
            pb = pd.get(15, pt)
            s[tops[0]] = (c, -(-(h + pt + pb - k) // st) + 1, -(-(w + pl + pr - k) // st) + 1)
        elif t == "Split":
            for top in tops:
                s[top] = (c, h, w)
        elif t == "Concat":
            s[tops[0]] = (sum(s[b][0] for b in bottoms), h, w)
        elif t == "Reorg":
            st = pd[0]
            s[tops[0]] = (c * st * st, h // st, w // st)
        elif t == "Interp":
            s[tops[0]] = (c, int(h * pd[1]), int(w * pd[2]))
        elif t in ("YoloDetectionOutput", "Yolov3DetectionOutput"):
            s[tops[0]] = None
        else:  # ReLU, BatchNorm, Scale, Eltwise: the bottom's shape
            s[tops[0]] = (c, h, w)
    return s
