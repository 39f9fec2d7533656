"""numpy restatement of include/feather_hip/feather_detect.h, line by line: Permute, Normalize, the softmax along an axis, PriorBox and
DetectionOutput, and `Net`, which runs a .param / .bin pair that holds them (every other layer as tests/atrous_ref.py restates it).

Functions that the header pins to the bit (permute, normalize, priorbox) compute in float32 with every product and sum rounded on its
own.  softmax() and detection_output() take a dtype: float32 is the header's arithmetic with numpy's exp, float64 the yardstick the
tolerances are measured against.  detection_output() also reports how stable the selection is (margins): the smallest distance of a score
from the confidence threshold, of a compared IoU from the NMS threshold, and the smallest non-zero gap between adjacent candidates."""
from __future__ import annotations

import numpy as np

import atrous_ref
from gconv_ref import _Bin, _pool, nerr, parse_param  # noqa: F401

F = np.float32
# the old dimension (w, h, c = 0, 1, 2) behind the new w, h, c
PERMUTE_SOURCE = ((0, 1, 2), (1, 0, 2), (0, 2, 1), (2, 0, 1), (1, 2, 0), (2, 1, 0))


def permute(x, order):
    """x [N][C][H][W] (rank 3) or [N][H][W] (rank 2)."""
    x = np.asarray(x)
    if x.ndim == 3:
        assert order in (0, 1)
        return np.ascontiguousarray(x.transpose(0, 2, 1) if order else x)
    axis = {0: 3, 1: 2, 2: 1}  # numpy axis of the old w, h, c
    sw, sh, sc = PERMUTE_SOURCE[order]
    return np.ascontiguousarray(x.transpose(0, axis[sc], axis[sh], axis[sw]))


def permute_concat(xs):
    return np.concatenate([permute(x, 3).reshape(x.shape[0], -1) for x in xs], axis=1)


def normalize(x, scale, eps, channel_shared=False):
    x = np.asarray(x, F)
    s = np.zeros((x.shape[0],) + x.shape[2:], F)
    for c in range(x.shape[1]):
        s = s + x[:, c] * x[:, c]
    a = F(1) / np.sqrt(s + F(eps))
    scale = np.asarray(scale, F)
    m = np.full(x.shape[1], scale[0], F) if channel_shared else scale
    return (x * a[:, None]) * m[None, :, None, None]


def softmax(x, axis, dtype=np.float64):
    x = np.asarray(x, dtype)
    e = np.exp(x - x.max(axis=axis, keepdims=True))
    return e / e.sum(axis=axis, keepdims=True, dtype=dtype)


def num_prior(num_min, num_max, num_ratios, flip):
    return num_min * (1 + num_ratios * (2 if flip else 1)) + num_max


def priorbox(h, w, image_w, image_h, min_sizes, max_sizes=(), aspect_ratios=(), variances=(0.1, 0.1, 0.2, 0.2), flip=True, clip=False, step_w=0.0,
             step_h=0.0, offset=0.5):
    """-> float32 [2][4 * h * w * num_prior]."""
    mins, maxs, ratios = (np.asarray(v, F).reshape(-1) for v in (min_sizes, max_sizes, aspect_ratios))
    sw = F(step_w) if step_w > 0 else F(image_w) / F(w)
    sh = F(step_h) if step_h > 0 else F(image_h) / F(h)
    iw, ih, half, off = F(image_w), F(image_h), F(0.5), F(offset)
    boxes = []
    for i in range(h):
        for j in range(w):
            cx, cy = (F(j) + off) * sw, (F(i) + off) * sh
            sizes = []
            for k, mn in enumerate(mins):
                sizes.append((mn, mn))
                if maxs.size:
                    e = np.sqrt(mn * maxs[k])
                    sizes.append((e, e))
                for ar in ratios:
                    root = np.sqrt(ar)
                    bw, bh = mn * root, mn / root
                    sizes.append((bw, bh))
                    if flip:
                        sizes.append((bh, bw))
            for bw, bh in sizes:
                boxes.append(((cx - bw * half) / iw, (cy - bh * half) / ih, (cx + bw * half) / iw, (cy + bh * half) / ih))
    row = np.asarray(boxes, F).reshape(-1)
    if clip:
        row = np.minimum(np.maximum(row, F(0)), F(1))
    return np.stack([row, np.tile(np.asarray(variances, F), row.size // 4)])


def decode(prior, loc, dtype):
    """prior [2][4P], loc [4P] -> boxes [P][4]."""
    T = dtype
    p = np.asarray(prior[0], T).reshape(-1, 4)
    v = np.asarray(prior[1], T).reshape(-1, 4)
    l = np.asarray(loc, T).reshape(-1, 4)
    half = T(0.5)
    pw, ph = p[:, 2] - p[:, 0], p[:, 3] - p[:, 1]
    pcx, pcy = (p[:, 0] + p[:, 2]) * half, (p[:, 1] + p[:, 3]) * half
    cx, cy = (v[:, 0] * l[:, 0]) * pw + pcx, (v[:, 1] * l[:, 1]) * ph + pcy
    bw, bh = np.exp(v[:, 2] * l[:, 2]) * pw, np.exp(v[:, 3] * l[:, 3]) * ph
    return np.stack([cx - bw * half, cy - bh * half, cx + bw * half, cy + bh * half], axis=1).astype(T)


def iou(a, b):
    """a [4], b [M][4], in their dtype."""
    T = b.dtype.type
    iw = np.minimum(a[2], b[:, 2]) - np.maximum(a[0], b[:, 0])
    ih = np.minimum(a[3], b[:, 3]) - np.maximum(a[1], b[:, 1])
    inter = np.where((iw <= 0) | (ih <= 0), T(0), iw * ih)
    aa, ab = (a[2] - a[0]) * (a[3] - a[1]), (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    with np.errstate(invalid="ignore", divide="ignore"):
        return inter / (aa + ab - inter)


def _gap(scores):
    d = np.abs(np.diff(np.asarray(scores, np.float64)))
    d = d[d > 0]
    return float(d.min()) if d.size else np.inf


def detection_output(loc, conf, prior, num_class, nms_threshold, nms_top_k, keep_top_k, confidence_threshold, dtype=np.float32, margins=None):
    """loc [N][4P], conf [N][P * num_class], prior [1 or N][2][4P] -> dtype [N][keep_top_k][6], zero rows past an image's count.
    margins: a dict that receives "threshold", "iou" and "gap" (see the module's text), the minima over the batch."""
    T = dtype
    loc, conf, prior = np.asarray(loc), np.asarray(conf), np.asarray(prior)
    n, P = loc.shape[0], loc.shape[1] // 4
    out = np.zeros((n, keep_top_k, 6), T)
    m = {"threshold": np.inf, "iou": np.inf, "gap": np.inf}
    thr_c, thr_n = T(F(confidence_threshold)), T(F(nms_threshold))
    for img in range(n):
        boxes = decode(prior[img if prior.shape[0] > 1 else 0], loc[img], T)
        scores = np.asarray(conf[img], T).reshape(P, num_class)
        m["threshold"] = min(m["threshold"], float(np.abs(scores[:, 1:].astype(np.float64) - float(thr_c)).min()))
        found = []  # (score, class, prior)
        for cls in range(1, num_class):
            s = scores[:, cls]
            cand = np.nonzero(s > thr_c)[0]
            cand = cand[np.lexsort((cand, -s[cand].astype(np.float64)))][:nms_top_k]  # score descending, then prior ascending
            m["gap"] = min(m["gap"], _gap(s[cand]))
            b = boxes[cand]
            alive = np.ones(cand.size, bool)
            for i in range(cand.size):
                if not alive[i]:
                    continue
                found.append((s[cand[i]], cls, cand[i]))
                later = np.nonzero(alive[i + 1:])[0] + i + 1
                if later.size:
                    v = iou(b[i], b[later])
                    ok = np.isfinite(v)
                    if ok.any():
                        m["iou"] = min(m["iou"], float(np.abs(v[ok].astype(np.float64) - float(thr_n)).min()))
                    alive[later[v > thr_n]] = False
        found.sort(key=lambda e: (-float(e[0]), e[1], e[2]))
        m["gap"] = min(m["gap"], _gap([e[0] for e in found]))
        for r, (s, cls, p) in enumerate(found[:keep_top_k]):
            out[img, r] = (T(cls), s) + tuple(boxes[p])
    if margins is not None:
        margins.update(m)
    return out


def trim(rows):
    """[N][keep_top_k][6] -> one (count_i, 6) array per image."""
    return [img[:int((img[:, 0] > 0).sum())] for img in np.asarray(rows)]


# ---- whole nets --------------------------------------------------------------------------------------------------------------------------
class Ranked:
    """A blob with its rank: data [N][C][H][W], dims 1 .. 3."""

    def __init__(self, data, dims=3):
        self.data, self.dims = np.ascontiguousarray(data, F), dims

    def image(self):
        """[N] + the extents of its rank."""
        return self.data.reshape((self.data.shape[0],) + self.data.shape[4 - self.dims:])


def _ranked(image, dims):
    return Ranked(image.reshape((image.shape[0],) + (1,) * (3 - dims) + image.shape[1:]), dims)


class Net:
    """The evaluator of a detection net (Net.SetDetection(True)): the new layers as above -- softmax and DetectionOutput in `dtype` -- and
    Convolution (dilated too), ReLU, Pooling, BatchNorm, Scale and Split as tests/atrous_ref.py's family does (convolutions in float64, every
    blob rounded to float32)."""
    WEIGHTLESS = ("Input", "ReLU", "Pooling", "Split", "Concat", "Softmax", "Permute", "Flatten", "Reshape", "PriorBox", "DetectionOutput")

    def __init__(self, param: bytes, weights: bytes, dtype=np.float32):
        self.layers, self.dtype = parse_param(param), dtype
        mb, self.w = _Bin(weights), {}
        for type_, name, _, _, pd in self.layers:
            if type_ in ("Convolution", "ConvolutionDepthWise"):
                group, kw, k = pd.get(7, 1), pd.get(1, 0), pd.get(0, 0)
                cg = pd.get(6, 0) // k // kw // kw
                wgt = mb.load(k * cg * kw * kw, True).reshape(k, cg, kw, kw)
                self.w[name] = (wgt, mb.load(k, False) if pd.get(5, 0) else None, group)
            elif type_ == "BatchNorm":
                c = pd.get(0, 0)
                slope, mean, var, bias = (mb.load(c, False) for _ in range(4))
                sq = np.sqrt(var + F(pd.get(1, 0.0)), dtype=F)
                self.w[name] = (slope / sq, bias - slope * mean / sq)
            elif type_ == "Scale":
                c = pd.get(0, 0)
                s = mb.load(c, False)
                self.w[name] = (s, mb.load(c, False) if pd.get(1, 0) else None)
            elif type_ == "Normalize":
                self.w[name] = mb.load(pd.get(3, 0), False)
            else:
                assert type_ in self.WEIGHTLESS, type_
        self.read = mb.o
        self.margins = {}

    def run(self, input_name, x, output_name=None, keep=False):
        """-> the output blob's data, or with keep every blob's ([N][C][H][W] arrays) -- and .ranks, their ranks."""
        blobs = {input_name: Ranked(x)}
        for type_, name, bottoms, tops, pd in self.layers:
            if type_ == "Input":
                continue
            a = blobs[bottoms[0]]
            if type_ in ("Convolution", "ConvolutionDepthWise"):
                wgt, b, group = self.w[name]
                s, p, d = pd.get(3, 1), pd.get(4, 0), pd.get(2, 1)
                y = Ranked(atrous_ref.atrous(a.data, wgt, b, group, (s, s), (p, p, p, p), (d, d)))
            elif type_ == "ReLU":
                y = Ranked(np.where(a.data > 0, a.data, F(0)))
            elif type_ == "Pooling":
                y = Ranked(_pool(a.data, pd))
            elif type_ in ("BatchNorm", "Scale"):
                m, b = self.w[name]
                y = a.data * m[None, :, None, None]
                y = Ranked(y if b is None else y + b[None, :, None, None])
            elif type_ == "Split":
                for t in tops:
                    blobs[t] = a
                continue
            elif type_ == "Permute":
                y = _ranked(permute(a.image(), pd.get(0, 0)), a.dims)
            elif type_ == "Flatten":
                y = _ranked(a.data.reshape(a.data.shape[0], -1), 1)
            elif type_ == "Reshape":
                w, h, c = pd.get(0, -233), pd.get(1, -233), pd.get(2, -233)
                old = {0: a.data.shape[3], 1: a.data.shape[2], 2: a.data.shape[1]}
                ext = [old[i] if v == 0 else v for i, v in enumerate((w, h, c)) if v != -233]
                y = _ranked(a.data.reshape([a.data.shape[0]] + ext[::-1]), len(ext))
            elif type_ == "Concat":
                axis = pd.get(0, 0)
                axis = axis + a.dims if axis < 0 else axis
                y = _ranked(np.concatenate([blobs[b].image() for b in bottoms], axis=1 + axis), a.dims)
            elif type_ == "Softmax":
                axis = pd.get(0, 0)
                axis = axis + a.dims if axis < 0 else axis
                y = _ranked(softmax(a.image(), 1 + axis, self.dtype).astype(F), a.dims)
            elif type_ == "Normalize":
                y = Ranked(normalize(a.data, self.w[name], pd.get(2, 1e-4), bool(pd.get(1, 0))))
            elif type_ == "PriorBox":
                im = blobs[bottoms[1]]
                step = lambda v: 0.0 if v == -233 else float(v)
                arr = lambda i: pd.get(i, [])
                rows = priorbox(a.data.shape[2], a.data.shape[3], pd.get(9, 0) if pd.get(9, 0) > 0 else im.data.shape[3],
                                pd.get(10, 0) if pd.get(10, 0) > 0 else im.data.shape[2], arr(0), arr(1), arr(2),
                                [pd.get(3 + k, (0.1, 0.1, 0.2, 0.2)[k]) for k in range(4)], bool(pd.get(7, 1)), bool(pd.get(8, 0)), step(pd.get(11, -233)),
                                step(pd.get(12, -233)), pd.get(13, 0.0))
                y = _ranked(rows[None], 2)
            elif type_ == "DetectionOutput":
                n = a.data.shape[0]
                y = _ranked(detection_output(a.data.reshape(n, -1), blobs[bottoms[1]].data.reshape(n, -1), blobs[bottoms[2]].image(), pd.get(0, 0),
                                             pd.get(1, 0.05), pd.get(2, 300), pd.get(3, 100), pd.get(4, 0.5), self.dtype, self.margins).astype(F), 2)
            else:
                raise RuntimeError(f"layer {type_} is not restated here")
            blobs[tops[0]] = y
        self.ranks = {k: v.dims for k, v in blobs.items()}
        return {k: v.data for k, v in blobs.items()} if keep else blobs[output_name].data
