"""The tables of the two-stage detection tests (tests/test_roi_cpu.py, tests/test_roi_gpu.py, tests/test_open_contract_cpu.py): the kernel
instantiations of libfeather_roi.so, the Proposal cases, the ROI layers' cases and the inputs of the net-level tests.

Stability.  A selection can only be compared where it is stable, so the generator rejects, on the CPU and in float64 (tests/roi_ref.py), any
draw in which some |extent - min box size| is below 1e-3 px or some compared |IoU - nms_thresh| is below 1e-3.  A rejected draw advances the
seed; the seeds that pass are committed (SEEDS: no entry = seed 0), tests/test_roi_cpu.py asserts that each case's seed passes and is the
first that does, and nothing is skipped on the GPU.  Scores are distinct values of a grid, permuted: they are moved, never computed, so the
order is exact.

Random deltas do not pass the IoU margin at thousands of candidates, so the inputs are built backwards from the boxes they should decode to:
  * the cells of a b x b block share one centre, the block's (+- 0.25 px), and anchor q takes the size class q % 3 -- 40, 28 or 19 px, square:
    boxes of one block and class overlap by at least 0.74 and suppress each other, boxes of different classes or blocks by at most 0.53;
  * a small share of the anchors are "late": a box of 6 px at the centre of the anchor's own cell, disjoint from the late boxes of other cells
    (two of one cell overlap by 0.58), with a score among the lowest 30 %: they survive the NMS, lie behind the default pre_nms_topN on the
    largest map, and are no candidates at min_size 16;
  * the deltas are solved from the target box in float64 and rounded to float32.
"""
import functools
import os

import numpy as np

import roi_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "feathercnn_amd", "libfeather_roi.so")
F = np.float32
CHUNK = 1024  # FHIP_ROI_CHUNK
MARGINS = dict(extent=1e-3, iou=1e-3)
NMS = 0.7
FEAT_STRIDE = 16

KERNELS = {"proposal_key_kernel", "proposal_select_kernel", "roi_pool_kernel", "roi_align_kernel", "psroi_pool_kernel"}
KEYS, SELECT, POOL, ALIGN, PSROI = range(1, 6)  # fhip_roi_op


def targets():
    """Every instantiation of the library, by the names fhip_roi_route reports."""
    return {"fhip::proposal_key_kernel", "fhip::proposal_select_kernel", "fhip::roi_pool_kernel", "fhip::roi_align_kernel<0>", "fhip::roi_align_kernel<1>",
            "fhip::psroi_pool_kernel"}


# ---- Proposal ----------------------------------------------------------------------------------------------------------------------------------
# name -> (h, w, the block of cells that share a centre, the share of late anchors): 135 anchors; 1728, past one selection chunk; 6912, past the selection
# buffer of two, so that it is sorted and cut, and past the default pre_nms_topN = 6000
MAPS = {"3x5": (3, 5, 1, 0.03), "12x16": (12, 16, 2, 0.03), "24x32": (24, 32, 4, 0.015)}
SIZES = (40.0, 28.0, 19.0)
# (map, n, pre_nms_topN, after_nms_topN, min_size, im_scale): every value of every axis, the large map where it matters
CASES = [("3x5", 1, 0, 16, 0, 1.0), ("3x5", 3, 100, 300, 16, 1.0), ("3x5", 1, 6000, 300, 16, 1.6),
         ("12x16", 1, 6000, 300, 0, 1.0), ("12x16", 3, 0, 16, 16, 1.0), ("12x16", 1, 100, 16, 0, 1.0), ("12x16", 3, 100, 300, 16, 1.0),
         ("24x32", 1, 6000, 300, 0, 1.0), ("24x32", 1, 0, 300, 0, 1.0), ("24x32", 3, 6000, 16, 16, 1.0), ("24x32", 1, 100, 300, 16, 1.0)]


def case_id(c):
    return "%s-n%d-pre%d-after%d-min%d-scale%g" % c


def draw(shape, n, seed, im_scale=1.0):
    """-> (score [n][18][h][w], bbox [n][36][h][w], im_info [n][3]) of one draw."""
    h, w, block, late = MAPS[shape]
    rng = np.random.default_rng(seed)
    a = R.generate_anchors().astype(np.float64)
    A, per = len(a), len(a) * h * w
    q, i, j = np.meshgrid(np.arange(A), np.arange(h), np.arange(w), indexing="ij")
    score = np.zeros((n, 2 * A, h, w), F)
    bbox = np.zeros((n, A, 4, h, w), F)
    for img in range(n):
        is_late = rng.uniform(0, 1, (A, h, w)) < late
        # the centre: the block's (the cells of a ragged last block share theirs too), or the cell's own for a late box
        cx = np.where(is_late, 16.0 * j + 8, 16.0 * block * (j // block) + 8.0 * min(block, w)) + np.where(is_late, 0, rng.uniform(-0.25, 0.25, (A, h, w)))
        cy = np.where(is_late, 16.0 * i + 8, 16.0 * block * (i // block) + 8.0 * min(block, h)) + np.where(is_late, 0, rng.uniform(-0.25, 0.25, (A, h, w)))
        size = np.where(is_late, 6.0, np.asarray(SIZES)[q % 3])
        aw, ah = (a[:, 2] - a[:, 0]).reshape(A, 1, 1), (a[:, 3] - a[:, 1]).reshape(A, 1, 1)
        acx, acy = a[:, 0].reshape(A, 1, 1) + 16.0 * j + aw * 0.5, a[:, 1].reshape(A, 1, 1) + 16.0 * i + ah * 0.5
        bbox[img, :, 0], bbox[img, :, 1] = (cx - acx) / aw, (cy - acy) / ah
        bbox[img, :, 2], bbox[img, :, 3] = np.log(size / aw), np.log(size / ah)
        key = rng.uniform(0, 1, per) * np.where(is_late.reshape(-1), 0.3, 1.0)
        rank = np.argsort(np.argsort(key))
        score[img, A:] = ((rank + 0.5) / per).reshape(A, h, w)
        score[img, :A] = 1 - score[img, A:]  # the background planes: never read
    im_info = np.tile(np.asarray([16.0 * h, 16.0 * w, im_scale], F), (n, 1))
    return score, bbox.reshape(n, 4 * A, h, w), im_info


def args_of(c):
    shape, n, pre, after, min_size, im_scale = c
    return dict(feat_stride=FEAT_STRIDE, pre_nms_topN=pre, after_nms_topN=after, nms_thresh=NMS, min_size=min_size)


def stable(m):
    return all(m[k] >= MARGINS[k] for k in MARGINS)


def first_stable_seed(c, start=0, tries=20):
    """The first seed from `start` whose draw passes the margins, in float64, with the inputs, the float64 result and the margins."""
    for seed in range(start, start + tries):
        inputs = draw(c[0], c[1], seed, c[5])
        m = {}
        want64 = R.proposal(*inputs, dtype=np.float64, margins=m, **args_of(c))
        if stable(m):
            return seed, inputs, want64, m
    raise AssertionError(f"no stable seed for {c}")


# case -> its seed where that is not 0 (first_stable_seed() of the case from 0); tests/test_roi_cpu.py asserts it case by case
SEEDS = {}


@functools.lru_cache(maxsize=None)
def case(c):
    """-> (inputs, arguments, (rois, scores) in float64, the same in float32, margins) of a case at its committed seed."""
    inputs = draw(c[0], c[1], SEEDS.get(c, 0), c[5])
    m = {}
    want64 = R.proposal(*inputs, dtype=np.float64, margins=m, **args_of(c))
    want32 = R.proposal(*inputs, dtype=np.float32, **args_of(c))
    return inputs, args_of(c), want64, want32, m


def tolerance(want64, want32, im_info):
    """Relative to the larger image extent: max(8 x e32, 2^-20), e32 the float32 restatement's own worst error against float64 on the case: the
    device's expf is good to 1 - 2 ulp where numpy's is correctly rounded, through a chain of about six rounded operations."""
    e32 = R.worst_coordinate_error(want32[0], want64[0], im_info)
    return max(8 * e32, 2.0 ** -20), e32


# ---- the ROI layers ----------------------------------------------------------------------------------------------------------------------------
FEATURES = (2, 37, 9, 13)
PS_FEATURES = (1, 18, 6, 6)  # output_dim 2, 3 x 3
ROIS = 64
# (pooled_w, pooled_h, spatial_scale)
POOLED = [(7, 7, 0.0625), (3, 2, 0.25), (1, 1, 0.25), (7, 7, 0.25)]
# (version, aligned, sampling_ratio, pooled_w, pooled_h, spatial_scale): every combination
ALIGN_CASES = [(v, a, s) + p for v in (0, 1) for a in (0, 1) for s in (0, 2) for p in POOLED]
PS_CASES = [(3, 3, 0.0625), (3, 3, 0.25)]


@functools.lru_cache(maxsize=None)
def features(shape=FEATURES):
    return np.random.default_rng(sum(shape)).uniform(-1, 1, shape).astype(F)


@functools.lru_cache(maxsize=None)
def rois(shape, scale):
    """[n][ROIS][4] for a map `shape` at `scale`: the hand-made ROIs first -- outside the image, inverted, zero-sized, on the border, the sentinel,
    the whole map, inside one pixel, halves that roundf sends away from zero -- then random ones that reach over every border."""
    n, _, h, w = shape
    W, H = w / scale, h / scale
    px = 1 / scale
    special = [(0, 0, -1, -1), (0, 0, W, H), (0, 0, W - 1, H - 1), (0, 0, 0, 0), (W - 1, H - 1, W - 1, H - 1), (W, H, W, H),
               (W + 3 * px, H + 2 * px, W + 9 * px, H + 7 * px), (-9 * px, -7 * px, -2 * px, -3 * px), (-5 * px, 2 * px, 3 * px, H + 4 * px),
               (0.6 * W, 0.7 * H, 0.2 * W, 0.1 * H), (0.5 * W, 0.2 * H, 0.5 * W - 2 * px, 0.9 * H), (3.3 * px, 2.2 * px, 3.3 * px, 2.2 * px),
               (4.2 * px, 3.3 * px, 4.6 * px, 3.8 * px), (2.5 * px, 1.5 * px, 6.5 * px, 4.5 * px), (0.5 * px, 0.5 * px, W - 0.5 * px, H - 0.5 * px),
               (-2 * W, -2 * H, 3 * W, 3 * H), (1.25 * px, 0, 1.75 * px, H), (0, H - px, W, H)]
    rng = np.random.default_rng(int(1000 * scale) + h * w)
    out = np.empty((n, ROIS, 4), F)
    for i in range(n):
        x1, y1 = rng.uniform(-0.2 * W, W, ROIS), rng.uniform(-0.2 * H, H, ROIS)
        out[i, :, 0], out[i, :, 1] = x1, y1
        out[i, :, 2], out[i, :, 3] = x1 + rng.uniform(-0.05, 0.8, ROIS) * W, y1 + rng.uniform(-0.05, 0.8, ROIS) * H
        k = len(special) if i == 0 else len(special) // 2
        out[i, :k] = np.roll(np.asarray(special, F), i, axis=0)[:k]
    return out


@functools.lru_cache(maxsize=None)
def pool_case(cfg):
    pw, ph, scale = cfg
    x, r = features(), rois(FEATURES, scale)
    return x, r, R.roi_pool(x, r, pw, ph, scale)


@functools.lru_cache(maxsize=None)
def align_case(cfg):
    version, aligned, sampling, pw, ph, scale = cfg
    x, r = features(), rois(FEATURES, scale)
    return x, r, R.roi_align(x, r, pw, ph, scale, sampling, aligned, version)


@functools.lru_cache(maxsize=None)
def psroi_case(cfg):
    pw, ph, scale = cfg
    x, r = features(PS_FEATURES), rois(PS_FEATURES, scale)
    return x, r, R.psroi_pool(x, r, 2, pw, ph, scale)


# ---- net level -------------------------------------------------------------------------------------------------------------------------------
NETS = {"tiny_faster_rcnn": dict(size=(48, 64), seed=0), "tiny_rfcn": dict(size=(48, 64), seed=0)}
NET_ROIS = 16  # after_nms_topN of the tiny nets


@functools.lru_cache(maxsize=None)
def net_model(name):
    """-> ((param, bin, inputs, outputs), the trace for model_zoo.numpy_forward)."""
    from feathercnn_amd import model_zoo
    trace = []
    return model_zoo.MODELS[name](trace=trace), trace


def proposal_args(param):
    """The arguments of R.proposal a net's Proposal layer holds, read out of its .param, and the layer's bottoms and tops."""
    t, _, bottoms, tops, pd = [l for l in R.parse_param(param) if l[0] == "Proposal"][0]
    return bottoms, tops, dict(anchors=R.generate_anchors(pd.get(1, 16)), feat_stride=pd.get(0, 16), pre_nms_topN=pd.get(2, 6000), after_nms_topN=pd.get(3, 300), nms_thresh=pd.get(4, 0.7), min_size=pd.get(5, 16))


@functools.lru_cache(maxsize=None)
def net_input(name, batch=3):
    """-> (x, im_info, every blob of the numpy forward, margins): the first input seed from the committed one whose Proposal passes the margins
    on the net's own head and proposes at least two ROIs per image.  Behind convolutions the scores are computed, not moved, and the ROI layers
    round the coordinates, so two more margins are asked here: adjacent candidates' scores differ by 1e-5 ("order"), and no ROI coordinate, raw
    or scaled, lies within 1e-3 of a half ("round")."""
    from feathercnn_amd import model_zoo
    (p, b, i, o), trace = net_model(name)
    (score, bbox, _), tops, args = proposal_args(p)
    hh, ww = NETS[name]["size"]
    info = np.tile(np.asarray([hh, ww, 1.0], F), (batch, 1)).reshape(batch, 1, 1, 3)
    for seed in range(NETS[name]["seed"], NETS[name]["seed"] + 40):
        x = np.random.default_rng(3000 + seed).uniform(-1, 1, (batch, 3, hh, ww)).astype(F)
        blobs = model_zoo.numpy_forward(trace, {"data": x, "im_info": info})
        m = {}
        want64 = R.proposal(blobs[score], blobs[bbox], info, dtype=np.float64, margins=m, **args)
        real = np.concatenate(R.trim(want64[0])).reshape(-1)
        m["round"] = float(min(np.abs(v - np.floor(v) - 0.5).min() for v in (real, real * 0.25)))
        if stable(m) and m["order"] >= 1e-5 and m["round"] >= 1e-3 and min(R.counts(want64[0])) >= 2:
            return x, info, blobs, m
    raise AssertionError(f"no stable input for {name}")
