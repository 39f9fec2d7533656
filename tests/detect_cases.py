"""The tables of the detection tests (tests/test_detect_cpu.py, tests/test_detect_gpu.py, tests/test_detect_contract_cpu.py): the kernel
instantiations of libfeather_detect.so, the shapes the layer tests run, the DetectionOutput cases and the inputs of the net-level tests.

Stability.  A selection can only be compared where it is stable, so every DetectionOutput input built here satisfies, in the float64
restatement (tests/detect_ref.py), all of: no score closer than MARGIN to the confidence threshold, no compared IoU closer than MARGIN to
the NMS threshold, no two distinct adjacent candidates closer than MARGIN.  Exact ties are allowed: the key decides them.  The builders
search seeds upward from their first one until the restatement alone meets this, and assert that one was found; nothing is skipped when
the tests run.  Scores of the C-ABI cases lie on a grid of P values per class with a step of 0.96 / P >= 9e-4, permuted per (image,
class), and the threshold lies half a step from its neighbours: `candidates` of them are above it in every class, exactly.
"""
import functools
import os

import numpy as np

import detect_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "feathercnn_amd", "libfeather_detect.so")
F = np.float32
MARGIN = 1e-4
CHUNK = 1024  # FHIP_DETECT_CHUNK

KERNELS = {"permute_tile_kernel", "permute_generic_kernel", "permute_concat_kernel", "normalize_kernel", "axis_softmax_kernel", "detect_select_kernel",
           "detect_merge_kernel"}


def targets():
    """Every instantiation of the library, by the names fhip_detect_route reports."""
    return {"fhip::permute_tile_kernel", "fhip::permute_generic_kernel", "fhip::permute_concat_kernel", "fhip::normalize_kernel<1>", "fhip::normalize_kernel<4>",
            "fhip::axis_softmax_kernel", "fhip::detect_select_kernel", "fhip::detect_merge_kernel"}


# the layer tests: planes 1x1, 2x3, 5x5 and 19x19 (none a multiple of the 32-wide tile, 19 x 19 = 361 needs twelve of them), channels 1, 12 and
# 63 (63 needs two row tiles), n 1 and 3; (2, 4) and (4, 4) planes of 8 and 16 pixels take Normalize's 16-byte form
PLANES = ((1, 1), (2, 3), (5, 5), (19, 19))
CHANNELS = (1, 12, 63)
BATCHES = (1, 3)
SHAPES = [(n, c, h, w) for n in BATCHES for c in CHANNELS for h, w in PLANES if not (n == 3 and (h, w) == (19, 19) and c != 12)]
NORMALIZE_SHAPES = SHAPES + [(2, 12, 2, 4), (3, 5, 4, 4)]


# ---- DetectionOutput through the C-ABI ---------------------------------------------------------------------------------------------------
# name, P, num_class, n, priorbox n, nms_top_k, keep_top_k, candidates per class, nms_threshold, kind ("random", "same": every prior and
# location equal, so one box suppresses everything; "ties": four score levels)
DETECTION_CASES = [
    ("p1_one", 1, 2, 1, 1, 1, 1, 1, 0.45, "random"),
    ("p1_none", 1, 2, 1, 1, 4, 4, 0, 0.45, "random"),
    ("p63_exactly_top_k", 63, 5, 3, 1, 16, 100, 16, 0.45, "random"),       # keep_top_k above the survivors
    ("p63_more_keep_cuts", 63, 5, 3, 3, 16, 8, 40, 0.45, "random"),        # more candidates than nms_top_k, keep_top_k cuts, priors per image
    ("p97_all", 97, 2, 2, 1, 1024, 1024, 97, 0.45, "random"),
    ("p97_suppressed", 97, 2, 2, 1, 100, 100, 50, 0.45, "same"),
    ("p97_ties", 97, 5, 2, 2, 50, 60, 60, 0.3, "ties"),
    ("p1025_past_a_chunk", CHUNK + 1, 5, 2, 1, 64, 50, 300, 0.45, "random"),
    ("p2600_sort_and_cut", 2600, 2, 1, 1, 100, 100, 2500, 0.45, "random"),  # more candidates than the selection buffer holds at once
    ("p1025_merge_cut", CHUNK + 1, 5, 1, 1, 1024, 1024, 1000, 0.99, "random"),  # more survivors than the merge buffer holds at once
]


def _detection_data(case, seed):
    name, P, C, n, pn, top_k, keep, cand, nms, kind = case
    rng = np.random.default_rng(seed)
    cx, cy = rng.uniform(0.2, 0.8, (pn, P)), rng.uniform(0.2, 0.8, (pn, P))
    bw, bh = rng.uniform(0.1, 0.4, (pn, P)), rng.uniform(0.1, 0.4, (pn, P))
    if kind == "same":
        cx[:], cy[:], bw[:], bh[:] = 0.5, 0.5, 0.3, 0.2
    boxes = np.stack([cx - bw / 2, cy - bh / 2, cx + bw / 2, cy + bh / 2], axis=2).reshape(pn, 4 * P)
    prior = np.stack([boxes, np.tile([0.1, 0.1, 0.2, 0.2], (pn, P))], axis=1).astype(F)
    loc = (np.zeros((n, 4 * P)) if kind == "same" else rng.normal(0, 1, (n, 4 * P))).astype(F)
    grid = 0.02 + 0.96 * (np.arange(P) + 0.5) / P
    if kind == "ties":
        grid = 0.02 + 0.96 * (np.floor(np.arange(P) * 4 / P) + 0.5) / 4  # four levels: exact ties inside each
    conf = np.full((n, P, C), 0.5)
    for i in range(n):
        for c in range(1, C):
            conf[i, :, c] = grid[rng.permutation(P)]
    threshold = 0.02 + 0.96 * (P - cand) / P if kind != "ties" else 0.02 + 0.96 * 0.25  # between the first and the second level: 3/4 of the priors
    return loc, conf.reshape(n, P * C).astype(F), prior, float(F(threshold))


@functools.lru_cache(maxsize=None)
def detection_case(index):
    """-> (case, loc, conf, prior, confidence_threshold, the float64 result, the float32 result, margins) of DETECTION_CASES[index], from the
    first seed whose float64 restatement is stable."""
    case = DETECTION_CASES[index]
    name, P, C, n, pn, top_k, keep, cand, nms, kind = case
    for seed in range(1000 * index, 1000 * index + 40):
        loc, conf, prior, thr = _detection_data(case, seed)
        m = {}
        want64 = R.detection_output(loc, conf, prior, C, nms, top_k, keep, thr, np.float64, m)
        if min(m.values()) >= MARGIN:
            want32 = R.detection_output(loc, conf, prior, C, nms, top_k, keep, thr, np.float32)
            if kind != "ties":
                assert int((conf.reshape(n, P, C)[:, :, 1:] > F(thr)).sum()) == cand * n * (C - 1), name
            return case, loc, conf, prior, thr, want64, want32, m
    raise AssertionError(f"no stable seed for {name}")


def detection_tolerance(want64, want32):
    """Elementwise: the larger of twice the float32 restatement's own worst deviation from float64 on this input and 4 ulp (float32) at the
    value's magnitude -- device expf and numpy's exp each carry about an ulp, scaled by the box extent."""
    own = float(np.abs(want32.astype(np.float64) - want64).max())
    return np.maximum(2 * own, 4 * np.spacing(np.abs(want64).astype(F)).astype(np.float64))


# Reshape extents that do not keep the element count of a 4-element blob [1][2][2]; the first multiplies to 2^64 + 4
BAD_RESHAPES = ("0=968973220 1=49477 2=384773", "0=2147483647 1=2147483647 2=2147483647", "0=2147483647 1=2", "0=3 1=-1", "0=-1 1=3", "0=8", "0=2 1=2 2=2")


def reshape_of_four(params):
    """A .param: Reshape `l` of a 4-element blob ([1][2][2]) and a Concat `c` of its own behind it."""
    lines = ["Input data 0 1 data 0=2 1=2 2=1", f"Reshape l 1 1 data l {params}", "Concat c 1 1 l c 0=0"]
    return ("7767517\n3 3\n" + "\n".join(lines) + "\n").encode()


# ---- net level -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tiny_ssd_model(size=(20, 28)):
    from feathercnn_amd import model_zoo
    return model_zoo.tiny_ssd(size=size)


@functools.lru_cache(maxsize=None)
def tiny_ssd_input(size=(20, 28), batch=3):
    """-> (x, every blob of the float64-softmax restatement, margins): the first seed whose restatement is stable: the margin is a hundred times what
    the device's convolutions and softmax move a score by."""
    p, b, i, o = tiny_ssd_model(size)
    net = R.Net(p, b, np.float64)
    for seed in range(100):
        x = np.random.default_rng(1000 + seed).uniform(-1, 1, (batch, 3) + tuple(size)).astype(F)
        blobs = net.run(i, x, keep=True)
        if min(net.margins.values()) >= MARGIN:
            counts = [len(d) for d in R.trim(blobs[o][:, 0])]
            assert min(counts) >= 1, counts  # every image detects something
            return x, blobs, dict(net.margins)
    raise AssertionError("no stable seed for tiny_ssd")


# MobileNet-SSD from pixels (tests/test_detect_gpu.py): the confidence gain and threshold leave few candidates, far apart
MOBILENET = dict(confidence_threshold=0.7, conf_gain=0.08)
MOBILENET_MEAN, MOBILENET_NORM = 127.5, 1 / 127.5


@functools.lru_cache(maxsize=None)
def mobilenet_ssd_model():
    from feathercnn_amd import model_zoo
    return model_zoo.mobilenet_ssd(**MOBILENET)


@functools.lru_cache(maxsize=None)
def mobilenet_ssd_input(batch=2):
    """-> (uint8 pixels [batch][300][300][3], every blob of the float64-softmax restatement of the whole net, margins): the first pixel seed from
    6 on whose restatement is stable.  A few seconds of numpy per seed."""
    p, b, i, o = mobilenet_ssd_model()
    net = R.Net(p, b, np.float64)
    for seed in range(6, 16):
        px = np.random.default_rng(seed).integers(0, 256, (batch, 300, 300, 3), dtype=np.uint8)
        x = ((px.astype(F) - F(MOBILENET_MEAN)) * F(MOBILENET_NORM)).transpose(0, 3, 1, 2)
        blobs = net.run(i, x, keep=True)
        if min(net.margins.values()) >= MARGIN:
            assert min(len(d) for d in R.trim(blobs[o][:, 0])) >= 1
            return px, blobs, dict(net.margins)
    raise AssertionError("no stable seed for mobilenet_ssd")
