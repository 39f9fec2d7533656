"""The tables of the YOLO tests (tests/test_yolo_cpu.py, tests/test_yolo_gpu.py, tests/test_open_contract_cpu.py): the kernel instantiations of
libfeather_yolo.so, the Reorg shapes, the detection cases and the inputs of the net-level tests.

Stability.  A selection can only be compared where it is stable, so the generator rejects, on the CPU and in float64 (tests/yolo_ref.py), any
draw in which some |confidence - threshold| is below 1e-4, some compared |IoU - nms_threshold| below 1e-3, two candidates' confidences differ
by less than 1e-5 without being equal, or a class leads its runner-up by less than 1e-5.  A rejected draw advances the seed; the seeds that
pass are committed -- seed 0 passes for every case of the table, so SEEDS below holds no exception -- tests/test_yolo_cpu.py asserts that each
case's seed passes and is the first that does, and nothing is skipped on the GPU.

Random heads do not pass these margins at more than a thousand candidates, so the inputs are built backwards from what they should decode to:
  * confidences lie on a grid of one value per box of an image, permuted, with a step of 0.88 / boxes >= 2.2e-4, and the threshold lies half a
    step from its neighbours; the objectness is solved from the grid value and the class factor;
  * the class scores are U(-1, 1) and the label's score is 8 .. 9 (version 2) or 3 .. 4 (version 3);
  * a box sits at the centre of its cell (+- 2 % of the cell) and is either "huge" (50 images wide: any two of them overlap almost fully) or
    tiny (0.012 of the image / 3^box, +- 3 %): tiny boxes of different cells and scales are disjoint, the tiny boxes of one cell overlap by
    about 1 / 9, and a "twin" takes the size of box 0 of its cell and overlaps it almost fully.
"""
import functools
import os

import numpy as np

import yolo_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "feathercnn_amd", "libfeather_yolo.so")
F = np.float32
CHUNK = 1024  # FHIP_YOLO_CHUNK
MARGINS = dict(threshold=1e-4, iou=1e-3, order=1e-5, **{"class": 1e-5})

KERNELS = {"reorg_tile_kernel", "reorg_direct_kernel", "yolo_score_kernel", "yolo_select_kernel"}


def targets():
    """Every instantiation of the library, by the names fhip_yolo_route reports."""
    return {"fhip::reorg_tile_kernel", "fhip::reorg_direct_kernel", "fhip::yolo_score_kernel<2>", "fhip::yolo_score_kernel<3>", "fhip::yolo_select_kernel"}


# (n, c, h, w, stride): even, stride 3, ragged planes (rows and columns past the last whole step are not read), the YOLOv2 passthrough
# plane of 26 x 26 at 64 channels (2 x 26 floats per output row: its 13 rows are one group of a tile), and a 40 x 300 plane: 600 floats per
# output row, 6 rows per tile, so 20 output rows take three whole groups and a ragged one of 2
REORG_SHAPES = [(2, 3, 4, 6, 2), (1, 5, 9, 6, 3), (2, 2, 7, 9, 2), (1, 64, 26, 26, 2), (1, 2, 40, 300, 2)]
# the direct kernel: stride 1, and a plane whose stride * w = 4100 floats pass the tile (ragged in w too)
REORG_DIRECT = [(1, 2, 3, 5, 1), (2, 2, 5, 2050, 2)]

BIASES = [1.5, 2.0, 3.0, 2.5, 2.0, 4.0, 5.0, 3.5, 6.0, 4.5, 7.0, 9.0]  # six anchors
# name -> (extents of the bottoms, num_box, rows, the fraction of boxes above the threshold, the fraction of huge boxes)
SHAPES = {
    "one_3x5": (((3, 5),), 2, 64, 0.5, 0.2),
    "two_4x4_8x8": (((4, 4), (8, 8)), 2, 64, 0.5, 0.2),
    "three_past_a_chunk": (((24, 24), (12, 12), (6, 6)), 2, 64, 0.8, 0.98),  # 1512 boxes, about 1210 candidates, all but some 25 of them suppressed
    # 3840 boxes, 3456 candidates, all but some 60 of them suppressed: four selection rounds, and within a round more keys than the 2048 of the
    # selection buffer, so it is sorted and cut (more than once) and later keys are passed over at the cut's last key
    "two_past_the_buffer": (((32, 32), (16, 16)), 3, 128, 0.9, 0.98),
}
NMS = 0.45


def case_ids():
    return [(version, shape, n, classes) for version in (2, 3) for shape in SHAPES for n in (1, 3) for classes in (1, 3, 80)]


def _logit(p):
    return np.log(p / (1 - p))


def draw(version, shape, n, classes, seed):
    """-> (bottoms, arguments of R.detection) of one draw."""
    extents, num_box, rows, above, huge = SHAPES[shape]
    rng = np.random.default_rng(seed)
    per = sum(num_box * h * w for h, w in extents)
    mask = [(b * num_box + pp + 1) % 6 for b in range(len(extents)) for pp in range(num_box)]
    scale = [float(2 ** (len(extents) - b)) for b in range(len(extents))]
    step = 0.88 / per
    threshold = float(F(0.02 + step * round(per * (1 - above))))
    bottoms, first = [], 0
    grid = np.stack([0.02 + step * (rng.permutation(per) + 0.5) for _ in range(n)])  # [n][per]
    for b, (h, w) in enumerate(extents):
        x = np.zeros((n, num_box, 5 + classes, h, w))
        s = rng.uniform(-1, 1, (n, num_box, classes, h, w))
        lab = rng.integers(0, classes, (n, num_box, 1, h, w))
        np.put_along_axis(s, lab, rng.uniform(8, 9, lab.shape) if version == 2 else rng.uniform(3, 4, lab.shape), axis=2)
        s = s.astype(F).astype(np.float64)
        best = np.take_along_axis(s, lab, axis=2)[:, :, 0]
        factor = 1 / np.exp(s - best[:, :, None]).sum(axis=2) if version == 2 else 1 / (1 + np.exp(-best))
        want = grid[:, first:first + num_box * h * w].reshape(n, num_box, h, w)
        x[:, :, 5:] = s
        x[:, :, 4] = _logit(want / factor)
        x[:, :, 0:2] = _logit(0.5 + rng.uniform(-0.02, 0.02, (n, num_box, 2, h, w)))
        size = 0.012 / 3.0 ** np.arange(num_box).reshape(1, num_box, 1, 1) * np.ones((n, num_box, h, w))
        twin = rng.uniform(0, 1, (n, 1, h, w)) < 0.3
        size[:, 1:] = np.where(twin, size[:, :1], size[:, 1:])
        size = np.where(rng.uniform(0, 1, (n, num_box, h, w)) < huge, 50.0, size)
        for k, cells in ((2, w), (3, h)):
            anchor = np.asarray([BIASES[2 * (pp if version == 2 else mask[b * num_box + pp]) + k - 2] for pp in range(num_box)]).reshape(1, num_box, 1, 1)
            x[:, :, k] = np.log(size * rng.uniform(0.97, 1.03, size.shape) * cells * (1.0 if version == 2 else scale[b]) / anchor)
        bottoms.append(x.reshape(n, num_box * (5 + classes), h, w).astype(F))
        first += num_box * h * w
    args = dict(version=version, num_class=classes, num_box=num_box, biases=BIASES, confidence_threshold=threshold, nms_threshold=NMS, rows=rows)
    if version == 3:
        args.update(mask=mask, anchors_scale=scale)
    return bottoms, args


def stable(m):
    return all(m[k] >= MARGINS[k] for k in MARGINS)


def first_stable_seed(version, shape, n, classes, start=0, tries=20):
    """The first seed from `start` whose draw passes the margins, in float64, with the margins and the float64 result."""
    for seed in range(start, start + tries):
        bottoms, args = draw(version, shape, n, classes, seed)
        m = {}
        want64 = R.detection(bottoms, dtype=np.float64, margins=m, **args)
        if stable(m):
            return seed, bottoms, args, want64, m
    raise AssertionError(f"no stable seed for {(version, shape, n, classes)}")


# case -> its seed where that is not 0 (first_stable_seed() of the case from 0).  Seed 0 passes the margins for every case of the table, so
# there is no entry; tests/test_yolo_cpu.py asserts it case by case
SEEDS = {}


@functools.lru_cache(maxsize=None)
def case(version, shape, n, classes):
    """-> (bottoms, arguments, the float64 result, the float32 result, margins) of a case at its committed seed."""
    bottoms, args = draw(version, shape, n, classes, SEEDS.get((version, shape, n, classes), 0))
    m = {}
    want64 = R.detection(bottoms, dtype=np.float64, margins=m, **args)
    want32 = R.detection(bottoms, dtype=np.float32, **args)
    return bottoms, args, want64, want32, m


def tolerance(want64, want32):
    """Relative: max(8 x e32, 2^-20), e32 the float32 restatement's own worst relative error against float64 on the case: the device's expf is
    good to 1 - 2 ulp where numpy's is correctly rounded, through a chain of about six rounded operations."""
    e32 = R.worst_relative(want32, want64)
    return max(8 * e32, 2.0 ** -20), e32


# ---- net level -------------------------------------------------------------------------------------------------------------------------
NETS = {"tiny_yolov2": dict(size=(12, 20), heads=("head",), seed=0), "tiny_yolov3": dict(size=(16, 24), heads=("head1", "head2"), seed=0)}


@functools.lru_cache(maxsize=None)
def net_model(name):
    """-> ((param, bin, input, output), the trace for model_zoo.numpy_forward)."""
    from feathercnn_amd import model_zoo
    trace = []
    return model_zoo.MODELS[name](trace=trace), trace


def head_args(param):
    """The arguments of R.detection a net's detection layer holds (rows excepted), read out of its .param."""
    t, _, bottoms, _, pd = [l for l in R.parse_param(param) if l[0] in ("YoloDetectionOutput", "Yolov3DetectionOutput")][0]
    args = dict(version=3 if t == "Yolov3DetectionOutput" else 2, num_class=pd[0], num_box=pd[1], confidence_threshold=pd[2], nms_threshold=pd[3], biases=pd[-23304])
    if args["version"] == 3:
        args.update(mask=[int(v) for v in pd[-23305]], anchors_scale=pd[-23306])
    return bottoms, args


@functools.lru_cache(maxsize=None)
def net_input(name, batch=3, rows=16):
    """-> (x, the heads of the numpy forward, the float64 detections of those heads, margins): the first input seed from the committed one whose
    restatement passes the margins on the net's head input."""
    from feathercnn_amd import model_zoo
    (p, b, i, o), trace = net_model(name)
    heads, args = head_args(p)
    for seed in range(NETS[name]["seed"], NETS[name]["seed"] + 40):
        x = np.random.default_rng(2000 + seed).uniform(-1, 1, (batch, 3) + NETS[name]["size"]).astype(F)
        blobs = model_zoo.numpy_forward(trace, i, x)
        m = {}
        want64 = R.detection([blobs[h] for h in heads], rows=rows, dtype=np.float64, margins=m, **args)
        if stable(m) and min(len(d) for d in R.trim(want64)) >= 1:
            return x, {h: blobs[h] for h in heads}, want64, m
    raise AssertionError(f"no stable input for {name}")
