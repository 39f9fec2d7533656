"""libfeather_detect.so and the detection layers of the Net runtime on the device, against tests/detect_ref.py.

* Permute (all six orders, both ranks), Normalize (both scale forms) and the fused permute-concat equal numpy exactly at planes 1x1, 2x3,
  5x5 and 19x19, channels 1, 12 and 63, n 1 and 3, from 16-byte aligned and from misaligned guarded buffers (tests/guarded.py); the strided
  softmax meets the bound of fhip_softmax's own test (tests/test_net_gpu.py::test_softmax: normalised error <= 1e-6 against float64).
* Concat on every rank and axis through a net, exact; rank 3 / axis 0 equal to the default net's Concat bit for bit.
* DetectionOutput through the C-ABI on the cases of tests/detect_cases.py: labels and row order exact; scores and coordinates within
  detect_cases.detection_tolerance of the float64 restatement.
* one kernel trace: the sweep launches every instantiation.
* tiny_ssd at fusion 0, 1, 2, in a captured graph and in 2 sub-batch replicas, re-planned across input sizes and batches; MobileNet-SSD
  from pixels at batch 2; a missing libfeather_detect.so.
"""
import glob
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import detect_cases as DC
import detect_ref as R
import detect_sweep as SW
import kernel_instances as KI
import ktrace
import side_contract
from feathercnn_amd import _lib

pytestmark = pytest.mark.gpu
F = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def lib(cuda):
    return side_contract.library("detect")


def _x(shape, seed=0):
    return np.random.default_rng(seed).uniform(-1, 1, shape).astype(F)


# ---- the layers through the C-ABI --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("order", range(6))
def test_permute_is_exact(lib, order, offset):
    for i, shape in enumerate(DC.SHAPES):
        x = _x(shape, i)
        got = SW.permute(lib, x, order, offset)
        assert np.array_equal(got, R.permute(x, order)), (order, shape)
        n, c, h, w = shape
        assert SW.route(lib, 0, order, 3, c, h, w) == ("fhip::permute_tile_kernel" if order in (1, 3) else "fhip::permute_generic_kernel")
        if order < 2 and c == 12:  # rank 2: (h, w) = (c * h, w) of the same data
            x2 = x.reshape(n, c * h, w)
            assert np.array_equal(SW.permute(lib, x2, order, offset), R.permute(x2, order)), (order, x2.shape)


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("shared", [False, True])
def test_normalize_is_exact(lib, shared, offset):
    routes = set()
    for i, shape in enumerate(DC.NORMALIZE_SHAPES):
        x = _x(shape, 10 + i)
        if i == 0:
            x[0, :, 0, 0] = 0  # an all-zero pixel: eps alone under the root
        scale = np.random.default_rng(i).uniform(0.5, 20, 1 if shared else shape[1]).astype(F)
        named = []
        got = SW.normalize(lib, x, scale, 1e-10, shared, offset, named)
        want = R.normalize(x, scale, 1e-10, shared)
        assert np.array_equal(got, want), (shape, int((got != want).sum()), float(np.abs(got - want).max()))
        assert named == ["fhip::normalize_kernel<%d>" % (4 if offset == 0 and (shape[2] * shape[3]) % 4 == 0 else 1)], (shape, named)
        routes.add(named[0][-3:])
    assert routes == ({"<4>", "<1>"} if offset == 0 else {"<1>"})


@pytest.mark.parametrize("offset", [0, 1])
def test_axis_softmax_meets_the_bound_of_fhip_softmax(lib, offset):
    for i, shape in enumerate(DC.SHAPES):
        x = (_x(shape, 20 + i) * 8).astype(F)  # U(-8, 8), as tests/test_net_gpu.py::test_softmax draws it
        for axis in (1, 2, 3):
            got = SW.axis_softmax(lib, x, axis, offset)
            assert R.nerr(got, R.softmax(x, axis)) <= 1e-6, (shape, axis)


@pytest.mark.parametrize("offset", [0, 1])
def test_permute_concat_is_exact(lib, offset):
    for n in DC.BATCHES:
        xs = [_x((n, c, h, w), c + h) for c, (h, w) in zip((12, 63, 1, 12, 63, 12, 1, 63), DC.PLANES * 2)]
        for k in (1, 3, 8):
            assert np.array_equal(SW.permute_concat(lib, xs[:k], offset), R.permute_concat(xs[:k])), (n, k)


@pytest.mark.parametrize("index", range(len(DC.DETECTION_CASES)), ids=[c[0] for c in DC.DETECTION_CASES])
def test_detection_output(lib, index):
    case, loc, conf, prior, thr, want64, want32, margins = DC.detection_case(index)
    assert min(margins.values()) >= DC.MARGIN, margins  # asserted where the table is built; nothing is skipped here
    got = SW.detection_output(lib, case, loc, conf, prior, thr, offset=index % 2)
    assert np.array_equal(got[:, :, 0], want64[:, :, 0]), (case[0], "labels or row order")
    counts = [len(d) for d in R.trim(want64)]
    assert not got[np.arange(got.shape[1])[None, :] >= np.asarray(counts)[:, None]].any(), "rows past the count are zero"
    err = np.abs(got.astype(np.float64) - want64)
    tol = DC.detection_tolerance(want64, want32)
    print(f"{case[0]}: counts {counts}, worst deviation from float64 {err.max():.3g} (float32 restatement: {np.abs(want32 - want64).max():.3g})")
    assert (err <= tol).all(), (case[0], float(err.max()), float((err - tol).max()))


def test_detection_output_refusals(lib):
    import ctypes
    n = ctypes.c_size_t()
    for args in ((1, 0, 2, 1, 1), (1, 1, 1, 1, 1), (1, 1, 257, 1, 1), (1, 1, 2, 1025, 1), (1, 1, 2, 1, 0), (65536, 1, 2, 1, 1), (1, (1 << 22) + 1, 2, 1, 1)):
        assert lib.fhip_detection_output_get_buffer_size(*args, ctypes.byref(n)) == side_contract.BADARG, args
    assert lib.fhip_detection_output_get_buffer_size(32, 24564, 256, 1024, 1024, ctypes.byref(n)) == 0 and n.value > 0  # the limits the header states


def test_the_sweep_launches_every_instantiation(cuda, tmp_path):
    """One child under rocprofv3 --kernel-trace (tests/detect_trace_child.py): the sweep launches every instantiation tests/detect_cases.targets()
    names -- which is every instantiation the library holds (tests/test_detect_contract_cpu.py)."""
    _, rows, _ = ktrace.trace("detect_trace_child.py", [], tmp_path, 240)
    launched = {KI.normalise(name) for _, name, *_ in rows}
    missing = sorted(DC.targets() - launched)
    assert launched and not missing, (missing, sorted(launched))


# ---- Concat on every rank and axis, through a net ------------------------------------------------------------------------------------------
def _concat_net(rank, axis, detection=True):
    from feathercnn_amd import model_zoo
    from feathercnn_amd.net import Net
    g = model_zoo.GraphBuilder(3)
    a, b, c = g.split("split", g.input("data", 5, 3, 4), 3)
    tops = [a, g.relu("relu", b), g.pool("pool", c, 1, 1)]  # three blobs of their own: the values, their ReLU, a copy
    if rank == 2:
        tops = [g.reshape(f"r{i}", t, 4, 15) for i, t in enumerate(tops)]
    elif rank == 1:
        tops = [g.flatten(f"f{i}", t) for i, t in enumerate(tops)]
    g.concat("out", tops, axis)
    p, w = g.finish()
    net = Net()
    net.SetDetection(detection)
    net.LoadParam(p)
    net.LoadWeights(w)
    return net


@pytest.mark.parametrize("rank,axis", [(3, 0), (3, 1), (3, 2), (3, -1), (2, 0), (2, 1), (2, -2), (1, 0), (1, -1)])
def test_concat_on_every_rank_and_axis(cuda, rank, axis):
    x = _x((3, 5, 3, 4), rank)
    net = _concat_net(rank, axis)
    net.FeedInput("data", x)
    net.Forward()
    got = net.Extract("out")
    parts = [x, np.maximum(x, 0), x]
    image = {3: lambda a: a, 2: lambda a: a.reshape(3, 15, 4), 1: lambda a: a.reshape(3, 60)}[rank]
    want = np.concatenate([image(a) for a in parts], axis=1 + (axis + rank if axis < 0 else axis))
    assert got.size == want.size and np.array_equal(got.reshape(want.shape), want)
    assert dict((nm, a) for _, nm, a in net.layers())["out"] == "DETECT"
    if (rank, axis) == (3, 0):  # what the default net's Concat gives, bit for bit, and the same shape
        plain = _concat_net(3, 0, detection=False)
        plain.FeedInput("data", x)
        plain.Forward()
        assert got.shape == plain.Extract("out").shape and np.array_equal(got, plain.Extract("out"))


@pytest.mark.parametrize("params", DC.BAD_RESHAPES)
def test_reshape_that_changes_the_element_count_is_minus_300(cuda, params):
    """Extents of up to 2^31 each whose product is not the 4 elements of the bottom -- the first multiplies to 2^64 + 4, which a wrapped 64-bit
    product would take for 4 -- are refused at Reshape, before any layer behind sees the view."""
    from feathercnn_amd import FeatherHipError
    from feathercnn_amd.net import Net
    net = Net()
    net.SetDetection(True)
    net.LoadParam(DC.reshape_of_four(params))
    net.LoadWeights(b"")
    net.FeedInput("data", np.ones((1, 1, 2, 2), F))
    with pytest.raises(FeatherHipError) as e:
        net.Forward()
    assert "code -300" in str(e.value) and "layer l" in str(e.value) and "element count" in str(e.value), str(e.value)
    good = Net()
    good.SetDetection(True)
    good.LoadParam(DC.reshape_of_four("0=-1 1=2"))
    good.LoadWeights(b"")
    good.FeedInput("data", np.arange(4, dtype=F).reshape(1, 1, 2, 2))
    good.Forward()
    assert good.Extract("c").shape == (1, 1, 2, 2) and good.Extract("c").reshape(-1).tolist() == [0, 1, 2, 3]


# ---- tiny_ssd ----------------------------------------------------------------------------------------------------------------------------
NET_BLOBS = ("conv2_norm", "mbox_loc", "mbox_conf", "mbox_conf_flatten", "mbox_priorbox", "detection_out")


def _tiny(level, graph=False, replicas=1):
    from feathercnn_amd.net import Net
    p, b, _, _ = DC.tiny_ssd_model()
    net = Net(fusion=level, graph=graph, sub_batches=replicas)
    net.SetDetection(True)
    net.LoadParam(p)
    net.LoadWeights(b)
    return net


def _check_tiny(net, size, batch, replicas=1):
    """Feed the stable input of (size, batch), run, and hold every stage to the restatement; -> the extracted blobs."""
    x, want, margins = DC.tiny_ssd_input(size, batch)
    assert min(margins.values()) >= DC.MARGIN
    net.FeedInput("data", x)
    net.Forward()
    got = {k: net.Extract(k) for k in NET_BLOBS}
    prior = got["mbox_priorbox"][:1] if replicas > 1 else got["mbox_priorbox"]  # one set of priors per replica
    assert np.array_equal(prior, want["mbox_priorbox"])  # shapes only: exact
    for k in ("conv2_norm", "mbox_loc", "mbox_conf", "mbox_conf_flatten"):  # behind device convolutions: the project's net-level bound
        assert got[k].shape == want[k].shape and R.nerr(got[k], want[k]) <= 1e-4, (k, R.nerr(got[k], want[k]))
    # the whole net against the restatement: the same detections in the same order
    assert got["detection_out"].shape == want["detection_out"].shape == (batch, 1, 20, 6)
    assert np.array_equal(got["detection_out"][:, 0, :, 0], want["detection_out"][:, 0, :, 0]), "labels or row order"
    assert np.abs(got["detection_out"] - want["detection_out"]).max() <= 1e-4
    # the layer from its own inputs, at its own tolerance
    n = batch
    args = (got["mbox_loc"].reshape(n, -1), got["mbox_conf_flatten"].reshape(n, -1), prior[:, 0], 3, 0.45, 40, 20, 0.95)
    m = {}
    w64, w32 = R.detection_output(*args, np.float64, m), R.detection_output(*args, np.float32)
    assert min(m.values()) >= DC.MARGIN / 2, m
    assert np.array_equal(got["detection_out"][:, 0, :, 0], w64[:, :, 0])
    assert (np.abs(got["detection_out"][:, 0].astype(np.float64) - w64) <= DC.detection_tolerance(w64, w32)).all()
    dets = net.ExtractDetections("detection_out")
    assert [d.shape for d in dets] == [d.shape for d in R.trim(w64)] and all(np.array_equal(a, b) for a, b in zip(dets, R.trim(got["detection_out"][:, 0])))
    return got


@pytest.fixture(scope="module")
def level0(cuda):
    return _check_tiny(_tiny(0), (20, 28), 3)


@pytest.mark.parametrize("level,graph,replicas", [(1, False, 1), (2, False, 1), (2, True, 1), (2, False, 2), (0, True, 2)])
def test_tiny_ssd_at_every_level_equals_level_0_bit_for_bit(level0, level, graph, replicas):
    net = _tiny(level, graph, replicas)
    got = _check_tiny(net, (20, 28), 3, replicas)
    if graph:  # replay the captured graph
        net.Forward()
        assert np.array_equal(net.Extract("detection_out"), got["detection_out"])
    for k in NET_BLOBS:
        if not (replicas > 1 and k == "mbox_priorbox"):
            assert np.array_equal(got[k], level0[k]), k
    names = [nm for _, nm, _ in net.layers()]
    assert ("mbox_loc" in names) and (("conv3_mbox_loc_perm" in names) == (level < 2))
    if level == 2:
        from feathercnn_amd import FeatherHipError
        with pytest.raises(FeatherHipError, match="fused"):
            net.Extract("conv3_mbox_loc_perm")


def test_tiny_ssd_replans_across_sizes_and_batches(cuda):
    for level, graph in ((2, True), (0, False)):
        net = _tiny(level, graph)
        first = _check_tiny(net, (20, 28), 3)
        other = _check_tiny(net, (24, 20), 2)  # 12 x 10, 6 x 5 and 3 x 3 cells: 576 priors instead of 678
        assert other["mbox_priorbox"].shape[3] == 4 * (120 * 3 + 30 * 6 + 9 * 4) and first["mbox_priorbox"].shape[3] == 4 * 678
        _check_tiny(net, (20, 28), 1)
        again = _check_tiny(net, (20, 28), 3)
        assert all(np.array_equal(again[k], first[k]) for k in NET_BLOBS)


# ---- MobileNet-SSD from pixels -------------------------------------------------------------------------------------------------------------
def _priors_of(param, sizes, image=300):
    """The restatement's priors of a zoo SSD: the PriorBox layers of `param` on source maps of `sizes` cells, concatenated."""
    rows = []
    for t, nm, _, _, pd in R.parse_param(param):
        if t == "PriorBox":
            cells = sizes[nm[:-len("_mbox_priorbox")]]
            step = 0.0 if pd[11] == -233 else float(pd[11])
            rows.append(R.priorbox(cells, cells, image, image, pd[0], pd.get(1, []), pd.get(2, []), [pd[3 + k] for k in range(4)], bool(pd[7]), bool(pd[8]),
                                   step, step, pd[13]))
    return np.concatenate(rows, axis=1)


def test_mobilenet_ssd_from_pixels(cuda):
    """FeedPixels -> mobilenet_ssd -> ExtractDetections, once, at batch 2 and fusion level 2, against the float64 restatement of the whole net
    (tests/detect_cases.mobilenet_ssd_input, which asserts the stability margins where it builds the input): the same detections in the same
    order, the priors exact, and DetectionOutput from its own inputs at its own tolerance."""
    from feathercnn_amd import PIXEL_RGB
    from feathercnn_amd.net import Net
    p, b, i, o = DC.mobilenet_ssd_model()
    px, want, margins = DC.mobilenet_ssd_input()
    assert min(margins.values()) >= DC.MARGIN, margins
    net = Net(fusion=2)
    net.SetDetection(True)
    net.LoadParam(p)
    net.LoadWeights(b)
    net.FeedPixels(i, px, PIXEL_RGB, mean=[DC.MOBILENET_MEAN] * 3, norm=[DC.MOBILENET_NORM] * 3)
    net.Forward()
    dets = net.ExtractDetections(o)
    loc, conf, prior = (net.Extract(k) for k in ("mbox_loc", "mbox_conf_flatten", "mbox_priorbox"))
    assert loc.shape == (2, 1, 1, 4 * 1917) and conf.shape == (2, 1, 1, 21 * 1917) and prior.shape == (1, 1, 2, 4 * 1917)
    sizes = {"conv11": 19, "conv13": 10, "conv14_2": 5, "conv15_2": 3, "conv16_2": 2, "conv17_2": 1}
    assert np.array_equal(prior[0, 0], _priors_of(p, sizes)) and np.array_equal(prior, want["mbox_priorbox"])
    assert abs(conf.reshape(2, 1917, 21).sum(axis=2) - 1).max() <= 1e-5
    for k, got_k in (("mbox_loc", loc), ("mbox_conf_flatten", conf)):  # behind 35 device convolutions: the project's net-level bound
        assert R.nerr(got_k, want[k]) <= 1e-4, (k, R.nerr(got_k, want[k]))
    got = net.Extract(o)[:, 0]
    whole = want[o][:, 0]
    print(f"mobilenet_ssd: {[len(d) for d in dets]} detections, margins of the restatement {margins}, worst deviation {np.abs(got - whole).max():.3g}")
    assert np.array_equal(got[:, :, 0], whole[:, :, 0]), "labels or row order against the restatement of the whole net"
    assert [len(d) for d in dets] == [len(d) for d in R.trim(whole)] and min(len(d) for d in dets) >= 1
    assert np.abs(got - whole).max() <= 1e-4
    args = (loc.reshape(2, -1), conf.reshape(2, -1), prior[:, 0], 21, 0.45, 100, 100, DC.MOBILENET["confidence_threshold"])
    w64, w32 = R.detection_output(*args, np.float64), R.detection_output(*args, np.float32)
    assert np.array_equal(got[:, :, 0], w64[:, :, 0])
    assert (np.abs(got.astype(np.float64) - w64) <= DC.detection_tolerance(w64, w32)).all()
    assert sum(a == "DETECT" and t == "Concat" for t, _, a in net.layers()) == 3 and not any(t == "Permute" for t, _, _ in net.layers())


def test_vgg16_ssd300_loads_and_runs(cuda):
    """vgg16_ssd300 with both switches, one forward at batch 1 and fusion level 2: 8732 priors equal to the restatement's, the dilated fc6 and
    the Normalize on their routes, softmax rows that sum to 1, and a well-formed DetectionOutput top.  (Its selection is not compared: a random
    net's 8732 x 20 scores are not chosen for stability, and MobileNet-SSD and tiny_ssd cover the comparison.)"""
    from feathercnn_amd import model_zoo
    from feathercnn_amd.net import Net
    p, b, i, o = model_zoo.vgg16_ssd300()
    net = Net(fusion=2)
    net.SetDetection(True)
    net.SetDilated(True)
    net.LoadParam(p)
    net.LoadWeights(b)
    net.FeedInput(i, np.random.default_rng(2).uniform(-1, 1, (1, 3, 300, 300)).astype(F))
    net.Forward()
    prior, loc, conf, out = (net.Extract(k) for k in ("mbox_priorbox", "mbox_loc", "mbox_conf_flatten", o))
    sizes = {"conv4_3_norm": 38, "fc7": 19, "conv6_2": 10, "conv7_2": 5, "conv8_2": 3, "conv9_2": 1}
    assert prior.shape == (1, 1, 2, 4 * 8732) and np.array_equal(prior[0, 0], _priors_of(p, sizes))
    assert loc.shape == (1, 1, 1, 4 * 8732) and conf.shape == (1, 1, 1, 21 * 8732) and out.shape == (1, 1, 200, 6)
    assert abs(conf.reshape(8732, 21).sum(axis=1) - 1).max() <= 1e-5 and np.isfinite(loc).all()
    routes = {nm: a for _, nm, a in net.layers()}
    assert routes["fc6"] == "ATROUS" and routes["conv4_3_norm"] == "DETECT" and routes["detection_out"] == "DETECT"
    rows = out[0, 0]
    count = int((rows[:, 0] > 0).sum())
    assert count >= 1 and not rows[count:].any() and (np.diff(rows[:count, 1]) <= 0).all() and (rows[:count, 1] > 0.01).all()
    assert set(rows[:count, 0]) <= set(map(float, range(1, 21))) and (rows[:count, 2] < rows[:count, 4]).all() and (rows[:count, 3] < rows[:count, 5]).all()
    [dets] = net.ExtractDetections(o)
    assert np.array_equal(dets, rows[:count])


# ---- a missing library -----------------------------------------------------------------------------------------------------------------------
def test_missing_library_is_an_error_at_reshape(cuda, tmp_path):
    """The tree's libraries in a directory without libfeather_detect.so (tests/detect_missing_child.py, a fresh process): a net of views and
    copies runs with the switch on and never maps it; one that needs it fails at its first Reshape with FHIP_E_UNSUPPORTED and a message that
    names the missing file.  With the whole tree the same nets run."""
    missing = _lib.path("detect")
    libs = glob.glob(os.path.join(os.path.dirname(_lib.lib_path()), "libfeather_*.so"))
    assert missing in libs
    for f in libs:
        if f != missing:
            shutil.copy(f, tmp_path / os.path.basename(f))
    for without in (True, False):
        env = dict(os.environ, PYTHONPATH=side_contract.ROOT)
        if without:
            env["FEATHER_HIP_LIB"] = str(tmp_path / os.path.basename(_lib.lib_path()))
        r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, os.path.join(HERE, "detect_missing_child.py")], capture_output=True, text=True, env=env,
                           cwd=str(tmp_path))
        assert r.returncode == 0, r.stderr[-2000:]
        lines = {ln.split()[0]: ln for ln in r.stdout.splitlines() if ln.split()}
        assert lines["plain"] == "plain ran unmapped", r.stdout
        for tag in ("permute", "normalize", "priorbox"):
            if without:
                assert lines[tag].startswith(tag + " refused:") and "libfeather_detect.so" in lines[tag] and "code -1" in lines[tag], r.stdout
                assert lines[tag].endswith(" unmapped"), r.stdout
            else:
                assert lines[tag] == f"{tag} ran mapped", r.stdout
