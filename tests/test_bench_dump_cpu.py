"""bench.py --dump-outputs, the part that needs no GPU: what dump_outputs writes for the arrays the timed path handed back -- one float32
.npy per net, never more than DUMP_LIMIT bytes in all, and the same seeded sample of images whenever an array has to be cut."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_small_outputs_are_written_whole_as_float32(tmp_path):
    rng = np.random.default_rng(1)
    outs = {"vgg16": rng.random((32, 1000, 1, 1), dtype=np.float32), "resnet50_global512": rng.random((512, 1000, 1, 1)).astype(np.float64)}
    bench.dump_outputs(outs, str(tmp_path / "d"))
    assert sorted(os.listdir(tmp_path / "d")) == ["resnet50_global512.npy", "vgg16.npy"]
    for name, want in outs.items():
        got = np.load(tmp_path / "d" / (name + ".npy"))
        assert got.dtype == np.float32 and got.shape == want.shape
        np.testing.assert_array_equal(got, want.astype(np.float32))


def test_large_outputs_are_cut_to_the_same_seeded_sample(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT", 64 * 1024)
    x = np.arange(200 * 256, dtype=np.float32).reshape(200, 256)  # 200 KB, one image = 1 KB
    y = np.ones((4, 8), dtype=np.float32)
    for d in ("a", "b"):
        bench.dump_outputs({"big": x, "small": y}, str(tmp_path / d))
    a, b = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    np.testing.assert_array_equal(a, b)
    assert a.shape == (32, 256) and a.nbytes <= 32 * 1024
    rows = a[:, 0].astype(np.int64) // 256  # the sample keeps whole images, in their order
    assert np.all(np.diff(rows) > 0) and np.array_equal(a, x[rows])
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "small.npy"), y)
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= 64 * 1024 + 2 * 256  # + the two .npy headers


def test_an_image_over_its_share_is_cut_to_a_seeded_sample_of_elements(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT", 8 * 1024)
    x = np.arange(1 * 4096, dtype=np.float32).reshape(1, 16, 16, 16)  # ONE image of 16 KB against a share of 4 KB
    y = np.arange(2 * 4096, dtype=np.float32).reshape(2, 4096)          # two images of 16 KB each
    for d in ("a", "b"):
        bench.dump_outputs({"one": x, "two": y}, str(tmp_path / d))
    for name, src in (("one", x), ("two", y)):
        a, b = np.load(tmp_path / "a" / (name + ".npy")), np.load(tmp_path / "b" / (name + ".npy"))
        np.testing.assert_array_equal(a, b)
        assert a.shape == (1024,) and a.nbytes <= 4 * 1024
        assert np.all(np.diff(a) > 0) and np.isin(a, src.reshape(-1)).all()  # distinct elements of the output, in order


class _CountingNet:
    """Stands in for feathercnn_amd.net.Net: Extract returns a probability vector (one-hot) that names how many Forwards have run."""
    made = []

    def __init__(self, **kw):
        self.forwards = 0
        _CountingNet.made.append(self)

    def LoadParam(self, p):
        pass

    def LoadWeights(self, b):
        pass

    def FeedInput(self, name, x):
        self.batch = x.shape[0]

    def Forward(self):
        self.forwards += 1

    def Extract(self, name):
        y = np.zeros((self.batch, 1000, 1, 1), np.float32)
        y[:, self.forwards % 1000] = 1.0
        return y

    def close(self):
        pass


def test_the_dump_is_the_output_of_the_last_timed_step(monkeypatch):
    """measure_net stores what Extract returns right after the K timed steps: not after the first (untimed) Forward, not after the
    steady-state cross-check steps that follow."""
    import types

    import torch

    import feathercnn_amd.net
    from benchkit import timing
    monkeypatch.setattr(feathercnn_amd.net, "Net", _CountingNet)
    monkeypatch.setattr(timing, "sustained_mfma", lambda: None)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    a = types.SimpleNamespace(sub_batches=1, fusion=3, no_graph=False, reference_selection=False, no_overlap=False)
    env = {"dev": torch.device("cpu"), "rank": 0, "world": 1}
    outputs = {}
    warmup, steps, steady = 3, 7, 11
    res, _ = timing.measure_net("vgg16", a, env, steps, warmup, batch=2, detail=False, steady=steady, model=(b"", b"", "data", "prob"),
                                outputs=outputs)
    assert res["steps"] == steps and res["steady_state"]["steps"] == steady
    net = _CountingNet.made[-1]
    assert net.forwards == 1 + warmup + steps + steady
    got = outputs["vgg16"]
    assert got.shape == (2, 1000, 1, 1) and np.argmax(got[0].reshape(-1)) == 1 + warmup + steps
