"""feather::Net's state across Forwards on the MI355X: ONE handle walked through shapes and settings (tests/lifecycle_cases.py), and after
EVERY Forward

  * against a fresh Net built with the walked net's current settings and fed only the current input (one Forward, two with graph): every
    blob either can Extract, bit for bit (int32 views) -- the same kernels with fixed-order reductions, the claim the concurrency and replica
    tests already make --, the same set of refused blobs with the same reason, the same layers() with their routes, conv_params(), chains(),
    canvases(), siblings(), residuals() and fused_pointwise();
  * against tests/seam_ref.py (float64, every blob rounded to float32): plane_nerr per (n, c) plane of the outputs and of every extractable
    intermediate, within the project's 1e-4 (the TOL of the seam tests and the net fuzzer);
  * the blobs refused as "transformed input" are exactly the tops the plan chained (chains()).

Over a route walk the plans must really change: the route of a 3x3 layer at every level; residuals(), siblings() and the one-kernel flag of
fused_pointwise() from level 2 (below it they must be empty: the plans do not exist); chains() and canvases() at level 3; F(4,3) -- 36
frequency points from fhip_winograd_f63_plan on the layer's conv_params() -- under tuned selection (without it a plane of at most 8 pixels is an
IM2COL layer by select_algo's rule).  Over the cycle walk net.memory() after the second and third pass equals its value after the first.

One test id per (walk, setting); each prints its worst plane_nerr, the distinct plans it saw and its time.  A HIP error ends the session
(pytest.exit), as in tests/test_seams_gpu.py: nothing more runs on the card."""
import ctypes
import time

import numpy as np
import pytest

import lifecycle_cases as LC
import seam_ref as R

pytestmark = pytest.mark.gpu
TOL = 1e-4
# the top a layer of the trunk writes once its ReLU (level 1) and pooling (level 2) are absorbed: what chains() stands for at level 3
CHAINED_TOP = {"conv0": "relu0", "conv1": "relu1", "conv2": "pool2", "conv3": "relu3"}
WINOGRADF63 = "WINOGRADF63"


def _tuple(p):
    return tuple(getattr(p, f[0]) for f in p._fields_)


class Walked:
    def __init__(self, row):
        self.walk_name, self.level, kw = row
        self.sub_batches = kw.get("sub_batches", 1)
        self.start = {k: bool(kw.get(k)) for k in ("tuned", "concurrency", "graph")}
        self.cur = dict(self.start)
        self.param, self.weights, self.input_name, _ = self.model()
        self.net = self.make()
        self.fed = None
        self.side = None  # the torch stream of a "stream" step: it must outlive the net's use of it
        self.worst = (0.0, None)
        self.bad = []
        self.seen = {k: set() for k in ("algo3x3", "chains", "canvases", "siblings", "residuals", "one_kernel", "points")}
        self.forwards = 0

    def model(self):
        return LC.deep_model() if self.walk_name == "deep" else LC.model()

    def make(self):
        from feathercnn_amd.net import Net
        net = Net(fusion=self.level, sub_batches=self.sub_batches, **self.cur)
        self.configure(net)
        net.LoadParam(self.param)
        net.LoadWeights(self.weights)
        return net

    def configure(self, net):
        pass

    def read(self, net, names):
        from feathercnn_amd import FeatherHipError
        out = {}
        for name in names:
            try:
                out[name] = net.Extract(name)
            except FeatherHipError as err:
                msg = str(err)
                if "fused into its consumer" in msg:
                    out[name] = "fused"
                elif "transformed input" in msg:
                    out[name] = "chained"
                else:
                    raise
        return out

    def plan(self, net):
        return {"layers": net.layers(), "conv_params": {i: (_tuple(p), b) for i, (p, b) in net.conv_params().items()},
                "chains": net.chains(raw=True), "canvases": net.canvases(), "siblings": net.siblings(), "residuals": net.residuals(),
                "fused_pointwise": {i: (_tuple(p), one) for i, (p, one) in net.fused_pointwise().items()}}

    def note(self, what, e=None):
        self.bad.append((self.forwards, self.fed, dict(self.cur), what) if e is None else (self.forwards, self.fed, dict(self.cur), what, e))

    def check(self):
        """Behind one Forward of the walked net."""
        from feathercnn_amd import _lib
        self.forwards += 1
        ref = LC.reference(*self.fed)
        x = LC.input(*self.fed)
        fresh = self.make()
        try:
            fresh.FeedInput(self.input_name, x)
            for _ in range(2 if self.cur["graph"] else 1):
                fresh.Forward()
            mine, theirs = self.plan(self.net), self.plan(fresh)
            for k in mine:
                if mine[k] != theirs[k]:
                    self.note(f"{k} differs from the fresh net's", (mine[k], theirs[k]))
            got, want = self.read(self.net, ref), self.read(fresh, ref)
        finally:
            fresh.close()
        for name in ref:
            a, b = got[name], want[name]
            if isinstance(a, str) or isinstance(b, str):
                if not (isinstance(a, str) and isinstance(b, str) and a == b):
                    self.note(f"Extract({name}): {a if isinstance(a, str) else 'ok'} here, {b if isinstance(b, str) else 'ok'} in the fresh net")
                if isinstance(a, str):
                    continue
            elif a.shape != b.shape or not np.array_equal(a.view(np.int32), b.view(np.int32)):
                diff = int((a.view(np.int32) != b.view(np.int32)).sum()) if a.shape == b.shape else -1
                self.note(f"{name} is not the fresh net's bit for bit ({diff} of {a.size} words differ)", R.plane_nerr(a, b) if a.shape == b.shape else None)
            if a.shape != ref[name].shape:
                self.note(f"{name} has shape {a.shape}, float64 says {ref[name].shape}")
                continue
            e = R.plane_nerr(a, ref[name])
            if self.worst[1] is None or e > self.worst[0]:
                self.worst = (e, f"{name}@{self.fed[0]}")
            if not e <= TOL:
                self.note(f"{name} against float64", e)
        if self.walk_name == "deep":
            return
        # the refusals are the plan's: a blob is "transformed input" exactly where chains() says its layer hands it over transformed
        names = {n: i for i, (_, n, _) in enumerate(mine["layers"])}
        planned = {CHAINED_TOP[n] for n, i in names.items() if n in CHAINED_TOP and mine["chains"].get(i, (0, 0))[1]}
        refused = {n for n, v in got.items() if isinstance(v, str) and v == "chained"}
        if planned != refused:
            self.note("chained blobs differ from the plan", (sorted(refused), sorted(planned)))
        if self.level == 0 and any(isinstance(v, str) for v in got.values()):
            self.note("a blob is refused without fusion")
        if self.level < 3 and (mine["chains"] or mine["canvases"]):
            self.note("a chain below level 3", (mine["chains"], mine["canvases"]))
        if self.level < 2 and (mine["siblings"] or mine["residuals"] or mine["fused_pointwise"]):
            self.note("a level-2 plan below level 2")
        lib = _lib.load_library()
        algos, points = [], set()
        for n in LC.CONV3X3:
            i = names[n]
            algos.append(mine["layers"][i][2])
            if mine["layers"][i][2] == WINOGRADF63:
                p, batch = self.net.conv_params()[i]
                pl = _lib.fhip_winograd_plan()
                assert lib.fhip_winograd_f63_plan(ctypes.byref(p), batch, ctypes.byref(pl)) == 0
                points.add(pl.frequency_points)
        self.seen["algo3x3"].add(tuple(algos))
        self.seen["points"] |= points
        self.seen["chains"].add(tuple(sorted(mine["chains"].items())))
        self.seen["canvases"].add(tuple(mine["canvases"]))
        self.seen["siblings"].add(tuple(sorted(mine["siblings"].items())))
        self.seen["residuals"].add(tuple(sorted(mine["residuals"].items())))
        self.seen["one_kernel"].add(tuple(sorted((i, one) for i, (_, one) in mine["fused_pointwise"].items())))

    def step(self, step):
        import torch
        kind = step[0]
        if kind == "feed":
            self.fed = (step[1], step[2] if len(step) > 2 else 0)
            self.net.FeedInput(self.input_name, LC.input(*self.fed))
        elif kind == "forward":
            for _ in range(step[1]):
                self.net.Forward()
                self.check()
        elif kind in ("set_tuned", "set_concurrency", "set_graph"):
            key = kind[4:]
            self.cur[key] = self.start[key] != step[1]
            getattr(self.net, kind)(self.cur[key])
        elif kind == "stream":
            self.side = torch.cuda.Stream()
            with torch.cuda.stream(self.side):
                self.net.use_current_stream()
        elif kind == "extract":
            _, name, at3 = step
            got = self.read(self.net, [name])[name]
            if self.level >= 3 and at3 == "chained":
                if not (isinstance(got, str) and got == "chained"):
                    self.note(f"Extract({name}) was not refused as chained")
            elif isinstance(got, str):
                self.note(f"Extract({name}) was refused ({got})")
            else:
                e = R.plane_nerr(got, LC.reference(*self.fed)[name])
                if not e <= TOL:
                    self.note(f"Extract({name}) against float64", e)
        else:
            raise AssertionError(step)


class WalkedMixed(Walked):
    """The model with int8 layers among fp32 ones (LC.mixed_model): after every Forward the fresh-net invariant on every blob and plan,
    every int8 layer against its restatement from the walked net's own bottom blob (np.array_equal; qseam_ref.int8_layers, which first
    asserts what each int8 layer absorbed), and the fp32 layers against float64 from the device's int8 outputs (plane_nerr <= TOL)."""

    def model(self):
        return LC.mixed_model()

    def configure(self, net):
        net.SetQuantized(True)

    def check(self):
        import qseam_ref as QR
        self.forwards += 1
        if not hasattr(self, "ref"):
            self.ref = R.Net(self.param, self.weights)
            self.names = [t for layer in self.ref.layers for t in layer[3]]
        x = LC.input(*self.fed)
        fresh = self.make()
        try:
            fresh.FeedInput(self.input_name, x)
            for _ in range(2 if self.cur["graph"] else 1):
                fresh.Forward()
            mine, theirs = self.plan(self.net), self.plan(fresh)
            for k in mine:
                if mine[k] != theirs[k]:
                    self.note(f"{k} differs from the fresh net's", (mine[k], theirs[k]))
            got, want = self.read(self.net, self.names), self.read(fresh, self.names)
        finally:
            fresh.close()
        for name in self.names:
            a, b = got[name], want[name]
            if isinstance(a, str) or isinstance(b, str):
                if not (isinstance(a, str) and isinstance(b, str) and a == b):
                    self.note(f"Extract({name}): {a if isinstance(a, str) else 'ok'} here, {b if isinstance(b, str) else 'ok'} in the fresh net")
            elif a.shape != b.shape or not np.array_equal(a.view(np.int32), b.view(np.int32)):
                self.note(f"{name} is not the fresh net's bit for bit", R.plane_nerr(a, b) if a.shape == b.shape else None)
        if any(v == "chained" for v in got.values() if isinstance(v, str)) or mine["chains"] or mine["fused_pointwise"] or mine["siblings"]:
            self.note("a chain, a pair or a sibling plan in a net whose neighbours are int8", (mine["chains"], mine["fused_pointwise"], mine["siblings"]))
        try:
            given = QR.int8_layers(self.ref, x, self.net, self.level)
        except AssertionError as err:
            self.note("an int8 layer against its restatement", str(err)[:400])
            return
        if sum(v is not None for v in given.values()) != len(LC.MIXED_INT8):
            self.note("not every int8 layer was compared", sorted(given))
        blobs = self.ref.run(self.input_name, x, keep=True, given=given)
        for name, a in got.items():
            if isinstance(a, str) or blobs.get(name) is None:
                continue
            e = R.plane_nerr(a, blobs[name]) if a.shape == blobs[name].shape else float("inf")
            if self.worst[1] is None or e > self.worst[0]:
                self.worst = (e, f"{name}@{self.fed[0]}")
            if not e <= TOL:
                self.note(f"{name} against float64", e)
        self.seen["residuals"].add(tuple(sorted(mine["residuals"].items())))


def _walk(row, cls=Walked, walks=None):
    t0 = time.perf_counter()
    w = cls(row)
    walk = (walks or LC.WALKS)[row[0]]
    memory = []
    try:
        for at, step in enumerate(walk):
            w.step(step)
            if row[0] == "cycle" and at + 1 in LC.PASS_ENDS:
                memory.append(w.net.memory())
    except Exception as err:
        if any(word in str(err) for word in ("illegal memory access", "unspecified launch failure", "hipError")):
            pytest.exit(f"GPU fault in {LC.row_id(row)} behind Forward {w.forwards} ({w.fed}, {w.cur}): {err}; nothing more runs on this GPU", returncode=3)
        raise
    finally:
        w.net.close()
    seen = {k: len(v) for k, v in w.seen.items() if k != "points"}
    print(f"{LC.row_id(row)}: {w.forwards} Forwards in {time.perf_counter() - t0:.2f} s; worst plane_nerr {w.worst[0]:.2e} ({w.worst[1]}); "
          f"distinct plans {seen}; frequency points {sorted(w.seen['points'])}" + (f"; memory per pass {memory}" if memory else ""))
    kinds = {}
    for entry in w.bad:  # every kind of miss once, with how often and where first: a walk reports all of its misses
        kinds.setdefault(entry[3], [0, entry])[0] += 1
    for what, (count, first) in kinds.items():
        print(f"  MISS x{count}: {what}; first behind Forward {first[0]} {first[1]} {first[2]}" + (f": {str(first[4])[:600]}" if len(first) > 4 else ""))
    assert not w.bad, (len(w.bad), sorted(kinds))
    return w, memory


@pytest.mark.parametrize("row", LC.table(), ids=LC.row_id)
def test_walked_net_equals_a_fresh_one(cuda, row):
    w, memory = _walk(row)
    level, tuned = row[1], bool(row[2].get("tuned"))
    if row[0] == "cycle":
        assert len(memory) == 3 and memory[1] == memory[0] and memory[2] == memory[0], memory
    if row[0] == "routes":
        # the walk did what it claims: every plan kind that exists at this level took at least two values
        assert len(w.seen["algo3x3"]) >= 2, w.seen["algo3x3"]
        for kind in ("residuals", "siblings", "one_kernel"):
            assert len(w.seen[kind]) >= (2 if level >= 2 else 1), (kind, w.seen[kind])
        for kind in ("chains", "canvases"):
            assert len(w.seen[kind]) >= (2 if level >= 3 else 1), (kind, w.seen[kind])
        assert (36 in w.seen["points"]) == tuned and 64 in w.seen["points"], w.seen["points"]


@pytest.mark.parametrize("row", LC.mixed_table(), ids=LC.row_id)
def test_walked_mixed_int8_net_equals_a_fresh_one_and_its_restatement(cuda, row):
    w, _ = _walk(row, WalkedMixed, LC.MIXED_WALKS)
    assert w.forwards == sum(s[1] for s in LC.MIXED_WALKS[row[0]] if s[0] == "forward")
    # the fp32 branch takes the add with the int8 branch's top from level 2 on: the one plan of this net
    assert all(bool(r) == (row[1] >= 2) for r in w.seen["residuals"]), w.seen["residuals"]
