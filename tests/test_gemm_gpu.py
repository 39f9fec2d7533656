"""Gemm and MatMul on the device: libfeather_gemm.so through feathercnn_amd.gemm over the case table of tests/gemm_cases.py, and
model_zoo.tiny_matmul through Net, against the float64 restatement tests/gemm_ref.py by the project's normalised error and its bound
TOL = 1e-4.  The refusals a net makes at Reshape stand here and not in tests/test_gemm_cpu.py: a net plans its shapes on a device."""
import numpy as np
import pytest

import gemm_cases as C
import gemm_ref as R

pytestmark = pytest.mark.gpu
F = np.float32


def _run(case):
    import torch
    from feathercnn_amd.gemm import GemmDesc, forward, gemm_route
    fields, bufs, d_idx, want = C.build(case)
    desc = GemmDesc(**fields)
    dev = {k: None if v is None else torch.from_numpy(v[0].copy()).cuda() for k, v in bufs.items()}
    view = lambda k: None if dev[k] is None else dev[k][bufs[k][1]:]  # noqa: E731
    forward(desc, view("a"), view("b"), view("c"), view("d"))
    torch.cuda.synchronize()
    out = dev["d"].cpu().numpy()
    rest = np.ones(out.shape, bool)
    rest[d_idx] = False
    assert (out[rest] == C.SENTINEL).all(), "a float outside D was written"
    return out[d_idx], want, gemm_route(desc)


@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_gemm_equals_the_float64_restatement(cuda, case):
    got, want, route = _run(case)
    err = R.normalised_error(got, want)
    print(f"gemm {C.case_id(case)} on {route}: error {err:.3g} (bound {C.TOL:g})")
    assert route == C.route_name(case[3])
    assert err <= C.TOL, (case, err)


def test_the_cases_reach_every_instantiation():
    assert {C.route_name(c[3]) for c in C.CASES} == C.targets()


def test_the_python_mirror(cuda):
    import torch
    from feathercnn_amd import gemm, matmul
    rng = np.random.default_rng(41)
    a, b, c = (rng.uniform(-1, 1, s).astype(F) for s in ((3, 20, 33), (70, 33), (70,)))
    got = gemm(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), torch.from_numpy(c).cuda(), alpha=0.5, beta=-2.0, trans_b=True, out_transpose=True)
    assert R.normalised_error(got.cpu().numpy(), R.gemm(a, b[None], c[None], 0.5, -2.0, trans_b=True, c_broadcast=4).transpose(0, 2, 1)) <= C.TOL
    for sa, sb, tb in (((33,), (33,), 0), ((20, 33), (33, 9), 0), ((33,), (33, 9), 0), ((20, 33), (33,), 1), ((3, 20, 33), (9, 33), 1), ((20, 33), (3, 33, 9), 0)):
        x, y = rng.uniform(-1, 1, sa).astype(F), rng.uniform(-1, 1, sb).astype(F)
        got = matmul(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(), trans_b=bool(tb)).cpu().numpy()
        assert got.shape == R.matmul(x, y, bool(tb)).shape and R.normalised_error(got, R.matmul(x, y, bool(tb))) <= C.TOL, (sa, sb)


# ---- the net -----------------------------------------------------------------------------------------------------------------------------
def _net(param, weights=b"", volumes=False, **kw):
    from feathercnn_amd.net import Net
    net = Net(fusion=1, **kw)
    net.SetGemm()
    if volumes:
        net.SetConv3d()  # lets an Input take a volume
    net.SetTransformer()
    net.SetDetection(True)
    net.LoadParam(param)
    net.LoadWeights(weights)
    return net


@pytest.mark.parametrize("kw", [dict(), dict(graph=True), dict(sub_batches=2)], ids=["eager", "graph", "replicas"])
@pytest.mark.parametrize("batch", [1, 2])
def test_tiny_matmul_through_net(cuda, batch, kw):
    from feathercnn_amd import model_zoo as Z
    W = {}
    param, weights, data, out = Z.tiny_matmul(trace=W)
    x = np.random.default_rng(50 + batch).uniform(-1, 1, (batch, 7, 16)).astype(F)
    want = Z.tiny_matmul_forward(W, x)
    net = _net(param, weights, **kw)
    for _ in range(3):  # a captured graph replays: every run gives the eager result
        net.FeedInput(data, x[:, None])
        net.Forward()
        got = net.Extract(out)
        assert got.shape == (batch, 1, 1, 16)
        err = R.normalised_error(got[:, 0, 0], want)
        print(f"tiny_matmul batch {batch} {kw}: error {err:.3g} (bound {C.TOL:g})")
        assert err <= C.TOL
    assert [a for t, _, a in net.layers() if t in ("Gemm", "MatMul")] == ["GEMM"] * 5


X = np.random.default_rng(9).uniform(-1, 1, (2, 3, 6, 8)).astype(F)
RESHAPE_REFUSALS = {
    "batch_extents_2_vs_3": ("MatMul l 2 1 a b top 0=1", dict(a=X[:, :2], b=X), "batch extents 2 and 3"),
    "k_differs": ("MatMul l 2 1 a b top", dict(a=X, b=X), "K differs"),
    "gemm_k_differs": ("Gemm l 2 1 a2 b2 top", dict(a=X[:, :1], b=X[:, :1]), "K differs"),
    "rank_4": ("MatMul l 2 1 a b top", dict(a=X[:, None], b=X), "layer l"),
}


@pytest.mark.parametrize("name", sorted(RESHAPE_REFUSALS))
def test_reshape_refusals(cuda, name):
    from feathercnn_amd import FeatherHipError
    line, feeds, word = RESHAPE_REFUSALS[name]
    lines = ["Input a 0 1 a", "Input b 0 1 b"] + (["Reshape a2 1 1 a a2 0=8 1=6", "Reshape b2 1 1 b b2 0=8 1=6"] if "a2" in line else []) + [line]
    net = _net(("7767517\n%d %d\n" % (len(lines), len(lines)) + "\n".join(lines) + "\n").encode(), volumes=name == "rank_4")
    for blob, x in feeds.items():
        net.FeedInput(blob, np.ascontiguousarray(x))
    with pytest.raises(FeatherHipError) as e:
        net.Forward()
    assert "layer l" in str(e.value) and word in str(e.value), str(e.value)
