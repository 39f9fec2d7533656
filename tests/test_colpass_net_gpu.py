"""fhip_net_set_colpass on the MI355X: the four-convolution net 3 -> 64 -> 64 (pool) -> 128 -> 128 at 224 pixels and batch 1
(tests/colpass_net_child.py).  c2 (224 px, pooled, the MULTI walk) and c3 (112 px, two row tiles) are the layers the library accepts in front
of a plain chained layer; their M is far below the size the default mode asks for, so mode 1 keeps the main route here and mode 2 forces
the new one.  Every value behind the column pass is bit-identical, so outputs are compared with array_equal."""
import glob
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import colpass_net_child as child
import ktrace
from feathercnn_amd import _lib

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROUTED = ["c2", "c3"]


def _run(mode, batch=1, graph=False, forwards=1):
    net, _ = child.net(mode, batch, graph)
    for _ in range(forwards):
        net.Forward()
    return net, net.Extract("r4")


@pytest.fixture(scope="module")
def main_route(cuda):
    """The output on the main route (mode 0), eager: computed once, never changed."""
    net, out = _run(0)
    assert net.colpasses() == [] and np.isfinite(out).all()
    out.setflags(write=False)
    return out


def test_modes_0_and_2_give_equal_outputs_eager_and_replayed(cuda, main_route):
    for graph, forwards in ((False, 1), (True, 3)):  # a graph is captured behind the first Forward and replayed from then on
        net, out = _run(2, graph=graph, forwards=forwards)
        assert [net.layers()[k][1] for k in net.colpasses()] == ROUTED
        assert np.array_equal(out, main_route), (graph, float(np.abs(out - main_route).max()))
    net, out = _run(0, graph=True, forwards=3)
    assert net.colpasses() == [] and np.array_equal(out, main_route)


def test_the_default_mode_keeps_the_main_route_at_this_size(cuda, main_route):
    net, out = _run(None)
    assert net.colpasses() == [] and np.array_equal(out, main_route)
    chains = {net.layers()[k][1]: v for k, v in net.chains().items()}
    assert chains.get("c3") == (True, True), chains  # the run the rule looks at exists


def test_replanning_on_one_handle_equals_fresh_nets(cuda, main_route):
    """Mode 2 -> 0 -> 2 and a batch change, on one handle with a captured graph: each equals a fresh net of that setting."""
    net, img = child.net(2, graph=True)
    for mode, routed in ((2, ROUTED), (0, []), (2, ROUTED)):
        net.SetColpass(mode)
        for _ in range(2):
            net.Forward()
        assert [net.layers()[k][1] for k in net.colpasses()] == routed, mode
        assert np.array_equal(net.Extract("r4"), main_route), mode
    fresh, want = _run(2, batch=2)
    net.FeedInput("data", np.random.default_rng(3).uniform(-1, 1, (2, 3, 224, 224)).astype(np.float32))  # child.net's images at batch 2
    for _ in range(2):
        net.Forward()
    assert [net.layers()[k][1] for k in net.colpasses()] == ROUTED
    got = net.Extract("r4")
    assert got.shape == want.shape == (2, 128, 112, 112) and np.array_equal(got, want)
    net.FeedInput("data", img)  # and back
    net.Forward()
    assert np.array_equal(net.Extract("r4"), main_route)


def test_kernel_trace_shows_the_new_kernels_at_mode_2_only(cuda, tmp_path):
    for mode in (2, 1):
        text, rows, _ = ktrace.trace("colpass_net_child.py", [mode], tmp_path, 240)
        names = [name for _, name, *_ in rows]
        gemm = sum("colpass_gemm_kernel" in k for k in names)
        chain = sum("colpass_chain_kernel" in k for k in names)
        if mode == 2:
            assert "colpass layers: c2,c3 mapped" in text, text[-500:]
            assert gemm == chain == 2 * len(ROUTED), (gemm, chain)  # two forwards
            # c2's pooled boundary walks its 1444 tiles (MULTI), c3's unpooled one holds whole planes: two instantiations
            assert len({k for k in names if "colpass_chain_kernel" in k}) == 2, sorted(set(names))
            assert not any("wino_chain_kernel" in k for k in names), sorted(set(names))  # c4 ends the run: the output transform
        else:
            assert "colpass layers: none unmapped" in text, text[-500:]  # the default mode does not even open the library here
            assert gemm == chain == 0 and sum("wino_chain_kernel" in k for k in names) == 2 * len(ROUTED), sorted(set(names))


def test_mode_2_without_the_library_fails_at_reshape_and_names_it(cuda, tmp_path):
    """The tree's libraries in a directory without libfeather_colpass.so, in fresh child processes: the default mode runs on the main route
    and says nothing, mode 2 is refused at the first Forward's Reshape with the file's name in the message."""
    missing = _lib.path("colpass")
    libs = glob.glob(os.path.join(os.path.dirname(_lib.lib_path()), "libfeather_*.so"))
    assert missing in libs
    for f in libs:
        if f != missing:
            shutil.copy(f, tmp_path / os.path.basename(f))
    env = dict(os.environ, PYTHONPATH=os.path.dirname(HERE), FEATHER_HIP_LIB=str(tmp_path / os.path.basename(_lib.lib_path())))
    for mode, want in ((1, "colpass layers: none unmapped"), (2, "refused:")):
        r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.join(HERE, "colpass_net_child.py"), str(mode)], capture_output=True,
                           text=True, env=env, cwd=str(tmp_path))
        assert r.returncode == 0 and want in r.stdout, (r.stdout[-1500:], r.stderr[-1500:])
        if mode == 2:
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("refused:")][0]
            assert "libfeather_colpass.so" in line and "code -1" in line and line.endswith(" unmapped"), line
