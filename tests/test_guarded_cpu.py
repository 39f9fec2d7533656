"""Self-tests of the contract-test harness that need no GPU: tests/guarded.py sees what it is meant to see (on CPU tensors), and every
`__global__` kernel of the library has a case in the route table of tests/contract_routes.py (or a reason in its exclusion list) -- a kernel
added later without a contract case fails here."""
import glob
import os
import re

import numpy as np

from guarded import CANARY, POISON, Guarded

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _g(n=16, fill="poison", offset=0):
    return Guarded(n, fill, offset, guard=64, device="cpu")


def test_write_before_the_body_is_seen():
    for off in (0, 1):
        g = _g(offset=off)
        assert g.guards_intact() is None
        g.raw[g.lo - 1] = 7
        assert g.guards_intact() == (-1, 7)


def test_write_after_the_body_is_seen():
    for off in (0, 1):
        g = _g(offset=off)
        g.raw[g.lo + g.n] = 7
        assert g.guards_intact() == (g.n, 7)


def test_unwritten_body_word_is_counted():
    g = _g()
    assert g.unwritten() == 16
    g.body[:] = 1.0
    assert g.unwritten() == 0
    g.raw[g.lo + 3] = POISON
    assert g.unwritten() == 1
    assert g.unwritten(live=slice(0, 3)) == 0


def test_changed_input_is_seen():
    x = np.arange(16, dtype=np.float32) - 8
    g = _g(fill=x, offset=1)
    assert np.array_equal(g.values(), x)
    snap = g.snapshot()
    assert g.unchanged(snap)
    g.body[5] = -0.0  # a bit change that a float comparison would miss
    g.body[5] = float(x[5])
    assert g.unchanged(snap)
    g.raw[g.lo + 5] = int(np.float32(-0.0).view(np.int32))
    assert not g.unchanged(snap) and g.first_change(snap)[0] == 5


def test_empty_body_is_a_valid_pointer_between_guards():
    g = _g(n=0)
    assert g.ptr != 0 and g.guards_intact() is None
    snap = g.snapshot()
    g.raw[g.lo] = 0  # the first word at the pointer belongs to the trailing guard
    assert g.guards_intact() == (0, 0) and not g.unchanged(snap)


def test_patterns_are_quiet_nans_compared_as_bits():
    for bits in (CANARY, POISON):
        f = np.array([bits], np.int32).view(np.float32)[0]
        assert np.isnan(f)
    assert CANARY != POISON


EXCLUDED_REASON_MIN = 10


def _kernels():
    names = set()
    for path in glob.glob(os.path.join(ROOT, "feathercnn_amd", "csrc", "*.hip")) + glob.glob(os.path.join(ROOT, "feathercnn_amd", "csrc", "*.h")):
        src = open(path).read()
        names |= set(re.findall(r"__global__\s+(?:__launch_bounds__\((?:[^()]|\([^()]*\))*\)\s+)?void\s+(\w+)", src))
    return names


def test_every_kernel_has_a_contract_case():
    from contract_routes import EXCLUDED, ROUTES
    kernels = _kernels()
    assert len(kernels) >= 30, sorted(kernels)  # the scan itself works
    covered = {k for r in ROUTES for k in r.kernels}
    missing = sorted(kernels - covered - set(EXCLUDED))
    assert not missing, f"kernels without a contract case in tests/contract_routes.py: {missing}"
    assert not covered - kernels, f"route table names kernels that do not exist: {sorted(covered - kernels)}"
    assert all(len(why) >= EXCLUDED_REASON_MIN for why in EXCLUDED.values())
    assert set(EXCLUDED) <= kernels
