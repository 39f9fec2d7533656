"""Every kernel instantiation of the library against fp64 (tests/instance_cases.py, tests/instance_sweep.py), and a kernel trace proving it ran.

test_instance_case: one case per parameter, scaled inputs, compared per output plane (or bit-exactly, or against the magnitude of its terms).
test_sweep_trace: the whole table once in a fresh child process under `rocprofv3 --kernel-trace` (no counters).  The sweep separates its cases
with fhip_relu launches of i + 1 blocks; the trace, sorted by start time, is cut at them.  Each case's window must hold its targets, and the
windows together every instantiation of the library but the EXCLUDED ones.
"""
from __future__ import annotations


import pytest

import instance_sweep as S
import ktrace
from instance_cases import CASES, EXCLUDED
from kernel_instances import base, instances, normalise

pytestmark = pytest.mark.gpu
TRACE_TIMEOUT = 600


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_instance_case(cuda, case):
    got, ref = S.run(case)
    bad = S.compare(case, got, ref())
    assert not bad, "\n".join(bad[:8])


def _windows(rows, ncases):
    """rows: (start, name, blocks) sorted by start -> [set of normalised names] per case, cut at the separators (relu_kernel of i + 1 blocks)."""
    wins, cur = [set() for _ in range(ncases)], -1
    for _, name, blocks in rows:
        if base(name) == "relu_kernel" and blocks == cur + 2:
            cur += 1
            continue
        if 0 <= cur < ncases:
            wins[cur].add(name)
    assert cur == ncases, f"found {cur + 1} of {ncases + 1} separators in the trace"
    return wins


def _blocks(rows):
    """ktrace's rows with normalised names and the grid in blocks: (start, name, blocks)."""
    rows = [(t, normalise(n), gx, wx) for t, n, gx, wx in rows]
    # the grid is reported in work-items: blocks = grid / workgroup (the first separator, one block, tells which unit the trace uses)
    first_sep = next(r for r in rows if base(r[1]) == "relu_kernel")
    per_item = first_sep[2] == first_sep[3] and first_sep[3] > 1
    return [(t, n, gx // wx if per_item else gx) for t, n, gx, wx in rows]


def test_sweep_trace(cuda, tmp_path):
    _, rows, _ = ktrace.trace("instance_sweep.py", [], tmp_path, TRACE_TIMEOUT, ok=None)  # the sweep ends with a JSON line of its own
    wins = _windows(_blocks(rows), len(CASES))
    import torch
    cus256 = torch.cuda.get_device_properties(0).multi_processor_count == 256
    missing = [f"{c.name}: {sorted(set(c.targets) - wins[i])} (ran {sorted(n for n in wins[i] if n.startswith('fhip::'))})"
               for i, c in enumerate(CASES) if (cus256 or not c.cus256) and not set(c.targets) <= wins[i]]
    assert not missing, "cases that did not run their target instantiation:\n" + "\n".join(missing)
    ran = set().union(*wins)
    uncovered = sorted(n for n in instances() if n not in ran and base(n) not in EXCLUDED)
    if not cus256:
        pytest.skip(f"not a 256-CU device: row-split / persistent cases run other instantiations here; uncovered: {uncovered}")
    assert not uncovered, f"instantiations no sweep case ran: {uncovered}"
