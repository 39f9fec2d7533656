"""One way to run libfeather_rnn.so on the device with every tensor between guards (tests/guarded.py): recurrent(), which
tests/test_rnn_gpu.py compares with tests/rnn_ref.py, and sweep(), which walks cases of tests/rnn_cases.py so that every instantiation of
rnn_cases.targets() is launched -- tests/rnn_trace_child.py runs it under the kernel trace."""
import ctypes

import numpy as np

import rnn_cases as C
import rnn_ref as R
import side_contract
from attn_sweep import Shifted, same_bits  # noqa: F401  (same_bits: for the tests)
from guarded import describe

F = np.float32
V = ctypes.c_void_p
TOL = 1e-4  # the project's bound (tests/test_net_gpu.py)


def route(lib, cell, h, n, t, forced=R.AUTO):
    name = ctypes.create_string_buffer(128)
    assert lib.fhip_rnn_route(cell, h, n, t, forced, name, 128) == 0, lib.fhip_rnn_last_error()
    return name.value.decode()


def _strided(a, stride):
    """The rows of a [n][T][w] array laid out with a row stride (the slack NaN: an input nothing may read)."""
    n, t, w = a.shape
    buf = np.full((n * t, stride), np.nan, F)
    buf[:, :w] = a.reshape(n * t, w)
    return buf


def recurrent(lib, cell, direction, xp, wh, bn=None, h0=None, c0=None, state_out=True, pad=0, offset=0, forced=R.AUTO):
    """-> (out, hn, cn) of fhip_rnn_forward_route from guarded buffers (hn, cn None where not asked for or not an LSTM's).  Every guard is
    checked, every output element must have been written, the slack of `out`'s rows must not, and the cell scratch starts poisoned: a read
    of it before its write turns the result into NaN."""
    import torch
    n, t, xw = xp.shape
    nd, h = wh.shape[0], wh.shape[2]
    xs, os_ = xw + pad, nd * h + pad
    inputs = {"xp": Shifted(n * t * xs, _strided(xp, xs), offset), "wh": Shifted(wh.size, wh, offset)}
    for name, a in (("bn", bn), ("h0", h0), ("c0", c0)):
        if a is not None:
            inputs[name] = Shifted(a.size, a, offset)
    out = Shifted(n * t * os_, "poison", offset)
    hn = Shifted(n * nd * h, "poison", offset) if state_out else None
    cn = Shifted(n * nd * h, "poison", offset) if state_out and cell == R.LSTM else None
    scratch = Shifted(nd * n * h, "poison", offset) if cell == R.LSTM else None
    at = lambda g: None if g is None else V(g.ptr)
    rc = lib.fhip_rnn_forward_route(cell, direction, n, t, h, at(inputs["xp"]), xs, at(inputs["wh"]), at(inputs.get("bn")), at(inputs.get("h0")), at(inputs.get("c0")),
                                    at(out), os_, at(hn), at(cn), at(scratch), side_contract.stream(), forced)
    assert rc == 0, lib.fhip_rnn_last_error()
    torch.cuda.synchronize()
    for g in list(inputs.values()) + [b for b in (out, hn, cn, scratch) if b is not None]:
        assert g.guards_intact() is None, describe(g.guards_intact())
    live = torch.zeros((n * t, os_), dtype=torch.bool, device="cuda")
    live[:, :nd * h] = True
    assert out.unwritten(live.reshape(-1)) == 0 and out.unwritten(~live.reshape(-1)) == n * t * pad, "out: an element unwritten, or its slack written"
    bits = lambda g, shape: g.bits().cpu().numpy().view(np.uint32).reshape(shape).view(F)
    got = bits(out, (n * t, os_))[:, :nd * h].reshape(n, t, nd * h).copy()
    for g in (hn, cn):
        assert g is None or g.unwritten() == 0
    return got, (None if hn is None else bits(hn, (n, nd, h))), (None if cn is None else bits(cn, (n, nd, h)))


def run_case(lib, case):
    """-> ((out, hn, cn) of the device, the case's data)."""
    cell, direction, h, n, t, _, state_out, pad, offset, forced, _ = case
    d = C.rnn_case(case)
    return recurrent(lib, cell, direction, d["xp"], d["wh"], d["bn"], d["h0"], d["c0"], bool(state_out), pad, offset, C.ROUTES[forced]), d


def worst_error(got, d):
    """The largest normalised error among out, hn and cn (where the call wrote them)."""
    return max(R.normalised_error(g, d[k]) for g, k in zip(got, ("out", "hn", "cn")) if g is not None)


def _sweep_cases():
    """One small case per instantiation."""
    chosen = {}
    for case in C.RNN_CASES:
        if case[10] == "plain" and case[3] * case[4] * case[2] <= 33 * 3 * 116:
            chosen.setdefault(C.case_route(case), case)
    return [chosen[k] for k in sorted(chosen)]


def sweep(lib, seen):
    """Launches every instantiation on small data, compared with the restatement as it goes; seen(route name) for each launch, in launch order:
    T of them for a call on the step route."""
    for case in _sweep_cases():
        cell, direction, h, n, t, _, _, _, _, forced, _ = case
        got, d = run_case(lib, case)
        assert worst_error(got, d) <= TOL, case
        name = route(lib, cell, h, n, t, C.ROUTES[forced])
        for _ in range(1 if "sequence" in name else t):
            seen(name)
