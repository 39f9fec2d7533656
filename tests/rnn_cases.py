"""The tables of the recurrent-layer tests (tests/test_rnn_cpu.py, tests/test_rnn_gpu.py, tests/test_later_contract_cpu.py): the kernel
instantiations of libfeather_rnn.so, the cases of the core and the inputs of the net-level tests.

Shapes are the smallest at which the kernels can still go wrong, against the tiles of feather_rnn.h.  A block of the step route owns 32 hidden
units and 32 sequences: batches of 1, 2, 31, 32, 33 and 65 end inside a sequence tile, on its edge and one past it, and 33 and 65 take more
than one block; H = 4, 8, 32, 36, 64, 96 and 256 (multiples of 4) run on the matrix kernel -- inside a unit tile, on its edge, one chunk of K
and several, with a ragged last one -- and 1, 3, 6 and 33 on the direct kernel.  The sequence route keeps Wh in LDS: H = 100 / 101 (LSTM),
115 / 116 (GRU) and 198 / 199 (RNN) lie on both sides of its bound.  T = 1 has no recurrence: only h0 and the projections.

Every case draws weights from U(-1, 1) / sqrt(H) and inputs from U(-1, 1): at that scaling a float32 restatement of all three cells stays
within 5e-7 of float64 up to H 256 and T 400, whereas with weights three times as large the plain tanh RNN is chaotic by T 400 and float32
itself errs by 0.11, which no kernel could pass.  tests/test_rnn_cpu.py asserts the float32 restatement of every case within 1e-5."""
import functools
import os

import numpy as np

import rnn_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "feathercnn_amd", "libfeather_rnn.so")
F = np.float32
L, G, N = R.LSTM, R.GRU, R.RNN
ROUTES = {"auto": R.AUTO, "step": R.STEP, "seq": R.SEQUENCE}

KERNELS = {"rnn_step_mfma_kernel", "rnn_step_direct_kernel", "rnn_sequence_kernel"}


def targets():
    """Every instantiation of the library, by the names fhip_rnn_route reports."""
    return {"fhip::rnn_%s_kernel<%d>" % (k, c) for k in ("step_mfma", "step_direct", "sequence") for c in (L, G, N)}


# (cell, direction, H, n, T, state_in, state_out, pad, offset, route, kind).  state_in: h0 (and c0) present; state_out: hn (and cn) asked for;
# pad: floats by which both row strides exceed their rows; offset: floats past a 16-byte boundary, every buffer; route: "auto" the header's
# rule (the sequence route where Wh fits and n <= FHIP_RNN_SEQUENCE_MAX_N), "step" / "seq" forced; kind: "plain"; "pm80" xp scaled so that the pre-activations reach +-80; "zero" all-zero xp and weights
RNN_CASES = [
    # the step route on the matrix kernel: every H of it, every batch, every T
    (L, 2, 32, 33, 3, 1, 1, 0, 0, "step", "plain"), (L, 0, 4, 1, 1, 1, 1, 3, 1, "step", "plain"), (L, 1, 8, 2, 2, 0, 1, 0, 2, "step", "plain"),
    (L, 2, 36, 31, 3, 1, 0, 5, 3, "step", "plain"), (L, 0, 64, 32, 2, 0, 0, 0, 0, "step", "plain"), (L, 2, 96, 65, 3, 1, 1, 1, 1, "step", "plain"),
    (L, 2, 256, 33, 26, 0, 1, 0, 0, "auto", "plain"), (G, 2, 32, 65, 3, 1, 1, 0, 0, "step", "plain"), (G, 1, 4, 2, 26, 0, 0, 2, 2, "step", "plain"),
    (G, 0, 36, 33, 2, 1, 1, 0, 1, "step", "plain"), (G, 2, 96, 31, 3, 0, 1, 0, 3, "step", "plain"), (G, 0, 256, 1, 3, 1, 0, 0, 0, "auto", "plain"),
    (N, 2, 8, 32, 3, 1, 1, 0, 0, "step", "plain"), (N, 1, 64, 65, 26, 0, 1, 4, 1, "step", "plain"), (N, 0, 256, 2, 2, 1, 1, 0, 2, "auto", "plain"),
    (N, 2, 36, 33, 1, 1, 0, 0, 3, "step", "plain"),
    # the step route on the direct kernel
    (L, 2, 1, 1, 3, 1, 1, 0, 0, "step", "plain"), (L, 0, 3, 33, 2, 0, 1, 1, 1, "step", "plain"), (L, 1, 6, 65, 3, 1, 0, 0, 2, "step", "plain"),
    (L, 2, 33, 32, 26, 0, 1, 3, 3, "step", "plain"), (G, 0, 1, 2, 1, 1, 1, 0, 0, "step", "plain"), (G, 2, 3, 31, 3, 0, 0, 0, 1, "step", "plain"),
    (G, 1, 33, 33, 2, 1, 1, 2, 0, "step", "plain"), (N, 2, 6, 65, 2, 1, 1, 0, 0, "step", "plain"), (N, 0, 33, 1, 26, 0, 1, 1, 3, "step", "plain"),
    (N, 1, 3, 32, 3, 1, 0, 0, 2, "step", "plain"),
    # the sequence route, and H on both sides of its bound for each cell (past it the rule takes a step kernel)
    (L, 2, 48, 1, 26, 1, 1, 0, 0, "auto", "plain"), (L, 0, 96, 4, 3, 0, 1, 2, 1, "auto", "plain"), (L, 1, 100, 5, 2, 1, 1, 0, 2, "auto", "plain"),
    (L, 2, 101, 2, 3, 1, 1, 0, 0, "auto", "plain"), (L, 0, 104, 2, 2, 0, 0, 0, 0, "auto", "plain"), (G, 2, 115, 3, 3, 1, 1, 1, 3, "auto", "plain"),
    (G, 0, 116, 3, 2, 1, 1, 0, 0, "auto", "plain"), (N, 1, 198, 8, 3, 1, 1, 0, 1, "auto", "plain"), (N, 2, 199, 2, 2, 0, 1, 0, 0, "auto", "plain"),
    (G, 1, 6, 1, 1, 1, 1, 0, 2, "auto", "plain"), (N, 0, 1, 2, 26, 0, 0, 3, 0, "auto", "plain"), (L, 2, 8, 33, 3, 1, 1, 0, 0, "seq", "plain"),
    # pre-activations of +-80 on every kernel family
    (L, 2, 32, 33, 3, 1, 1, 0, 0, "step", "pm80"), (G, 0, 6, 33, 3, 1, 1, 0, 0, "step", "pm80"), (N, 1, 48, 2, 3, 1, 1, 0, 0, "auto", "pm80"),
    (L, 0, 48, 2, 3, 1, 1, 0, 0, "auto", "pm80"), (G, 2, 36, 9, 2, 1, 1, 0, 0, "step", "pm80"), (N, 0, 3, 9, 2, 1, 1, 0, 0, "step", "pm80"),
    # all-zero input and weights: h is exactly 0 for LSTM and RNN and exactly h0 / 2^steps for the GRU
    (L, 2, 8, 9, 3, 0, 1, 0, 0, "step", "zero"), (G, 2, 8, 9, 3, 1, 1, 0, 0, "step", "zero"), (N, 2, 6, 9, 3, 1, 1, 0, 0, "step", "zero"),
    (L, 0, 8, 2, 3, 0, 1, 0, 0, "auto", "zero"), (G, 1, 8, 2, 3, 1, 1, 0, 0, "auto", "zero"), (N, 0, 8, 2, 3, 1, 1, 0, 0, "auto", "zero"),
    (G, 1, 48, 2, 3, 1, 1, 0, 0, "auto", "pm80"),
    # the rule's upper side: more sequences than FHIP_RNN_SEQUENCE_MAX_N take the step route whatever H
    (N, 0, 4, 257, 2, 0, 0, 0, 0, "auto", "plain"),
]


def rnn_id(c):
    return "%s-dir%d-H%d-n%d-T%d-in%d-out%d-pad%d-off%d-%s-%s" % ((("lstm", "gru", "rnn")[c[0]],) + tuple(c[1:]))


def case_route(case):
    """The kernel the case runs on, by the restatement's rule."""
    cell, direction, h, n, t, _, _, _, _, route, _ = case
    return R.route(cell, h, n, t, ROUTES[route])


@functools.lru_cache(maxsize=None)
def rnn_case(case):
    """-> dict(xp, wh, bn, h0, c0, out, hn, cn): the inputs (absent ones None) and the float64 results of a case, shared among the tests, which
    leave them unchanged."""
    cell, direction, h, n, t, state_in, _, _, _, _, kind = case
    nd, g = (2 if direction == 2 else 1), R.GATES[cell]
    rng = np.random.default_rng(11000 + RNN_CASES.index(case))
    s = F(1.0 / np.sqrt(h))
    xp = rng.uniform(-1, 1, (n, t, nd * g * h)).astype(F)
    wh = (rng.uniform(-1, 1, (nd, g * h, h)).astype(F) * s).astype(F)
    bn = (rng.uniform(-1, 1, (nd, h)).astype(F) * s).astype(F) if cell == G else None
    h0 = rng.uniform(-1, 1, (n, nd, h)).astype(F) if state_in else None
    c0 = rng.uniform(-1, 1, (n, nd, h)).astype(F) if state_in and cell == L else None
    if kind == "pm80":
        xp = (xp * F(80.0 / np.abs(xp).max())).astype(F)
    if kind == "zero":
        xp, wh = np.zeros_like(xp), np.zeros_like(wh)
        bn = None if bn is None else np.zeros_like(bn)
    out, hn, cn = R.recurrent(cell, direction, xp, wh, bn, h0, c0)
    d = dict(xp=xp, wh=wh, bn=bn, h0=h0, c0=c0, out=out, hn=hn, cn=cn)
    for a in d.values():
        if a is not None:
            a.setflags(write=False)
    return d


# ---- net level -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def net_model(width=24):
    """-> ((param, bin, input, output), the trace for model_zoo.numpy_forward) of tiny_crnn at an image width (T = width / 4 - 1): the same
    weights at every width."""
    from feathercnn_amd import model_zoo
    trace = []
    return model_zoo.tiny_crnn(size=(8, width), trace=trace), trace


@functools.lru_cache(maxsize=None)
def net_input(batch=3, width=24):
    """-> (x, every blob of the numpy forward)."""
    from feathercnn_amd import model_zoo
    (p, b, i, o), trace = net_model(width)
    x = np.random.default_rng(12000 + batch + 3 * width).uniform(-1, 1, (batch, 3, 8, width)).astype(F)
    return x, model_zoo.numpy_forward(trace, i, x)


def net_shapes(width=24, classes=11):
    """Every blob of tiny_crnn: name -> ((c, h, w), rank)."""
    t = width // 4 - 1
    return {"data": ((3, 8, width), 3), "conv1": ((8, 8, width), 3), "relu1": ((8, 8, width), 3), "pool1": ((8, 4, width // 2), 3), "conv2": ((16, 4, width // 2), 3),
            "relu2": ((16, 4, width // 2), 3), "pool2": ((16, 2, width // 4), 3), "conv3": ((32, 1, t), 3), "relu3": ((32, 1, t), 3), "flat": ((1, 32, t), 2),
            "to_tokens": ((1, t, 32), 2), "bilstm": ((1, t, 16), 2), "gru": ((1, t, 6), 2), "gru_h": ((1, 1, 6), 2), "rnn": ((1, t, 8), 2), "classes": ((1, t, classes), 2),
            "prob": ((1, t, classes), 2)}


@functools.lru_cache(maxsize=None)
def states_model():
    """-> ((param, bin, input, output), trace) of tiny_lstm_states: an LSTM with state Inputs and state tops."""
    from feathercnn_amd import model_zoo
    trace = []
    return model_zoo.tiny_lstm_states(trace=trace), trace
