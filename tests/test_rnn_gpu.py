"""The recurrent layers on the device: libfeather_rnn.so through its C-ABI from guarded buffers (tests/guarded.py, element offsets 0 .. 3,
row strides above the rows, a poisoned cell scratch), and tiny_crnn through feather::Net.

* The core against the float64 restatement (tests/rnn_ref.py) by the project's normalised error and its bound TOL = 1e-4
  (tests/test_net_gpu.py): every case of tests/rnn_cases.RNN_CASES -- the three kernels of each cell, every direction, states absent and
  present, pre-activations that reach +-80, all-zero input and weights (exact).  The worst error observed is printed.
  Every call checks the guards around every buffer, that every output element was written and that no slack element was.
* Bit for bit: a reverse layer is the forward one on the time-reversed input; each half of a bidirectional layer is the single-direction
  call; a run over T = 8 is two runs over T = 4 that hand the state on.  On the step route and on the sequence route.
* Batch independence at TOL; one kernel trace; the Python mirror.
* tiny_crnn against model_zoo.numpy_forward at TOL at fusion 0 .. 3, with and without the graph, 1 and 2 sub-batch replicas, batch 1 and 3;
  re-plans to another width (another T) and another batch and back; state blobs through the Net; what only a Reshape can refuse (-100);
  a q8 bottom in front of every type (-300)."""
import struct

import numpy as np
import pytest

import kernel_instances as KI
import ktrace
import rnn_cases as C
import rnn_ref as R
import rnn_sweep as SW
import side_contract

pytestmark = pytest.mark.gpu
F = np.float32
TOL = SW.TOL  # the project's bound (tests/test_net_gpu.py)

lib = side_contract.fixture("rnn", gpu=True)


# ---- the C-ABI ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.RNN_CASES, ids=C.rnn_id)
def test_the_core_equals_the_float64_restatement(lib, case):
    cell, direction, h, n, t, state_in, state_out, pad, offset, forced, kind = case
    got, d = SW.run_case(lib, case)
    name = SW.route(lib, cell, h, n, t, C.ROUTES[forced])
    err = SW.worst_error(got, d)
    print(f"{C.rnn_id(case)} on {name}: error {err:.3g} (bound {TOL:g})")
    assert name == C.case_route(case)
    assert (got[1] is not None) == bool(state_out) and (got[2] is not None) == (bool(state_out) and cell == R.LSTM)
    for g in got:
        assert g is None or np.isfinite(g).all(), case
    assert err <= TOL, (case, err)
    if kind == "pm80":  # saturated gates, no NaN: |h| <= 1, and a tanh cell reaches the bound
        assert float(np.abs(got[0]).max()) <= 1.0 and (cell == R.LSTM or float(np.abs(got[0]).max()) > 0.99)
    if kind == "zero":
        if cell == R.GRU:
            assert np.array_equal(got[1], (d["h0"].astype(np.float64) / 2.0 ** t).astype(F)) and got[1].any()
        else:
            assert not got[0].any() and not got[1].any()


def _inputs(cell, nd, h, n, t, seed, states=True):
    rng = np.random.default_rng(seed)
    g, s = R.GATES[cell], F(1.0 / np.sqrt(h))
    xp = rng.uniform(-1, 1, (n, t, nd * g * h)).astype(F)
    wh = (rng.uniform(-1, 1, (nd, g * h, h)).astype(F) * s).astype(F)
    bn = (rng.uniform(-1, 1, (nd, h)).astype(F) * s).astype(F) if cell == R.GRU else None
    h0 = rng.uniform(-1, 1, (n, nd, h)).astype(F) if states else None
    c0 = rng.uniform(-1, 1, (n, nd, h)).astype(F) if states and cell == R.LSTM else None
    return xp, wh, bn, h0, c0


# (H, n, the route forced): the matrix kernel, the direct kernel, the sequence kernel
BITWISE = [(36, 33, R.STEP), (6, 33, R.STEP), (8, 5, R.SEQUENCE)]


@pytest.mark.parametrize("h,n,forced", BITWISE, ids=["mfma", "direct", "sequence"])
@pytest.mark.parametrize("cell", [R.LSTM, R.GRU, R.RNN], ids=["lstm", "gru", "rnn"])
def test_reverse_and_bidirectional_equal_the_single_direction_calls_bit_for_bit(lib, cell, h, n, forced):
    t, g = 3, R.GATES[cell]
    xp, wh, bn, h0, c0 = _inputs(cell, 2, h, n, t, 500 + cell + h)
    both = SW.recurrent(lib, cell, 2, xp, wh, bn, h0, c0, forced=forced)
    half = lambda a, d: None if a is None else np.ascontiguousarray(a[:, d:d + 1] if a.ndim == 3 and a.shape[1] == 2 else a[d:d + 1])
    for d in (0, 1):
        x_d = np.ascontiguousarray(xp[:, :, d * g * h:(d + 1) * g * h])
        one = SW.recurrent(lib, cell, d, x_d, wh[d:d + 1], None if bn is None else bn[d:d + 1], half(h0, d), half(c0, d), forced=forced)
        assert SW.same_bits(one[0], both[0][:, :, d * h:(d + 1) * h]) and SW.same_bits(one[1], both[1][:, d:d + 1]), (d, "direction 2's half")
        assert one[2] is None or SW.same_bits(one[2], both[2][:, d:d + 1])
        if d == 1:  # and the reverse layer is the forward one on the time-reversed input, time-reversed
            fwd = SW.recurrent(lib, cell, 0, np.ascontiguousarray(x_d[:, ::-1]), wh[1:2], None if bn is None else bn[1:2], half(h0, 1), half(c0, 1), forced=forced)
            assert SW.same_bits(np.ascontiguousarray(fwd[0][:, ::-1]), one[0]) and SW.same_bits(fwd[1], one[1])
            assert fwd[2] is None or SW.same_bits(fwd[2], one[2])


@pytest.mark.parametrize("h,n,forced", BITWISE, ids=["mfma", "direct", "sequence"])
@pytest.mark.parametrize("cell", [R.LSTM, R.GRU, R.RNN], ids=["lstm", "gru", "rnn"])
def test_a_run_equals_two_runs_that_hand_the_state_on_bit_for_bit(lib, cell, h, n, forced):
    xp, wh, bn, h0, c0 = _inputs(cell, 1, h, n, 8, 600 + cell + h)
    whole = SW.recurrent(lib, cell, 0, xp, wh, bn, h0, c0, forced=forced)
    first = SW.recurrent(lib, cell, 0, np.ascontiguousarray(xp[:, :4]), wh, bn, h0, c0, forced=forced)
    second = SW.recurrent(lib, cell, 0, np.ascontiguousarray(xp[:, 4:]), wh, bn, first[1], first[2], forced=forced)
    assert SW.same_bits(np.concatenate([first[0], second[0]], axis=1), whole[0]) and SW.same_bits(second[1], whole[1])
    assert whole[2] is None or SW.same_bits(second[2], whole[2])
    assert SW.same_bits(whole[1][:, 0], whole[0][:, -1])  # hn is the last step's h


def test_a_sequence_does_not_depend_on_its_batch(lib):
    """Row i of a batch of 33 equals the same sequence run alone, at TOL -- and not bit for bit where the two take different routes: the batch
    runs on the step route here (forced), the single sequence where the rule sends it, which at H = 36 is the sequence route, whose sums run
    in another order; at H = 256 both are on the matrix kernel and the bits agree."""
    for cell, h in ((R.LSTM, 36), (R.GRU, 36), (R.RNN, 36), (R.LSTM, 256)):
        xp, wh, bn, h0, c0 = _inputs(cell, 2, h, 33, 3, 700 + cell + h)
        batch = SW.recurrent(lib, cell, 2, xp, wh, bn, h0, c0, forced=R.STEP)
        same_route = SW.route(lib, cell, h, 33, 3, R.STEP) == SW.route(lib, cell, h, 1, 3)
        assert same_route == (h == 256)
        for i in (0, 31, 32):
            alone = SW.recurrent(lib, cell, 2, xp[i:i + 1], wh, bn, h0[i:i + 1], None if c0 is None else c0[i:i + 1])
            for a, b in zip(alone, batch):
                if a is not None:
                    assert R.normalised_error(a, b[i:i + 1]) <= TOL
                    assert not same_route or SW.same_bits(a, b[i:i + 1])


def test_the_python_mirror(cuda):
    import torch
    from feathercnn_amd import rnn
    case = [c for c in C.RNN_CASES if c[0] == R.GRU and c[1] == 2 and c[2] == 32][0]
    d = C.rnn_case(case)
    wide = torch.full((case[3], case[4], d["xp"].shape[2] + 5), float("nan"), device="cuda")  # a view with a larger row stride
    wide[:, :, :d["xp"].shape[2]] = torch.from_numpy(d["xp"].copy()).cuda()
    dev = lambda a: torch.from_numpy(a.copy()).cuda()
    out, hn, cn = rnn.recurrent(rnn.GRU, wide[:, :, :d["xp"].shape[2]], dev(d["wh"]), 2, bn=dev(d["bn"]), h0=dev(d["h0"]), states=True, route=C.ROUTES[case[9]])
    assert cn is None and R.normalised_error(out.cpu().numpy(), d["out"]) <= TOL and R.normalised_error(hn.cpu().numpy(), d["hn"]) <= TOL
    assert rnn.rnn_route(rnn.GRU, 32, case[3], case[4], C.ROUTES[case[9]]) == C.case_route(case)  # the route the case names, forced as the case forces it
    lstm = [c for c in C.RNN_CASES if c[0] == R.LSTM and c[2] == 48 and c[10] == "plain"][0]
    d = C.rnn_case(lstm)
    out = rnn.recurrent(rnn.LSTM, dev(d["xp"]), dev(d["wh"]), lstm[1], h0=dev(d["h0"]), c0=dev(d["c0"]))
    assert R.normalised_error(out.cpu().numpy(), d["out"]) <= TOL
    with pytest.raises(ValueError):
        rnn.recurrent(rnn.LSTM, dev(d["xp"]), dev(d["wh"]), 0)  # a bidirectional Wh with direction 0


def test_the_sweep_launches_what_the_route_names(cuda, tmp_path):
    """One child under rocprofv3 --kernel-trace (tests/rnn_trace_child.py): the library's kernels in the trace are, launch for launch, the
    routes fhip_rnn_route named -- T of them for a call on the step route, one for a call on the sequence route -- and together every
    instantiation tests/rnn_cases.targets() names, which is every instantiation the library holds (tests/test_later_contract_cpu.py)."""
    text, rows, _ = ktrace.trace("rnn_trace_child.py", [], tmp_path, 240)
    named = [ln[len("route "):] for ln in text.splitlines() if ln.startswith("route ")]
    launched = [KI.normalise(name) for _, name, *_ in rows]
    launched = [nm for nm in launched if nm in C.targets()]
    assert launched == named, (launched, named)
    assert set(launched) == C.targets()
    steps = [c for c in SW._sweep_cases() if "step" in C.case_route(c)]
    assert len(named) == sum(c[4] for c in steps) + sum(1 for c in SW._sweep_cases() if "sequence" in C.case_route(c)) and any(c[4] > 1 for c in steps)


# ---- the net -----------------------------------------------------------------------------------------------------------------------------
def _net(level=2, graph=False, replicas=1, model=None):
    from feathercnn_amd.net import Net
    p, b, i, o = model or C.net_model()[0]
    net = Net(fusion=level, graph=graph, sub_batches=replicas)
    net.SetRecurrent()
    net.SetDetection(True)
    net.SetTransformer()
    net.LoadParam(p)
    net.LoadWeights(b)
    return net


def _run(net, batch=3, width=24):
    (p, b, i, o), _ = C.net_model(width)
    x, want = C.net_input(batch, width)
    net.FeedInput(i, x)
    net.Forward()
    return want, net.Extract(o)


@pytest.mark.parametrize("batch", [3, R.SEQUENCE_MAX_N + 1])
def test_tiny_crnn_every_blob_at_level_0(cuda, batch):
    """Batch 3 runs the three layers on the sequence route, a batch above FHIP_RNN_SEQUENCE_MAX_N on the step route: the LSTM (H = 8) on the
    matrix kernel, the GRU (H = 6) on the direct one."""
    (p, b, i, o), _ = C.net_model()
    net = _net(0)
    want, out = _run(net, batch)
    worst = 0.0
    for name, (chw, rank) in C.net_shapes().items():
        got = net.Extract(name)
        assert got.shape == (batch,) + chw == want[name].shape, name
        err = R.normalised_error(got, want[name])
        worst = max(worst, err)
        assert err <= TOL, (name, err)
    print(f"tiny_crnn level 0 batch {batch}: the worst blob is within {worst:.3g} of the float64 forward (bound {TOL:g})")
    assert [(t, a) for t, _, a in net.layers() if t in ("LSTM", "GRU", "RNN")] == [("LSTM", "RNN"), ("GRU", "RNN"), ("RNN", "RNN")]
    assert {a for t, nm, a in net.layers() if t == "InnerProduct"} == {"IM2COL"}
    assert ("sequence" in R.route(R.LSTM, 8, batch, 5)) == (batch == 3) and R.route(R.GRU, 6, R.SEQUENCE_MAX_N + 1, 5) == "fhip::rnn_step_direct_kernel<1>"
    assert R.route(R.LSTM, 8, R.SEQUENCE_MAX_N + 1, 5) == "fhip::rnn_step_mfma_kernel<0>"


def test_tiny_crnn_at_every_setting(cuda):
    (p, b, i, o), _ = C.net_model()
    outs = {}
    for level, graph, replicas, batch in ((0, False, 1, 3), (1, False, 1, 3), (2, False, 1, 3), (3, False, 1, 3), (0, True, 1, 3), (1, True, 1, 3), (2, True, 1, 3), (3, True, 2, 3),
                                          (1, False, 2, 3), (0, True, 1, 1), (1, False, 1, 1), (2, False, 1, 1), (3, False, 1, 1), (2, True, 2, 1)):
        net = _net(level, graph, replicas)
        want, out = _run(net, batch)
        hidden = net.Extract("gru_h")
        if graph:  # replay the captured graph
            net.Forward()
            assert np.array_equal(net.Extract(o), out) and np.array_equal(net.Extract("gru_h"), hidden)
        err = max(R.normalised_error(out, want[o]), R.normalised_error(hidden, want["gru_h"]))
        print(f"tiny_crnn level {level} graph {graph} replicas {replicas} batch {batch}: error {err:.3g} against the float64 forward (bound {TOL:g})")
        assert out.shape == want[o].shape == (batch, 1, 5, 11) and hidden.shape == (batch, 1, 1, 6) and err <= TOL, (level, graph, replicas, batch, err)
        assert [nm for t, nm, _ in net.layers() if t in ("LSTM", "GRU", "RNN")] == ["bilstm", "gru", "rnn"]  # nothing fuses into these layers
        if replicas == 1 and not graph:
            outs[(level, batch)] = out, hidden, net.Extract("bilstm")
    for batch in (1, 3):  # levels 1 to 3 are bit-equal among themselves
        for level in (2, 3):
            for got, ref in zip(outs[(level, batch)], outs[(1, batch)]):
                assert SW.same_bits(got, ref), (level, batch)


def test_tiny_crnn_replans_to_another_width_and_another_batch_and_back(cuda):
    (p, b, i, o), _ = C.net_model()
    for graph in (False, True):
        net = _net(2, graph=graph)
        want3, first = _run(net, 3, 24)
        want_wide, wide = _run(net, 3, 32)  # another image width: T = 7
        assert wide.shape == (3, 1, 7, 11) and R.normalised_error(wide, want_wide[o]) <= TOL and net.Extract("bilstm").shape == (3, 1, 7, 16)
        _, again = _run(net, 3, 24)
        assert SW.same_bits(again, first) and R.normalised_error(first, want3[o]) <= TOL
        big = R.SEQUENCE_MAX_N + 1
        want_big, many = _run(net, big, 24)  # another batch, and the step route
        assert many.shape == (big, 1, 5, 11) and R.normalised_error(many, want_big[o]) <= TOL
        want1, one = _run(net, 1, 24)
        assert R.normalised_error(one, want1[o]) <= TOL
        _, again = _run(net, 3, 24)
        assert SW.same_bits(again, first)


@pytest.mark.parametrize("batch", [2, R.SEQUENCE_MAX_N + 1])
def test_crnn_lite_lstm_against_the_float64_forward(cuda, batch):
    """A recogniser of real size -- BiLSTM(48) on 26 tokens of 96 floats -- through the Net: the sequence route at batch 2, the matrix step
    kernel above FHIP_RNN_SEQUENCE_MAX_N."""
    from feathercnn_amd import model_zoo
    from feathercnn_amd.net import Net
    trace = []
    p, b, i, o = model_zoo.crnn_lite_lstm(trace=trace)
    x = np.random.default_rng(900 + batch).uniform(-1, 1, (batch, 3, 32, 100)).astype(F)
    want = model_zoo.numpy_forward(trace, i, x)
    net = Net(fusion=2)
    net.SetRecurrent()
    net.SetDetection(True)
    net.SetTransformer()
    net.SetFrame()
    net.LoadParam(p)
    net.LoadWeights(b)
    net.FeedInput(i, x)
    net.Forward()
    for name in ("to_tokens", "bilstm", o):
        got = net.Extract(name)
        err = R.normalised_error(got, want[name])
        print(f"crnn_lite_lstm batch {batch} blob {name}: error {err:.3g} (bound {TOL:g})")
        assert got.shape == want[name].shape and err <= TOL, (name, err)
    assert net.Extract(o).shape == (batch, 1, 26, 37) and np.allclose(net.Extract(o).sum(axis=3), 1, atol=1e-5)
    assert ("sequence" in R.route(R.LSTM, 48, batch, 26)) == (batch == 2)


@pytest.mark.parametrize("replicas", [1, 2])
def test_state_blobs_through_the_net(cuda, replicas):
    """An LSTM fed its initial states through Inputs and writing its final states as tops; the state Inputs are dealt out to the sub-batch
    replicas with the sequences.  Two runs that hand the states on equal one run over both halves."""
    from feathercnn_amd import model_zoo
    (p, b, i, o), trace = C.states_model()
    rng = np.random.default_rng(800 + replicas)
    n = 4
    feeds = {"data": rng.uniform(-1, 1, (n, 1, 3, 5)).astype(F), "hidden": rng.uniform(-1, 1, (n, 1, 1, 4)).astype(F), "cell": rng.uniform(-1, 1, (n, 1, 1, 4)).astype(F)}
    want = model_zoo.numpy_forward(trace, feeds)
    net = _net(1, replicas=replicas, model=(p, b, i, o))
    for name, x in feeds.items():
        net.FeedInput(name, x)
    net.Forward()
    got = {name: net.Extract(name) for name in ("l", "l_h", "l_c")}
    for name in got:
        assert got[name].shape == want[name].shape and R.normalised_error(got[name], want[name]) <= TOL, name
    assert SW.same_bits(got["l_h"][:, 0, 0], got["l"][:, 0, -1])
    nxt = rng.uniform(-1, 1, (n, 1, 3, 5)).astype(F)
    for name, x in (("data", nxt), ("hidden", got["l_h"]), ("cell", got["l_c"])):
        net.FeedInput(name, x)
    net.Forward()
    whole = R.layer(R.LSTM, 0, np.concatenate([feeds["data"][:, 0], nxt[:, 0]], axis=1), *[trace[-1][4][k] for k in ("wx", "bias", "wh")], feeds["hidden"][:, 0], feeds["cell"][:, 0])
    assert R.normalised_error(net.Extract("l")[:, 0], whole[0][:, 3:]) <= TOL and R.normalised_error(net.Extract("l_c")[:, 0], whole[2]) <= TOL


# ---- what only a Reshape can refuse --------------------------------------------------------------------------------------------------------
def _param(lines):
    tops = sum(int(ln.split()[3]) for ln in lines)
    return ("7767517\n%d %d\n" % (len(lines), tops) + "\n".join(lines) + "\n").encode()


def _zeros(cell, nd, h, size):
    g = R.GATES[cell]
    return b"".join(struct.pack("<I", 0) + bytes(4 * count) for count in (nd * g * h * size, nd * (1 if cell == R.RNN else 4) * h, nd * g * h * h))


def _planned(lines, feeds, weights, level=1):
    from feathercnn_amd.net import Net
    net = Net(fusion=level)
    net.SetRecurrent()
    net.SetDetection(True)
    net.LoadParam(_param(lines))
    net.LoadWeights(weights)
    for name, x in feeds.items():
        net.FeedInput(name, x)
    net.Forward()
    return net


X = np.random.default_rng(5).uniform(-1, 1, (2, 4, 6, 8)).astype(F)
TOKENS = ["Input in0 0 1 in0 0=8 1=6 2=1", "Reshape tok 1 1 in0 tok 0=8 1=6"]  # a blob of rank 2, [6][8]
STATES = ["Input h 0 1 h 0=4 1=1 2=1", "Input c 0 1 c 0=4 1=1 2=1"]
S = np.zeros((2, 1, 1, 4), F)
RESHAPE_REFUSALS = {
    "a_bottom_of_rank_3": (["Input in0 0 1 in0 0=8 1=6 2=1", "LSTM l 1 1 in0 top 0=4 1=128 2=0"], dict(in0=X[:, :1]), _zeros(R.LSTM, 1, 4, 8), "rank 3"),
    "a_bottom_of_rank_3_with_channels": (["Input in0 0 1 in0 0=8 1=6 2=4", "GRU l 1 1 in0 top 0=4 1=96 2=0"], dict(in0=X), _zeros(R.GRU, 1, 4, 8), "rank 3"),
    "a_wrong_width": (TOKENS + ["RNN l 1 1 tok top 0=4 1=28 2=0"], dict(in0=X[:, :1]), _zeros(R.RNN, 1, 4, 7), "[T][7]"),
    "a_wrong_width_bidirectional": (TOKENS + ["LSTM l 1 1 tok top 0=4 1=128 2=2"], dict(in0=X[:, :1]), _zeros(R.LSTM, 2, 4, 4), "[T][4]"),
    "a_state_blob_of_the_wrong_shape": (TOKENS + ["Input h 0 1 h 0=5 1=1 2=1", STATES[1], "LSTM l 3 3 tok h c top hn cn 0=4 1=128 2=0"],
                                        dict(in0=X[:, :1], h=np.zeros((2, 1, 1, 5), F), c=S), _zeros(R.LSTM, 1, 4, 8), "state blob"),
    "a_state_blob_for_one_direction_of_two": (TOKENS + [STATES[0], "GRU l 2 2 tok h top hn 0=4 1=192 2=2"], dict(in0=X[:, :1], h=S), _zeros(R.GRU, 2, 4, 8), "state blob"),
    "a_state_blob_of_the_wrong_batch": (TOKENS + STATES + ["LSTM l 3 3 tok h c top hn cn 0=4 1=128 2=0"], dict(in0=X[:, :1], h=S, c=np.zeros((3, 1, 1, 4), F)),
                                        _zeros(R.LSTM, 1, 4, 8), "state blob"),
}


@pytest.mark.parametrize("name", sorted(RESHAPE_REFUSALS))
def test_reshape_refusals(cuda, name):
    from feathercnn_amd import FeatherHipError
    lines, feeds, weights, word = RESHAPE_REFUSALS[name]
    with pytest.raises(FeatherHipError, match="code -100") as e:
        _planned(lines, {k: np.ascontiguousarray(v) for k, v in feeds.items()}, weights)
    assert "layer l" in str(e.value) and word in str(e.value), str(e.value)


def test_the_forms_only_a_reshape_accepts_run(cuda):
    """A bidirectional GRU with its state Input and top, and an RNN whose input is ONE float wide (the GEMM of the main library with a single
    input channel, which a convolution would take for a depthwise layer): each against the restatement."""
    rng = np.random.default_rng(6)
    for cell, type_, nd, size, lines, extra in ((R.GRU, "GRU", 2, 8, TOKENS + ["Input h 0 1 h 0=4 1=2 2=1", "GRU l 2 2 tok h top hn 0=4 1=192 2=2"], True),
                                               (R.RNN, "RNN", 1, 1, ["Input in0 0 1 in0 0=1 1=6 2=1", "Reshape tok 1 1 in0 tok 0=1 1=6", "RNN l 1 1 tok top 0=4 1=4 2=1"], False)):
        g = R.GATES[cell]
        wx, bias, wh = rng.uniform(-0.5, 0.5, (nd, g * 4, size)).astype(F), rng.uniform(-0.5, 0.5, (nd, 1 if cell == R.RNN else 4, 4)).astype(F), rng.uniform(-0.5, 0.5, (nd, g * 4, 4)).astype(F)
        blob = b"".join(struct.pack("<I", 0) + a.tobytes() for a in (wx, bias, wh))
        x = np.ascontiguousarray(X[:, :1, :, :size])
        h0 = rng.uniform(-1, 1, (2, 1, nd, 4)).astype(F)
        net = _planned(lines, dict(in0=x, h=h0) if extra else dict(in0=x), blob)
        want = R.layer(cell, 2 if nd == 2 else 1, x[:, 0], wx, bias, wh, h0[:, 0] if extra else None)
        assert R.normalised_error(net.Extract("top")[:, 0], want[0]) <= TOL, type_
        if extra:
            assert R.normalised_error(net.Extract("hn")[:, 0], want[1]) <= TOL


# ---- q8 blobs (the int8 activation behind a requantised convolution, Net.SetRequantized) ---------------------------------------------------
Q8_READERS = {"LSTM": lambda g, x: g.lstm("r", x, 8, 4), "GRU": lambda g, x: g.gru("r", x, 8, 4, direction=2), "RNN": lambda g, x: g.rnn("r", x, 8, 4, direction=1)}


@pytest.mark.parametrize("name", sorted(Q8_READERS))
@pytest.mark.parametrize("level", [0, 2])
def test_a_recurrent_layer_cannot_read_a_q8_blob(cuda, name, level):
    """A q8 bottom is refused at Reshape by the check every layer that cannot read one meets: NET_E_TOPOLOGY (-300), naming the producer and
    the layer."""
    from feathercnn_amd import FeatherHipError, model_zoo
    from feathercnn_amd.net import Net
    g = model_zoo.GraphBuilder(3, quant={})
    Q8_READERS[name](g, g.conv("c1", g.input("data", 3, 8, 8), 3, 16, 3, 1, 1, requant=20.0))
    p, b = g.finish()
    net = Net(fusion=level)
    net.SetRecurrent()
    net.SetDetection(True)
    net.SetQuantized(True)
    net.SetRequantized(True)
    net.LoadParam(p)
    net.LoadWeights(b)
    net.FeedInput("data", np.random.default_rng(2).uniform(-1, 1, (2, 3, 8, 8)).astype(F))
    with pytest.raises(FeatherHipError) as e:
        net.Forward()
    msg = str(e.value)
    assert "code -300" in msg and "layer c1" in msg and name + " layer r" in msg and "blob c1" in msg, msg
