"""The recurrent layers without a GPU: the restatement tests/rnn_ref.py against torch.nn.LSTM / GRU / RNN in float64; the conditioning of
every case of tests/rnn_cases.py (its float32 restatement next to the float64 one); the switch fhip_net_set_recurrent; every refusal of the
new param and weight readers with its code; the host-side refusals of libfeather_rnn.so; the zoo's nets; and the readers on hostile files in
a stand-alone program whose host side runs under AddressSanitizer and UndefinedBehaviorSanitizer (never loaded into python)."""
import ctypes
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import rnn_cases as C
import rnn_ref as R
import side_contract as SC

F = np.float32
ROOT = SC.ROOT
INT_MAX = 2 ** 31 - 1
TYPES = {"LSTM": (R.LSTM, "0=4 1=96 2=0"), "GRU": (R.GRU, "0=4 1=72 2=0"), "RNN": (R.RNN, "0=4 1=24 2=0")}  # size 6, H 4, forward


def _one(type_, params="", bottoms=1, tops=1, c=1, h=5, w=6):
    """A net of `bottoms` Inputs in0 .. (one at least) and one layer `l` of `type_` that reads `bottoms` of them."""
    lines = [f"Input in{k} 0 1 in{k} 0={w} 1={h} 2={c}" for k in range(max(bottoms, 1))]
    lines.append(f"{type_} l {bottoms} {tops} " + " ".join(f"in{k}" for k in range(bottoms)) + " " + " ".join("t%d" % k for k in range(tops)) + " " + params)
    return ("7767517\n%d %d\n" % (len(lines), max(bottoms, 1) + tops) + "\n".join(lines) + "\n").encode()


def _net(param, weights=None, recurrent=True, detection=True, transformer=True, level=1):
    from feathercnn_amd.net import Net
    net = Net(fusion=level)
    if recurrent:
        net.SetRecurrent()
    if detection:
        net.SetDetection(True)
    if transformer:
        net.SetTransformer()
    net.LoadParam(param)
    if weights is not None:
        net.LoadWeights(weights)
    return net


def _refused(param, code, word, **kw):
    from feathercnn_amd import FeatherHipError
    with pytest.raises(FeatherHipError, match=f"code {code}") as e:
        _net(param, **kw)
    assert word in str(e.value), str(e.value)
    return str(e.value)


# ---- the restatement against an independent oracle -----------------------------------------------------------------------------------------
def _torch_layer(cell, direction, x, wx, bias, wh, h0, c0):
    """ncnn's layer computed by torch.nn.LSTM / GRU / RNN in float64: gate rows permuted (torch orders an LSTM's i, f, g, o), the bias on the
    input side, the GRU's BN row as b_hn; a reverse layer is the forward one on the time-reversed input, time-reversed."""
    import torch
    nd, g = wx.shape[0], R.GATES[cell]
    h, size = wh.shape[2], wx.shape[2]
    mod = {R.LSTM: torch.nn.LSTM, R.GRU: torch.nn.GRU, R.RNN: torch.nn.RNN}[cell](size, h, batch_first=True, bidirectional=nd == 2).double()
    rows = np.concatenate([np.arange(k * h, (k + 1) * h) for k in ((0, 1, 3, 2) if cell == R.LSTM else range(g))])
    with torch.no_grad():
        for d, suffix in enumerate(("", "_reverse")[:nd]):
            b = np.asarray(bias, np.float64).reshape(nd, -1, h)[d]
            getattr(mod, "weight_ih_l0" + suffix).copy_(torch.from_numpy(np.asarray(wx[d], np.float64)[rows]))
            getattr(mod, "weight_hh_l0" + suffix).copy_(torch.from_numpy(np.asarray(wh[d], np.float64)[rows]))
            getattr(mod, "bias_ih_l0" + suffix).copy_(torch.from_numpy(b[:g].reshape(-1)[rows]))
            hh = np.zeros(g * h)
            if cell == R.GRU:
                hh[2 * h:] = b[3]
            getattr(mod, "bias_hh_l0" + suffix).copy_(torch.from_numpy(hh))
        xs = torch.from_numpy(np.asarray(x, np.float64))
        if direction == 1:
            xs = xs.flip(1)
        state = None
        if h0 is not None:
            hs = torch.from_numpy(np.asarray(h0, np.float64)).transpose(0, 1).contiguous()
            state = (hs, torch.from_numpy(np.asarray(c0, np.float64)).transpose(0, 1).contiguous()) if cell == R.LSTM else hs
        out, last = mod(xs, state)
        if direction == 1:
            out = out.flip(1)
        hn, cn = (last if cell == R.LSTM else (last, None))
    return out.numpy(), hn.transpose(0, 1).numpy(), None if cn is None else cn.transpose(0, 1).numpy()


@pytest.mark.parametrize("state", [False, True], ids=["zeros", "state"])
@pytest.mark.parametrize("direction", [0, 1, 2])
@pytest.mark.parametrize("cell", [R.LSTM, R.GRU, R.RNN], ids=["lstm", "gru", "rnn"])
def test_the_restatement_equals_torch_in_float64(cell, direction, state):
    rng = np.random.default_rng(100 + 10 * cell + 3 * direction + state)
    n, t, size, h, nd, g = 3, 7, 5, 6, (2 if direction == 2 else 1), R.GATES[cell]
    x = rng.uniform(-1, 1, (n, t, size))
    wx, wh = rng.uniform(-0.5, 0.5, (nd, g * h, size)), rng.uniform(-0.5, 0.5, (nd, g * h, h))
    bias = rng.uniform(-0.5, 0.5, (nd, 1 if cell == R.RNN else 4, h))
    h0 = rng.uniform(-1, 1, (n, nd, h)) if state else None
    c0 = rng.uniform(-1, 1, (n, nd, h)) if state and cell == R.LSTM else None
    got = R.layer(cell, direction, x, wx, bias, wh, h0, c0)
    want = _torch_layer(cell, direction, x, wx, bias, wh, h0, c0)
    for a, b, what in zip(got, want, ("out", "hn", "cn")):
        assert (a is None) == (b is None), what
        if a is not None:
            assert a.shape == b.shape and R.normalised_error(a, b) <= 1e-12, (what, R.normalised_error(a, b))


@pytest.mark.parametrize("case", C.RNN_CASES, ids=C.rnn_id)
def test_every_case_leaves_float32_room(case):
    """The float32 restatement of the case lies within 1e-5 of the float64 one: a device result that misses the bound cannot blame the case."""
    d = C.rnn_case(case)
    got = R.recurrent(case[0], case[1], d["xp"], d["wh"], d["bn"], d["h0"], d["c0"], dtype=np.float32)
    for a, k in zip(got, ("out", "hn", "cn")):
        if a is not None:
            assert np.isfinite(d[k]).all() and R.normalised_error(a, d[k]) <= 1e-5, (k, R.normalised_error(a, d[k]))
    if case[10] == "pm80":  # the pre-activations do reach +-80, where an (e^2x - 1) / (e^2x + 1) tanh overflows
        assert abs(float(np.abs(d["xp"]).max()) - 80) < 1e-3 and np.exp(2 * 80.0) > np.finfo(F).max
    if case[10] == "zero":  # LSTM and RNN: exactly 0; GRU: exactly h0 halved once per step
        if case[0] == R.GRU:
            assert np.array_equal(d["hn"], d["h0"].astype(np.float64) / 2.0 ** case[4]) and d["hn"].any()
        else:
            assert not d["out"].any() and not d["hn"].any()


def test_the_cases_cover_what_the_issue_lists_and_every_kernel():
    cases = C.RNN_CASES
    assert len(set(cases)) == len(cases) and 40 <= len(cases) <= 60
    step = [c for c in cases if "step" in C.case_route(c)]
    assert {c[3] for c in step} >= {1, 2, 31, 32, 33, 65}
    assert {c[2] for c in cases if "mfma" in C.case_route(c)} >= {4, 8, 32, 36, 64, 96, 256}
    assert {c[2] for c in cases if "direct" in C.case_route(c)} >= {1, 3, 6, 33}
    assert {c[4] for c in cases} >= {1, 2, 3, 26}
    for cell in (R.LSTM, R.GRU, R.RNN):
        mine = [c for c in cases if c[0] == cell]
        assert {c[1] for c in mine} == {0, 1, 2} and {c[5] for c in mine} == {0, 1} == {c[6] for c in mine}
        edge = R.SEQUENCE_MAX_H[cell]
        assert R.sequence_fits(cell, edge) and not R.sequence_fits(cell, edge + 1)
        assert "sequence" in C.case_route([c for c in mine if c[2] == edge][0]) and "step" in C.case_route([c for c in mine if c[2] == edge + 1][0])
        assert {k for c in mine if c[10] == "pm80" for k in ("step", "sequence") if k in C.case_route(c)} == {"step", "sequence"}
        assert {k for c in mine if c[10] == "zero" for k in ("step", "sequence") if k in C.case_route(c)} == {"step", "sequence"}
    assert {c[8] for c in cases} == {0, 1, 2, 3} and any(c[7] for c in cases)
    assert {C.case_route(c) for c in cases} == C.targets()
    assert R.UNIT_TILE == 32 == R.SEQ_TILE  # what the batches and widths above are stated against


# ---- the switch ----------------------------------------------------------------------------------------------------------------------------
def test_tiny_crnn_loads_with_the_switches_and_is_refused_without_with_the_hint():
    (p, b, i, o), _ = C.net_model()
    net = _net(p, b)
    layers = net.layers()
    assert [(t, a) for t, _, a in layers if t in TYPES] == [("LSTM", "RNN"), ("GRU", "RNN"), ("RNN", "RNN")]
    assert [a for t, nm, a in layers if t == "InnerProduct"] == ["IM2COL"]
    msg = _refused(p, -200, "LSTM", recurrent=False)
    assert "(fhip_net_set_recurrent lifts this)" in msg
    _refused(p, -200, "fhip_net_set_detection", detection=False)  # Reshape, the first type that needs it


@pytest.mark.parametrize("type_", sorted(TYPES))
def test_default_net_refuses_the_new_types_with_the_hint_and_both_switches_are_needed(type_):
    p = _one(type_, TYPES[type_][1])
    for kw in (dict(recurrent=False), dict(recurrent=False, detection=False, transformer=False)):
        assert "(fhip_net_set_recurrent lifts this)" in _refused(p, -200, type_, **kw)
    msg = _refused(p, -200, "fhip_net_set_detection", detection=False)  # the blob ranks: the recurrent switch alone is not enough
    assert type_ in msg and "set both" in msg
    assert (type_, "l", "RNN") in _net(p).layers() and (type_, "l", "RNN") in _net(p, transformer=False).layers()


def test_on_then_off_equals_the_default_and_the_switch_is_refused_after_loadparam():
    from feathercnn_amd import FeatherHipError
    from feathercnn_amd.net import Net
    net = Net()
    net.SetRecurrent()
    net.SetRecurrent(False)
    net.SetDetection(True)
    with pytest.raises(FeatherHipError, match="code -200") as e:
        net.LoadParam(_one("GRU", TYPES["GRU"][1]))
    assert "(fhip_net_set_recurrent lifts this)" in str(e.value)
    net = _net(_one("ReLU"))
    with pytest.raises(FeatherHipError, match="before LoadParam"):
        net.SetRecurrent()
    with pytest.raises(FeatherHipError, match="before LoadParam"):
        net.SetRecurrent(False)


def test_the_route_code_the_bindings_and_the_macros():
    import feathercnn_amd
    from feathercnn_amd import _lib, net, rnn
    header = open(SC.INCLUDE + "/feather_hip/feather_rnn.h").read()
    macro = lambda name: int(re.search(r"#define\s+FHIP_RNN_%s\s+(\d+)" % name, header).group(1))
    assert macro("NET_ROUTE") == net.RNN_ROUTE == rnn.NET_ROUTE == R.NET_ROUTE == feathercnn_amd.RNN_NET_ROUTE == 114 and net.ROUTE_NAMES[114] == "RNN"
    for name, mine, theirs in (("LSTM", rnn.LSTM, R.LSTM), ("GRU", rnn.GRU, R.GRU), ("RNN", rnn.RNN, R.RNN), ("ROUTE_AUTO", rnn.ROUTE_AUTO, R.AUTO),
                               ("ROUTE_STEP", rnn.ROUTE_STEP, R.STEP), ("ROUTE_SEQUENCE", rnn.ROUTE_SEQUENCE, R.SEQUENCE), ("UNIT_TILE", rnn.UNIT_TILE, R.UNIT_TILE),
                               ("SEQ_TILE", rnn.SEQ_TILE, R.SEQ_TILE), ("MFMA_MULTIPLE", rnn.MFMA_MULTIPLE, R.MFMA_MULTIPLE), ("SEQUENCE_TILE", rnn.SEQUENCE_TILE, R.SEQUENCE_TILE),
                               ("SEQUENCE_LDS_FLOATS", rnn.SEQUENCE_LDS_FLOATS, R.SEQUENCE_LDS_FLOATS), ("SEQUENCE_MAX_N", rnn.SEQUENCE_MAX_N, R.SEQUENCE_MAX_N),
                               ("SEQUENCE_MAX_H_LSTM", rnn.SEQUENCE_MAX_H[rnn.LSTM], R.SEQUENCE_MAX_H[R.LSTM]), ("SEQUENCE_MAX_H_GRU", rnn.SEQUENCE_MAX_H[rnn.GRU], R.SEQUENCE_MAX_H[R.GRU]),
                               ("SEQUENCE_MAX_H_RNN", rnn.SEQUENCE_MAX_H[rnn.RNN], R.SEQUENCE_MAX_H[R.RNN])):
        assert macro(name) == mine == theirs, name
    assert (feathercnn_amd.LSTM, feathercnn_amd.GRU, feathercnn_amd.RNN) == (0, 1, 2) and R.SEQUENCE_LDS_FLOATS * 4 == 160 * 1024
    for cell in (R.LSTM, R.GRU, R.RNN):  # the macros are the bound's solutions, and the library's answer
        for h in (1, R.SEQUENCE_MAX_H[cell], R.SEQUENCE_MAX_H[cell] + 1, 4096):
            assert rnn.sequence_fits(cell, h) == R.sequence_fits(cell, h) == (h <= R.SEQUENCE_MAX_H[cell]), (cell, h)
    text = open(SC.INCLUDE + "/feather_hip/feather_net.h").read()
    cxx = open(SC.INCLUDE + "/feather/net.h").read()
    assert "fhip_net_set_recurrent" in text and "fhip_net_set_recurrent" in _lib.SIGNATURES and "SetRecurrent(bool on = true)" in cxx
    assert "T launches" in header  # the entry says what it enqueues
    for f in ("recurrent", "rnn_route"):
        assert callable(getattr(feathercnn_amd, f)) and f in feathercnn_amd.__all__, f
    grid = [(cell, h, n, t) for cell in (R.LSTM, R.GRU, R.RNN) for h in (1, 3, 4, 33, 96, 100, 101, 115, 116, 198, 199, 256) for n in (1, R.SEQUENCE_MAX_N, R.SEQUENCE_MAX_N + 1, 65)
            for t in (1, 26)]
    seen = set()
    for cell, h, n, t in grid:
        name = rnn.rnn_route(cell, h, n, t)
        assert name == R.route(cell, h, n, t), (cell, h, n, t)
        assert rnn.rnn_route(cell, h, n, t, rnn.ROUTE_STEP) == R.route(cell, h, n, t, R.STEP) and "step" in R.route(cell, h, n, t, R.STEP)
        seen.add(name)
    assert seen == C.targets()
    assert rnn.rnn_route(R.LSTM, 48, 1, 26) == "fhip::rnn_sequence_kernel<0>" and rnn.rnn_route(R.GRU, 6, R.SEQUENCE_MAX_N + 1, 3) == "fhip::rnn_step_direct_kernel<1>"
    assert rnn.rnn_route(R.RNN, 256, 1, 3) == "fhip::rnn_step_mfma_kernel<2>" and rnn.rnn_route(R.LSTM, 8, R.SEQUENCE_MAX_N + 1, 3, rnn.ROUTE_SEQUENCE) == "fhip::rnn_sequence_kernel<0>"


# ---- refusals at LoadParam (-100) ------------------------------------------------------------------------------------------------------
LOADPARAM_REFUSALS = [(t, params, bottoms, tops, word) for t, g in (("LSTM", 4), ("GRU", 3), ("RNN", 1)) for params, bottoms, tops, word in (
    ("", 1, 1, "num_output (0=0)"), ("0=0 1=24 2=0", 1, 1, "0=0"), ("0=-4 1=24 2=0", 1, 1, "0=-4"),
    (f"0=4 1={24 * g} 2=3", 1, 1, "2=3"), (f"0=4 1={24 * g} 2=-1", 1, 1, "2=-1"),
    ("0=4 2=0", 1, 1, "weight_data_size (1=0)"), (f"0=4 1={24 * g + 1} 2=0", 1, 1, f"1={24 * g + 1}"), ("0=4 1=-96 2=0", 1, 1, "1=-96"),
    (f"0=4 1={20 * g} 2=2", 1, 1, f"1={20 * g}"),  # a multiple of G * H, not of 2 * G * H
    (f"0=4 1={24 * g} 2=0 8=1", 1, 1, "8=1"), (f"0=4 1={24 * g} 2=0 8=2", 1, 1, "8=2"),
    (f"0=4 1={24 * g} 2=0", 4, 1, "bottoms"), (f"0=4 1={24 * g} 2=0", 1, 4, "tops"),
    (f"0=4 1={24 * g} 2=0", 3 if g != 4 else 2, 1, "bottoms"), (f"0=4 1={24 * g} 2=0", 1, 3 if g != 4 else 2, "tops"),
    (f"0={INT_MAX} 1={INT_MAX} 2=0", 1, 1, "2^31"), (f"0=46341 1={46341 * g} 2=2", 1, 1, "2^31"),
)]
LOADPARAM_REFUSALS += [("LSTM", "0=4 1=96 2=0 3=8", 1, 1, "projection"), ("LSTM", "0=4 1=96 2=0 3=0", 1, 1, "3=0"), ("LSTM", "0=4 1=96 2=0 3=-4", 1, 1, "3=-4")]


@pytest.mark.parametrize("type_,params,bottoms,tops,word", LOADPARAM_REFUSALS, ids=lambda v: str(v).replace(" ", "_"))
def test_loadparam_refusals(type_, params, bottoms, tops, word):
    msg = _refused(_one(type_, params, bottoms, tops), -100, word)
    assert "layer l" in msg and type_ in msg


def test_good_forms_load():
    """Each type at each direction and each bottom and top count; a size of 1; the LSTM with and without 3=."""
    for type_, (cell, _) in TYPES.items():
        g, full = R.GATES[cell], (3 if cell == R.LSTM else 2)
        for direction in (0, 1, 2):
            nd = 2 if direction == 2 else 1
            for bottoms in (1, full):
                for tops in (1, full):
                    for size in (1, 6):
                        params = f"0=4 1={nd * g * 4 * size} 2={direction}" + (" 3=4" if cell == R.LSTM and size == 6 else "")
                        assert (type_, "l", "RNN") in _net(_one(type_, params, bottoms, tops, w=size)).layers(), (type_, params, bottoms, tops)


def _blob(cell, nd=1, h=4, size=6, tag=0):
    """The .bin of one layer: three tagged arrays, zeros; tag 0x01306B47 writes fp16 payloads."""
    g = R.GATES[cell]
    out = b""
    for count in (nd * g * h * size, nd * (1 if cell == R.RNN else 4) * h, nd * g * h * h):
        out += struct.pack("<I", tag) + (np.full(count, 0.25, np.float16).tobytes() + bytes(-2 * count % 4) if tag else np.full(count, 0.25, F).tobytes())
    return out


@pytest.mark.parametrize("type_", sorted(TYPES))
def test_truncated_weights_fail_loadweights_naming_the_layer_and_fp16_tagged_weights_load(type_):
    from feathercnn_amd import FeatherHipError
    cell, params = TYPES[type_]
    whole = _blob(cell)
    _net(_one(type_, params), whole)
    _net(_one(type_, params), _blob(cell, tag=0x01306B47))  # fp16-tagged weights load as they do elsewhere
    g = R.GATES[cell]
    marks = (0, 3, 4, 4 + 4 * g * 4 * 6 - 1, 4 + 4 * g * 4 * 6, 4 + 4 * g * 4 * 6 + 5, len(whole) // 2, len(whole) - 4, len(whole) - 1)
    for cut in marks:
        with pytest.raises(FeatherHipError) as e:
            _net(_one(type_, params), whole[:cut])
        assert "Layer l loading weights failed" in str(e.value), (cut, str(e.value))
    with pytest.raises(FeatherHipError, match="weights have not been loaded"):
        _net(_one(type_, params)).Forward()


# ---- the zoo -------------------------------------------------------------------------------------------------------------------------------
def test_the_numpy_forward_of_tiny_crnn_has_every_blob_with_its_shape_and_rank():
    (p, b, i, o), trace = C.net_model()
    x, blobs = C.net_input(3)
    shapes = C.net_shapes()
    tops = {t for line in p.decode().splitlines()[2:] for t in line.split()[4 + int(line.split()[2]):4 + int(line.split()[2]) + int(line.split()[3])]}
    assert tops == set(shapes) == set(blobs), sorted(tops ^ set(shapes))
    for name, (chw, rank) in shapes.items():
        assert blobs[name].shape == (3,) + chw, name
        assert rank == 3 or chw[0] == 1, name  # a blob of rank 2 is [n][1][h][w]
    assert np.allclose(blobs[o].sum(axis=3), 1, atol=1e-6) and float(blobs[o].max()) < 0.9  # a softmax along the classes, not a saturated one
    assert np.array_equal(blobs["gru_h"][:, 0, 0], blobs["gru"][:, 0, 0])  # a reverse layer's final state is its output at t = 0
    text = p.decode()
    assert "LSTM bilstm 1 1 to_tokens bilstm 0=8 1=2048 2=2 3=8" in text and "GRU gru 1 2 bilstm gru gru_h 0=6 1=288 2=1" in text and "RNN rnn 1 1 gru rnn 0=8 1=48 2=0" in text
    from feathercnn_amd import model_zoo
    wide = model_zoo.tiny_crnn(size=(8, 32))
    assert wide[1] == b and [ln for ln in wide[0].splitlines() if not ln.startswith(b"Input")] == [ln for ln in p.splitlines() if not ln.startswith(b"Input")]
    (sp, sb, si, so), strace = C.states_model()
    feeds = {"data": np.ones((2, 1, 3, 5), F), "hidden": np.full((2, 1, 1, 4), 0.5, F), "cell": np.full((2, 1, 1, 4), -0.5, F)}
    got = model_zoo.numpy_forward(strace, feeds)
    assert got["l"].shape == (2, 1, 3, 4) and got["l_h"].shape == got["l_c"].shape == (2, 1, 1, 4) and np.array_equal(got["l_h"][:, 0, 0], got["l"][:, 0, -1])


def test_the_published_net_has_its_published_size():
    """CRNN (Shi et al. 2015): 8.3 million parameters.  As pytorch counts them, with the 37 classes of the released model: 8 331 301.  Here an
    LSTM direction has one bias where torch has two (4 x 4 x 256 fewer), the first convolution reads three channels (1152 more) and a BatchNorm
    carries its mean and variance (2 x 1280 more); the .bin adds a 4-byte tag per tagged array."""
    from feathercnn_amd import model_zoo
    p, nbytes, i, o = model_zoo.crnn_vgg_bilstm(dry=True)
    text = p.decode()
    published = 8331301
    tags = text.count("Convolution ") + text.count("InnerProduct ") + 3 * text.count("LSTM ")
    assert (nbytes - 4 * tags) // 4 == published - 4 * 4 * 256 + 1152 + 2 * 1280
    assert abs(nbytes / 4 - 8.3e6) / 8.3e6 < 0.01
    assert text.count("LSTM ") == 2 and "LSTM bilstm1 1 1 to_tokens bilstm1 0=256 1=1048576 2=2 3=256" in text and "0=256 1=524288 2=2 3=256" in text
    assert text.count("Convolution ") == 7 and text.count("BatchNorm ") == 3 and "InnerProduct embed2 1 1 bilstm2 embed2 0=37" in text
    assert "Pooling pool3 1 1 pad3 pool3 0=0 1=2 11=2 2=1 12=2" in text and text.count("Padding ") == 2  # 2 x 2, stride (2, 1), pad (0, 1)
    p, nbytes, i, o = model_zoo.crnn_lite_lstm(dry=True)
    assert p.decode().count("LSTM ") == 1 and "0=48 1=36864 2=2 3=48" in p.decode() and nbytes < 2 ** 20
    for hidden in (48, 96):  # what a small batch takes: the sequence route
        assert "sequence" in R.route(R.LSTM, hidden, 1, 26) and "sequence" in R.route(R.LSTM, hidden, 4, 26)


# ---- the library's refusals on the host --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    return SC.library("rnn")


A, B, D, E = (ctypes.c_void_p(0x100000 + 0x40000 * k) for k in range(4))  # aligned addresses that are never dereferenced: every call below is refused first
ODD = ctypes.c_void_p(0x100002)


def _bad(lib, rc, word=""):
    assert rc == SC.BADARG, rc
    msg = lib.fhip_rnn_last_error().decode()
    assert msg and word in msg, msg


def test_the_library_refuses_on_the_host(lib):
    def fwd(cell=0, direction=0, n=2, t=3, h=4, xp=A, xs=None, wh=B, bn=None, h0=None, c0=None, out=D, os_=None, hn=None, cn=None, cs=E, route=None):
        nd, g = (2 if direction == 2 else 1), {0: 4, 1: 3, 2: 1}.get(cell, 1)
        args = (cell, direction, n, t, h, xp, nd * g * h if xs is None else xs, wh, bn, h0, c0, out, nd * h if os_ is None else os_, hn, cn, cs, None)
        return lib.fhip_rnn_forward(*args) if route is None else lib.fhip_rnn_forward_route(*args, route)
    for kw in (dict(n=0), dict(t=0), dict(h=0), dict(n=-1), dict(t=-3), dict(h=-4)):
        _bad(lib, fwd(**kw), "< 1")
    _bad(lib, fwd(xs=15), "xp_stride")
    _bad(lib, fwd(direction=2, xs=16), "xp_stride")
    _bad(lib, fwd(os_=3), "out_stride")
    _bad(lib, fwd(direction=2, os_=4), "out_stride")
    _bad(lib, fwd(n=1 << 16, t=1 << 15), "2^31")  # the rows themselves
    _bad(lib, fwd(n=1 << 14, t=1 << 13, h=4), "2^31")  # rows * xp_stride
    _bad(lib, fwd(cell=2, n=1 << 14, t=1 << 13, h=4, os_=16), "2^31")  # strides included
    _bad(lib, fwd(h=1 << 15), "2^31")  # Wh
    for cell in (-1, 3, 9):
        _bad(lib, fwd(cell=cell), "cell")
    for direction in (-1, 3):
        _bad(lib, fwd(direction=direction), "direction")
    for route in (-1, 3):
        _bad(lib, fwd(route=route), "route")
    _bad(lib, fwd(h=104, route=R.SEQUENCE), "sequence route")
    _bad(lib, fwd(xp=None), "null")
    _bad(lib, fwd(wh=None), "null")
    _bad(lib, fwd(out=None), "null")
    _bad(lib, fwd(cs=None), "null")  # the LSTM's cell scratch
    _bad(lib, fwd(cell=1), "null")  # the GRU's bn
    for kw in (dict(xp=ODD), dict(wh=ODD), dict(out=ODD), dict(h0=ODD), dict(c0=ODD), dict(hn=ODD), dict(cn=ODD), dict(cs=ODD), dict(cell=1, bn=ODD)):
        _bad(lib, fwd(**kw), "aligned")
    _bad(lib, fwd(out=A), "overlap")
    _bad(lib, fwd(out=ctypes.c_void_p(A.value + 4 * 2 * 3 * 16 - 4)), "overlap")  # the last float of xp
    name = ctypes.create_string_buffer(64)
    _bad(lib, lib.fhip_rnn_route(0, 4, 1, 1, 0, None, 64), "null")
    _bad(lib, lib.fhip_rnn_route(0, 4, 1, 1, 0, name, 0), "null")
    _bad(lib, lib.fhip_rnn_route(3, 4, 1, 1, 0, name, 64), "cell")
    _bad(lib, lib.fhip_rnn_route(0, 0, 1, 1, 0, name, 64), "< 1")
    _bad(lib, lib.fhip_rnn_route(0, 4, 1, 1, 5, name, 64), "route")
    _bad(lib, lib.fhip_rnn_route(0, 101, 1, 1, 2, name, 64), "sequence route")
    assert lib.fhip_rnn_sequence_fits(7, 4) == 0 and lib.fhip_rnn_sequence_fits(0, 0) == 0 and lib.fhip_rnn_sequence_fits(0, -5) == 0 and lib.fhip_rnn_sequence_fits(2, INT_MAX) == 0


# ---- the readers on hostile files, host side under sanitizers ------------------------------------------------------------------------------
HOSTILE = ("-1", "0", "1", "7", str(INT_MAX), str(-INT_MAX - 1), "-233", "65536", "46341", "3.5", "-1.0", "1e38", "inf.0", "nan.0", "1e-46", "")


def _hostile_cases():
    """-> [(param, bin, must_load)]: tiny_crnn as it is; every value of every param of its recurrent layers replaced by each of HOSTILE, and
    absent ids (3, 8 and others) added; other bottom and top counts; the .bin cut at many places."""
    (p, b, i, o), _ = C.net_model()
    lines = p.decode().splitlines()
    cases = [(p, b, True)]
    for at, line in enumerate(lines):
        tok = line.split()
        if tok[0] not in TYPES:
            continue
        first = 4 + int(tok[2]) + int(tok[3])
        ids = [t.split("=")[0] for t in tok[first:]]
        for position in range(len(ids)):
            for value in HOSTILE:
                t = list(tok)
                t[first + position] = ids[position] + "=" + value
                cases.append(("\n".join(lines[:at] + [" ".join(t)] + lines[at + 1:]).encode() + b"\n", b, False))
        for absent in [i_ for i_ in (3, 8, 4, 31) if str(i_) not in ids][:3]:
            for value in HOSTILE:
                cases.append(("\n".join(lines[:at] + [" ".join(tok + [f"{absent}={value}"])] + lines[at + 1:]).encode() + b"\n", b, False))
        for counts in ((0, 1), (2, 1), (1, 0), (4, 1), (1, 4), (3, 3)):
            t = list(tok)
            t[2], t[3] = str(counts[0]), str(counts[1])
            cases.append(("\n".join(lines[:at] + [" ".join(t)] + lines[at + 1:]).encode() + b"\n", b, False))
    for cut in sorted({0, 3, 4, len(b) // 7, len(b) // 3, len(b) // 2, len(b) - 4, len(b) - 1} | {64 * k + 2 for k in range(0, len(b) // 64, 5)}):
        cases.append((p, b[:cut], False))
    cases.append((p, b + b"\0\0\0\0", True))  # more than the net reads is no error (ncnn's readers stop where the layers do)
    return cases


def _judge(cases, stdout):
    lines = [l for l in stdout.splitlines() if l.startswith("case ")]
    assert len(lines) == len(cases), f"{len(lines)} lines for {len(cases)} cases"
    loaded = 0
    for k, ((p, b, must_load), line) in enumerate(zip(cases, lines)):
        m = re.match(r"case (\d{4}) param (-?\d+) weights (-?\d+|skip) \| (.*)$", line)
        assert m and int(m.group(1)) == k, line
        refused = int(m.group(2)) or (int(m.group(3)) if m.group(3) != "skip" else 0)
        assert not (must_load and refused), f"the control did not load: {line}"
        assert not refused or m.group(4).strip(), f"refused without a message: {line}"
        if len(b) < len(cases[0][1]):
            assert refused, f"a truncated weight file loaded: {line}"
        loaded += not refused
    return loaded


def test_the_new_readers_on_hostile_files_plain_and_under_sanitizers(tmp_path):
    """The table once through a plain build against the library as built, once through a build whose host side runs under ASan and UBSan:
    a stand-alone program with its own main, never loaded into python."""
    from feathercnn_amd import _lib
    cases = _hostile_cases()
    assert 300 <= len(cases) <= 4000
    d = tmp_path / "cases"
    d.mkdir()
    for k, (p, b, _) in enumerate(cases):
        (d / f"{k:04d}.param").write_bytes(p)
        (d / f"{k:04d}.bin").write_bytes(b)
    driver = os.path.join(ROOT, "tests", "cpp", "rnn_loader_hostile_main.cpp")
    libdir = os.path.dirname(_lib.lib_path())
    exe = str(tmp_path / "rnn_loader_hostile")
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), driver, "-o", exe, "-L" + libdir, "-lfeather_hip", "-Wl,-rpath," + libdir],
                   check=True, capture_output=True, text=True)
    out = subprocess.run([exe, str(d), str(len(cases))], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    loaded = _judge(cases, out.stdout)
    print(f"{len(cases)} hostile cases, {loaded} loaded")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    objdir = str(tmp_path / "obj")
    san = "-fsanitize=address,undefined"
    host = f"-Xarch_host {san} -Xarch_host -fno-sanitize-recover=undefined -g"
    subprocess.run(["make", "-s", "-j", str(min(8, os.cpu_count() or 1)), "-C", os.path.join(ROOT, "feathercnn_amd", "csrc"), "OBJDIR=" + objdir, "EXTRA=" + host, "objects"],
                   check=True, capture_output=True, text=True)
    objs = sorted(os.path.join(objdir, f) for f in os.listdir(objdir) if f.endswith(".o"))
    exe = str(tmp_path / "rnn_loader_hostile_san")
    subprocess.run([hipcc, "-std=c++17", "-O1", "-g", "-Xarch_host", san, "-Xarch_host", "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"),
                    "-x", "c++", driver, "-x", "none"] + objs + [san, "-o", exe, "-ldl"], check=True, capture_output=True, text=True)
    out = subprocess.run([exe, str(d), str(len(cases))], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    assert "ERROR: AddressSanitizer" not in out.stderr and "runtime error:" not in out.stderr and "LeakSanitizer" not in out.stderr, out.stderr[-3000:]
    assert _judge(cases, out.stdout) == loaded
