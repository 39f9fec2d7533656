"""The decoder layers on the device: libfeather_decoder.so through its C-ABI from guarded buffers (the attention core) and through
feathercnn_amd.decoder (the small kernels), against the float64 restatement tests/decoder_ref.py by the project's normalised error and its
bound TOL = 1e-4.  One kernel trace: the sweep launches what fhip_decoder_route names, and that is every instantiation of the library."""
import numpy as np
import pytest

import decoder_cases as C
import decoder_ref as R
import kernel_instances as KI
import ktrace
import side_contract

pytestmark = pytest.mark.gpu
F = np.float32

lib = side_contract.fixture("decoder", gpu=True)


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("layout", ["dense", "cache"])
@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_sdpa_equals_the_float64_restatement(lib, case, layout, offset):
    want = C.case_data(case)[5]
    got, route, splits = C.run(lib, case, layout, offset)
    err = R.normalised_error(got, want)
    print(f"sdpa {C.case_id(case)} {layout} offset {offset} on {route}, {splits} split(s): error {err:.3g} (bound {C.TOL:g})")
    assert route in C.targets() and (case[10] == 0 or splits == min(case[10], (case[1] + 31) // 32))
    assert err <= C.TOL, (case, err)
    if case[7] and case[0] > 1:
        assert not got[:, :, 0].any()  # the fully masked row is zeros, not NaN


def test_the_splits_agree_with_each_other(lib):
    one, three, many = (C.run(lib, c)[0] for c in C.CASES if c[:8] == (1, 70, 64, 8, 2, 2, 0, None))
    assert R.normalised_error(three, one) <= C.TOL and R.normalised_error(many, one) <= C.TOL


def test_the_python_mirror_and_the_auto_rule(cuda):
    import torch
    from feathercnn_amd import decoder as D
    q, k, v, m, scale, want = C.case_data(C.CASES[11])  # a mask per head and image, group 2
    qkv = [torch.from_numpy(a).cuda() for a in (q, k, v, m)]
    assert R.normalised_error(D.sdpa(*qkv, scale=float(scale)).cpu().numpy(), want) <= C.TOL
    rng = np.random.default_rng(5)
    q, k, v = (rng.uniform(-1, 1, s).astype(F) for s in ((1, 8, 1, 64), (1, 2, 1024, 64), (1, 2, 1024, 64)))  # decoding: 2 blocks, 32 key tiles
    cache = torch.from_numpy(np.stack([k, v])).cuda()
    desc = D.SdpaDesc(n=1, heads=8, kv_heads=2, tq=1, tk=1024, d=64, q_row_stride=64, k_row_stride=64, v_row_stride=64, out_row_stride=64, scale=0.125)
    assert D.sdpa_plan(desc)[1] == 16 == min(-(-D.SPLIT_TARGET // 2), 32 // D.SPLIT_MIN_TILES)  # the auto rule
    got = D.sdpa(torch.from_numpy(q).cuda(), cache[0], cache[1])
    assert R.normalised_error(got.cpu().numpy(), R.sdpa(q, k, v)) <= C.TOL


def test_kv_concat_and_embed_are_bit_copies(cuda):
    import torch
    from feathercnn_amd import decoder as D
    rng = np.random.default_rng(6)
    for d, tp in ((8, 5), (6, 5), (8, 0)):  # 16-byte units, 4-byte units, no past
        past, fresh = rng.uniform(-1, 1, (2, 3, tp, d)).astype(F), rng.uniform(-1, 1, (2, 3, 2, d)).astype(F)
        got = D.kv_concat(torch.from_numpy(past).cuda() if tp else None, torch.from_numpy(fresh).cuda())
        assert np.array_equal(got.cpu().numpy().view(np.uint32), R.kv_concat(past if tp else None, fresh).view(np.uint32)), (d, tp)
    weight, bias = rng.uniform(-1, 1, (50, 33)).astype(F), rng.uniform(-1, 1, 33).astype(F)
    ids = np.array([[0, 49, -1, 50, 7], [2 ** 31 - 1, -2 ** 31, 3, 3, 48]], np.int32)  # -1 and vocab are clamped
    for b in (None, bias):
        got = D.embed(torch.from_numpy(ids).cuda(), torch.from_numpy(weight).cuda(), None if b is None else torch.from_numpy(b).cuda())
        assert got.shape == (2, 5, 33) and np.array_equal(got.cpu().numpy().view(np.uint32), R.embed(ids, weight, b).view(np.uint32))


@pytest.mark.parametrize("l", [1, 2, 64, 65, 256, 257, 1025])  # 256 / 257: the last row a wave takes and the first a block takes
@pytest.mark.parametrize("rows", [1, 3])
def test_rms_norm_equals_float64(cuda, rows, l):
    import torch
    from feathercnn_amd import decoder as D
    rng = np.random.default_rng(100 * l + rows)
    x, gamma = rng.uniform(-1, 1, (rows, l)).astype(F), rng.uniform(0.5, 1.5, l).astype(F)
    x[-1] *= F(1e4)  # a row of magnitude 10^4
    for g in (None, gamma):
        got = D.rms_norm(torch.from_numpy(x).cuda(), None if g is None else torch.from_numpy(g).cuda(), 1e-5)
        for i in range(rows):  # row by row: the small rows are not hidden behind the large one
            assert R.normalised_error(got.cpu().numpy()[i], R.rms_norm(x, g, 1e-5)[i]) <= C.TOL, (rows, l, i)
    assert D.decoder_route(D.RMS_NORM, l) == D.route_rule(D.RMS_NORM, l)


@pytest.mark.parametrize("d", [2, 4, 64])
@pytest.mark.parametrize("t", [1, 3])
@pytest.mark.parametrize("interleaved", [0, 1])
def test_rotary_equals_float64(cuda, interleaved, t, d):
    import torch
    from feathercnn_amd import decoder as D
    rng = np.random.default_rng(1000 * d + 10 * t + interleaved)
    x, angle = rng.uniform(-1, 1, (2, 3, t, d)).astype(F), rng.uniform(-3, 3, (2, t, d // 2))
    for per_image in (False, True):
        cos, sin = (f(angle if per_image else angle[0]).astype(F) for f in (np.cos, np.sin))
        got = D.rotary(*(torch.from_numpy(a).cuda() for a in (x, cos, sin)), interleaved=bool(interleaved))
        assert R.normalised_error(got.cpu().numpy(), R.rotary(x, cos, sin, bool(interleaved))) <= C.TOL, per_image


# ---- the net -----------------------------------------------------------------------------------------------------------------------------
def _net(param, weights=b"", graph=False):
    from feathercnn_amd.net import Net
    net = Net(fusion=1, graph=graph)
    net.SetDecoder()
    net.SetTransformer()
    net.SetDetection(True)
    net.LoadParam(param)
    net.LoadWeights(weights)
    return net


def _feed(net, ids, cos, sin, mask, past=()):
    n = ids.shape[0]
    tile = lambda a: np.broadcast_to(a.astype(F), (n, 1) + a.shape)  # noqa: E731
    feeds = dict(ids=ids.astype(np.int32).view(F).reshape(n, 1, 1, -1), cos=tile(cos), sin=tile(sin), mask=tile(mask))
    for b, (k, v) in enumerate(past):
        feeds[f"past_k{b}"], feeds[f"past_v{b}"] = k, v
    for name, x in feeds.items():
        net.FeedInput(name, np.ascontiguousarray(x))
    net.Forward()
    return net.Extract("logits")[:, 0]


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("batch", [1, 2])
def test_tiny_llama_prefill_then_decode(cuda, batch, graph):
    """A prefill of 7 tokens, then 3 decode steps feeding the caches back: every step's logits against tiny_llama_forward, the decode logits
    against one 10-token prefill, with and without the graph (a replay gives the same bits); every new layer reports the new route."""
    from feathercnn_amd import model_zoo as Z
    W = {}
    pp, dp, wb = Z.tiny_llama(trace=W)
    ids = np.random.default_rng(30 + batch).integers(0, 50, (batch, 10))
    angle = np.outer(np.arange(10), 10000.0 ** (-np.arange(4) / 4))
    cos, sin = np.cos(angle), np.sin(angle)
    causal = np.where(np.tril(np.ones((10, 10))) > 0, 0.0, -np.inf)
    whole = Z.tiny_llama_forward(W, ids, cos, sin, causal)[0]
    want, ref_past = Z.tiny_llama_forward(W, ids[:, :7], cos[:7], sin[:7], causal[:7, :7])
    prefill, decode = _net(pp, wb, graph), _net(dp, wb, graph)
    got = _feed(prefill, ids[:, :7], cos[:7], sin[:7], causal[:7, :7])
    past = [(prefill.Extract(f"b{b}_krot"), prefill.Extract(f"b{b}_vh")) for b in range(2)]
    errs = [R.normalised_error(got, want)]
    for t in range(7, 10):
        got = _feed(decode, ids[:, t:t + 1], cos[t:t + 1], sin[t:t + 1], np.zeros((1, t + 1)), past)
        if graph:
            decode.Forward()
            assert np.array_equal(decode.Extract("logits")[:, 0], got)
        want, ref_past = Z.tiny_llama_forward(W, ids[:, t:t + 1], cos[t:t + 1], sin[t:t + 1], np.zeros((1, t + 1)), ref_past)
        errs += [R.normalised_error(got, want), R.normalised_error(got, whole[:, t:t + 1])]
        past = [(decode.Extract(f"b{b}_present_k"), decode.Extract(f"b{b}_present_v")) for b in range(2)]
        assert past[0][0].shape == (batch, 2, t + 1, 8)
    print(f"tiny_llama batch {batch} graph {graph}: the worst logits are within {max(errs):.3g} (bound {C.TOL:g})")
    assert max(errs) <= C.TOL, errs
    for net in (prefill, decode):
        assert {a for t, _, a in net.layers() if t in ("SDPA", "RMSNorm", "RotaryEmbed", "Embed")} == {"DECODER"}


X = np.random.default_rng(9).uniform(-1, 1, (2, 4, 6, 8)).astype(F)
RESHAPE_REFUSALS = {
    "sdpa_dv_is_not_d": ("SDPA l 3 1 q k v top", dict(q=X, k=X[:, :2], v=X[:, :2, :, :4]), "dv"),
    "sdpa_rank": ("SDPA l 3 1 q2 k v top", dict(q=X, k=X, v=X), "rank 2"),
    "sdpa_heads_no_multiple": ("SDPA l 3 1 q k v top", dict(q=X, k=X[:, :3], v=X[:, :3]), "multiple"),
    "sdpa_mask_does_not_fit": ("SDPA l 4 1 q k v m top 5=1", dict(q=X, k=X, v=X, m=X[:, :1, :, :5]), "mask"),
    "sdpa_d_refused": ("SDPA l 3 1 q k v top", dict(q=X[..., :6], k=X[..., :6], v=X[..., :6]), "multiple of 4"),
    "sdpa_past_does_not_fit": ("SDPA l 5 3 q k v a b top pk pv 7=1", dict(q=X, k=X, v=X, a=X[:, :2], b=X), "past"),
    "rms_norm_width": ("RMSNorm l 1 1 q top 0=7 2=0", dict(q=X), "affine_size 7"),
    "rotary_tables": ("RotaryEmbed l 3 1 q k v top", dict(q=X, k=X[:, :1, :, :4], v=X[:, :1, :, :3]), "cos and sin"),
}


@pytest.mark.parametrize("name", sorted(RESHAPE_REFUSALS))
def test_reshape_refusals(cuda, name):
    from feathercnn_amd import FeatherHipError
    line, feeds, word = RESHAPE_REFUSALS[name]
    lines = ["Input %s 0 1 %s" % (b, b) for b in "qkvmab"] + ["Reshape q2 1 1 q q2 0=-1 1=8", line]
    net = _net(("7767517\n%d %d\n" % (len(lines), len(lines) + 2) + "\n".join(lines) + "\n").encode())
    for b, x in dict(dict.fromkeys("qkvmab", X), **feeds).items():  # every Input is fed: those a case does not name, with X
        net.FeedInput(b, np.ascontiguousarray(x))
    with pytest.raises(FeatherHipError, match="code -100") as e:
        net.Forward()
    assert "layer l" in str(e.value) and word in str(e.value), str(e.value)


def test_the_sweep_launches_what_the_route_names(cuda, tmp_path):
    """One child under rocprofv3 --kernel-trace (tests/decoder_trace_child.py): the library's kernels in the trace are, launch for launch, the
    routes fhip_decoder_route named, and together every instantiation tests/decoder_cases.targets() names -- which is every instantiation
    the library holds (tests/test_later_contract_cpu.py)."""
    text, rows, _ = ktrace.trace("decoder_trace_child.py", [], tmp_path, 240)
    named = [ln[len("route "):] for ln in text.splitlines() if ln.startswith("route ")]
    launched = [nm for nm in (KI.normalise(name) for _, name, *_ in rows) if nm in C.targets()]
    assert launched == named, (launched, named)
    assert set(launched) == C.targets()
