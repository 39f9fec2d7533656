"""The transformer layers on the device: libfeather_attn.so through its C-ABI from guarded buffers (tests/guarded.py, element offsets 0 .. 3),
and tiny_vit through feather::Net.

* Attention against the float64 restatement (tests/attn_ref.py) by the project's normalised error and its bound TOL = 1e-4
  (tests/test_net_gpu.py): every case of tests/attn_cases.ATTENTION_CASES -- both routes, dense and strided inputs, scores that reach +-80, a row
  of equal scores.  The worst error observed is printed (DESIGN.md 3.28 records it).
* LayerNorm against float64 at TOL, rows of mean 10^4 included; the add + LayerNorm entry equals the two calls bit for bit.
* GELU at TOL and on +-0, +-inf, NaN; the binary operations bit for bit against numpy float32 (div at TOL), every operand form, misaligned.
* One kernel trace: the sweep launches what fhip_attn_route names, and that is every instantiation of the library.
* tiny_vit against model_zoo.numpy_forward at TOL at fusion 0 .. 3, with and without the graph, 1 and 2 sub-batch replicas, batch 1 and 3;
  fusion 2 equals fusion 1 bit for bit; a re-plan to another input size and back; the route of every new layer.
* What only a Reshape can refuse (-100: LayerNorm sizes, MultiHeadAttention ranks, widths and bottoms that do not fit, BinaryOp shapes) and
  the forms only a Reshape accepts; a q8 bottom in front of every new type (-300); the SE block of a net with the switch."""
import numpy as np
import pytest

import attn_cases as C
import attn_ref as R
import attn_sweep as SW
import kernel_instances as KI
import ktrace
import side_contract

pytestmark = pytest.mark.gpu
F = np.float32
TOL = SW.TOL  # the project's bound (tests/test_net_gpu.py)

lib = side_contract.fixture("attn", gpu=True)


# ---- the C-ABI ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.ATTENTION_CASES, ids=C.attention_id)
def test_attention_equals_the_float64_restatement(lib, case):
    tq, tk, d, heads, n, layout, offset, kind = case
    q, k, v, want = C.attention_case(case)
    got = SW.attention(lib, q, k, v, heads, layout, offset)
    err = R.normalised_error(got, want)
    print(f"attention {C.attention_id(case)} on {SW.route(lib, C.ATTENTION, d * heads, heads)}: error {err:.3g} (bound {TOL:g})")
    assert SW.route(lib, C.ATTENTION, d * heads, heads) == R.attention_route(d * heads, heads)
    assert err <= TOL, (case, err)


def test_the_python_mirror(cuda):
    import torch
    from feathercnn_amd import attn
    case = [c for c in C.ATTENTION_CASES if c[5] == "fused" and c[2] == 64][0]
    q, k, v, want = C.attention_case(case)
    qkv = torch.from_numpy(np.concatenate([q, k, v], axis=2)).cuda()
    e = q.shape[2]
    got = attn.attention(qkv[:, :, :e], qkv[:, :, e:2 * e], qkv[:, :, 2 * e:], case[3])
    assert R.normalised_error(got.cpu().numpy(), want) <= TOL
    x, gamma, beta = (torch.tensor(t).cuda() for t in C.layer_norm_case(197, 192))
    s, y = attn.add_layer_norm(x, x.flip(0).contiguous(), gamma, beta)
    assert torch.equal(s, attn.binary(attn.ADD, x, x.flip(0).contiguous())) and torch.equal(y, attn.layer_norm(s, gamma, beta))
    assert torch.equal(attn.binary(attn.MUL, x, 0.5), x * 0.5) and torch.equal(attn.binary(attn.SUB, x, gamma, swap=True), gamma - x)
    assert R.normalised_error(attn.gelu(x).cpu().numpy(), R.gelu(x.cpu().numpy())) <= TOL


@pytest.mark.parametrize("l", C.LN_LENGTHS)
def test_layer_norm_equals_float64_and_the_add_form_equals_the_pair(lib, l):
    for rows in C.LN_ROWS:
        for k, offset_mean in enumerate((False, True)):
            x, gamma, beta = C.layer_norm_case(rows, l, offset_mean)
            offset = (l + rows + k) % 4
            affine = (gamma, beta) if k == 0 else (None, None)
            got = SW.layer_norm(lib, x, *affine, offset=offset)
            want = R.layer_norm(x, *affine)
            if l > 1 or not offset_mean:
                assert R.normalised_error(got, want) <= TOL, (rows, l, offset_mean, R.normalised_error(got, want))
            else:
                assert np.array_equal(got, np.zeros_like(got))  # a row of one element is its own mean
            assert SW.route(lib, C.LAYER_NORM, l, 0) == "fhip::layer_norm_kernel<%d, 0>" % int(l > R.LN_WAVE_MAX)
        x, gamma, beta = C.layer_norm_case(rows, l)
        other = np.ascontiguousarray(x[::-1, ::-1])
        s, y = SW.add_layer_norm(lib, x, other, gamma, beta, offset=l % 4)
        assert SW.same_bits(s, SW.binary(lib, R.ADD, x, other)) and SW.same_bits(s, x + other)
        assert SW.same_bits(y, SW.layer_norm(lib, s, gamma, beta, offset=(l + 1) % 4)), (rows, l)  # bit for bit, whatever the alignment


def test_gelu(lib):
    x = np.concatenate([np.random.default_rng(3).uniform(-6, 6, 1023).astype(F), np.linspace(-12, 12, 49).astype(F)])
    for fast in (0, 1):
        for offset in range(4):
            got = SW.gelu(lib, x[offset:], fast, offset)
            assert R.normalised_error(got, R.gelu(x[offset:], bool(fast))) <= TOL, (fast, offset)
            assert SW.route(lib, C.GELU, fast, int(offset == 0)) == "fhip::gelu_kernel<%d, %d>" % (fast, int(offset == 0))
        got, want = SW.gelu(lib, C.SPECIALS, fast), R.gelu(C.SPECIALS, bool(fast))
        assert np.array_equal(got[:2].view(np.uint32), [0, 0x80000000]) and np.array_equal(want[:2].astype(F).view(np.uint32), [0, 0x80000000])  # +0 and -0, by their bits
        assert got[2] == np.inf and np.isnan(got[3]) == np.isnan(want[3]) and np.isnan(got[4]), (fast, got, want)


@pytest.mark.parametrize("count", C.BINARY_COUNTS)
def test_binary_is_exact(lib, count):
    rng = np.random.default_rng(40 + count)
    a = rng.uniform(-2, 2, (3, count)).astype(F)
    full, image = rng.uniform(0.5, 2, (3, count)).astype(F), rng.uniform(0.5, 2, count).astype(F)
    for op in range(6):
        for k, (b, swap) in enumerate(((F(1.5), 0), (full, 0), (image, 0), (image, 1), (full, 1), (F(0.75), 1))):
            for offset, b_offset in ((0, 0), ((op + k) % 3 + 1, (op + k) % 4), (0, 2)):
                got = SW.binary(lib, op, a, float(b) if np.isscalar(b) or b.ndim == 0 else b, swap, offset, b_offset)
                want = R.binary(op, a, b, bool(swap))
                if op == R.DIV:
                    assert R.normalised_error(got, want) <= TOL, (op, k, offset)
                else:
                    assert SW.same_bits(got, want), (op, k, offset, b_offset)
    specials = np.array([[0.0, -0.0, np.inf, np.nan, 1.0]], F)
    for op in (R.MAX, R.MIN):  # fmaxf / fminf: a NaN operand gives the other one
        assert np.array_equal(SW.binary(lib, op, specials, 0.5), R.binary(op, specials, F(0.5)))


def test_the_sweep_launches_what_the_route_names(cuda, tmp_path):
    """One child under rocprofv3 --kernel-trace (tests/attn_trace_child.py): the library's kernels in the trace are, launch for launch, the
    routes fhip_attn_route named, and together every instantiation tests/attn_cases.targets() names -- which is every instantiation the
    library holds (tests/test_later_contract_cpu.py)."""
    text, rows, _ = ktrace.trace("attn_trace_child.py", [], tmp_path, 240)
    named = [ln[len("route "):] for ln in text.splitlines() if ln.startswith("route ")]
    launched = [KI.normalise(name) for _, name, *_ in rows]
    launched = [nm for nm in launched if nm in C.targets()]
    assert launched == named, (launched, named)
    assert set(launched) == C.targets()


# ---- the net -----------------------------------------------------------------------------------------------------------------------------
def _net(level=2, graph=False, replicas=1, model=None):
    from feathercnn_amd.net import Net
    p, b, i, o = model or C.net_model()[0]
    net = Net(fusion=level, graph=graph, sub_batches=replicas)
    net.SetTransformer()
    net.SetDetection(True)
    net.SetFrame()
    net.LoadParam(p)
    net.LoadWeights(b)
    return net


def _run(net, batch=3, size=16):
    (p, b, i, o), _ = C.net_model()
    x, want = C.net_input(batch, size)
    net.FeedInput(i, x)
    net.Forward()
    return want, net.Extract(o)


def test_tiny_vit_every_blob_at_level_0(cuda):
    (p, b, i, o), _ = C.net_model()
    net = _net(0)
    want, out = _run(net)
    worst = 0.0
    for name, (chw, rank) in C.net_shapes().items():
        got = net.Extract(name)
        assert got.shape == (3,) + chw == want[name].shape, name
        err = R.normalised_error(got, want[name])
        worst = max(worst, err)
        assert err <= TOL, (name, err)
    print(f"tiny_vit level 0: the worst blob is within {worst:.3g} of the float64 forward (bound {TOL:g})")
    new = {"MemoryData", "LayerNorm", "GELU", "MultiHeadAttention", "BinaryOp"}
    routes = {(t, a) for t, _, a in net.layers() if t in new}
    assert routes == {(t, "ATTN") for t in new}, routes
    assert {a for t, nm, a in net.layers() if t == "InnerProduct"} == {"IM2COL"}


def test_tiny_vit_at_every_setting(cuda):
    (p, b, i, o), _ = C.net_model()
    outs = {}
    for level, graph, replicas, batch in ((0, False, 1, 3), (1, False, 1, 3), (2, False, 1, 3), (3, False, 1, 3), (2, True, 1, 3), (3, True, 2, 3), (1, False, 2, 3), (0, True, 1, 1),
                                          (1, False, 1, 1), (2, False, 1, 1), (2, True, 2, 1)):
        net = _net(level, graph, replicas)
        want, out = _run(net, batch)
        if graph:  # replay the captured graph
            net.Forward()
            assert np.array_equal(net.Extract(o), out)
        err = R.normalised_error(out, want[o])
        print(f"tiny_vit level {level} graph {graph} replicas {replicas} batch {batch}: error {err:.3g} against the float64 forward (bound {TOL:g})")
        assert out.shape == want[o].shape == (batch, 10, 1, 1) and err <= TOL, (level, graph, replicas, batch, err)
        names = [nm for _, nm, _ in net.layers()]
        assert ("blk0_ln2" in names) == (level < 2) and ("norm" in names)  # level 2 runs the LayerNorm behind a residual add with the add
        if replicas == 1 and not graph:
            outs[(level, batch)] = out, net.Extract("blk1_ln2"), net.Extract("blk1_add1")
    for batch in (1, 3):  # fusion 2 equals fusion 1 bit for bit: the output, a fused LayerNorm's top and the sum it normalises
        for got, ref in zip(outs[(2, batch)], outs[(1, batch)]):
            assert SW.same_bits(got, ref), batch
    assert SW.same_bits(outs[(3, 3)][0], outs[(2, 3)][0])


def test_tiny_vit_replans_to_another_input_size_and_back(cuda):
    (p, b, i, o), _ = C.net_model()
    from feathercnn_amd import FeatherHipError, model_zoo
    wide_p, wide_b = model_zoo.tiny_vit(size=(8, 32))[:2]  # 2 x 8 patches: another input size, the same 17 tokens, the same file but for the Input's line
    assert wide_b == b and [ln for ln in wide_p.splitlines() if not ln.startswith(b"Input")] == [ln for ln in p.splitlines() if not ln.startswith(b"Input")]
    for graph in (False, True):
        net = _net(2, graph=graph)
        want16, first = _run(net, 3, 16)
        want_wide, wide = _run(net, 3, (8, 32))
        assert R.normalised_error(wide, want_wide[o]) <= TOL and net.Extract("patch_embed").shape == (3, 16, 2, 8)
        _, again = _run(net, 3, 16)
        assert SW.same_bits(again, first) and R.normalised_error(first, want16[o]) <= TOL
        x24 = np.zeros((3, 3, 24, 24), F)  # 6 x 6 patches: the position embedding no longer fits the tokens
        net.FeedInput(i, x24)
        with pytest.raises(FeatherHipError, match="code -100"):
            net.Forward()
        _, again = _run(net, 3, 16)
        assert SW.same_bits(again, first)


def test_tiny_vit_replans_to_another_batch_and_back(cuda):
    (p, b, i, o), _ = C.net_model()
    for graph in (False, True):
        net = _net(2, graph=graph)
        want3, first = _run(net, 3)
        want1, one = _run(net, 1)
        _, again = _run(net, 3)
        assert R.normalised_error(one, want1[o]) <= TOL and one.shape == (1, 10, 1, 1)
        assert SW.same_bits(again, first) and R.normalised_error(first, want3[o]) <= TOL
        assert net.Extract("pos_embed").shape == (3, 1, 17, 16) and SW.same_bits(net.Extract("pos_embed"), want3["pos_embed"])


# ---- what only a Reshape can refuse --------------------------------------------------------------------------------------------------------
def _param(lines):
    tops = sum(int(ln.split()[3]) for ln in lines)
    return ("7767517\n%d %d\n" % (len(lines), tops) + "\n".join(lines) + "\n").encode()


def _mha_weights(e):
    import struct
    return (struct.pack("<I", 0) + b"\0" * (4 * e * e) + b"\0" * (4 * e)) * 4


def _planned(lines, feeds, weights=b"", level=1):
    from feathercnn_amd.net import Net
    net = Net(fusion=level)
    net.SetTransformer()
    net.SetDetection(True)
    net.SetFrame()
    net.LoadParam(_param(lines))
    net.LoadWeights(weights)
    for name, x in feeds.items():
        net.FeedInput(name, x)
    net.Forward()
    return net


X468 = np.random.default_rng(5).uniform(-1, 1, (2, 4, 6, 8)).astype(F)
TOKENS = ["Input in0 0 1 in0 0=8 1=6 2=1", "Reshape tok 1 1 in0 tok 0=8 1=6"]  # a blob of rank 2, [6][8]
RESHAPE_REFUSALS = {
    # LayerNorm: affine_size is neither w nor, on a blob of rank 3, h * w
    "layer_norm_size_fits_nothing": (["Input in0 0 1 in0 0=8 1=6 2=4", "LayerNorm l 1 1 in0 top 0=5 2=0"], dict(in0=X468), b"", "affine_size 5"),
    "layer_norm_size_is_the_channel_count": (["Input in0 0 1 in0 0=8 1=6 2=4", "LayerNorm l 1 1 in0 top 0=4 2=0"], dict(in0=X468), b"", "affine_size 4"),
    "layer_norm_plane_on_a_blob_of_rank_2": (TOKENS + ["LayerNorm l 1 1 tok top 0=48 2=0"], dict(in0=X468[:, :1]), b"", "affine_size 48"),
    # MultiHeadAttention: rank, width, and bottoms that do not fit each other
    "attention_on_a_blob_of_rank_3": (["Input in0 0 1 in0 0=8 1=6 2=1", "MultiHeadAttention l 1 1 in0 top 0=8 1=2 2=64"], dict(in0=X468[:, :1]), _mha_weights(8), "rank 3"),
    "attention_width_is_not_embed_dim": (TOKENS + ["MultiHeadAttention l 1 1 tok top 0=16 1=2 2=256"], dict(in0=X468[:, :1]), _mha_weights(16), "[T][16]"),
    "attention_k_and_v_differ_in_length": (TOKENS + ["Input in1 0 1 in1 0=8 1=5 2=1", "Reshape k 1 1 in1 k 0=8 1=5", "Input in2 0 1 in2 0=8 1=6 2=1", "Reshape v 1 1 in2 v 0=8 1=6",
                                                     "MultiHeadAttention l 3 1 tok k v top 0=8 1=2 2=64"],
                                           dict(in0=X468[:, :1], in1=X468[:, 1:2, :5], in2=X468[:, 2:3]), _mha_weights(8), "differ"),
    "attention_q_and_k_differ_in_batch": (TOKENS + ["Input in1 0 1 in1 0=8 1=6 2=1", "Reshape k 1 1 in1 k 0=8 1=6", "MultiHeadAttention l 2 1 tok k top 0=8 1=2 2=64"],
                                          dict(in0=X468[:, :1], in1=np.concatenate([X468[:, 1:2], X468[:1, 2:3]])), _mha_weights(8), "differ"),
    # BinaryOp: operands of different shapes, and different batches of which none is 1
    "binary_shapes_differ": (["Input in0 0 1 in0 0=8 1=6 2=4", "Input in1 0 1 in1 0=8 1=3 2=4", "BinaryOp l 2 1 in0 in1 top 0=0"], dict(in0=X468, in1=X468[:, :, :3]), b"", "one shape"),
    "binary_batches_differ": (["Input in0 0 1 in0 0=8 1=6 2=4", "Input in1 0 1 in1 0=8 1=6 2=4", "BinaryOp l 2 1 in0 in1 top 0=0"],
                              dict(in0=np.concatenate([X468, X468[:1]]), in1=X468), b"", "one shape"),
}


@pytest.mark.parametrize("name", sorted(RESHAPE_REFUSALS))
def test_reshape_refusals(cuda, name):
    from feathercnn_amd import FeatherHipError
    lines, feeds, weights, word = RESHAPE_REFUSALS[name]
    with pytest.raises(FeatherHipError, match="code -100") as e:
        _planned(lines, {k: np.ascontiguousarray(v) for k, v in feeds.items()}, weights)
    assert "layer l" in str(e.value) and word in str(e.value), str(e.value)


def test_the_forms_only_a_reshape_accepts_run(cuda):
    """LayerNorm over the planes of a blob of rank 3 (affine_size == h * w), a BinaryOp whose second or first bottom is a single image, cross-
    attention with three bottoms of two lengths: each against the restatement."""
    rng = np.random.default_rng(6)
    gamma, beta = rng.uniform(0.5, 1.5, 48).astype(F), rng.uniform(-0.5, 0.5, 48).astype(F)
    net = _planned(["Input in0 0 1 in0 0=8 1=6 2=4", "LayerNorm l 1 1 in0 top 0=48 1=1e-5"], dict(in0=X468), gamma.tobytes() + beta.tobytes())
    got = net.Extract("top")
    want = R.layer_norm(X468.reshape(2, 4, 48), gamma, beta, 1e-5).reshape(X468.shape)
    assert got.shape == X468.shape and R.normalised_error(got, want) <= TOL
    one = np.ascontiguousarray(X468[1:, ::-1])
    for order, swap in ((("in0", "in1"), False), (("in1", "in0"), True)):  # a - one[0] over the batch, then one[0] - a
        net = _planned(["Input in0 0 1 in0 0=8 1=6 2=4", "Input in1 0 1 in1 0=8 1=6 2=4", "BinaryOp l 2 1 %s %s top 0=1" % order], dict(in0=X468, in1=one))
        assert SW.same_bits(net.Extract("top"), R.binary(R.SUB, X468, one[0], swap)), order
        assert [a for t, _, a in net.layers() if t == "BinaryOp"] == ["ATTN"]
    w = [rng.uniform(-0.4, 0.4, s).astype(F) for _ in range(4) for s in ((8, 8), (8,))]
    import struct
    blob = b"".join((struct.pack("<I", 0) if a.ndim == 2 else b"") + a.tobytes() for a in w)
    lines, feeds, _, _ = RESHAPE_REFUSALS["attention_k_and_v_differ_in_length"]
    feeds = dict(feeds, in2=X468[:, 2:3, :5])
    lines = [ln.replace("Input in2 0 1 in2 0=8 1=6 2=1", "Input in2 0 1 in2 0=8 1=5 2=1").replace("Reshape v 1 1 in2 v 0=8 1=6", "Reshape v 1 1 in2 v 0=8 1=5") for ln in lines]
    net = _planned(lines, {k: np.ascontiguousarray(v) for k, v in feeds.items()}, blob)
    want = R.multi_head_attention(feeds["in0"][:, 0], feeds["in1"][:, 0], feeds["in2"][:, 0], 2, w)
    assert R.normalised_error(net.Extract("top")[:, 0], want) <= TOL


# ---- q8 blobs (the int8 activation behind a requantised convolution, Net.SetRequantized) ---------------------------------------------------
Q8_READERS = {"LayerNorm": lambda g, x: g.layer_norm("r", x, 8), "GELU": lambda g, x: g.gelu("r", x), "BinaryOp_scalar": lambda g, x: g.binary("r", 2, x, 0.5),
              "BinaryOp_memory": lambda g, x: g.binary("r", 0, x, g.memory_data("m", 8, 8, 16)),
              "MultiHeadAttention": lambda g, x: g.multi_head_attention("r", x, 8, 2), "MultiHeadAttention_keys": lambda g, x: g.multi_head_attention("r", g.memory_data("m", 8, 4), 8, 2, k=x),
              "InnerProduct_tokens": lambda g, x: g.fc_tokens("r", x, 8, 4), "InnerProduct_int8": lambda g, x: g.fc("r", x, 16 * 8 * 8, 4, quant=True)}


@pytest.mark.parametrize("name", sorted(Q8_READERS))
@pytest.mark.parametrize("level", [0, 2])
def test_a_transformer_layer_cannot_read_a_q8_blob(cuda, name, level):
    """A q8 bottom is refused at Reshape by the check every layer that cannot read one meets: NET_E_TOPOLOGY (-300), naming the producer and
    the layer -- whichever bottom it is, and for the InnerProduct of a net with the switch in its int8 form too."""
    from feathercnn_amd import FeatherHipError, model_zoo
    from feathercnn_amd.net import Net
    g = model_zoo.GraphBuilder(3, quant={})
    Q8_READERS[name](g, g.conv("c1", g.input("data", 3, 8, 8), 3, 16, 3, 1, 1, requant=20.0))
    p, b = g.finish()
    net = Net(fusion=level)
    net.SetTransformer()
    net.SetDetection(True)
    net.SetQuantized(True)
    net.SetRequantized(True)
    net.LoadParam(p)
    net.LoadWeights(b)
    net.FeedInput("data", np.random.default_rng(2).uniform(-1, 1, (2, 3, 8, 8)).astype(F))
    with pytest.raises(FeatherHipError) as e:
        net.Forward()
    msg = str(e.value)
    reader = name.split("_")[0] + " layer r"
    assert "code -300" in msg and "layer c1" in msg and reader in msg and "blob c1" in msg, msg


# ---- the SE block of a net with the switch -------------------------------------------------------------------------------------------------
def _se_net(op):
    from feathercnn_amd import model_zoo
    g = model_zoo.GraphBuilder(9)
    x = g.relu("relu1", g.conv("conv1", g.input("data", 3, 8, 8), 3, 8, 3, 1, 1))
    g.conv("out", g.se_block("se", x, 8, 4, spelling="ncnn"), 8, 4, 1)
    p, b = g.finish()
    assert p.count(b"BinaryOp se_mul") == 1 and b" 0=2\n" in p[p.index(b"BinaryOp se_mul"):]
    head, tail = p[:p.index(b"BinaryOp se_mul")], p[p.index(b"BinaryOp se_mul"):]
    return head + tail.replace(b" 0=2\n", b" 0=%d\n" % op, 1), b


def test_the_gate_block_collapse_takes_a_multiply_only(cuda):
    """With the switch on every BinaryOp is the element-wise layer.  The multiply of an SE block is the gate it was: fusion 2 collapses the
    block, and every level equals the default net's bits.  Any other op behind the gate's activation is no gate: the same refusal at every
    level (-100, the shapes), never a block computed as a multiply."""
    from feathercnn_amd import FeatherHipError
    from feathercnn_amd.net import Net
    x = np.random.default_rng(8).uniform(-1, 1, (2, 3, 8, 8)).astype(F)
    p, b = _se_net(2)
    outs = {}
    for switch in (False, True):
        for level in (0, 2):
            net = Net(fusion=level)
            if switch:
                net.SetTransformer()
                net.SetDetection(True)
            net.LoadParam(p)
            net.LoadWeights(b)
            net.FeedInput("data", x)
            net.Forward()
            outs[(switch, level)] = net.Extract("out")
            assert ("se_mul" in [nm for _, nm, _ in net.layers()]) == (level == 0)
            if level == 0:
                assert [a for t, nm, a in net.layers() if nm == "se_mul"] == ["GATE"]
    for level in (0, 2):
        assert SW.same_bits(outs[(True, level)], outs[(False, level)]), level
    for op in (0, 1, 3, 4, 5):
        p, b = _se_net(op)
        for level in (0, 1, 2):
            net = Net(fusion=level)
            net.SetTransformer()
            net.SetDetection(True)
            net.LoadParam(p)
            net.LoadWeights(b)
            net.FeedInput("data", x)
            with pytest.raises(FeatherHipError, match="code -100") as e:
                net.Forward()
            assert "layer se_mul" in str(e.value) and "one shape" in str(e.value), (op, level, str(e.value))
