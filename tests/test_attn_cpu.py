"""The transformer layers without a GPU: the Net loads tiny_vit with the switches on and refuses it without them; every refusal of the new param
and weight readers with its code; the restatement tests/attn_ref.py against an independent float64 einsum statement; the tables of
tests/attn_cases.py; the host-side refusals of libfeather_attn.so; and the readers on hostile files in a stand-alone program whose host
side runs under AddressSanitizer and UndefinedBehaviorSanitizer (never loaded into python)."""
import ctypes
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import attn_cases as C
import attn_ref as R
import side_contract as SC

F = np.float32
ROOT = SC.ROOT
INT_MAX = 2 ** 31 - 1
NEW_TYPES = {"MemoryData": ("0=4 1=3", 0), "LayerNorm": ("0=8", 1), "GELU": ("", 1), "MultiHeadAttention": ("0=8 1=2 2=64", 1)}


def _one(type_, params="", bottoms=1, tops=1, c=1, h=6, w=8):
    """A net of `bottoms` Inputs in0 .. (one at least) and one layer `l` of `type_` that reads `bottoms` of them."""
    lines = [f"Input in{k} 0 1 in{k} 0={w} 1={h} 2={c}" for k in range(max(bottoms, 1))]
    lines.append(f"{type_} l {bottoms} {tops} " + " ".join(f"in{k}" for k in range(bottoms)) + " " + " ".join("t%d" % k for k in range(tops)) + " " + params)
    return ("7767517\n%d %d\n" % (len(lines), max(bottoms, 1) + tops) + "\n".join(lines) + "\n").encode()


def _net(param, weights=None, transformer=True, detection=True, frame=True, level=1):
    from feathercnn_amd.net import Net
    net = Net(fusion=level)
    if transformer:
        net.SetTransformer()
    if detection:
        net.SetDetection(True)
    if frame:
        net.SetFrame()
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


# ---- the switch ----------------------------------------------------------------------------------------------------------------------------
def test_tiny_vit_loads_with_the_switches_and_is_refused_without_with_the_hint():
    (p, b, i, o), _ = C.net_model()
    net = _net(p, b)
    types = [t for t, _, _ in net.layers()]
    assert {"MemoryData", "LayerNorm", "GELU", "MultiHeadAttention", "BinaryOp", "InnerProduct", "Crop", "Reshape"} <= set(types)
    msg = _refused(p, -200, "MemoryData", transformer=False)  # the first type a default net does not know
    assert "(fhip_net_set_transformer lifts this)" in msg
    _refused(p, -200, "fhip_net_set_detection", detection=False)  # Reshape, the first type that needs it
    msg = _refused(_one("GELU"), -200, "fhip_net_set_detection", detection=False)  # the blob ranks: the transformer switch alone is not enough
    assert "GELU" in msg and "set both" in msg


@pytest.mark.parametrize("type_", sorted(NEW_TYPES))
def test_default_net_refuses_the_new_types_with_the_hint(type_):
    params, bottoms = NEW_TYPES[type_]
    p = _one(type_, params, bottoms)
    for kw in (dict(transformer=False), dict(transformer=False, detection=False, frame=False)):
        assert "(fhip_net_set_transformer lifts this)" in _refused(p, -200, type_, **kw)
    assert (type_, "l", "ATTN") in _net(p).layers()


def test_on_then_off_equals_the_default_and_the_switch_is_refused_after_loadparam():
    from feathercnn_amd import FeatherHipError
    from feathercnn_amd.net import Net
    net = Net()
    net.SetTransformer()
    net.SetTransformer(False)
    net.SetDetection(True)
    with pytest.raises(FeatherHipError, match="code -200"):
        net.LoadParam(_one("GELU"))
    with pytest.raises(FeatherHipError, match="code -100") as e:  # and BinaryOp is what it was
        Net().LoadParam(_one("BinaryOp", "0=0", 2))
    assert "only BinaryOp mul" in str(e.value)
    net = _net(_one("ReLU"))
    with pytest.raises(FeatherHipError, match="before LoadParam"):
        net.SetTransformer()
    # without the blob ranks BinaryOp and InnerProduct are what a default net loads: the gate multiply loads, an add is refused as ever
    assert ("BinaryOp", "l", "GATE") in _net(_one("BinaryOp", "0=2", 2), detection=False).layers()
    assert ("InnerProduct", "l", "IM2COL") in _net(_one("InnerProduct", "0=5 1=1 2=40"), detection=False).layers()
    assert "only BinaryOp mul" in _refused(_one("BinaryOp", "0=0", 2), -100, "BinaryOp", detection=False)


def test_the_route_code_and_the_bindings():
    import feathercnn_amd
    from feathercnn_amd import _lib, attn, net
    header = open(SC.INCLUDE + "/feather_hip/feather_attn.h").read()
    code = int(re.search(r"#define\s+FHIP_ATTN_NET_ROUTE\s+(\d+)", header).group(1))
    assert code == net.ATTN_ROUTE == attn.NET_ROUTE == feathercnn_amd.ATTN_NET_ROUTE == 113 and net.ROUTE_NAMES[113] == "ATTN"
    for name, value in (("MFMA_MAX_D", attn.MFMA_MAX_D), ("DIRECT_MAX_D", attn.DIRECT_MAX_D), ("QUERY_TILE", attn.QUERY_TILE), ("KEY_TILE", attn.KEY_TILE),
                        ("LN_WAVE_MAX", attn.LN_WAVE_MAX)):
        assert int(re.search(r"#define\s+FHIP_ATTN_%s\s+(\d+)" % name, header).group(1)) == value, name
    assert (attn.MFMA_MAX_D, attn.DIRECT_MAX_D, attn.LN_WAVE_MAX) == (R.MFMA_MAX_D, R.DIRECT_MAX_D, R.LN_WAVE_MAX)
    text = open(SC.INCLUDE + "/feather_hip/feather_net.h").read()
    cxx = open(SC.INCLUDE + "/feather/net.h").read()
    assert "fhip_net_set_transformer" in text and "fhip_net_set_transformer" in _lib.SIGNATURES and "SetTransformer(bool on = true)" in cxx
    for f in ("attention", "layer_norm", "add_layer_norm", "gelu", "binary", "attn_route"):
        assert callable(getattr(feathercnn_amd, f)) and f in feathercnn_amd.__all__, f
    seen = {attn.attn_route(attn.ATTENTION, d * h, h) for d in (1, 3, 4, 8, 32, 36, 64, 96, 100, 128, 132) for h in (1, 3)}
    seen |= {attn.attn_route(attn.LAYER_NORM, l, a) for l in (1, 256, 257) for a in (0, 1)}
    seen |= {attn.attn_route(attn.GELU, f, v) for f in (0, 1) for v in (0, 1)} | {attn.attn_route(attn.BINARY, f, v) for f in (0, 1, 2) for v in (0, 1)}
    assert seen == C.targets()
    for d, h in ((4, 1), (128, 3), (132, 1), (2, 2), (1, 1), (3, 3), (36, 1)):
        assert attn.attn_route(attn.ATTENTION, d * h, h) == R.attention_route(d * h, h)
    assert attn.attn_route(attn.ATTENTION, 128, 1) == "fhip::attention_mfma_kernel<4>" and "direct" in attn.attn_route(attn.ATTENTION, 2, 1)
    assert attn.attn_route(attn.LAYER_NORM, 256, 0) == "fhip::layer_norm_kernel<0, 0>" and attn.attn_route(attn.LAYER_NORM, 257, 1) == "fhip::layer_norm_kernel<1, 1>"


# ---- refusals at LoadParam (-100) ------------------------------------------------------------------------------------------------------
LOADPARAM_REFUSALS = [
    ("MemoryData", "", 0, "w (0=0)"), ("MemoryData", "0=-4", 0, "0=-4"), ("MemoryData", "0=4 1=-1", 0, "1=-1"), ("MemoryData", "0=4 2=3", 0, "where it has c"),
    ("MemoryData", f"0={INT_MAX} 1={INT_MAX}", 0, "2^31"), ("MemoryData", "0=4", 1, "no bottom"),
    ("LayerNorm", "", 1, "affine_size"), ("LayerNorm", "0=-8", 1, "0=-8"), ("LayerNorm", "0=8 1=-1.0", 1, "eps"), ("LayerNorm", "0=8 1=nan.0", 1, "eps"),
    ("LayerNorm", "0=8 2=2", 1, "2=2"), ("LayerNorm", "0=8", 2, "one bottom"),
    ("GELU", "0=2", 1, "0=2"), ("GELU", "0=-1", 1, "0=-1"), ("GELU", "", 2, "one bottom"),
    ("BinaryOp", "0=6", 2, "0=6"), ("BinaryOp", "0=-1", 2, "0=-1"), ("BinaryOp", "0=9", 2, "0=9"), ("BinaryOp", "0=0 1=2", 1, "1=2"), ("BinaryOp", "0=0 1=1 2=1.0", 2, "one bottom"),
    ("BinaryOp", "0=0", 1, "two bottoms"), ("BinaryOp", "0=0", 3, "two bottoms"),
    ("MultiHeadAttention", "0=8 1=2 2=64 5=1", 1, "mask"), ("MultiHeadAttention", "0=8 1=2 2=64 3=4", 1, "kdim"), ("MultiHeadAttention", "0=8 1=2 2=64 4=16", 1, "vdim"),
    ("MultiHeadAttention", "0=8 1=2 2=63", 1, "weight_data_size"), ("MultiHeadAttention", "0=8 1=2", 1, "weight_data_size"), ("MultiHeadAttention", "0=8 1=3 2=64", 1, "multiple"),
    ("MultiHeadAttention", "0=0 1=2 2=0", 1, "positive"), ("MultiHeadAttention", "0=8 1=0 2=64", 1, "positive"), ("MultiHeadAttention", "0=8 1=2 2=64", 4, "one to three"),
    ("MultiHeadAttention", f"0={INT_MAX} 1=1 2=1", 1, "weight_data_size"), ("MultiHeadAttention", "0=46341 1=1 2=-2147479015", 1, "weight_data_size"),
]


@pytest.mark.parametrize("type_,params,bottoms,word", LOADPARAM_REFUSALS, ids=lambda v: str(v).replace(" ", "_"))
def test_loadparam_refusals(type_, params, bottoms, word):
    msg = _refused(_one(type_, params, bottoms), -100, word)
    assert "layer l" in msg


def test_good_forms_load():
    for type_, forms in (("MemoryData", (("0=4", 0), ("0=4 1=3", 0), ("0=4 1=3 2=2", 0))), ("LayerNorm", (("0=8", 1), ("0=8 1=1e-5 2=0", 1), ("0=48", 1))),
                         ("GELU", (("", 1), ("0=1", 1))), ("BinaryOp", (("0=0", 2), ("0=5", 2), ("0=3 1=1 2=2.0", 1), ("0=2", 2))),
                         ("MultiHeadAttention", (("0=8 1=2 2=64", 1), ("0=8 1=8 2=64 6=0.5", 2), ("0=8 1=1 2=64 3=8 4=8 5=0", 3))),
                         ("InnerProduct", (("0=5 1=1 2=40", 1),))):
        for params, bottoms in forms:
            assert type_ in [t for t, _, _ in _net(_one(type_, params, bottoms)).layers()]


def _weights_of(type_, params, bottoms, floats):
    """LoadWeights of a one-layer net on a .bin of `floats` zero floats -> the error text, or None."""
    from feathercnn_amd import FeatherHipError
    net = _net(_one(type_, params, bottoms))
    try:
        net.LoadWeights(b"\0" * (4 * floats))
    except FeatherHipError as e:
        return str(e)
    return None


@pytest.mark.parametrize("type_,params,bottoms,needs", [("MemoryData", "0=4 1=3", 0, 12), ("LayerNorm", "0=8", 1, 16), ("MultiHeadAttention", "0=8 1=2 2=64", 1, 4 * (1 + 64 + 8)),
                                                        ("InnerProduct", "0=5 1=1 2=40", 1, 1 + 40 + 5)])
def test_truncated_weights_fail_loadweights_naming_the_layer(type_, params, bottoms, needs):
    assert _weights_of(type_, params, bottoms, needs) is None
    for floats in (0, 1, needs // 2, needs - 1):
        msg = _weights_of(type_, params, bottoms, floats)
        assert msg and "Layer l loading weights failed" in msg, (floats, msg)
    from feathercnn_amd import FeatherHipError
    with pytest.raises(FeatherHipError, match="weights have not been loaded"):
        _net(_one(type_, params, bottoms)).Forward()


def test_layers_without_weights_need_no_weight_file():
    assert _weights_of("GELU", "", 1, 0) is None and _weights_of("BinaryOp", "0=0", 2, 0) is None and _weights_of("LayerNorm", "0=8 2=0", 1, 0) is None


# ---- the restatement -------------------------------------------------------------------------------------------------------------------
def _einsum_attention(q, k, v, heads):
    """The same attention stated independently: all heads at once, float64."""
    n, tq, e = q.shape
    d = e // heads
    qh, kh, vh = (t.astype(np.float64).reshape(n, -1, heads, d) for t in (q, k, v))
    s = np.einsum("nthc,nuhc->nhtu", qh, kh)
    s = s - s.max(axis=3, keepdims=True)
    p = np.exp(s)
    p /= p.sum(axis=3, keepdims=True)
    return np.einsum("nhtu,nuhc->nthc", p, vh).reshape(n, tq, e)


@pytest.mark.parametrize("case", C.ATTENTION_CASES, ids=C.attention_id)
def test_the_attention_restatement_equals_a_float64_einsum(case):
    q, k, v, want = C.attention_case(case)
    other = _einsum_attention(q, k, v, case[3])
    assert want.dtype == np.float64 and want.shape == q.shape and np.isfinite(want).all()
    assert R.normalised_error(want, other) <= 1e-12
    tq, tk, d, heads, n, layout, offset, kind = case
    s = np.einsum("tc,uc->tu", q[0, :, :d].astype(np.float64), k[0, :, :d].astype(np.float64))
    if kind == "pm80":  # the maximum must matter: without it float32 leaves its range of normal numbers on one side or the other
        big = max(float(np.abs(np.einsum("tc,uc->tu", q[i, :, h * d:(h + 1) * d].astype(np.float64), k[i, :, h * d:(h + 1) * d].astype(np.float64))).max())
                  for i in range(n) for h in range(heads))
        assert abs(big - 80) < 1e-3 and np.exp(big) > 1e34 and np.exp(-big) < 1e-34
    if kind == "equal":
        assert np.ptp(s[0]) == 0 and np.allclose(want[0, 0, :d], v[0, :, :d].astype(np.float64).mean(axis=0), rtol=0, atol=1e-12)


def test_the_cases_cover_what_the_issue_lists_and_every_attention_kernel():
    lengths, ds = {1, 2, 31, 32, 33, 65, 197}, {4, 8, 32, 64, 128, 1, 3, 6, 132}
    assert {c[0] for c in C.ATTENTION_CASES} == lengths == {c[1] for c in C.ATTENTION_CASES} and ds <= {c[2] for c in C.ATTENTION_CASES}
    assert any(c[0] != c[1] for c in C.ATTENTION_CASES) and {c[3] for c in C.ATTENTION_CASES} == {1, 3} == {c[4] for c in C.ATTENTION_CASES}
    assert {c[5] for c in C.ATTENTION_CASES} == {"dense", "fused", "kv"} and {c[6] for c in C.ATTENTION_CASES} == {0, 1, 2, 3}
    routes = {R.attention_route(c[2] * c[3], c[3]) for c in C.ATTENTION_CASES}
    assert routes == {t for t in C.targets() if "attention" in t}
    for kind in ("pm80", "equal"):
        assert {"mfma" in R.attention_route(c[2] * c[3], c[3]) for c in C.ATTENTION_CASES if c[7] == kind} == {True, False}
    assert {1, 2, 3, 63, 64, 65, 192, 768, 1025, R.LN_WAVE_MAX, R.LN_WAVE_MAX + 1} <= set(C.LN_LENGTHS)


def test_layer_norm_and_gelu_and_binary_restatements():
    import torch
    x, gamma, beta = C.layer_norm_case(197, 192)
    want = torch.nn.functional.layer_norm(torch.tensor(x).double(), (192,), torch.tensor(gamma).double(), torch.tensor(beta).double(), float(F(1e-3))).numpy()
    assert R.normalised_error(R.layer_norm(x, gamma, beta), want) <= 1e-12
    x, _, _ = C.layer_norm_case(1, 65, True)  # mean 10^4, spread 1: the centred form keeps the spread
    y = R.layer_norm(x)
    assert abs(float(y.std()) - 1) < 1e-2 and abs(float(y.mean())) < 1e-9
    t = np.linspace(-6, 6, 101).astype(F)
    assert R.normalised_error(R.gelu(t), torch.nn.functional.gelu(torch.from_numpy(t).double()).numpy()) <= 1e-7  # the constant is float32's
    assert R.normalised_error(R.gelu(t, True), torch.nn.functional.gelu(torch.from_numpy(t).double(), approximate="tanh").numpy()) <= 1e-7
    got = R.gelu(C.SPECIALS)
    assert got[0] == 0 and got[1] == 0 and got[2] == np.inf and np.isnan(got[3]) and np.isnan(got[4])
    a, b = np.arange(12, dtype=F).reshape(3, 4) - 5, np.array([1, -2, 0.5, 4], F)
    assert np.array_equal(R.binary(R.SUB, a, b), a - b[None]) and np.array_equal(R.binary(R.SUB, a, b, swap=True), b[None] - a)
    assert np.array_equal(R.binary(R.MAX, a, F(0.5)), np.maximum(a, F(0.5))) and R.binary(R.DIV, a, a + 7).dtype == F


def test_the_numpy_forward_of_tiny_vit_has_every_blob_with_its_shape_and_rank():
    (p, b, i, o), trace = C.net_model()
    x, blobs = C.net_input(3)
    shapes = C.net_shapes()
    tops = set(re.findall(r"^\S+ \S+ \d+ \d+ (.*)$", p.decode(), re.M) and [t for line in p.decode().splitlines()[2:] for t in line.split()[4 + int(line.split()[2]):4 + int(line.split()[2]) + int(line.split()[3])]])
    assert tops == set(shapes) == set(blobs), sorted(tops ^ set(shapes))
    for name, (chw, rank) in shapes.items():
        assert blobs[name].shape == (3,) + chw, name
        assert rank == 3 or chw[0] == 1, name  # a blob of rank 2 is [n][1][h][w]
    assert np.isfinite(blobs[o]).all() and float(np.abs(blobs[o]).max()) > 0.05
    # the class token row is the MemoryData plus the position embedding, whatever the image
    assert np.array_equal(blobs["add_pos"][:, 0, 0], (blobs["cls_token"][:, 0, 0] + blobs["pos_embed"][:, 0, 0]).astype(F))
    fusible = [ln.split()[1] for ln in p.decode().splitlines() if ln.startswith("BinaryOp") and "_add1" in ln or "add_pos" in ln.split()[1:2]]
    assert "add_pos" in fusible and "blk0_add1" in fusible  # the adds a Split hands to a LayerNorm: what level 2 fuses


def test_the_published_nets_have_their_published_sizes():
    from feathercnn_amd import model_zoo
    for fn, embed, depth, heads, params in ((model_zoo.deit_tiny_patch16_224, 192, 12, 3, 5.7e6), (model_zoo.vit_base_patch16_224, 768, 12, 12, 86.6e6)):
        p, nbytes, i, o = fn(dry=True)
        text = p.decode()
        assert text.count("MultiHeadAttention ") == depth and f"0={embed} 1={heads} 2={embed * embed}" in text and "MemoryData pos_embed 0 1 pos_embed 0=%d 1=197" % embed in text
        assert abs(nbytes / 4 - params) / params < 0.02, nbytes / 4  # the published parameter count


# ---- the library's refusals on the host --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    return SC.library("attn")


A, B, D = (ctypes.c_void_p(0x10000 + 0x4000 * k) for k in range(3))  # aligned addresses that are never dereferenced: every call below is refused first
NULL = None


def _bad(lib, rc, word=""):
    assert rc == SC.BADARG, rc
    msg = lib.fhip_attn_last_error().decode()
    assert msg and word in msg, msg


def test_the_library_refuses_on_the_host(lib):
    fl = ctypes.c_float
    att = lambda n=1, heads=2, tq=3, tk=3, e=8, q=A, qs=8, k=B, ks=8, v=D, vs=8, out=ctypes.c_void_p(0x30000): lib.fhip_attention_forward(n, heads, tq, tk, e, q, qs, k, ks, v, vs, out, None)
    _bad(lib, att(e=9), "E % heads")
    _bad(lib, att(tk=0), "tk < 1")
    _bad(lib, att(tq=0), "< 1")
    _bad(lib, att(heads=0), "< 1")
    _bad(lib, att(qs=7), "stride")
    _bad(lib, att(n=1 << 16, tq=1 << 12, e=8, qs=8), "2^31")
    _bad(lib, att(n=1 << 14, tk=1 << 14, ks=8), "2^31")
    _bad(lib, att(tk=1 << 28, vs=8), "2^31")
    _bad(lib, att(q=NULL), "null")
    _bad(lib, att(out=ctypes.c_void_p(0x30002)), "aligned")
    _bad(lib, att(heads=1, e=4097, qs=4097, ks=4097, vs=4097), "4096")
    _bad(lib, lib.fhip_layer_norm_forward(0, 8, None, None, fl(1e-3), A, B, None), "< 1")
    _bad(lib, lib.fhip_layer_norm_forward(1 << 16, 1 << 15, None, None, fl(1e-3), A, B, None), "2^31")
    _bad(lib, lib.fhip_layer_norm_forward(2, 8, None, None, fl(-1), A, B, None), "eps")
    _bad(lib, lib.fhip_layer_norm_forward(2, 8, None, None, fl(1e-3), A, A, None), "overlap")
    _bad(lib, lib.fhip_add_layer_norm_forward(2, 8, None, None, fl(1e-3), A, A, B, D, None), "overlap")
    _bad(lib, lib.fhip_add_layer_norm_forward(2, 8, None, None, fl(1e-3), ctypes.c_void_p(0x10004), ctypes.c_void_p(0x30000), A, B, None), "sum must be")
    _bad(lib, lib.fhip_gelu_forward(2, A, B, 8, None), "fast_gelu")
    _bad(lib, lib.fhip_gelu_forward(0, A, B, 0, None), "count")
    _bad(lib, lib.fhip_gelu_forward(0, A, B, 1 << 31, None), "2^31")
    _bad(lib, lib.fhip_gelu_forward(0, A, NULL, 8, None), "null")
    for op in (-1, 6, 7, 9):
        _bad(lib, lib.fhip_binary_forward(op, 1, 0, A, B, D, fl(0), 8, 0, None), "op")
    _bad(lib, lib.fhip_binary_forward(0, 3, 0, A, B, D, fl(0), 8, 0, None), "form")
    _bad(lib, lib.fhip_binary_forward(0, 1, 2, A, B, D, fl(0), 8, 0, None), "swap")
    _bad(lib, lib.fhip_binary_forward(0, 2, 0, A, B, D, fl(0), 8, 3, None), "count % per")
    _bad(lib, lib.fhip_binary_forward(0, 1, 0, A, B, NULL, fl(0), 8, 0, None), "null")
    _bad(lib, lib.fhip_binary_forward(0, 1, 0, A, B, D, fl(0), 1 << 31, 0, None), "2^31")
    name = ctypes.create_string_buffer(64)
    _bad(lib, lib.fhip_attn_route(9, 0, 0, name, 64), "unknown")
    _bad(lib, lib.fhip_attn_route(0, 9, 2, name, 64), "E % heads")
    _bad(lib, lib.fhip_attn_route(1, 0, 0, name, 64), "l < 1")
    _bad(lib, lib.fhip_attn_route(3, 3, 0, name, 64), "form")
    _bad(lib, lib.fhip_attn_route(0, 8, 2, None, 64), "null")


# ---- the readers on hostile files, host side under sanitizers ------------------------------------------------------------------------------
HOSTILE = ("-1", "0", "1", "7", str(INT_MAX), str(-INT_MAX - 1), "-233", "65536", "46341", "3.5", "-1.0", "1e38", "inf.0", "nan.0", "1e-46", "")
CONTROLS = 1  # case 0000 is tiny_vit as it is


def _hostile_cases():
    """-> [(param, bin, must_load)]: tiny_vit as it is; every value of every param of every transformer layer of it replaced by each of
    HOSTILE, and one absent id added; the .bin cut at every block boundary of the new weighted types and in the middle of each block."""
    (p, b, i, o), _ = C.net_model()
    lines = p.decode().splitlines()
    cases = [(p, b, True)]
    new = ("MemoryData", "LayerNorm", "GELU", "BinaryOp", "MultiHeadAttention", "InnerProduct")
    for at, line in enumerate(lines):
        tok = line.split()
        if tok[0] not in new:
            continue
        first = 4 + int(tok[2]) + int(tok[3])
        ids = [t.split("=")[0] for t in tok[first:]]
        for position in range(len(ids)):  # every value the line holds, replaced
            for value in HOSTILE:
                t = list(tok)
                t[first + position] = ids[position] + "=" + value
                cases.append(("\n".join(lines[:at] + [" ".join(t)] + lines[at + 1:]).encode() + b"\n", b, False))
        for absent in [i_ for i_ in range(7) if str(i_) not in ids][:2]:  # two ids the line does not hold, appended
            for value in HOSTILE:
                cases.append(("\n".join(lines[:at] + [" ".join(tok + [f"{absent}={value}"])] + lines[at + 1:]).encode() + b"\n", b, False))
        for counts in ((0, 1), (2, 1), (1, 0), (4, 1)):  # bottom and top counts
            t = list(tok)
            t[2], t[3] = str(counts[0]), str(counts[1])
            cases.append(("\n".join(lines[:at] + [" ".join(t)] + lines[at + 1:]).encode() + b"\n", b, False))
    for cut in sorted({0, 3, 4, len(b) // 7, len(b) // 3, len(b) // 2, len(b) - 4, len(b) - 1} | {64 * k + 2 for k in range(0, len(b) // 64, 9)}):
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
    assert 400 <= len(cases) <= 4000
    d = tmp_path / "cases"
    d.mkdir()
    for k, (p, b, _) in enumerate(cases):
        (d / f"{k:04d}.param").write_bytes(p)
        (d / f"{k:04d}.bin").write_bytes(b)
    driver = os.path.join(ROOT, "tests", "cpp", "attn_loader_hostile_main.cpp")
    libdir = os.path.dirname(_lib.lib_path())
    exe = str(tmp_path / "attn_loader_hostile")
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
    exe = str(tmp_path / "attn_loader_hostile_san")
    subprocess.run([hipcc, "-std=c++17", "-O1", "-g", "-Xarch_host", san, "-Xarch_host", "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"),
                    "-x", "c++", driver, "-x", "none"] + objs + [san, "-o", exe, "-ldl"], check=True, capture_output=True, text=True)
    out = subprocess.run([exe, str(d), str(len(cases))], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    assert "ERROR: AddressSanitizer" not in out.stderr and "runtime error:" not in out.stderr and "LeakSanitizer" not in out.stderr, out.stderr[-3000:]
    assert _judge(cases, out.stdout) == loaded
