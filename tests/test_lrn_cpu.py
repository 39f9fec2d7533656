"""libfeather_lrn.so (LRN, alone and with the Pooling layer behind it) without a GPU.

Checks of the yardstick, which need no library: the float64 restatement the GPU tests compare against (tests/lrn_ref.py) equals
torch.nn.functional.local_response_norm across channels and a loop-by-loop evaluation within a channel; the float32 restatement (the
header step by step) stays within E_REF of it on the whole table; dropping one tap of a window -- the first, the last, the one across a
chunk boundary -- moves the result by at least 100 x the tolerance on every across-channel row, so the GPU sweep can see such a mistake;
the restatement runs tiny_lrn.

Checks of the feature (every one fails on the parent commit, where there is no library and LRN is refused with the switch on): the header
states the chunk, the LDS budget and the size limit the tests use; the route functions select the
instantiation the header states; bad arguments are refused on the host with their word; feather::Net refuses LRN by default and names the
switch, loads it with route LRN after SetExtendedLayers, and answers every hostile param line with its code and a message; fusion level 2
makes LRN -> Pooling one layer and leaves an LRN with two readers, a Pooling -> LRN and an LRN -> global Pooling as written; the zoo nets
are the published ones and load at every level.  What the library shares with the other run-time libraries -- its exports, the instantiations it holds, its route code, the build
of its application, its last-error state -- is in tests/test_side_contract_cpu.py."""
import ctypes
import os

import numpy as np
import pytest

import lrn_cases as LC
import lrn_ref as R
import side_contract

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "feather_hip", "feather_lrn.h")
BADARG = -2


lib = side_contract.fixture("lrn")


def _both(r, **kw):
    x = LC.make_input(r)
    return (R.lrn(x, r.local_size, r.alpha, r.beta, r.bias, r.region, np.float32, **kw), R.lrn(x, r.local_size, r.alpha, r.beta, r.bias, r.region, np.float64, **kw))


# ---- the definition ------------------------------------------------------------------------------------------------------------------
def test_float64_restatement_against_torch_across_channels():
    """torch.nn.functional.local_response_norm is the across-channel layer (zero padding along the channels, alpha / size, k = bias); it is
    handed the float32 values of alpha and beta the library gets.  Bound: 32 * 2^-53 relative -- both sides are float64 and differ by the
    order of the window's sum, torch's sum / size * alpha and the power -- plus the float32 rounding of alpha / local_size the restatement
    takes over from the library (2^-24 relative in a, at most beta * 2^-24 in y)."""
    import torch
    import torch.nn.functional as F
    for r in LC.ACROSS_ROWS + [LC.PUBLISHED]:
        x = LC.make_input(r).astype(np.float64)
        got = R.lrn(x, r.local_size, r.alpha, r.beta, r.bias, 0, np.float64)
        want = F.local_response_norm(torch.from_numpy(x), r.local_size, alpha=float(np.float32(r.alpha)), beta=float(np.float32(r.beta)), k=r.bias).numpy()
        assert got.shape == want.shape and LC.rel_err(got, want) <= 32 * 2.0 ** -53 + r.beta * 2.0 ** -24, r.id


def test_float64_restatement_within_channel_loop_by_loop():
    for r in LC.WITHIN_ROWS:
        x = LC.make_input(r).astype(np.float64)
        half = r.local_size // 2
        want = np.empty_like(x)
        a = np.float64(np.float32(r.alpha) / (np.float32(r.local_size) * np.float32(r.local_size)))
        for y in range(r.h):
            for xx in range(r.w):
                win = x[:, :, max(y - half, 0):y + half + 1, max(xx - half, 0):xx + half + 1]
                want[:, :, y, xx] = x[:, :, y, xx] * (r.bias + a * (win * win).sum(axis=(2, 3))) ** -np.float64(np.float32(r.beta))
        assert LC.rel_err(R.lrn(x, r.local_size, r.alpha, r.beta, r.bias, 1, np.float64), want) <= 64 * 2.0 ** -53, r.id


def test_float32_restatement_agrees_with_float64_within_e_ref():
    worst, at = LC.measure_e_ref()
    print(f"lrn_ref float32 vs float64 over the table: E_ref = {worst:.4e} at {at!r}; lrn_cases.E_REF = {LC.E_REF:.4e}, T = {LC.T:.4e}")
    assert 0 < worst <= LC.E_REF
    assert LC.T == LC.E_REF + 16 * 2.0 ** -24
    for r in LC.LRN_ROWS:
        a, b = _both(r)
        assert a.dtype == np.float32 and b.dtype == np.float64 and a.shape == (r.n, r.c, r.h, r.w)
    # every row but the published one has a = 1 and bias = 1
    assert all(R.scale_a(r.region, r.local_size, r.alpha) == 1 and r.bias == 1 for r in LC.LRN_ROWS if r is not LC.PUBLISHED)
    assert R.scale_a(0, 5, LC.PUBLISHED.alpha) == np.float32(1e-4) / np.float32(5)


def test_the_table_holds_what_it_must():
    ch = {(r.c, r.local_size) for r in LC.ACROSS_ROWS}
    for ls in LC.SIZES:
        for c in [1, 2, max(ls - 1, 1), ls] + [c for k in LC.CHUNKS for c in (k - 1, k, k + 1, 2 * k + 3)]:
            assert (c, ls) in ch, (c, ls)
        assert {(r.h, r.w) for r in LC.ACROSS_ROWS if r.local_size == ls} >= set(LC.PLANES)
        assert {r.n for r in LC.ACROSS_ROWS if r.local_size == ls} >= {1, 3}
    assert {r.beta for r in LC.ACROSS_ROWS} >= {0.75, 0.5, 0.6}
    assert any(r.h < r.local_size and r.w < r.local_size for r in LC.WITHIN_ROWS) and any(r.h == r.w == r.local_size for r in LC.WITHIN_ROWS)
    assert any((r.h, r.w) == (9, 7) for r in LC.WITHIN_ROWS)
    assert len({r.id for r in LC.LRN_ROWS}) == len(LC.LRN_ROWS) and len({p.id for p in LC.POOL_ROWS}) == len(LC.POOL_ROWS)


def _perturbations(r):
    """(what, drop list) for an across-channel row: the first tap of every channel's window, the last, and the taps that cross each chunk
    boundary (from either side)."""
    half = r.local_size // 2
    first = [(c, max(c - half, 0)) for c in range(r.c)]
    last = [(c, min(c + half, r.c - 1)) for c in range(r.c)]
    out = [("first tap", first), ("last tap", last)]
    if half:
        for b in range(min(LC.CHUNKS), r.c, min(LC.CHUNKS)):  # the boundaries of chunks of 4 are those of 8 and 16 too
            out.append((f"tap {b} of channel {b - 1} (chunk boundary)", [(b - 1, b)]))
            out.append((f"tap {b - 1} of channel {b} (chunk boundary)", [(b, b - 1)]))
            if half > 1 and b - half >= 0 and b + half - 1 < r.c:
                out.append((f"the farthest tap across boundary {b}", [(b - half, b), (b + half - 1, b - 1)]))
    return out


def test_a_missing_tap_is_visible_on_every_across_channel_row():
    """The float64 restatement with one tap dropped differs from the true one, at its worst element, by at least 100 T on every
    across-channel row (a = 1, x ~ N(0, 1)): the sweep's element-wise tolerance cannot hide a window that is short by a tap or a chunk
    that does not read its halo.  The published row (a = 2e-5) is printed next to it: the same mistake is two orders of magnitude
    smaller there, which is why the table does not use those parameters."""
    least = np.inf
    for r in LC.ACROSS_ROWS:
        _, want = _both(r)
        for what, drop in _perturbations(r):
            _, got = _both(r, drop=drop)
            e = LC.rel_err(got, want)
            least = min(least, e)
            assert e >= 100 * LC.T, (r.id, what, e)
    print(f"smallest effect of a dropped tap over the across-channel rows: {least:.3e} = {least / LC.T:.0f} T")
    r = LC.PUBLISHED
    e = LC.rel_err(_both(r, drop=[(c, max(c - 2, 0)) for c in range(r.c)])[1], _both(r)[1])
    print(f"the first tap dropped on the published row: {e:.3e} = {e / LC.T:.0f} T")
    assert any(len(_perturbations(r)) > 2 for r in LC.ACROSS_ROWS)  # rows with a chunk boundary exist


def test_pooling_restatement_and_tiny_lrn():
    from feathercnn_amd import model_zoo
    p, b, i, o = model_zoo.tiny_lrn()
    ref = R.Net(p, b)
    assert ref.read == len(b)
    x = np.random.default_rng(3).uniform(-1, 1, (2, 3, 16, 16)).astype(np.float32)
    blobs = ref.run(i, x, o, keep=True)
    want = {"norm1": (20, 16, 16), "pool1": (20, 8, 8), "norm2": (12, 8, 8), "pool2": (12, 4, 4), "norm3": (12, 4, 4), "norm4": (12, 2, 2), "norm5": (3, 4, 4),
            "pool5": (3, 4, 4)}
    assert {k: blobs[k].shape[1:] for k in want} == want
    assert np.allclose(blobs["prob"].reshape(2, -1).sum(axis=1), 1.0, atol=1e-5)
    assert all(np.abs(blobs[k]).max() > 1e-3 for k in want)  # no layer of the net is dead
    # lrn_ref.pooling is the Pooling layer of the family's evaluator: the max exactly, the average up to its float32 roundings
    assert np.array_equal(R.pooling(blobs["norm1"], 3, 2), blobs["pool1"]) and np.array_equal(R.pooling(blobs["norm3"], 2, 2), blobs["pool3"])
    assert np.abs(R.pooling(blobs["norm2"], 2, 2, avg=True) - blobs["pool2"]).max() <= 4 * 2.0 ** -24 * np.abs(blobs["pool2"]).max()
    assert np.abs(R.pooling(blobs["norm5"], 3, 1, (1, 1, 1, 1), avg=True) - blobs["pool5"]).max() <= 16 * 2.0 ** -24 * np.abs(blobs["pool5"]).max()
    # the LRN layers from their inputs, and an LRN that matters: norm1 moves its input by far more than the net's tolerance
    assert np.array_equal(blobs["norm1"], R.lrn(blobs["relu1"], 5, 1.0, 0.75, 1.0, 0, np.float64).astype(np.float32))
    assert np.array_equal(blobs["norm2"], R.lrn(blobs["relu2"], 3, 2.0, 0.5, 1.0, 1, np.float64).astype(np.float32))
    assert R.nerr(blobs["norm1"], blobs["relu1"]) > 1e-2
    assert R.pool_output_dim(16, 16, 3, 2, (0, 0, 0, 0)) == (8, 8) and R.pool_output_dim(13, 13, 3, 2, (0, 0, 0, 0)) == (6, 6)


# ---- the library ---------------------------------------------------------------------------------------------------------------------
def test_header_states_the_chunk_the_lds_budget_and_the_size_limit():
    text = open(HEADER).read()
    assert f"#define FHIP_LRN_CHUNK {LC.CHUNK}\n" in text and f"#define FHIP_LRN_POOL_LDS_FLOATS {LC.POOL_LDS_FLOATS}\n" in text
    import importlib
    L = importlib.import_module("feathercnn_amd.lrn")  # (the package's attribute of that name is the function)
    assert (L.CHUNK, L.POOL_LDS_FLOATS) == (LC.CHUNK, LC.POOL_LDS_FLOATS)
    assert "2^31" in text  # the size limit stands next to the functions


def _held(ls):
    return ls if ls in (3, 5) else 0


def _pool_param(p):
    from feathercnn_amd.net import pool_param
    r = p.lrn
    return pool_param(r.c, r.h, r.w, p.kernel, p.stride, (p.pad,) * 4, int(p.avg))


def test_instantiations_and_route_names(lib):
    name = ctypes.create_string_buffer(96)
    v = ctypes.c_void_p
    seen = set()
    for r in LC.LRN_ROWS:
        for off_out, off_in in ((0, 0), (1, 0), (0, 1), (1, 1), (2, 2)):
            assert lib.fhip_lrn_route(r.region, r.local_size, r.n, r.c, r.h, r.w, v(0x100000 + 4 * off_out), v(0x200000 + 4 * off_in), name, 96) == 0
            if r.region == 0:
                want = f"fhip::lrn_across_kernel<{4 if r.h * r.w % 4 == 0 and not off_out and not off_in else 1}, {_held(r.local_size)}>"
            else:
                want = "fhip::lrn_within_kernel"
            assert name.value.decode() == want, (r.id, off_out, off_in, name.value.decode())
            seen.add(want)
        assert lib.fhip_lrn_route(r.region, r.local_size, r.n, r.c, r.h, r.w, None, None, name, 96) == 0  # NULL counts as aligned
        assert name.value.decode() == (f"fhip::lrn_across_kernel<{4 if r.h * r.w % 4 == 0 else 1}, {_held(r.local_size)}>" if r.region == 0 else "fhip::lrn_within_kernel")
    for p in LC.POOL_ROWS:
        r = p.lrn
        q = _pool_param(p)
        assert lib.fhip_lrn_pool_route(r.region, r.local_size, r.n, r.c, r.h, r.w, ctypes.byref(q), None, None, name, 96) == 0
        assert name.value.decode() == p.route, (p.id, name.value.decode())
        # the header's rule: 16 channels of kernel_h rows in 8192 floats of LDS, across channels only
        assert (p.route != "fhip::lrn_pool_direct_kernel") == (r.region == 0 and LC.CHUNK * p.kernel * r.w <= LC.POOL_LDS_FLOATS)
        seen.add(p.route)
    assert seen == LC.targets()  # the tables reach every instantiation the library holds
    # a 16-byte path only where plane and pointers allow
    assert {(r.h * r.w % 4 == 0) for r in LC.ACROSS_ROWS} == {True, False}
    assert lib.fhip_lrn_route(2, 5, 1, 1, 4, 4, None, None, name, 96) == BADARG and "region_type 2" in lib.fhip_lrn_last_error().decode()


def test_refusals_come_before_any_device_call(lib):
    err = lambda: lib.fhip_lrn_last_error().decode()
    v = lambda p: ctypes.c_void_p(p) if p else None
    nan, inf = float("nan"), float("inf")
    from feathercnn_amd.net import pool_param

    def args(region=0, ls=5, alpha=1.0, beta=0.75, bias=1.0, n=2, c=3, h=4, w=4):
        return (region, ls, alpha, beta, bias, n, c, h, w)

    def lrn(out=0x100000, x=0x200000, **kw):
        return lib.fhip_lrn_forward(*args(**kw), v(out), v(x), None)

    def pooled(out=0x100000, x=0x200000, pool=None, **kw):
        a = args(**kw)
        q = pool if pool is not None else pool_param(a[6], a[7], a[8], 3, 2)
        return lib.fhip_lrn_pool_forward(*a, ctypes.byref(q) if q else None, v(out), v(x), None)

    common = (({"region": 2}, "region_type 2"), ({"region": -1}, "region_type"), ({"ls": 0}, "local_size 0"), ({"ls": -3}, "local_size"), ({"ls": 4}, "local_size 4"),
              ({"ls": 2}, "even"), ({"alpha": nan}, "finite"), ({"alpha": inf}, "finite"), ({"beta": nan}, "finite"), ({"beta": -inf}, "finite"),
              ({"bias": nan}, "finite"), ({"bias": inf}, "finite"), ({"bias": 0.0}, "bias > 0"), ({"bias": -1.0}, "bias > 0"), ({"alpha": -1e-4}, "alpha >= 0"),
              ({"n": 0}, "dimension"), ({"c": 0}, "dimension"), ({"h": 0}, "dimension"), ({"w": -1}, "dimension"),
              ({"n": 1 << 15, "c": 1 << 10, "h": 8, "w": 8}, "2^31"), ({"out": None}, "null"), ({"x": None}, "null"), ({"out": 0x100002}, "aligned"),
              ({"x": 0x200001}, "aligned"), ({"out": 0x200000}, "overlap"))
    for kw, word in common:
        assert lrn(**kw) == BADARG and word in err(), (kw, err())
        assert pooled(**kw) == BADARG and word in err(), (kw, err())
    for kw, word in (({"out": 0x200000 + 4 * (2 * 3 * 4 * 4 - 1)}, "overlap"), ({"x": 0x100000 + 4 * (2 * 3 * 4 * 4 - 1)}, "overlap")):
        assert lrn(**kw) == BADARG and word in err(), (kw, err())
    # what fhip_lrn_pool_forward refuses in addition
    P = lambda **kw: pool_param(kw.pop("c", 3), kw.pop("h", 4), kw.pop("w", 4), kw.pop("k", 3), kw.pop("s", 2), **kw)
    for pool, word in ((P(global_pooling=True), "global"), (P(c=4), "must equal"), (P(h=5), "must equal"), (P(w=3), "must equal"), (P(k=0), "at least 1"),
                       (P(s=0), "at least 1"), (P(pad=(0, 0, -1, 0)), "negative"), (P(k=9), "empty pooling output"), (P(k=1 << 30), "too large"),
                       (P(pad=(1 << 30, 0, 0, 0)), "too large"),
                       # a window that covers the unpadded plane goes through fhip_pooling's plane-reduce kernels, whose order is not restated
                       (P(k=4, s=1), "whole unpadded plane"), (P(k=4, s=4), "whole unpadded plane"), (P(k=5, s=2), "whole unpadded plane"),
                       (P(k=6, s=3, pooling_type=1), "whole unpadded plane")):
        assert pooled(pool=pool) == BADARG and word in err(), err()
    name = ctypes.create_string_buffer(96)
    q = P(k=4, s=1)
    assert lib.fhip_lrn_pool_route(0, 5, 2, 3, 4, 4, ctypes.byref(q), None, None, name, 96) == BADARG and "whole unpadded plane" in err()
    q = P(k=4, s=1, pad=(1, 0, 0, 0))  # padded: the generic kernel's geometry
    assert lib.fhip_lrn_pool_route(0, 5, 2, 3, 4, 4, ctypes.byref(q), None, None, name, 96) == 0
    # a launch takes fewer than 2^32 lanes: thin tensors are refused up front, with their word, not by the launch
    far = dict(out=0x10000000, x=0x100000000)
    assert lrn(n=1 << 24, c=1, h=1, w=1, **far) == BADARG and "2^24 - 1 blocks" in err()
    assert lrn(n=(1 << 24) - 1, c=1, h=1, w=1, out=None, x=0x100000000) == BADARG and "null" in err()  # one block fewer passes that check
    assert pooled(n=1 << 24, c=1, **far) == BADARG and "2^24 - 1 blocks" in err()
    assert lrn(n=1, c=1 << 20, h=1, w=1, **far) == BADARG and "65535 chunks" in err()
    assert lib.fhip_lrn_pool_forward(*args(), None, v(0x100000), v(0x200000), None) == BADARG and "null pool" in err()
    # the chunked entry
    ch = lambda chunk, **kw: lib.fhip_lrn_forward_chunked(*args(**kw)[1:], chunk, v(0x100000), v(0x200000), None)
    assert ch(-1) == BADARG and "chunk" in err()
    assert ch(1, n=1, c=1 << 17, h=1, w=1) == BADARG and "65535" in err()
    assert ch(0, ls=2) == BADARG and "even" in err()
    name = ctypes.create_string_buffer(8)
    assert lib.fhip_lrn_route(0, 5, 1, 1, 4, 4, None, None, None, 8) == BADARG and "null" in err()
    assert lib.fhip_lrn_route(0, 5, 1, 1, 4, 4, None, None, name, 0) == BADARG and "null" in err()
    q = P()
    assert lib.fhip_lrn_pool_route(0, 5, 2, 3, 4, 4, ctypes.byref(q), None, None, None, 8) == BADARG and "null" in err()


# ---- feather::Net --------------------------------------------------------------------------------------------------------------------
def _two(line, blobs=6):
    """An input [8][8][8], its global average and one more layer."""
    return f"7767517\n3 {blobs}\nInput data 0 1 data 0=8 1=8 2=8\nPooling gap 1 1 data gap 0=1 4=1\n{line}\n".encode()


def _load(line, extended=True):
    from feathercnn_amd.net import Net
    net = Net()
    if extended:
        net.SetExtendedLayers(True)
    net.LoadParam(_two(line))
    return net


def _refused(line, extended=True):
    from feathercnn_amd import FeatherHipError
    with pytest.raises(FeatherHipError) as e:
        _load(line, extended)
    return str(e.value)


def test_a_default_net_refuses_lrn_and_names_the_switch():
    for line in ("LRN n 1 1 data n", "LRN n 1 1 data n 0=0 1=5 2=1e-4 3=0.75"):
        msg = _refused(line, extended=False)
        assert "code -200" in msg and "LRN" in msg and "fhip_net_set_extended_layers" in msg, msg


def test_load_param_accepts_lrn():
    for line in ("LRN n 1 1 data n", "LRN n 1 1 data n 0=0 1=5 2=1.0e-04 3=0.75", "LRN n 1 1 data n 0=1 1=3 2=2.0 3=0.5 4=2.0", "LRN n 1 1 gap n 1=1",
                 "LRN n 1 1 data n 1=9 2=0.0", "LRN n 1 1 data n 0=0 1=5 2=1e-4 3=-0.75 4=1e-3"):
        net = _load(line)
        assert net.layers()[2] == ("LRN", "n", "LRN"), line
        net.LoadWeights(b"")  # the layer has no weights
    assert _load("HardSwish m 1 1 data m").layers()[2] == ("HardSwish", "m", "RESAMPLE")  # the other extended types load as before


# A param value is stored as ncnn stores it: a token with '.', 'e' or 'E' is a float, any other token goes through atoi ("nan" and "inf" are
# 0), and the reader takes the 32 bits as the type it wants: the int -1 and 2147483647 are NaNs to a float reader, the float 1e30 is the int
# 1900671690 to an int reader, nan.0 the int 2143289344 and inf.0 the int 2139095040 (both even), -1.5 a negative int.
OK = None
HOSTILE_VALUES = ("-1", "0", "2147483647", "nan", "inf", "-1.5", "0.0", "1e30", "nan.0", "inf.0")  # the ten of tests/test_resample_cpu.py
HOSTILE = {
    # 0 = region_type: nothing but 0 and 1
    0: {"-1": "region_type", "0": OK, "2147483647": "region_type", "nan": OK, "inf": OK, "-1.5": "region_type", "0.0": OK, "1e30": "region_type",
        "nan.0": "region_type", "inf.0": "region_type"},
    # 1 = local_size: odd and at least 1; 2147483647 is odd, and a window wider than the tensor is every channel there is
    1: {**dict.fromkeys(HOSTILE_VALUES, "local_size"), "2147483647": OK},
    # 2 = alpha: finite, not negative
    2: {"-1": "finite", "0": OK, "2147483647": "finite", "nan": OK, "inf": OK, "-1.5": "alpha >= 0", "0.0": OK, "1e30": OK, "nan.0": "finite", "inf.0": "finite"},
    # 3 = beta: finite
    3: {"-1": "finite", "0": OK, "2147483647": "finite", "nan": OK, "inf": OK, "-1.5": OK, "0.0": OK, "1e30": OK, "nan.0": "finite", "inf.0": "finite"},
    # 4 = bias: finite, positive
    4: {"-1": "finite", "0": "bias > 0", "2147483647": "finite", "nan": "bias > 0", "inf": "bias > 0", "-1.5": "bias > 0", "0.0": "bias > 0", "1e30": OK,
        "nan.0": "finite", "inf.0": "finite"},
}


@pytest.mark.parametrize("pid", sorted(HOSTILE))
def test_hostile_param_values(pid):
    """Every id of the layer with negative, zero, huge, NaN and inf values: accepted where the definition gives the value a meaning, else
    -100 with a message that names the layer; nothing crashes."""
    import test_resample_cpu
    assert HOSTILE_VALUES == test_resample_cpu.HOSTILE_VALUES and set(HOSTILE[pid]) == set(HOSTILE_VALUES)
    for value, word in HOSTILE[pid].items():
        line = f"LRN m 1 1 data m {pid}={value}"
        if word is OK:
            assert _load(line).layers()[2] == ("LRN", "m", "LRN"), line
        else:
            msg = _refused(line)
            assert "code -100" in msg and "layer m" in msg and word in msg, (line, msg)


@pytest.mark.parametrize("line,code,word", [("LRN m 2 1 data gap m", -100, "one bottom"), ("LRN m 1 2 data m m2", -100, "one top"), ("LRN m 0 1 m", -300, "0 bottoms"),
                                            ("LRN m 1 1 data m 1=4", -100, "local_size 4"), ("LRN m 1 1 data m 1=6 2=1e-4", -100, "local_size 6"),
                                            ("LRN m 1 1 data m 0=2", -100, "region_type 2"), ("LRN m 1 1 nowhere m", -300, "nowhere"),
                                            ("LRN m 1 1 data m 40=1.0", -2, "out of range"), ("Normalize m 1 1 data m", -200, "Normalize")])
def test_load_param_refuses_with_the_switch_on(line, code, word):
    msg = _refused(line)
    assert f"code {code}" in msg and word in msg, msg


def _fused_layers(param, weights, level, keep_net=False):
    """The layer list after the fusion pass: Forward runs it first and then stops at the input that has not been fed."""
    from feathercnn_amd import FeatherHipError
    from feathercnn_amd.net import Net
    net = Net(fusion=level)
    net.SetExtendedLayers(True)
    net.LoadParam(param)
    net.LoadWeights(weights)
    with pytest.raises(FeatherHipError, match="has not been fed"):
        net.Forward()
    return net if keep_net else net.layers()


def test_fusion_2_makes_lrn_and_the_pooling_behind_it_one_layer():
    from feathercnn_amd import FeatherHipError, model_zoo
    p, b, _, _ = model_zoo.tiny_lrn()
    every = [nm for _, nm, *_ in R.resample_ref.shuffle_ref.parse_param(p)]
    fuse, keep = model_zoo.LRN_POOLS["tiny_lrn"]
    pools = {"norm1": "pool1", "norm2": "pool2", "norm5": "pool5"}
    for level in (0, 1):
        got = _fused_layers(p, b, level)
        routes = {nm: (t, a) for t, nm, a in got}
        assert all(routes[nm] == ("LRN", "LRN") for nm in fuse + keep) and all(routes[pl] == ("Pooling", None) for pl in pools.values())
        assert [nm for _, nm, _ in got] == [nm for nm in every if nm in routes]
    for level in (2, 3):
        net = _fused_layers(p, b, level, keep_net=True)
        got = net.layers()
        names = [nm for _, nm, _ in got]
        routes = {nm: (t, a) for t, nm, a in got}
        assert all(routes[nm] == ("LRN", "LRN") for nm in fuse + keep)
        assert not any(pl in names for pl in pools.values())  # the pooling layers behind norm1, norm2 and norm5 are gone ...
        assert all(pl in names for pl in ("pool3", "pool4", "gap_a", "gap_c"))  # ... the one beside conv3, the one in front of norm4 and the global ones stay
        assert names == [nm for nm in every if nm in names]  # nothing moved
        for blob, inside in (("norm1", True), ("norm2", True), ("norm5", True), ("pool1", False), ("pool2", False), ("norm3", False), ("norm4", False), ("pool5", False)):
            if inside:  # the normalised tensor has no storage
                with pytest.raises(FeatherHipError, match="fused into its consumer"):
                    net.ExtractDevice(blob)
            else:
                net.ExtractDevice(blob)


@pytest.mark.parametrize("name,size,lrns", [("alexnet", 67, 2), ("caffenet", 67, 2), ("googlenet", 31, 2)])
def test_net_loads_the_zoo_nets(name, size, lrns):
    from feathercnn_amd import FeatherHipError, model_zoo
    from feathercnn_amd.net import Net
    assert name in model_zoo.EXTENDED_NETS and name in model_zoo.MODELS
    p, b, i, o = model_zoo.MODELS[name](size=size)
    layers = R.resample_ref.shuffle_ref.parse_param(p)
    assert R.Net(p, b).read == len(b)  # the restatement reads every weight byte ...
    new = [nm for t, nm, *_ in layers if t == "LRN"]
    assert len(new) == lrns and tuple(new) == tuple(sorted(sum(model_zoo.LRN_POOLS[name], ()), key=new.index))
    assert model_zoo.MODELS[name](dry=True, size=size) == (p, len(b), i, o)  # the dry builder writes the same .param and counts the same bytes
    for level in (0, 1):
        net = Net(fusion=level)
        net.SetExtendedLayers(True)
        net.LoadParam(p)
        net.LoadWeights(b)  # ... and so does the runtime (a short read is an error)
        got = net.layers()
        assert [(t, nm) for t, nm, _ in got] == [(t, nm) for t, nm, *_ in layers]
        assert [nm for _, nm, a in got if a == "LRN"] == new
    fuse, keep = model_zoo.LRN_POOLS[name]
    names = [nm for _, nm, _ in _fused_layers(p, b, 2)]
    behind = {nm: layers[[l[1] for l in layers].index(nm) + 1][1] for nm in new}  # the layer written behind each LRN
    assert all(nm in names for nm in new)
    assert all(behind[nm] not in names for nm in fuse) and all(behind[nm] in names for nm in keep)  # LRN -> Pooling is one layer, Pooling -> LRN is not
    with pytest.raises(FeatherHipError) as e:  # without the switch the file is refused at its first LRN
        Net().LoadParam(p)
    assert "code -200" in str(e.value) and "LRN" in str(e.value)


def test_zoo_nets_are_the_published_ones():
    from feathercnn_amd import model_zoo
    parse = R.resample_ref.shuffle_ref.parse_param
    count = lambda p, t: sum(tt == t for tt, *_ in parse(p))
    for name, published in (("alexnet", 61.0e6), ("caffenet", 61.0e6), ("googlenet", 7.0e6)):
        p, nbytes, i, o = model_zoo.MODELS[name](dry=True)
        params = (nbytes - 4 * (count(p, "Convolution") + count(p, "ConvolutionDepthWise") + count(p, "InnerProduct"))) / 4  # without the 4-byte tags
        assert abs(params - published) <= 0.01 * published, (name, params)
        assert count(p, "LRN") == 2 and (i, o) == ("data", "prob")
        assert all(pd == {0: 0, 1: 5, 2: pytest.approx(1e-4), 3: 0.75, 4: 1.0} for t, _, _, _, pd in parse(p) if t == "LRN")
    p = model_zoo.alexnet(dry=True)[0]
    assert b"Input data 0 1 data 0=227 1=227 2=3" in p and count(p, "ConvolutionDepthWise") == 3  # conv2 / conv4 / conv5 in two groups
    assert [l[1] for l in parse(p) if l[0] in ("LRN", "Pooling")] == ["norm1", "pool1", "norm2", "pool2", "pool5"]
    assert [l[1] for l in parse(model_zoo.caffenet(dry=True)[0]) if l[0] in ("LRN", "Pooling")] == ["pool1", "norm1", "pool2", "norm2", "pool5"]
    assert model_zoo.alexnet(dry=True)[1] == model_zoo.caffenet(dry=True)[1]
    p = model_zoo.googlenet(dry=True)[0]
    assert count(p, "Concat") == 9 and count(p, "Convolution") == 57 and count(p, "InnerProduct") == 1 and count(p, "Dropout") == 1
    order = [l[1] for l in parse(p)]
    assert order.index("pool1/3x3_s2") + 1 == order.index("pool1/norm1") and order.index("conv2/norm2") + 1 == order.index("pool2/3x3_s2")
    assert not any("loss1" in nm or "loss2" in nm for nm in order)  # no auxiliary heads


def test_existing_builders_write_what_they_wrote():
    """GraphBuilder gained a method only: the .param text of nets that do not use it keeps its digest."""
    import hashlib
    from feathercnn_amd import model_zoo
    want = {"tiny_allsorts": "b910eddbebf3", "resnet50": "9346900569a1", "tiny_shuffle": "c8606d220268", "tiny_dilated": "a04e50b121f6", "tiny_generative": "89d183a43348"}
    got = {k: hashlib.sha256(model_zoo.MODELS[k](dry=True)[0]).hexdigest()[:12] for k in want}
    assert got == want, got
