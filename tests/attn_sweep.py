"""One way to run the entry points of libfeather_attn.so on the device with every tensor between guards (tests/guarded.py): attention(),
layer_norm(), add_layer_norm(), gelu() and binary(), which tests/test_attn_gpu.py compares with tests/attn_ref.py, and sweep(), which walks
tables of tests/attn_cases.py so that every instantiation of attn_cases.targets() is launched -- tests/attn_trace_child.py runs it under the
kernel trace."""
import ctypes

import numpy as np

import attn_cases as C
import attn_ref as R
import side_contract
from guarded import CANARY, GUARD, Guarded, describe

F = np.float32
V = ctypes.c_void_p
TOL = 1e-4  # the project's bound (tests/test_net_gpu.py)


class Shifted(Guarded):
    """A Guarded buffer whose body starts `offset` = 0 .. 3 floats past a 16-byte boundary (Guarded itself knows 0 and 1)."""

    def __init__(self, n, fill="poison", offset=0):
        import torch
        if offset not in (0, 1, 2, 3):
            raise ValueError("offset must be 0 .. 3")
        self.n, self.offset, self.guard = int(n), offset, GUARD
        self.raw = torch.full((2 * GUARD + offset + self.n,), CANARY, dtype=torch.int32, device="cuda")
        self.lo = GUARD + offset
        self.body = self.raw.view(torch.float32)[self.lo:self.lo + self.n]
        self.fill(fill)
        assert self.raw.data_ptr() % 16 == 0 and (self.ptr - self.raw.data_ptr()) % 16 == 4 * offset


def route(lib, what, a=0, b=0):
    name = ctypes.create_string_buffer(128)
    assert lib.fhip_attn_route(what, a, b, name, 128) == 0, lib.fhip_attn_last_error()
    return name.value.decode()


def _finish(buffers, out, shape):
    import torch
    torch.cuda.synchronize()
    for g in buffers:
        assert g.guards_intact() is None, describe(g.guards_intact())
    assert out.unwritten() == 0, out.unwritten()
    return out.bits().cpu().numpy().view(np.uint32).reshape(shape).view(F)


def attention(lib, q, k, v, heads, layout="dense", offset=0):
    """-> the attention of q, k, v from guarded buffers laid out as `layout` says (attn_cases.ATTENTION_CASES)."""
    n, tq, e = q.shape
    tk = k.shape[1]
    if layout == "fused":
        buf = Shifted(n * tq * 3 * e, np.concatenate([q, k, v], axis=2), offset)
        ptrs, strides, buffers = (buf.ptr, buf.ptr + 4 * e, buf.ptr + 8 * e), (3 * e,) * 3, [buf]
    elif layout == "kv":
        bq, bkv = Shifted(q.size, q, offset), Shifted(n * tk * 2 * e, np.concatenate([k, v], axis=2), offset)
        ptrs, strides, buffers = (bq.ptr, bkv.ptr, bkv.ptr + 4 * e), (e, 2 * e, 2 * e), [bq, bkv]
    else:
        buffers = [Shifted(t.size, t, offset) for t in (q, k, v)]
        ptrs, strides = tuple(b.ptr for b in buffers), (e, e, e)
    out = Shifted(n * tq * e, "poison", offset)
    rc = lib.fhip_attention_forward(n, heads, tq, tk, e, V(ptrs[0]), strides[0], V(ptrs[1]), strides[1], V(ptrs[2]), strides[2], V(out.ptr), side_contract.stream())
    assert rc == 0, lib.fhip_attn_last_error()
    return _finish(buffers + [out], out, (n, tq, e))


def layer_norm(lib, x, gamma=None, beta=None, eps=1e-3, offset=0):
    rows, l = x.shape
    src, out = Shifted(x.size, x, offset), Shifted(x.size, "poison", offset)
    g, b = (None if t is None else Shifted(l, t, offset) for t in (gamma, beta))
    rc = lib.fhip_layer_norm_forward(rows, l, None if g is None else V(g.ptr), None if b is None else V(b.ptr), ctypes.c_float(eps), V(out.ptr), V(src.ptr),
                                     side_contract.stream())
    assert rc == 0, lib.fhip_attn_last_error()
    return _finish([src, out] + [t for t in (g, b) if t is not None], out, x.shape)


def add_layer_norm(lib, a, b, gamma=None, beta=None, eps=1e-3, offset=0):
    """-> (a + b, LayerNorm(a + b)) of one launch."""
    rows, l = a.shape
    sa, sb, s, y = Shifted(a.size, a, offset), Shifted(b.size, b, offset), Shifted(a.size, "poison", offset), Shifted(a.size, "poison", offset)
    g, bt = (None if t is None else Shifted(l, t, offset) for t in (gamma, beta))
    rc = lib.fhip_add_layer_norm_forward(rows, l, None if g is None else V(g.ptr), None if bt is None else V(bt.ptr), ctypes.c_float(eps), V(s.ptr), V(y.ptr),
                                         V(sa.ptr), V(sb.ptr), side_contract.stream())
    assert rc == 0, lib.fhip_attn_last_error()
    buffers = [sa, sb, s, y] + [t for t in (g, bt) if t is not None]
    return _finish(buffers, s, a.shape), _finish(buffers, y, a.shape)


def gelu(lib, x, fast=0, offset=0):
    src, out = Shifted(x.size, x, offset), Shifted(x.size, "poison", offset)
    rc = lib.fhip_gelu_forward(fast, V(out.ptr), V(src.ptr), x.size, side_contract.stream())
    assert rc == 0, lib.fhip_attn_last_error()
    return _finish([src, out], out, x.shape)


def binary(lib, op, a, b, swap=0, offset=0, b_offset=None):
    """b: a number (the scalar form), an array of a's size (tensor) or of a whole fraction of it (broadcast)."""
    sa, out = Shifted(a.size, a, offset), Shifted(a.size, "poison", offset)
    buffers = [sa, out]
    if np.isscalar(b):
        form, pb, scalar, per = C.SCALAR, None, float(b), 0
    else:
        sb = Shifted(b.size, b, offset if b_offset is None else b_offset)
        buffers.append(sb)
        form, pb, scalar, per = (C.TENSOR if b.size == a.size else C.BROADCAST), V(sb.ptr), 0.0, b.size
    rc = lib.fhip_binary_forward(op, form, swap, V(out.ptr), V(sa.ptr), pb, ctypes.c_float(scalar), a.size, per, side_contract.stream())
    assert rc == 0, lib.fhip_attn_last_error()
    return _finish(buffers, out, a.shape)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


# one attention case per instantiation: d = 32, 64, 96, 128 and a direct one
SWEEP_ATTENTION = [c for c in C.ATTENTION_CASES if c[:3] in ((33, 65, 32), (65, 197, 64), (31, 33, 96), (33, 32, 128), (65, 33, 3)) and c[7] == "plain"]


def sweep(lib, seen):
    """Launches every instantiation once on small data, compared with the restatement as it goes; seen(route name) for each launch, in launch
    order."""
    for case in SWEEP_ATTENTION:
        tq, tk, d, heads, n, layout, offset, _ = case
        q, k, v, want = C.attention_case(case)
        assert R.normalised_error(attention(lib, q, k, v, heads, layout, offset), want) <= TOL, case
        seen(route(lib, C.ATTENTION, d * heads, heads))
    for l in (64, 257):
        x, gamma, beta = C.layer_norm_case(3, l)
        want = R.layer_norm(x, gamma, beta)
        assert R.normalised_error(layer_norm(lib, x, gamma, beta), want) <= TOL, l
        seen(route(lib, C.LAYER_NORM, l, 0))
        s, y = add_layer_norm(lib, x, x[::-1].copy(), gamma, beta)
        assert same_bits(s, x + x[::-1]) and R.normalised_error(y, R.layer_norm(s, gamma, beta)) <= TOL, l
        seen(route(lib, C.LAYER_NORM, l, 1))
    x = np.random.default_rng(1).uniform(-4, 4, 37).astype(F)
    for fast in (0, 1):
        for offset in (0, 1):
            assert R.normalised_error(gelu(lib, x, fast, offset), R.gelu(x, bool(fast))) <= TOL, (fast, offset)
            seen(route(lib, C.GELU, fast, 1 - offset))
    y = np.random.default_rng(2).uniform(1, 2, 40).astype(F)
    for b in (0.5, y[:37].copy(), None):
        for offset in (0, 1):
            a = x if b is not None else np.tile(x, 3)[:40 * 2].copy()
            operand = y if b is None else b  # the broadcast: 80 elements, 40 an image
            assert same_bits(binary(lib, R.MUL, a, operand, offset=offset), R.binary(R.MUL, a.reshape(-1, 40) if b is None else a, operand).reshape(a.shape)), (type(b), offset)
            seen(route(lib, C.BINARY, C.SCALAR if np.isscalar(operand) else (C.TENSOR if operand.size == a.size else C.BROADCAST), 1 - offset))
