"""One way to run the entry points of libfeather_detect.so on the device with every tensor between guards (tests/guarded.py): call() for the
layers with one output, the case runners tests/test_detect_gpu.py compares with tests/detect_ref.py, and sweep(), which walks them so that
every instantiation of tests/detect_cases.targets() is launched -- tests/detect_trace_child.py runs it under the kernel trace."""
import ctypes

import numpy as np

import detect_cases as DC
import detect_ref as R
import side_contract
from guarded import Guarded, describe

F = np.float32
V = ctypes.c_void_p


def call(lib, entry, out_count, inputs, offset=0, probe=None):
    """entry(out pointer, [input pointers], stream) -> rc, with the output (poison) and every input in guarded buffers `offset` floats past a
    16-byte boundary: -> the output's values; asserts success, that every output word was written and that no guard word changed.
    probe(out pointer, [input pointers]) is called first with the same pointers (fhip_detect_route on them)."""
    import torch
    ins = [Guarded(np.asarray(a).size, np.asarray(a, F), offset) for a in inputs]
    out = Guarded(out_count, "poison", offset)
    if probe:
        probe(V(out.ptr), [V(g.ptr) for g in ins])
    rc = entry(V(out.ptr), [V(g.ptr) for g in ins], side_contract.stream())
    assert rc == 0, lib.fhip_detect_last_error()
    torch.cuda.synchronize()
    for g in [out] + ins:
        assert g.guards_intact() is None, describe(g.guards_intact())
    assert out.unwritten() == 0, out.unwritten()
    return out.values()


def route(lib, what, a=0, b=0, c=1, h=1, w=1, out=None, x=None):
    name = ctypes.create_string_buffer(128)
    assert lib.fhip_detect_route(what, a, b, c, h, w, out, x, name, 128) == 0, lib.fhip_detect_last_error()
    return name.value.decode()


def permute(lib, x, order, offset=0):
    """x [N][C][H][W] or [N][H][W]."""
    dims = x.ndim - 1
    n, (c, h, w) = x.shape[0], ((1,) + x.shape[1:] if dims == 2 else x.shape[1:])
    got = call(lib, lambda o, i, s: lib.fhip_permute_forward(order, dims, n, c, h, w, o, i[0], s), x.size, [x], offset)
    return got.reshape(R.permute(x, order).shape)


def permute_concat(lib, xs, offset=0):
    k, n = len(xs), xs[0].shape[0]
    c = (ctypes.c_int * k)(*[x.shape[1] for x in xs])
    hw = (ctypes.c_int * k)(*[x.shape[2] * x.shape[3] for x in xs])
    total = sum(x.size for x in xs)
    return call(lib, lambda o, i, s: lib.fhip_permute_concat_forward(k, c, hw, n, o, (V * k)(*i), s), total, xs, offset).reshape(n, -1)


def normalize(lib, x, scale, eps, shared, offset=0, routes=None):
    """routes: a list that receives the instantiation fhip_detect_route names for the very pointers of the call."""
    n, c, h, w = x.shape
    probe = None if routes is None else (lambda o, i: routes.append(route(lib, 1, 0, 0, c, h, w, o, i[0])))
    return call(lib, lambda o, i, s: lib.fhip_normalize_forward(n, c, h, w, int(shared), eps, o, i[0], i[1], s), x.size, [x, scale], offset, probe).reshape(x.shape)


def axis_softmax(lib, x, axis, offset=0):
    outer, inner = int(np.prod(x.shape[:axis], dtype=np.int64)), int(np.prod(x.shape[axis + 1:], dtype=np.int64))
    return call(lib, lambda o, i, s: lib.fhip_axis_softmax_forward(outer, x.shape[axis], inner, o, i[0], s), x.size, [x], offset).reshape(x.shape)


def detection_output(lib, case, loc, conf, prior, thr, offset=0):
    """-> [n][keep_top_k][6]; the scratch lies between guards too and starts as poison."""
    import torch
    name, P, C, n, pn, top_k, keep, cand, nms, kind = case
    nbytes = ctypes.c_size_t()
    assert lib.fhip_detection_output_get_buffer_size(n, P, C, top_k, keep, ctypes.byref(nbytes)) == 0, lib.fhip_detect_last_error()
    scratch = Guarded((nbytes.value + 3) // 4, "poison", 0)
    got = call(lib, lambda o, i, s: lib.fhip_detection_output_forward(n, P, C, nms, top_k, keep, thr, pn, o, i[0], i[1], i[2], V(scratch.ptr), s), n * keep * 6,
               [loc, conf, prior], offset)
    torch.cuda.synchronize()
    assert scratch.guards_intact() is None, describe(scratch.guards_intact())
    return got.reshape(n, keep, 6)


def sweep(lib, seen):
    """Launches every instantiation once on small data, compared with the restatement as it goes; seen(route name) for each launch."""
    rng = np.random.default_rng(5)
    x = rng.uniform(-1, 1, (2, 12, 2, 4)).astype(F)
    for order in (3, 4):
        assert np.array_equal(permute(lib, x, order), R.permute(x, order))
        seen(route(lib, 0, order, 3, 12, 2, 4))
    xs = [x, rng.uniform(-1, 1, (2, 5, 3, 3)).astype(F)]
    assert np.array_equal(permute_concat(lib, xs), R.permute_concat(xs))
    seen(route(lib, 5))
    scale = rng.uniform(0.5, 2, 12).astype(F)
    for offset in (0, 1):  # 16-byte aligned planes of 8 pixels: <4>; a misaligned base: <1>
        named = []
        assert np.array_equal(normalize(lib, x, scale, 1e-10, False, offset, named), R.normalize(x, scale, 1e-10))
        assert named == ["fhip::normalize_kernel<%d>" % (1 if offset else 4)], named
        seen(named[0])
    assert R.nerr(axis_softmax(lib, x, 1), R.softmax(x, 1)) <= 1e-6
    seen(route(lib, 2))
    case, loc, conf, prior, thr, want64, _, _ = DC.detection_case(2)
    assert np.array_equal(detection_output(lib, case, loc, conf, prior, thr)[:, :, 0], want64[:, :, 0])
    seen(route(lib, 3))
    seen(route(lib, 4))
