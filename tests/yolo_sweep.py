"""One way to run the entry points of libfeather_yolo.so on the device with every tensor between guards (tests/guarded.py): reorg() and
detection(), which tests/test_yolo_gpu.py compares with tests/yolo_ref.py, and sweep(), which walks them so that every instantiation of
tests/yolo_cases.targets() is launched -- tests/yolo_trace_child.py runs it under the kernel trace."""
import ctypes

import numpy as np

import side_contract
import yolo_cases as C
import yolo_ref as R
from guarded import Guarded, describe

F = np.float32
V = ctypes.c_void_p


def route(lib, what, a=0, b=0):
    name = ctypes.create_string_buffer(128)
    assert lib.fhip_yolo_route(what, a, b, name, 128) == 0, lib.fhip_yolo_last_error()
    return name.value.decode()


def _finish(buffers, out):
    import torch
    torch.cuda.synchronize()
    for g in buffers:
        assert g.guards_intact() is None, describe(g.guards_intact())
    assert out.unwritten() == 0, out.unwritten()
    return out.values()


def reorg(lib, x, stride, mode=0, offset=0):
    """x [N][C][H][W] -> Reorg(x), input and output (poison) in guarded buffers `offset` floats past a 16-byte boundary."""
    n, c, h, w = x.shape
    oc, oh, ow = c * stride * stride, h // stride, w // stride
    src, out = Guarded(x.size, x, offset), Guarded(n * oc * oh * ow, "poison", offset)
    rc = lib.fhip_reorg_forward(stride, mode, n, c, h, w, V(out.ptr), V(src.ptr), side_contract.stream())
    assert rc == 0, lib.fhip_yolo_last_error()
    return _finish([src, out], out).reshape(n, oc, oh, ow)


def detection(lib, bottoms, version, num_class, num_box, biases, confidence_threshold, nms_threshold, rows, mask=None, anchors_scale=None, offset=0):
    """-> [n][rows][6]; the bottoms, the output (poison) and the scratch (poison) lie between guards."""
    n, k = bottoms[0].shape[0], len(bottoms)
    h, w = (ctypes.c_int * k)(*[x.shape[2] for x in bottoms]), (ctypes.c_int * k)(*[x.shape[3] for x in bottoms])
    nbytes = ctypes.c_size_t()
    assert lib.fhip_yolo_get_buffer_size(n, k, num_box, num_class, h, w, ctypes.byref(nbytes)) == 0, lib.fhip_yolo_last_error()
    ins = [Guarded(x.size, x, offset) for x in bottoms]
    out, scratch = Guarded(n * rows * 6, "poison", offset), Guarded((nbytes.value + 3) // 4, "poison", 0)
    b = (ctypes.c_float * len(biases))(*biases)
    m = (ctypes.c_int * len(mask))(*mask) if mask is not None else None
    s = (ctypes.c_float * len(anchors_scale))(*anchors_scale) if anchors_scale is not None else None
    rc = lib.fhip_yolo_detection_forward(version, n, k, num_box, num_class, h, w, confidence_threshold, nms_threshold, b, len(biases), m, s, rows, V(out.ptr),
                                         (V * k)(*[g.ptr for g in ins]), V(scratch.ptr), side_contract.stream())
    assert rc == 0, lib.fhip_yolo_last_error()
    return _finish(ins + [out, scratch], out).reshape(n, rows, 6)


def sweep(lib, seen):
    """Launches every instantiation once on small data, compared with the restatement as it goes; seen(route name) for each launch, in launch
    order."""
    n, c, h, w, s = C.REORG_SHAPES[0]
    x = np.random.default_rng(5).uniform(-1, 1, (n, c, h, w)).astype(F)
    assert np.array_equal(reorg(lib, x, s), R.reorg(x, s))
    seen(route(lib, 0, s, w))
    n, c, h, w, s = C.REORG_DIRECT[0]
    x = np.random.default_rng(6).uniform(-1, 1, (n, c, h, w)).astype(F)
    assert np.array_equal(reorg(lib, x, s), R.reorg(x, s))
    seen(route(lib, 0, s, w))
    for version in (2, 3):
        bottoms, args, want64, want32, _ = C.case(version, "two_4x4_8x8", 1, 3)
        assert np.array_equal(detection(lib, bottoms, **args)[:, :, 0], want32[:, :, 0])
        seen(route(lib, 1, version))
        seen(route(lib, 2))
