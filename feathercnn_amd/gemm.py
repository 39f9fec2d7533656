"""Python host-side mirror of include/feather_hip/feather_gemm.h (``libfeather_gemm.so``): the product of two run-time matrices -- ncnn's Gemm
and MatMul -- batched, with either operand transposed, on torch CUDA tensors.  Every device call goes through the C-ABI on the current
stream; there is no fallback path.
"""
from __future__ import annotations

import ctypes

from . import _lib
from .booster import _stream

NET_ROUTE = 121  # FHIP_GEMM_NET_ROUTE
TILE_SMALL, TILE_WIDE, K_STEP, WIDE_BLOCKS, THIN_MAX = 64, 128, 16, 512, 8  # FHIP_GEMM_*

_check = _lib.checker(_lib.load_gemm_library, "fhip_gemm_last_error")

_INTS = "m n k batch trans_a trans_b out_transpose c_broadcast lda ldb ldc ldd a_batch_stride b_batch_stride c_batch_stride d_batch_stride tile".split()


class GemmDesc(ctypes.Structure):
    """fhip_gemm_desc, field for field."""
    _fields_ = [(name, ctypes.c_int) for name in _INTS] + [("alpha", ctypes.c_float), ("beta", ctypes.c_float)]


def gemm_route(desc: GemmDesc) -> str:
    """The kernel instantiation a call would launch (fhip_gemm_route): no device call."""
    name = ctypes.create_string_buffer(96)
    _check(_lib.load_gemm_library().fhip_gemm_route(ctypes.byref(desc), name, 96), "fhip_gemm_route")
    return name.value.decode()


def _f32(t, what):
    import torch
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32:
        raise ValueError(f"{what} must be a float32 CUDA tensor")
    return ctypes.c_void_p(t.data_ptr())


def forward(desc: GemmDesc, a, b, c, d):
    """fhip_gemm_forward on the memory the tensors start at, exactly as the description says (its strides, not the tensors'): the form for
    views of larger buffers.  c: None where desc.c_broadcast is -1."""
    _check(_lib.load_gemm_library().fhip_gemm_forward(ctypes.byref(desc), _f32(a, "a"), _f32(b, "b"), None if c is None else _f32(c, "c"), _f32(d, "d"), _stream()),
           "fhip_gemm_forward")
    return d


def _matrices(t, what):
    """(rows, cols, ld, batch or 0, batch stride) of a [rows][cols] or [batch][rows][cols] view with contiguous columns."""
    _f32(t, what)
    if t.dim() not in (2, 3) or (t.shape[-1] > 1 and t.stride(-1) != 1):
        raise ValueError(f"{what} must be [rows][cols] or [batch][rows][cols] with unit column stride")
    rows, cols = t.shape[-2:]
    ld = t.stride(-2) if rows > 1 else cols
    return rows, cols, ld, (t.shape[0] if t.dim() == 3 else 0), (t.stride(0) if t.dim() == 3 and t.shape[0] > 1 else 0)


def gemm(a, b, c=None, alpha: float = 1.0, beta: float = 1.0, trans_a: bool = False, trans_b: bool = False, out_transpose: bool = False, c_broadcast=None,
         tile: int = 0, out=None):
    """D = alpha op(A) op(B) + beta bcast(C) (fhip_gemm_forward).  a: [M][K] ([K][M] with trans_a), b: [K][N] ([N][K] with trans_b), each
    optionally with a leading batch; an operand without one is broadcast.  c: None, or a tensor whose shape says how it broadcasts, as in
    ncnn -- one element, [M], [N] (where N != M), [M][1], [M][N], [1][N] -- or whatever `c_broadcast` (0 .. 4) names; shared by the batch.
    -> out [batch][M][N] ([batch][N][M] with out_transpose), without the batch where neither operand has one."""
    import torch
    ra, ca, lda, ba, sa = _matrices(a, "a")
    rb, cb_, ldb, bb, sb = _matrices(b, "b")
    (k, m), (k2, n) = ((ra, ca) if trans_a else (ca, ra)), ((cb_, rb) if trans_b else (rb, cb_))
    if k != k2 or (ba and bb and ba != bb):
        raise ValueError("a and b must agree in K and in batch")
    batch = max(ba, bb, 1)
    kind, ldc = -1, n
    if c is not None:
        _f32(c, "c")
        shape = tuple(c.shape)
        kind = c_broadcast if c_broadcast is not None else (0 if c.numel() == 1 else {(m,): 1, (m, 1): 2, (m, n): 3, (1, n): 4, (n,): 4}.get(shape, -2))
        if kind not in range(5) or not c.is_contiguous() or c.numel() != (1, m, m, m * n, n)[kind]:
            raise ValueError("c must be contiguous and broadcast to [M][N] by one of the five rules")
    shape = (n, m) if out_transpose else (m, n)
    if out is None:
        out = torch.empty(((batch,) if ba or bb else ()) + shape, device=a.device, dtype=torch.float32)
    if tuple(out.shape[-2:]) != shape or not out.is_contiguous() or out.numel() != batch * m * n:
        raise ValueError("out must be contiguous [batch][M][N] ([batch][N][M] with out_transpose)")
    desc = GemmDesc(m=m, n=n, k=k, batch=batch, trans_a=int(bool(trans_a)), trans_b=int(bool(trans_b)), out_transpose=int(bool(out_transpose)), c_broadcast=kind,
                    lda=lda, ldb=ldb, ldc=ldc, ldd=shape[1], a_batch_stride=sa, b_batch_stride=sb, c_batch_stride=0, d_batch_stride=m * n, tile=int(tile),
                    alpha=float(alpha), beta=float(beta))
    return forward(desc, a, b, c, out)


def matmul(a, b, trans_b: bool = False):
    """ncnn's MatMul, numpy's rules on tensors of rank 1 to 3: rank 1 . rank 1 -> [1]; [M][K] . [K][N] -> [M][N]; [K] . [K][N] -> [N];
    [M][K] . [K] -> [M]; rank 3 on either side is a batch, an operand of rank 2 is broadcast.  trans_b reads b's last two dimensions as
    [N][K]; it has no effect on a b of rank 1."""
    ra, rb = a.dim(), b.dim()
    if not 1 <= ra <= 3 or not 1 <= rb <= 3 or (1 in (ra, rb) and 3 in (ra, rb)):
        raise ValueError("matmul takes tensors of rank 1 to 3, and no rank 1 with rank 3")
    out = gemm(a[None] if ra == 1 else a, b[None] if rb == 1 else b, trans_b=trans_b or rb == 1, beta=0.0)  # a column of K floats is [1][K] read as [N][K]
    return out.reshape(-1) if 1 in (ra, rb) else out
