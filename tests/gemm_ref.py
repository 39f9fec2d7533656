"""include/feather_hip/feather_gemm.h restated in float64 numpy: what tests/test_gemm_gpu.py holds libfeather_gemm.so to, and the rank rules
of the MatMul layer (feather_net.h)."""
import numpy as np

from decoder_ref import normalised_error  # noqa: F401  (the project's error, one definition)


def gemm(a, b, c=None, alpha=1.0, beta=1.0, trans_a=False, trans_b=False, c_broadcast=-1):
    """a [batch or 1][M][K] ([K][M] with trans_a), b [batch or 1][K][N] ([N][K] with trans_b), c: the floats of one broadcast type per
    batch, [batch or 1][...] -> the UNtransposed D [batch][M][N]."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    a, b = (a.transpose(0, 2, 1) if trans_a else a), (b.transpose(0, 2, 1) if trans_b else b)
    batch = max(a.shape[0], b.shape[0])  # a batch of 1 is broadcast (batch stride 0)
    d = float(np.float32(alpha)) * np.einsum("bmk,bkn->bmn", np.broadcast_to(a, (batch,) + a.shape[1:]), np.broadcast_to(b, (batch,) + b.shape[1:]))
    if c_broadcast < 0:
        return d
    m, n = d.shape[1:]
    c = np.asarray(c, np.float64)
    c = c.reshape(c.shape[0], *{0: (1, 1), 1: (m, 1), 2: (m, 1), 3: (m, n), 4: (1, n)}[c_broadcast])
    return d + float(np.float32(beta)) * c


def matmul(a, b, trans_b=False):
    """The MatMul layer on one image: a and b of rank 1 to 3 (no rank 1 with rank 3); trans_b reads b's last two dimensions as [N][K] and has
    no effect on a b of rank 1.  rank 1 . rank 1 -> [1]."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    ra, rb = a.ndim, b.ndim
    if trans_b and rb > 1:
        b = np.swapaxes(b, -1, -2)
    a3, b3 = (a.reshape((1,) * (3 - ra) + a.shape) if ra > 1 else a.reshape(1, 1, -1)), (b.reshape((1,) * (3 - rb) + b.shape) if rb > 1 else b.reshape(1, -1, 1))
    d = gemm(a3, b3)
    return d if 3 in (ra, rb) else (d[0] if (ra, rb) == (2, 2) else d.reshape(-1))
