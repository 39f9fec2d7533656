"""The tables of the colpass tests (tests/test_colpass_contract_cpu.py, tests/test_colpass_gpu.py, tests/test_colpass_net_gpu.py): the kernel
instantiations of libfeather_colpass.so, the shapes that select them, and the butterflies of csrc/wino_butterfly.h restated on arrays.

A case: (name, K, H, W, batch, pool); C = 64 throughout, the layer is 3x3 / stride 1 / pad 1, its consumer K -> K on the (pooled) plane.
batch = None: chosen from the plan so that the columns cross a column-block boundary of the blocked layout."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "feathercnn_amd", "libfeather_colpass.so")
M_NT_BYTES = 150 << 20  # csrc/wino_gemm_policy.h FHIP_M_NT_BYTES: from this size of the 64-plane M on, M stores are `nt`

_B = {True: "true", False: "false"}
SHAPE = "2, 16, 6"  # waves along the columns, rows of the operands per stage, LDS buffers (csrc_colpass/colpass.hip COLPASS_*)


def GEMM(v_nt, m_nt):
    return f"fhip::colpass_gemm_kernel<{SHAPE}, {int(v_nt) + 2 * int(m_nt)}>"


def CHAIN(bias, relu, pool, multi):
    return f"fhip::colpass_chain_kernel<{_B[bias]}, {_B[relu]}, {_B[pool]}, {_B[multi]}>"


KERNELS = {"colpass_gemm_kernel", "colpass_chain_kernel"}
CASES = [
    ("k64_12x12_n3", 64, 12, 12, 3, False),         # one ragged column tile
    ("k128_20x26_n2", 128, 20, 26, 2, False),       # two row tiles, non-square, tiles past the image edge
    ("k64_28x22_n3_pool", 64, 28, 22, 3, True),
    ("k128_112_n1", 128, 112, 112, 1, False),       # T = 361, the whole-plane form
    ("k64_224_n1_pool", 64, 224, 224, 1, True),     # T = 1444, the MULTI walk
    ("k64_28x22_blocks_pool", 64, 28, 22, None, True),  # the columns cross a column-block boundary
]
# the sizes from which M leaves through `nt` stores, one per V policy; compared with the main route only (no host restatement at this size)
BIG = [
    ("k64_224_n7_pool_big", 64, 224, 224, 7, True),
    ("k128_112_n14_big", 128, 112, 112, 14, False),
]
EPILOGUES = ((True, True), (False, False), (True, False), (False, True))  # (bias, relu)
REFUSALS = [("C = 32", 32, 64, 1), ("C = 128", 128, 64, 1), ("K = 96", 64, 96, 1), ("stride 2", 64, 64, 2)]


def tiles(h, w):
    return (w + 2 + 3) // 6, (h + 2 + 3) // 6  # pad 1 all round


def kernels_of(case, bias, relu):
    """The two instantiations the case launches with this epilogue."""
    _, k, h, w, batch, pool = case
    tx, ty = tiles(h, w)
    ah, aw = (h // 2, w // 2) if pool else (h, w)
    tx2, ty2 = tiles(ah, aw)
    multi = max(tx * ty, tx2 * ty2) > 512
    cols = tx * ty * (batch or 1)
    pp = -(-cols // 128) * 128 if not (k <= 64 and cols > 1024) else -(-cols // 1024) * 1024
    big = batch is not None and 64 * k * pp * 4 >= M_NT_BYTES
    return GEMM(k == 64, big), CHAIN(bias, relu, pool, multi)


def targets():
    out = set()
    for case in CASES + BIG:
        for bias, relu in EPILOGUES:
            out |= set(kernels_of(case, bias, relu))
    out.add(GEMM(False, False))  # K = 128 below the `nt` size: CASES' K = 128 rows (listed for the reader; kernels_of gives it too)
    return out


def at6(m):
    """csrc/wino_butterfly.h at6 on the first axis (8 -> 6), the association of the function text, in the dtype of `m`."""
    m0, m1, m2, m3, m4, m5, m6, m7 = m
    t = m.dtype.type
    a12, d12 = m1 + m2, m1 - m2
    a34, d34 = m3 + m4, m3 - m4
    a56, d56 = m5 + m6, m5 - m6
    return np.stack([(m0 + a12) + (a34 + t(32) * a56), (d12 + t(2) * d34) + t(16) * d56, (a12 + t(4) * a34) + t(8) * a56,
                     (d12 + t(8) * d34) + t(4) * d56, (a12 + t(16) * a34) + t(2) * a56, ((d12 + t(32) * d34) + d56) + m7])


def bt8(r):
    """csrc/wino_butterfly.h bt8 on the first axis (8 -> 8)."""
    r0, r1, r2, r3, r4, r5, r6, r7 = r
    t = r.dtype.type
    t1, t2 = (r2 + r6) - t(4.25) * r4, (r1 + r5) - t(4.25) * r3
    p1, p2 = r6 + (t(0.25) * r2 - t(1.25) * r4), (t(0.5) * r1 - t(2.5) * r3) + t(2) * r5
    q1, q2 = r6 + t(4) * (r2 - t(1.25) * r4), (t(2) * r1 - t(2.5) * r3) + t(0.5) * r5
    return np.stack([(r0 - r6) + t(5.25) * (r4 - r2), t1 + t2, t1 - t2, p1 + p2, p1 - p2, q1 + q2, q1 - q2, (r7 - r1) + t(5.25) * (r3 - r5)])


def column_pass(m):
    """M [64 xi][K][P] -> M48 [48][K][P], plane 8 a + j = at6 over i of xi = 8 i + j, in M's dtype."""
    k, p = m.shape[1:]
    return at6(m.reshape(8, 8, k, p)).reshape(48, k, p)


def next_input(m, bias, relu, pool, h, w, batch):
    """The boundary in float64: M [64][K][>= batch * T] of an h x w layer -> V' [64][K][batch * T2] of its pad-1 consumer."""
    m = np.asarray(m, np.float64)
    k = m.shape[1]
    tx, ty = tiles(h, w)
    t = tx * ty
    m = m[:, :, :batch * t].reshape(8, 8, k, batch, ty, tx)
    y = at6(np.moveaxis(at6(m), 1, 0))  # column pass over i, then row pass over j: [b][a][k][n][ty][tx]
    y = np.transpose(y, (2, 3, 4, 1, 5, 0)).reshape(k, batch, 6 * ty, 6 * tx)[:, :, :h, :w]
    if bias is not None:
        y = y + np.asarray(bias, np.float64)[:, None, None, None]
    if relu:
        y = np.maximum(y, 0)
    if pool:
        y = y.reshape(k, batch, h // 2, 2, w // 2, 2).max(axis=(3, 5))
    ah, aw = y.shape[2:]
    tx2, ty2 = tiles(ah, aw)
    d = np.zeros((k, batch, 6 * ty2 + 2, 6 * tx2 + 2))
    d[:, :, 1:1 + ah, 1:1 + aw] = y
    win = np.stack([np.stack([d[:, :, i:i + 6 * ty2:6, j:j + 6 * tx2:6] for j in range(8)]) for i in range(8)])  # [i][j][k][n][ty2][tx2]
    v = bt8(np.moveaxis(bt8(win), 1, 0))  # over i, then over j: [j][i][...]
    return np.moveaxis(v, 1, 0).reshape(64, k, batch * ty2 * tx2)
