"""The tables of the decoder-layer tests (tests/test_decoder_cpu.py, tests/test_decoder_gpu.py, tests/test_later_contract_cpu.py): the kernel
instantiations of libfeather_decoder.so and the attention cases, against the tiles of feather_decoder.h.  A block owns 32, 64 or 128 stacked
rows (R = group * tq <= 32, <= 64, above) and walks the keys in tiles of 32; a head is 1 .. 4 chunks of 32 columns.  Lengths of 33, 40, 70
and 97 end one past a key tile or inside one; 129 and 150 stacked rows take two row tiles, the second boundary inside a head."""
import ctypes
import functools
import os

import numpy as np

import decoder_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "feathercnn_amd", "libfeather_decoder.so")
F = np.float32
TOL = 1e-4  # the project's bound on the normalised error (tests/test_net_gpu.py)
SDPA, COMBINE, KV_CONCAT, RMS_NORM, ROTARY, EMBED = range(6)  # fhip_decoder_op

KERNELS = {"sdpa_kernel", "sdpa_combine_kernel", "kv_concat_kernel", "rms_norm_kernel", "rotary_kernel", "embed_kernel"}


def targets():
    """Every instantiation of the library, by the names fhip_decoder_route reports."""
    return ({"fhip::sdpa_kernel<%d, %d>" % (dc, rw) for dc in (1, 2, 3, 4) for rw in (1, 2, 4)} | {"fhip::sdpa_combine_kernel", "fhip::embed_kernel"} |
            {"fhip::%s_kernel<%d>" % (k, i) for k in ("kv_concat", "rms_norm", "rotary") for i in (0, 1)})


# (tq, tk, d, heads, kv_heads, n, causal, mask, kind, row_tile, splits).  mask: None; "rank2" one [tq][tk]; "full" [n][heads][tq][tk] -- each with
# scattered -inf, row 0 fully masked and keys 32 .. 63 (a whole key tile, and the second of three splits) masked for every row.  kind: "plain", or
# "pm80" q scaled so that the scores reach +-80.
CASES = [
    (1, 1, 4, 1, 1, 1, 0, None, "plain", 0, 0),        # <1, 1>
    (129, 33, 8, 2, 2, 1, 0, None, "plain", 0, 0),     # <1, 4>: one past the row tile and the key tile
    (40, 33, 4, 1, 1, 1, 0, None, "plain", 0, 0),      # <1, 2>
    (50, 40, 36, 6, 2, 2, 0, None, "plain", 0, 0),     # <2, 4>: group 3, 150 stacked rows, the tile boundary inside head 2, a partial chunk
    (97, 97, 64, 2, 1, 1, 1, None, "plain", 0, 0),     # causal: the first row sees one key; the second row tile starts at query 31
    (97, 97, 64, 2, 1, 1, 1, None, "plain", 32, 0),    # <2, 1>: the same in tiles of 32 rows, whose first loads one key tile of four
    (40, 33, 64, 1, 1, 1, 0, None, "plain", 0, 0),     # <2, 2>
    (5, 70, 128, 4, 1, 1, 1, None, "plain", 0, 0),     # <4, 1>: causal with a past of 65
    (12, 40, 128, 4, 1, 1, 0, None, "plain", 0, 0),    # <4, 2>
    (65, 96, 128, 2, 2, 1, 0, None, "pm80", 0, 0),     # <4, 4>: scores of +-80
    (33, 70, 96, 1, 1, 1, 0, "rank2", "plain", 0, 0),  # <3, 2>
    (9, 70, 96, 4, 2, 2, 0, "full", "plain", 0, 0),    # <3, 1>: a mask per head and image
    (70, 40, 96, 2, 1, 1, 1, None, "plain", 0, 0),     # <3, 4>
    (1, 70, 64, 8, 2, 2, 0, None, "plain", 0, 1), (1, 70, 64, 8, 2, 2, 0, None, "plain", 0, 3), (1, 70, 64, 8, 2, 2, 0, None, "plain", 0, 99),  # decoding
    (1, 70, 64, 8, 2, 2, 0, "full", "plain", 0, 3),    # the mask empties the second split
    (3, 70, 64, 8, 2, 2, 1, None, "plain", 0, 3),      # causal, three queries
]
case_id = lambda c: "-".join(str(x) for x in c)  # noqa: E731


@functools.lru_cache(maxsize=None)
def case_data(case):
    """-> (q, k, v, mask or None, scale, the float64 result), shared among the tests, which leave them unchanged."""
    tq, tk, d, heads, kvh, n, causal, mask, kind = case[:9]
    rng = np.random.default_rng(20000 + 13 * tq + 7 * tk + d + heads + (mask is not None))
    q, k, v = (rng.uniform(-1, 1, (n, h, t, d)).astype(F) for h, t in ((heads, tq), (kvh, tk), (kvh, tk)))
    scale = F(1 / np.sqrt(d))
    if kind == "pm80":
        scale = F(80.0 / np.abs(np.einsum("nhtc,nhuc->nhtu", q.astype(np.float64), np.repeat(k, heads // kvh, 1).astype(np.float64))).max())
    m = None
    if mask:
        m = rng.uniform(-2, 2, (tq, tk) if mask == "rank2" else (n, heads, tq, tk)).astype(F)
        m[rng.uniform(size=m.shape) < 0.2] = -np.inf
        m[..., 32:64] = -np.inf
        if tq > 1:
            m[..., 0, :] = -np.inf
    want = R.sdpa(q, k, v, m, bool(causal), scale)
    for a in (q, k, v, m, want):
        if a is not None:
            a.setflags(write=False)
    return q, k, v, m, scale, want


def run(lib, case, layout="dense", offset=0):
    """fhip_sdpa_forward on guarded buffers (tests/guarded.py) `offset` floats past a 16-byte boundary -> (out [n][heads][tq][d], the route,
    the splits used).  layout "dense": head-major blobs; "cache": k and v are views of caches of capacity tk + 3 (head stride > tk d), q and
    out token-major [n][tq][heads][d].  Asserts the guards of every buffer."""
    import side_contract
    from feathercnn_amd.decoder import SdpaDesc
    from guarded import Guarded
    tq, tk, d, heads, kvh, n, causal, _, _, row_tile, splits = case
    q, k, v, m, scale, _ = case_data(case)
    desc = SdpaDesc(n=n, heads=heads, kv_heads=kvh, tq=tq, tk=tk, d=d, causal=causal, splits=splits, row_tile=row_tile, scale=float(scale))
    if layout == "dense":
        cap = tk
        qh = q
        qs = (heads * tq * d, tq * d, d)
    else:
        cap = tk + 3
        qh = q.transpose(0, 2, 1, 3)
        qs = (tq * heads * d, d, heads * d)
    desc.q_image_stride, desc.q_head_stride, desc.q_row_stride = desc.out_image_stride, desc.out_head_stride, desc.out_row_stride = qs
    desc.k_image_stride, desc.k_head_stride, desc.k_row_stride = desc.v_image_stride, desc.v_head_stride, desc.v_row_stride = kvh * cap * d, cap * d, d
    pad = lambda a: np.concatenate([a, np.full((n, kvh, cap - tk, d), np.nan, F)], axis=2)  # the unfilled rows of a cache are never read
    bufs = [Guarded(q.size, np.ascontiguousarray(qh), offset), Guarded(n * kvh * cap * d, pad(k), offset), Guarded(n * kvh * cap * d, pad(v), offset)]
    if m is not None:
        bufs.append(Guarded(m.size, m, offset))
        desc.mask_image_stride, desc.mask_head_stride = (heads * tq * tk, tq * tk) if m.ndim == 4 else (0, 0)
    size, used = ctypes.c_size_t(), ctypes.c_int()
    assert lib.fhip_sdpa_get_buffer_size(ctypes.byref(desc), ctypes.byref(size), ctypes.byref(used)) == 0, lib.fhip_decoder_last_error()
    out, scratch = Guarded(q.size, "poison", offset), Guarded(size.value // 4, "poison", 0)
    rc = lib.fhip_sdpa_forward(ctypes.byref(desc), bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr if m is not None else None, out.ptr,
                               scratch.ptr if size.value else None, side_contract.stream())
    assert rc == 0, lib.fhip_decoder_last_error()
    for b in bufs + [out, scratch]:
        assert b.guards_intact() is None
    assert out.unwritten() == 0
    got = out.values().reshape(qh.shape)
    name = ctypes.create_string_buffer(128)
    assert lib.fhip_decoder_route(SDPA, d, heads // kvh * tq, row_tile, name, 128) == 0
    return (got if layout == "dense" else got.transpose(0, 2, 1, 3)), name.value.decode(), used.value
