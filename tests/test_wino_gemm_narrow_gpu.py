"""Narrow last column tile of the LDS-DMA Winograd tile GEMM (wino_gemm_glds.h; the function replaced is reference TensorGEMM,
src/booster/avx/winograd_kernels_F63.cpp:518-692).  A whole-tile block of the last 64-column tile whose live columns fit in 32 re-tiles
its four waves 4 x 1 and computes columns n0 .. n0 + 31 only.  Every case runs the stage entry points (weight transform, input transform,
tile GEMM) on NaN-filled U, V and M and checks the live columns of M twice:

  * against the fp64 product U_xi . V_xi of the U and V the launch read, at test_parity_gpu.py's bar for M (normalised error <= 1e-5);
  * bit for bit against the full-tile path of the same kernel: the same U and the same V columns [0, P) in a second problem of the same
    plane size and a larger batch, chosen so that every tile holding one of those columns is a full 64-column tile and the launch is still
    routed to wino_gemm_glds_kernel (the arithmetic is next to each case).

All shapes have C = 128 (8 k-tiles: the LDS-DMA kernel) and K >= 128 (whole rows of V and M).  With c96(P) = ceil(P / 96) * 96 and
c64(P) = ceil(P / 64) * 64, wino_gemm_prefers_96(P) is c96 < c64 or (P % 96 == 0 and P <= 576); it must be false for P and P'."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

# (id, K, plane, batch, P, live columns of the last tile, larger batch, P')
CASES = [
    # a: one narrow tile per row tile.  c96(18) = 96 > c64 = 64.  P' = 12 x 9 = 108: c96 = 192 > c64 = 128; columns 0 .. 17 lie in tile 0 of 2
    ("a", 128, 14, 2, 18, 18, 12, 108),
    # b: K = 192 is 1.5 row tiles, rows past K masked in the narrow epilogue.  c96(216) = 288 > c64 = 256.  P' = 33 x 9 = 297: c96 = 384 > c64 =
    # 320; columns 0 .. 215 lie in tiles 0 .. 3 of 5
    ("b", 192, 14, 24, 216, 24, 33, 297),
    # c: exactly 32 live columns.  c96(160) = 192 = c64, 160 % 96 != 0.  P' = 13 x 16 = 208: c96 = 288 > c64 = 256; columns 0 .. 159 lie in
    # tiles 0 .. 2 of 4 (tile 3 of P' is narrow itself and holds none of them)
    ("c", 128, 20, 10, 160, 32, 13, 208),
    # d: 33 live columns, the full-tile path.  c96(225) = 288 > c64 = 256.  P' = 297 as in b; columns 0 .. 224 lie in tiles 0 .. 3 of 5
    ("d", 128, 14, 25, 225, 33, 33, 297),
    # e: 7-pixel planes run F(4x4,3x3), 36 frequency points, 4 tiles per image.  c96(200) = 288 > c64 = 256.  P' = 75 x 4 = 300: c96 = 384 >
    # c64 = 320, 300 % 96 != 0; columns 0 .. 199 lie in tiles 0 .. 3 of 5
    ("e", 128, 7, 50, 200, 8, 75, 300),
    # f: M of 64 x 128 x 5248 floats = 172 MB, the `nt`-store instantiation.  c96(5152) = 5184 = c64, 5152 % 96 = 64.  P' = 325 x 16 = 5200:
    # c96 = 5280 > c64 = 5248 (M again 172 MB); columns 0 .. 5151 lie in tiles 0 .. 80 of 82
    ("f", 128, 24, 322, 5152, 32, 325, 5200),
    # g: 64 x 1 x 9 = 576 tiles = 2 x 256 + 64: on 256 CUs the last 64 tiles are cut into quarter row pieces (SPLIT instantiation); the last
    # column tiles of frequency points 0 .. 55 are whole tiles and run narrow, those of 56 .. 63 are row pieces and stay 64 wide.
    # c96(522) = 576 = c64, 522 % 96 != 0.  P' = 65 x 9 = 585: c96 = 672 > c64 = 640; columns 0 .. 521 lie in tiles 0 .. 8 of 10 (640 tiles =
    # 2 x 256 + 128: half pieces on 256 CUs, each 64 columns wide)
    ("g", 128, 14, 58, 522, 10, 65, 585),
]


def _prefers_96(columns):
    c96, c64 = -(-columns // 96) * 96, -(-columns // 64) * 64
    return c96 < c64 or (columns % 96 == 0 and columns <= 576)


def _stages(cuda, k, plane, batch, seed, u=None, v_cols=None):
    """U, V and M (the latter two as [xi][rows][Pp] views) of one 128 -> k layer on plane x plane images: NaN-filled, then written by the
    stage entry points.  `u`: take this U instead of transforming weights; `v_cols`: overwrite V's first columns with these before the GEMM."""
    from feathercnn_amd import ConvParam, _lib, booster
    lib = _lib.load_library()
    p = ConvParam.make(128, k, plane, 3, 1, 1, batch=batch)
    pl = booster.winograd_plan(p)
    assert pl.column_block == pl.columns_padded  # whole rows: winograd_rows is a view, not a copy
    c = p._c()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    dv = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    gen = torch.Generator(device=cuda).manual_seed(seed)
    nxi, pp = pl.frequency_points, pl.columns_padded
    V = torch.full((nxi, 128, pp), float("nan"), device=cuda)
    M = torch.full((nxi, k, pp), float("nan"), device=cuda)
    x = torch.rand((batch, 128, plane, plane), device=cuda, generator=gen) * 2 - 1
    assert lib.fhip_winograd_f63_input_transform(ctypes.byref(c), batch, dv(V), dv(x), st) == 0
    if u is None:
        u = torch.full((nxi, pl.in_channels_padded, pl.out_channels_padded), float("nan"), device=cuda)
        w = torch.rand((k, 128, 3, 3), device=cuda, generator=gen) * 2 - 1
        assert lib.fhip_winograd_f63_transform_kernel(ctypes.byref(c), dv(u), dv(w), st) == 0
    if v_cols is not None:
        booster.winograd_rows(V, pl, 128)[:, :, :v_cols.shape[2]] = v_cols
    assert lib.fhip_winograd_f63_tile_gemm(ctypes.byref(c), batch, dv(M), dv(u), dv(V), st) == 0
    torch.cuda.synchronize()
    return pl, u, booster.winograd_rows(V, pl, 128), booster.winograd_rows(M, pl, k)


@pytest.mark.parametrize("name,k,plane,batch,cols,live,big_batch,big_cols", CASES, ids=[c[0] for c in CASES])
def test_narrow_last_tile_matches_fp64_and_the_full_tile_path(cuda, name, k, plane, batch, cols, live, big_batch, big_cols):
    pl, U, V, M = _stages(cuda, k, plane, batch, seed=7)
    P = pl.columns
    assert P == cols and P - (P - 1) // 64 * 64 == live and not _prefers_96(P)
    if name == "g" and torch.cuda.get_device_properties(0).multi_processor_count == 256:
        tiles = pl.frequency_points * (-(-k // 128)) * (-(-P // 64))
        assert tiles == 576 and tiles % 256 == 64  # quarter row pieces behind 512 whole tiles (another CU count: another class, same checks)
    # fp64: M_xi [K][P] = sum over the C = 128 channels of U_xi [C][K] and V_xi [C][P]
    got = M[:, :k, :P]
    want = torch.einsum("xck,xcp->xkp", U[:, :128, :k].double(), V[:, :, :P].double())
    err = float((got.double() - want).abs().max() / want.abs().max())
    print(f"case {name}: P = {P}, {live} live columns in the last tile, normalised error of M against fp64 = {err:.3e}")
    assert torch.isfinite(got).all()
    assert err <= 1e-5
    if live <= 32:
        # the narrow path was the one that ran: it leaves the other half of its tile as it found it (frequency point 0 is a whole tile in g too)
        n0 = (P - 1) // 64 * 64
        assert torch.isnan(M[0, :k, n0 + 32:n0 + 64]).all()
    # the same columns inside full tiles of a larger launch of the same kernel
    pl2, _, V2, M2 = _stages(cuda, k, plane, big_batch, seed=8, u=U, v_cols=V[:, :, :P])
    assert pl2.columns == big_cols and not _prefers_96(big_cols) and pl2.frequency_points == pl.frequency_points
    assert (P - 1) // 64 < -(-big_cols // 64) - 1  # the tile of column P - 1 is not the last one of the larger launch
    assert torch.equal(V2[:, :, :P], V[:, :, :P])
    assert torch.equal(M2[:, :k, :P], got)
