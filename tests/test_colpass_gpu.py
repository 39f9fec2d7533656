"""libfeather_colpass.so on the MI355X, through ctypes like the other side libraries: the tile GEMM that writes the column-passed M (48
planes) and the chained transform that reads it, against the main library's route on the same V (bit for bit) and against the float64
restatement of tests/colpass_cases.py (the project's bound).  V, M48 and V' are filled with NaN before every run: a column nobody wrote
shows up.  The GEMM of a case runs once and is shared by its epilogues."""
import ctypes
import functools

import numpy as np
import pytest

import colpass_cases as CC
from inorm_ref import plane_nerr

pytestmark = pytest.mark.gpu
WINO = 4  # FHIP_WINOGRADF63
TOL = 1e-4


def _param(ic, oc, h, w, bias, relu, batch):
    from feathercnn_amd import ConvParam
    p = ConvParam(output_channels=oc, input_channels=ic, input_h=h, input_w=w, kernel_h=3, kernel_w=3, stride_h=1, stride_w=1, pad_left=1,
                  pad_right=1, pad_top=1, pad_bottom=1, group=1, bias_term=bias, activation=1 if relu else 0, batch=batch)
    p.AssignOutputDim()
    return p


def _batch(case):
    """The case's batch; None = the first batch whose columns cross the column block of the blocked layout."""
    from feathercnn_amd.booster import winograd_plan
    name, k, h, w, batch, pool = case
    if batch is not None:
        return batch
    tx, ty = CC.tiles(h, w)
    batch = 1024 // (tx * ty) + 1
    pl = winograd_plan(_param(64, k, h, w, True, True, batch))
    assert pl.column_block < pl.columns <= pl.columns_padded and pl.columns % pl.column_block, "the columns do not cross a block boundary"
    return batch


@functools.lru_cache(maxsize=None)
def _gemms(case):
    """Both tile GEMMs of the case on one seeded V -> (layer, plan, V, M, M48)."""
    import torch

    from feathercnn_amd import ConvLayer, _lib
    from feathercnn_amd.booster import _check, _ptr, _stream, winograd_plan
    name, k, h, w, _, pool = case
    batch = _batch(case)
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(len(name) + k + h)
    wt = torch.from_numpy((rng.standard_normal((k, 64, 3, 3)) / np.sqrt(9 * 64)).astype(np.float32)).to(dev)
    prm = _param(64, k, h, w, True, True, batch)
    layer = ConvLayer(prm, wt, None, algo=WINO)
    pl = winograd_plan(prm)
    assert pl.frequency_points == 64
    v = torch.from_numpy(rng.uniform(-1, 1, pl.v_bytes // 4).astype(np.float32)).to(dev)  # every column, the padding too, holds data
    m = torch.full((pl.m_bytes // 4,), float("nan"), dtype=torch.float32, device=dev)
    m48 = torch.full((pl.m_bytes // 4,), float("nan"), dtype=torch.float32, device=dev)  # the existing M slot holds it
    c = prm._c()
    _check(_lib.load_library().fhip_winograd_f63_tile_gemm(ctypes.byref(c), batch, _ptr(m), _ptr(layer.packed), _ptr(v), _stream()), "tile_gemm")
    lib = _lib.load_colpass_library()
    rc = lib.fhip_colpass_tile_gemm(ctypes.byref(c), batch, ctypes.byref(pl), _ptr(m48), _ptr(layer.packed), _ptr(v), _stream())
    assert rc == 0, lib.fhip_colpass_last_error()
    torch.cuda.synchronize()
    return layer, pl, v, m, m48


def _rows48(buf, pl, rows):
    """M48 as [48][rows][Pp]: wino_layout(rows, Pp, BP, 48)."""
    pp, bp = pl.columns_padded, pl.column_block
    flat = buf.reshape(-1)[:48 * rows * pp]
    return flat.reshape(48, rows, pp) if bp >= pp else flat.reshape(pp // bp, 48, rows, bp).permute(1, 2, 0, 3).reshape(48, rows, pp)


def _boundaries(case, bias, relu):
    """Both chained transforms of the case with this epilogue -> (V' of the main route, V' of the new one, consumer's plan, bias on the host)."""
    import torch

    from feathercnn_amd import _lib
    from feathercnn_amd.booster import _check, _ptr, _stream, winograd_plan
    name, k, h, w, _, pool = case
    batch = _batch(case)
    layer, pl, v, m, m48 = _gemms(case)
    dev = v.device
    b = np.random.default_rng(5).uniform(-0.5, 0.5, k).astype(np.float32) if bias else None
    bd = torch.from_numpy(b).to(dev) if bias else None
    p = _param(64, k, h, w, bias, relu, batch)
    ah, aw = (h // 2, w // 2) if pool else (h, w)
    nx = _param(k, k, ah, aw, True, True, batch)
    pn = winograd_plan(nx)
    cp, cn = p._c(), nx._c()
    want = torch.full((pn.v_bytes // 4,), float("nan"), dtype=torch.float32, device=dev)
    got = torch.full((pn.v_bytes // 4,), float("nan"), dtype=torch.float32, device=dev)
    _check(_lib.load_library().fhip_winograd_f63_output_to_next_input(ctypes.byref(cp), ctypes.byref(cn), batch, _ptr(want), _ptr(m), _ptr(bd), int(pool),
                                                                      _stream()), "output_to_next_input")
    lib = _lib.load_colpass_library()
    rc = lib.fhip_colpass_output_to_next_input(ctypes.byref(cp), ctypes.byref(cn), batch, ctypes.byref(pl), ctypes.byref(pn), _ptr(got), _ptr(m48),
                                               _ptr(bd), int(pool), _stream())
    assert rc == 0, lib.fhip_colpass_last_error()
    torch.cuda.synchronize()
    return want, got, pn, b


@pytest.mark.parametrize("case", CC.CASES, ids=[c[0] for c in CC.CASES])
def test_m48_is_the_column_pass_of_the_main_gemms_m(cuda, case):
    from feathercnn_amd.booster import winograd_rows
    name, k, h, w, _, pool = case
    layer, pl, v, m, m48 = _gemms(case)
    cols = pl.columns
    m_host = winograd_rows(m, pl, k)[:, :, :cols].cpu().numpy()
    got = _rows48(m48, pl, k)[:, :, :cols].cpu().numpy()
    assert np.isfinite(m_host).all() and np.isfinite(got).all()
    want = CC.column_pass(m_host)
    assert want.dtype == np.float32 and np.array_equal(got, want), float(np.abs(got - want).max())


# every case with and without bias and ReLU; the small planes with one of them alone too (every instantiation of the chained kernel)
BOUNDARIES = [(c, b, r) for c in CC.CASES for b, r in (CC.EPILOGUES if c[2] <= 28 else CC.EPILOGUES[:2])]


@pytest.mark.parametrize("case,bias,relu", BOUNDARIES, ids=[f"{c[0]}-bias{int(b)}-relu{int(r)}" for c, b, r in BOUNDARIES])
def test_next_input_equals_the_main_routes_and_the_float64_restatement(cuda, case, bias, relu):
    import torch

    from feathercnn_amd.booster import winograd_rows
    name, k, h, w, _, pool = case
    batch = _batch(case)
    want, got, pn, b = _boundaries(case, bias, relu)
    g, wv = winograd_rows(got, pn, k)[:, :, :pn.columns], winograd_rows(want, pn, k)[:, :, :pn.columns]
    assert not torch.isnan(g).any(), "NaN: a column of V' nobody wrote"
    assert torch.equal(g, wv), f"{name}: V' max diff {(g - wv).abs().max().item():.3e}"
    layer, pl, v, m, m48 = _gemms(case)
    # float64 from the same V and the packed filter: M = U V per frequency point, then the boundary
    u = layer.packed[:64 * pl.in_channels_padded * pl.out_channels_padded].reshape(64, pl.in_channels_padded, pl.out_channels_padded)[:, :64, :k]
    vv = winograd_rows(v, pl, 64)[:, :, :pl.columns]
    m64 = torch.einsum("xck,xcp->xkp", u.double(), vv.double()).cpu().numpy()
    ref = CC.next_input(m64, b, relu, pool, h, w, batch)
    e = plane_nerr(g.cpu().numpy().reshape(64, k, 1, -1), ref.reshape(64, k, 1, -1))
    print(f"{name} bias={bias} relu={relu}: plane_nerr of V' vs float64 = {e:.3e}")
    assert e <= TOL, e


@pytest.mark.parametrize("case", CC.BIG, ids=[c[0] for c in CC.BIG])
def test_an_m_of_the_nt_size_class_equals_the_main_routes(cuda, case):
    """The sizes from which M leaves through `nt` stores (a 64-plane M of FHIP_M_NT_BYTES): V' of both routes, bit for bit."""
    import torch

    from feathercnn_amd.booster import winograd_rows
    name, k, h, w, batch, pool = case
    assert CC.kernels_of(case, True, True)[0] == CC.GEMM(k == 64, True)
    want, got, pn, _ = _boundaries(case, True, True)
    g, wv = winograd_rows(got, pn, k)[:, :, :pn.columns], winograd_rows(want, pn, k)[:, :, :pn.columns]
    assert not torch.isnan(g).any() and torch.equal(g, wv)
    _gemms.cache_clear()  # hundreds of MB per case
