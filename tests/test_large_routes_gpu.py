"""Every route once on a tensor that crosses a named power of two (tests/test_large_gpu.py does this for three convolution routes): 2^30 floats,
where a byte offset passes 2^32; 2^31 elements, where a signed index overflows; 2^32 elements, where an unsigned one does (the count-based
layers only).  The side libraries run just below their stated limit of 2^31 elements (tests/limit_cases.py), so their units pass 2^30 and
their byte offsets 2^32.

Each case states which quantity crosses which threshold and asserts it, asserts through the route query that the intended kernel family ran,
starts from an output full of NaN, and compares with tests/large_ref.py: bit for bit on whole slabs for the exact-class operations, at 4000
sampled positions (half of them beyond the threshold, a quarter in the first image) for the rest.  Tolerances are the project's: 1e-4 x scale for
convolutions (scale = max |y| of the first 64 images), 1e-6 x the fp64 sum of |terms| for affine, averages and softmax
(tests/instance_sweep.py), 1e-4 normalised for the side libraries (their own GPU tests).  Peak device memory stays below the 37 GB of
test_large_gpu.py's winograd_V_and_M case.

Routes that cannot reach a threshold, with the figure that rules it out (the route queries are igemm_split / igemm_tail / ip_profitable of
implicit_gemm.hip, seen through fhip_conv_get_buffer_size):

  route                      largest size its query still selects                                              nearest threshold run here
  split-K + reduce           fewer than 512 tiles of 128 x 64 (or 64 x 128): K * columns < 2^22 and at most     the input (the B operand) past 2^31
                             32 pieces, so output and partial sums stay below 2^27 floats; C is not bounded    floats with 40960 channels: run below
  tail split + reduce        at most 8 tiles per CU (2048 tiles): K * columns <= 2^24, scratch < 2^27 floats;   the input past 2^31 floats with 5120
                             C is not bounded                                                                  channels at stride 2: run below
  InnerProduct stream        batch <= 32 and a 1 x 1 image: activations and outputs are tiny, but the weight    weights past 2^30 floats (byte
                             matrix is not limited                                                              offsets past 2^32): run below
  conv_smallc, 2^31 tiles    a tile holds up to 128 outputs of one channel and K <= 64: 2^31 tiles mean more    the output past 2^31 floats
                             than 2^33 output floats (32 GB) at the very least                                  (VGG-16's conv1_1): run below
  fhip_gconv_forward lanes   4 outputs per lane and channel chunk: 2^31 lanes mean 2^33 output floats           tensors past 2^31 elements
  canvas planes (2^31)       a plane holds at least 36 floats: 2^31 planes are 288 GB                           M past 2^31 floats: run below

How a case knows its kernel: where a route query names the kernel (the side libraries) the name is asserted.  The main library's queries tell
families apart (depthwise / implicit GEMM with or without scratch / streamed 1x1 / F(6,3) whole rows / column blocks / F(4,3)), not the
ConvGemmPolicy mode or the depthwise form: those cases use the very geometries that tests/contract_routes.py pins to their kernels by name
(checked there by kernel trace), scaled in the batch only, which none of those choices depends on except where the case says so."""
import ctypes
import gc

import pytest

import large_ref as R
import side_contract

pytestmark = pytest.mark.gpu
TOL, MAG_TOL = 1e-4, 1e-6
NAIVE, IM2COL, DEPTHWISE, WINO = 0, 1, 3, 4
P30, P31, P32 = 2 ** 30, 2 ** 31, 2 ** 32


@pytest.fixture(autouse=True)
def _free_device_memory():
    """Every case frees its tensors; and a case that met a device fault ends the session: nothing more is started on that device."""
    yield
    import torch
    gc.collect()
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"the device reported an error after this case, stopping: {e}", returncode=3)
    torch.cuda.empty_cache()


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


_stream = side_contract.stream


def _main():
    from feathercnn_amd import _lib
    return _lib.load_library()


def _sync():
    import torch
    torch.cuda.synchronize()


def _check_mag(got, want, mag, what):
    err = (got.double() - want).abs()
    assert not bool(err.isnan().any()), f"{what}: unwritten (NaN) output"
    worst = float((err - MAG_TOL * mag).max())
    assert worst <= 0, (what, float(err.max()))


# ---- convolution routes of the main library ---------------------------------------------------------------------------------------------------

def _confirm(what, prm, algo, batch, nbuf):
    """The `what` column of tests/contract_routes.py, evaluated through the launch-free queries."""
    from feathercnn_amd import booster
    lib, c, sel = _main(), prm._c(), ctypes.c_int(-1)
    streams = lib.fhip_conv_streams_1x1(ctypes.byref(c), algo, batch)
    if what.startswith("dw"):
        lib.fhip_conv_select_algo(ctypes.byref(c), ctypes.byref(sel))
        return sel.value == DEPTHWISE and nbuf == 0
    if what in ("igemm_no_scratch", "smallc"):  # contract_routes tells the two apart by geometry: so do the cases here
        return nbuf == 0 and not streams
    if what == "scratch":
        return nbuf > 0
    if what == "streams_1x1":
        return streams == 1 and nbuf == 0
    pl = booster.winograd_plan(prm)
    return {"f63": pl.frequency_points == 64 and pl.column_block >= pl.columns_padded, "f43": pl.frequency_points == 36,
            "column_blocks": pl.frequency_points == 64 and pl.column_block < pl.columns_padded}[what]


def _conv(cuda, c, k, h, ks, s, p, group, batch, algo, what, crosses, threshold=P31, w=None, mode="plain"):
    """One convolution whose `crosses` tensor ("input", "output" or "scratch") holds more than `threshold` floats, against the sampled fp64 direct
    convolution.  mode: "plain", "maxpool2" (fhip_conv_forward_maxpool2) or "residual" (fhip_conv_forward_residual)."""
    import torch

    from feathercnn_amd import ConvLayer, ConvParam
    prm = ConvParam.make(c, k, h, ks, s, p, group=group, bias=True, act=1, w=w, batch=batch)
    gen = torch.Generator(device=cuda).manual_seed(5)
    cpg = c // group
    wt = (torch.rand((prm.output_channels, cpg, ks, ks), device=cuda, generator=gen) * 2 - 1) / (cpg * ks * ks) ** 0.5
    b = (torch.rand((prm.output_channels,), device=cuda, generator=gen) * 2 - 1) * 0.1
    lyr = ConvLayer(prm, wt, b, algo=algo)
    assert lyr.booster.algo == algo
    assert _confirm(what, prm, algo, batch, lyr.buffer_bytes // 4), f"not the {what} route"
    lib, cp = _main(), prm._c()
    x = R.fill(torch.empty((batch, c, h, prm.input_w), device=cuda), 6)
    oh, ow = prm.output_h, prm.output_w
    pooled = mode == "maxpool2"
    if pooled:
        assert lib.fhip_conv_can_fuse_maxpool2(ctypes.byref(cp), algo) == 1
    if mode == "residual":
        assert lib.fhip_conv_can_fuse_residual(ctypes.byref(cp), algo) == 1
    shape = (batch, prm.output_channels, oh // 2, ow // 2) if pooled else (batch, prm.output_channels, oh, ow)
    per_image = {"input": x[0].numel(), "output": shape[1] * shape[2] * shape[3], "scratch": lyr.buffer_bytes // 4 // 2 // batch}[crosses]
    assert per_image * batch > threshold, (crosses, per_image * batch)
    first_beyond = threshold // per_image + 1  # every tensor element of this image and the following ones lies beyond the threshold
    assert first_beyond < batch
    y = R.nans(shape, cuda)
    scratch = torch.empty(max(lyr.buffer_bytes // 4, 1), device=cuda)
    res = R.fill(torch.empty(shape, device=cuda), 7) if mode == "residual" else None
    args = (ctypes.byref(cp), algo, batch, _p(y), _p(x), _p(lyr.packed), _p(scratch), _p(b))
    rc = {"plain": lambda: lib.fhip_conv_forward(*args, _stream()), "maxpool2": lambda: lib.fhip_conv_forward_maxpool2(*args, _stream()),
          "residual": lambda: lib.fhip_conv_forward_residual(*args, _p(res), _stream())}[mode]()
    assert rc == 0, lib.fhip_last_error()
    _sync()
    pos, _ = R.positions(shape, first_beyond * shape[1] * shape[2] * shape[3], cuda)
    if pooled:  # the maximum of the four positions under each pooled one (ReLU and max commute)
        n_, k_, py, px = pos
        want = torch.stack([R.conv_at(x, wt, b, (n_, k_, 2 * py + dy, 2 * px + dx), s, p, 1, group)[0] for dy in (0, 1) for dx in (0, 1)]).amax(0)
    elif mode == "residual":
        want = (R.conv_at(x, wt, b, pos, s, p, 1, group, relu=False)[0] + res[pos].double()).clamp_min(0)
    else:
        want = R.conv_at(x, wt, b, pos, s, p, 1, group)[0]
    got = y[pos].double()
    scale = float(y[:64].abs().max())
    err = (got - want).abs()
    assert not bool(err.isnan().any()), "unwritten (NaN) output"
    assert float(err.max()) <= TOL * scale, (float(err.max()), scale)
    assert float(got[R.S // 2:].abs().max()) > 0, "the images beyond the threshold came back empty"


def test_winograd_staged_input_and_persistent_output_V_past_2_31(cuda):
    """V and M: 64 * 16 * 100 * 21000 = 2.15e9 floats each (> 2^31): staged input transform, SmallM tile GEMM, persistent staged output."""
    _conv(cuda, 16, 16, 56, 3, 1, 1, 1, 21000, WINO, "column_blocks", "scratch")


def test_winograd_glds_tile_gemm_V_past_2_31(cuda):
    """V and M: 64 * 128 * 9 * 29200 = 2.15e9 floats each (> 2^31): wino_gemm_glds / glds96 with whole-row V and M."""
    _conv(cuda, 128, 128, 14, 3, 1, 1, 1, 29200, WINO, "f63", "scratch")


def test_winograd_f43_V_past_2_31(cuda):
    """F(4x4,3x3) on 8-pixel planes: V and M are 36 * 64 * 4 * 233100 = 2.15e9 floats each (> 2^31)."""
    _conv(cuda, 64, 64, 8, 3, 1, 1, 1, 233100, WINO, "f43", "scratch")


def test_winograd_one_shot_output_wide_rows_V_past_2_31(cuda):
    """TX > 256 (1560-pixel rows, 260 tiles each) takes the one-shot output transform: V and M are 64 * 16 * 260 * 8100 = 2.156e9 floats each
    (> 2^31).  An output past 2^31 floats would need 23 GB each of V and M, more than a case may hold: the scratch crosses instead."""
    _conv(cuda, 16, 16, 4, 3, 1, 1, 1, 8100, WINO, "column_blocks", "scratch", w=1560)


def test_winograd_fused_maxpool2_V_past_2_31(cuda):
    """fhip_conv_forward_maxpool2: V and M past 2^31 floats (as the staged case), the pooled output written from the output transform."""
    _conv(cuda, 16, 16, 56, 3, 1, 1, 1, 21000, WINO, "column_blocks", "scratch", mode="maxpool2")


def test_igemm_mode0_3x3_output_past_2_31(cuda):
    """ConvGemmPolicy<0>, Big tile: output 116600 * 128 * 144 = 2.149e9 floats (> 2^31)."""
    _conv(cuda, 16, 128, 12, 3, 1, 1, 1, 116600, IM2COL, "igemm_no_scratch", "output")


def test_igemm_mode1_1x1_stride2_input_past_2_31(cuda):
    """ConvGemmPolicy<1>: input 42900 * 64 * 784 = 2.152e9 floats (> 2^31)."""
    _conv(cuda, 64, 128, 28, 1, 2, 0, 1, 42900, IM2COL, "igemm_no_scratch", "input")


def test_igemm_mode5_ragged_1x1_input_past_2_31(cuda):
    """ConvGemmPolicy<5> (7 x 7 planes as pixel slots), SmallM tile: input 913100 * 48 * 49 = 2.148e9 floats (> 2^31)."""
    _conv(cuda, 48, 40, 7, 1, 1, 0, 1, 913100, IM2COL, "igemm_no_scratch", "input")


def test_igemm_streamed_1x1_input_past_2_31(cuda):
    """stream_gemm_kernel: input 42900 * 256 * 196 = 2.152e9 floats (> 2^31), output 1.08e9 (> 2^30)."""
    _conv(cuda, 256, 128, 14, 1, 1, 0, 1, 42900, IM2COL, "streams_1x1", "input")


def test_igemm_residual_output_past_2_31(cuda):
    """fhip_conv_forward_residual (ConvGemmPolicy<2> with the residual read in the epilogue): output and residual 85700 * 128 * 196 = 2.15e9."""
    _conv(cuda, 32, 128, 14, 1, 1, 0, 1, 85700, IM2COL, "igemm_no_scratch", "output", mode="residual")


def test_naive_output_past_2_31(cuda):
    """FHIP_NAIVE (the implicit GEMM without the activation): output 116600 * 128 * 144 floats (> 2^31); the reference applies no ReLU."""
    import torch

    from feathercnn_amd import ConvLayer, ConvParam
    batch = 116600
    prm = ConvParam.make(16, 128, 12, 3, 1, 1, bias=True, act=1, batch=batch)
    gen = torch.Generator(device=cuda).manual_seed(5)
    wt = (torch.rand((128, 16, 3, 3), device=cuda, generator=gen) * 2 - 1) / 12.0
    b = (torch.rand((128,), device=cuda, generator=gen) * 2 - 1) * 0.1
    lyr = ConvLayer(prm, wt, b, algo=NAIVE)
    assert _confirm("igemm_no_scratch", prm, NAIVE, batch, lyr.buffer_bytes // 4)
    x = R.fill(torch.empty((batch, 16, 12, 12), device=cuda), 6)
    y = R.nans((batch, 128, 12, 12), cuda)
    assert y.numel() > P31
    lyr.Forward(x, out=y)
    _sync()
    pos, _ = R.positions(tuple(y.shape), P31, cuda)
    want = R.conv_at(x, wt, b, pos, 1, 1, relu=False)[0]
    err = (y[pos].double() - want).abs()
    assert not bool(err.isnan().any()) and float(err.max()) <= TOL * float(y[:64].abs().max())


def test_depthwise_flat_14px_past_2_31(cuda):
    """depthwise3x3_flat_kernel: input and output 342400 * 32 * 196 = 2.148e9 floats each (> 2^31)."""
    _conv(cuda, 32, 32, 14, 3, 1, 1, 32, 342400, DEPTHWISE, "dw_flat", "input")


def test_depthwise_direct_30px_past_2_31(cuda):
    """depthwise3x3_direct_kernel: input and output 298300 * 8 * 900 = 2.148e9 floats each (> 2^31)."""
    _conv(cuda, 8, 8, 30, 3, 1, 1, 8, 298300, DEPTHWISE, "dw_k3", "input")


def test_depthwise_chunk_7px_stride2_input_past_2_31(cuda):
    """depthwise3x3_chunk_kernel (small stride-2 planes): input 5478700 * 8 * 49 = 2.148e9 floats (> 2^31)."""
    _conv(cuda, 8, 8, 7, 3, 2, 1, 8, 5478700, DEPTHWISE, "dw_k3", "input")


def test_depthwise_lds_scalar_5x5_past_2_31(cuda):
    """depthwise_lds_scalar_kernel (5 x 5 filters on 16-pixel planes): input and output 1048700 * 8 * 256 = 2.148e9 floats each (> 2^31)."""
    _conv(cuda, 8, 8, 16, 5, 1, 2, 8, 1048700, DEPTHWISE, "dw_not_k3", "input")


def test_depthwise_generic_5x5_64px_past_2_31(cuda):
    """depthwise_generic_kernel (planes too large for the LDS form): input and output 131100 * 4 * 4096 = 2.148e9 floats each (> 2^31)."""
    _conv(cuda, 4, 4, 64, 5, 1, 2, 4, 131100, DEPTHWISE, "dw_generic", "input")


def test_conv_smallc_first_layer_output_past_2_31(cuda):
    """conv_smallc_kernel (contract_routes' "first 3x3": VGG-16's conv1_1, 3 -> 64 at 224 px): output 670 * 64 * 224 * 224 = 2.152e9 floats
    (> 2^31).  2^31 tiles are out of reach (the table above)."""
    _conv(cuda, 3, 64, 224, 3, 1, 1, 1, 670, IM2COL, "smallc", "output")


def _scratch_bytes(prm, batch):
    b, k, cp = ctypes.c_size_t(), ctypes.c_size_t(), prm._c()
    assert _main().fhip_conv_get_buffer_size(ctypes.byref(cp), IM2COL, batch, ctypes.byref(b), ctypes.byref(k)) == 0
    return b.value


def test_igemm_split_k_input_past_2_31(cuda):
    """Split-K with its reduce (igemm_split: 500 tiles of 64 x 128, 2560 k-tiles -> 3 pieces): a 1 x 1 layer 40960 -> 64 on 16 x 16 planes at
    batch 250.  The input, the GEMM's B operand, holds 250 * 40960 * 256 = 2.68e9 floats (> 2^31), and every piece reads it from a k offset of
    its own.  K = 64 keeps the layer off the streamed 1x1 route."""
    from feathercnn_amd import ConvParam
    c, k, batch = 40960, 64, 250
    prm = ConvParam.make(c, k, 16, 1, 1, 0, bias=True, act=1, batch=batch)
    assert _scratch_bytes(prm, batch) == 3 * k * batch * 256 * 4  # [pieces][K][columns] partial sums: three pieces
    _conv(cuda, c, k, 16, 1, 1, 0, 1, batch, IM2COL, "scratch", "input")


def test_igemm_tail_split_input_past_2_31(cuda):
    """The tail split with its reduce (igemm_tail, cut for 256 CUs): a 1 x 1 / stride-2 layer 5120 -> 128 on 16 x 16 planes at batch 1824 has 1824
    tiles of 128 x 64 = 7 rounds of 256 + 32, so the last 32 column tiles run in 8 pieces: scratch 8 * 128 * 2048 floats.  The input holds
    1824 * 5120 * 256 = 2.39e9 floats (> 2^31); the tail columns are the last images, the ones beyond that offset."""
    import torch

    from feathercnn_amd import ConvParam
    if torch.cuda.get_device_properties(0).multi_processor_count != 256:
        pytest.skip("the geometry is cut for 256 CUs (tests/test_tail_split_gpu.py): on another count the route would be a different one")
    c, k, batch = 5120, 128, 1824
    prm = ConvParam.make(c, k, 16, 1, 2, 0, bias=True, act=1, batch=batch)
    assert _scratch_bytes(prm, batch) == 8 * k * 32 * 64 * 4  # what igemm_buffer_bytes gives: [8 pieces][K][32 tail tiles of 64 columns]
    _conv(cuda, c, k, 16, 1, 2, 0, 1, batch, IM2COL, "scratch", "input")


def test_inner_product_stream_weights_past_2_30(cuda):
    """ip_pack_input / ip_stream / ip_reduce (a 1 x 1 convolution over a 1 x 1 image at batch 32): 40960 x 32768 weights = 1.34e9 floats, so the
    streamed weight image is read at offsets past 2^30 floats (byte offsets past 2^32).  Half of the sampled outputs belong to the rows beyond
    that offset."""
    import torch

    from feathercnn_amd import ConvLayer, ConvParam
    c, k, batch = 32768, 40960, 32
    assert c * k > P30
    prm = ConvParam.make(c, k, 1, 1, 1, 0, bias=True, act=1, batch=batch)
    wt = R.fill(torch.empty((k, c, 1, 1), device=cuda), 21, -1.0 / c ** 0.5, 1.0 / c ** 0.5)
    b = R.fill(torch.empty((k,), device=cuda), 22, -0.1, 0.1)
    lyr = ConvLayer(prm, wt, b, algo=IM2COL)
    layout, cp = ctypes.c_int(), prm._c()
    assert _main().fhip_conv_packed_layout(ctypes.byref(cp), IM2COL, ctypes.byref(layout)) == 0 and layout.value & 2  # the streamed weight image exists
    assert _confirm("scratch", prm, IM2COL, batch, lyr.buffer_bytes // 4)  # and the route keeps its pieces in the scratch
    x = R.fill(torch.empty((batch, c, 1, 1), device=cuda), 23)
    y = R.nans((batch, k, 1, 1), cuda)
    lyr.Forward(x, out=y)
    _sync()
    g = torch.Generator().manual_seed(3)
    first_beyond = P30 // c + 1
    rows = torch.cat([torch.tensor([0, 1, k - 2, k - 1]), torch.randint(0, k, (122,), generator=g), torch.randint(first_beyond, k, (130,), generator=g)]).to(cuda)
    assert int((rows >= first_beyond).sum()) * 2 >= rows.numel()
    want = (wt.view(k, c)[rows].double() @ x.view(batch, c).double().t() + b.double()[rows][:, None]).clamp_min(0)  # [rows][batch]
    got = y.view(batch, k)[:, rows].t().double()
    assert not bool(y.isnan().any())
    assert float((got - want).abs().max()) <= TOL * float(y.abs().max())


def _dw_pw(cuda, c, k, h, w, batch):
    """fhip_conv_forward_dw_pw: a 3 x 3 / pad-1 depthwise layer (+ bias, ReLU) inside the 1 x 1 layer that consumes it (+ bias, ReLU); the output
    holds more than 2^31 floats.  Against the fp64 composition at sampled positions."""
    import torch

    from feathercnn_amd import ConvLayer, ConvParam
    lib = _main()
    pd = ConvParam.make(c, c, h, 3, 1, 1, group=c, bias=True, act=1, w=w, batch=batch)
    pp = ConvParam.make(c, k, h, 1, 1, 0, bias=True, act=1, w=w, batch=batch)
    gen = torch.Generator(device=cuda).manual_seed(17)
    wd = (torch.rand((c, 1, 3, 3), device=cuda, generator=gen) * 2 - 1) / 3
    wp = (torch.rand((k, c, 1, 1), device=cuda, generator=gen) * 2 - 1) / c ** 0.5
    bd, bp = ((torch.rand((n,), device=cuda, generator=gen) * 2 - 1) * 0.1 for n in (c, k))
    ld, lp = ConvLayer(pd, wd, bd, algo=DEPTHWISE), ConvLayer(pp, wp, bp, algo=IM2COL)
    cd, cp = pd._c(), pp._c()
    assert lib.fhip_conv_can_fuse_dw_pw(ctypes.byref(cd), ctypes.byref(cp), batch) == 1
    shape = (batch, k, h, w)
    assert batch * k * h * w > P31
    x = R.fill(torch.empty((batch, c, h, w), device=cuda), 18)
    y = R.nans(shape, cuda)
    assert lib.fhip_conv_forward_dw_pw(ctypes.byref(cd), ctypes.byref(cp), batch, _p(y), _p(x), _p(ld.packed), _p(bd), _p(lp.packed), _p(bp), _stream()) == 0, \
        lib.fhip_last_error()
    _sync()
    pos, _ = R.positions(shape, P31, cuda)
    n_, k_, oy, ox = pos
    mid = torch.stack([R.conv_at(x, wd, bd, (n_, torch.full_like(k_, ch), oy, ox), 1, 1, 1, c)[0] for ch in range(c)], 1)  # [S][c], after ReLU
    want = ((mid * wp.double().view(k, c)[k_]).sum(1) + bp.double()[k_]).clamp_min(0)
    err = (y[pos].double() - want).abs()
    assert not bool(err.isnan().any()) and float(err.max()) <= TOL * float(y[:64].abs().max()), float(err.max())


def test_dw_pw_gemm_form_output_past_2_31(cuda):
    """ConvGemmPolicy<3> computes the GEMM's B operand from the depthwise input (contract_routes' "dw_pw s1": 16 -> 72 on 16 x 16): output
    116600 * 72 * 256 = 2.149e9 floats (> 2^31)."""
    _dw_pw(cuda, 16, 72, 16, 16, 116600)


def test_dw_pw_band_form_output_past_2_31(cuda):
    """dwpw_band_kernel (contract_routes' "dw_pw band": 32 -> 64 on rows of 112 pixels): output 8100 * 64 * 37 * 112 = 2.148e9 floats (> 2^31),
    input 1.07e9 (> 2^30)."""
    _dw_pw(cuda, 32, 64, 37, 112, 8100)


def test_siblings_one_gemm_output_and_input_past_2_31(cuda):
    """fhip_conv_forward_siblings (contract_routes' "siblings s2": 64 -> 128 and 64 -> 32, 1 x 1 / stride 2 on 28 pixels, ConvGemmPolicy<1, TWIN>):
    the first output holds 85700 * 128 * 196 = 2.15e9 floats (> 2^31), the input 85700 * 64 * 784 = 4.3e9 (> 2^32)."""
    import torch

    from feathercnn_amd import ConvParam
    from feathercnn_amd.booster import SiblingConvs
    lib, batch = _main(), 85700
    pa = ConvParam.make(64, 128, 28, 1, 2, 0, bias=True, act=0, batch=batch)
    pb = ConvParam.make(64, 32, 28, 1, 2, 0, bias=True, act=1, batch=batch)
    gen = torch.Generator(device=cuda).manual_seed(19)
    wa, wb = ((torch.rand((n, 64, 1, 1), device=cuda, generator=gen) * 2 - 1) / 8 for n in (128, 32))
    ba, bb = ((torch.rand((n,), device=cuda, generator=gen) * 2 - 1) * 0.1 for n in (128, 32))
    sib = SiblingConvs(pa, wa, ba, pb, wb, bb)
    assert sib.applicable(batch)
    x = R.fill(torch.empty((batch, 64, 28, 28), device=cuda), 20)
    ya, yb = R.nans((batch, 128, 14, 14), cuda), R.nans((batch, 32, 14, 14), cuda)
    assert ya.numel() > P31 and x.numel() > P32
    ca, cb = pa._c(), pb._c()
    assert lib.fhip_conv_forward_siblings(ctypes.byref(ca), ctypes.byref(cb), batch, _p(ya), _p(yb), _p(x), _p(sib.layer.packed), _p(sib.bias), _stream()) == 0, \
        lib.fhip_last_error()
    _sync()
    for y, wt, b, relu, per in ((ya, wa, ba, False, 128 * 196), (yb, wb, bb, True, 32 * 196)):
        first_beyond = P32 // (64 * 784) + 1  # the images whose input lies beyond 2^32 floats (and, for the first output, beyond 2^31 output floats)
        pos, _ = R.positions(tuple(y.shape), first_beyond * per, cuda)
        want = R.conv_at(x, wt, b, pos, 2, 0, relu=relu)[0]
        err = (y[pos].double() - want).abs()
        assert not bool(err.isnan().any()) and float(err.max()) <= TOL * float(y[:64].abs().max()), float(err.max())


def test_canvas_entry_and_output_M_past_2_31(cuda):
    """libfeather_canvas.so: a plain 4 -> 16 layer on 28 pixels, pooled into 2 x 2 image canvases of a 16 -> 16 layer on 14 pixels
    (fhip_canvas_output_to_next_input, ENTRY form, then fhip_canvas_output_transform).  The first layer's M, which the ENTRY kernel reads,
    holds 64 * 16 * 25 * 84000 = 2.15e9 floats (> 2^31); the canvas layer's V is a quarter of that (byte offsets past 2^31).  Against the
    fp64 composition of the two layers with the pooling between them."""
    import torch

    from feathercnn_amd import ConvLayer, ConvParam
    from feathercnn_amd.canvas import canvas_param, forward_chained_canvas, plan_canvas
    batch = 84000
    gen = torch.Generator(device=cuda).manual_seed(23)
    w0 = (torch.rand((16, 4, 3, 3), device=cuda, generator=gen) * 2 - 1) / 6
    w1 = (torch.rand((16, 16, 3, 3), device=cuda, generator=gen) * 2 - 1) / 12
    b0, b1 = ((torch.rand((16,), device=cuda, generator=gen) * 2 - 1) * 0.1 for _ in range(2))
    l0 = ConvLayer(ConvParam.make(4, 16, 28, 3, 1, 1, bias=True, act=1, batch=batch), w0, b0, algo=WINO)
    l1 = ConvLayer(ConvParam.make(16, 16, 14, 3, 1, 1, bias=True, act=1, batch=batch), w1, b1, algo=WINO)
    assert canvas_param(l1.param, batch) is not None and plan_canvas(l1.param, batch, True).columns == batch // 4 * 25  # the canvas plan
    assert plan_canvas(l0.param, batch, False).m_bytes // 4 > P31
    x = R.fill(torch.empty((batch, 4, 28, 28), device=cuda), 24)
    y = forward_chained_canvas([l0, l1], x, [True, False], [False, True], fill=float("nan"))
    _sync()
    assert tuple(y.shape) == (batch, 16, 14, 14)
    first_beyond = P31 // (64 * 16 * 25) + 1  # M's columns run with the image index
    assert first_beyond < batch
    pos, _ = R.positions(tuple(y.shape), first_beyond * 16 * 196, cuda)
    want = R.two_layers_at(x, w0, b0, w1, b1, pos, True)
    err = (y[pos].double() - want).abs()
    assert not bool(err.isnan().any()) and float(err.max()) <= TOL * float(y[:64].abs().max()), float(err.max())


@pytest.mark.parametrize("batch", [90, 91], ids=["V_below_2GiB_shared_columns", "V_above_2GiB_plain_stores"])
def test_first_layer_inside_conv1_2_on_both_sides_of_V_2GiB(cuda, batch):
    """VGG-16's conv1_1 (3 -> 64, 224 px) inside conv1_2's input transform (wino_first.h): at batch 90 V is 2 130 706 432 bytes and the
    shared-column form writes it with buffer stores; at batch 91 it is 2 164 260 864 bytes (> 2^31) and the plain-store form runs.  Against the
    fp64 composition of the two layers at sampled positions."""
    import torch

    from feathercnn_amd import ConvLayer, ConvParam
    from feathercnn_amd.booster import can_fuse_first_winograd, forward_chained, winograd_plan
    gen = torch.Generator(device=cuda).manual_seed(11)
    p0 = ConvParam.make(3, 64, 224, 3, 1, 1, bias=True, act=1, batch=batch)
    p1 = ConvParam.make(64, 64, 224, 3, 1, 1, bias=True, act=1, batch=batch)
    w0 = (torch.rand((64, 3, 3, 3), device=cuda, generator=gen) * 2 - 1) / 27 ** 0.5
    w1 = (torch.rand((64, 64, 3, 3), device=cuda, generator=gen) * 2 - 1) / 576 ** 0.5
    b0, b1 = ((torch.rand((64,), device=cuda, generator=gen) * 2 - 1) * 0.1 for _ in range(2))
    l1 = ConvLayer(p1, w1, b1, algo=WINO)
    assert can_fuse_first_winograd(p0, l1, batch)
    v_bytes = winograd_plan(p1).v_bytes
    assert (v_bytes <= P31) == (batch == 90) and (v_bytes > P31) == (batch == 91), v_bytes
    x = R.fill(torch.empty((batch, 3, 224, 224), device=cuda), 12)
    y = forward_chained([l1], x, first=(p0, w0, b0))
    _sync()
    # the last images are the ones whose V columns lie beyond 2 GiB (batch 91) or just below it (batch 90)
    pos, _ = R.positions(tuple(y.shape), (batch - 2) * 64 * 224 * 224, cuda)
    want = R.two_layers_at(x, w0, b0, w1, b1, pos, False)
    err = (y[pos].double() - want).abs()
    assert not bool(err.isnan().any()) and float(err.max()) <= TOL * float(y[:64].abs().max()), float(err.max())


@pytest.mark.parametrize("pool", [False, True], ids=["plain", "pooled"])
def test_chained_winograd_transforms_V_past_2_31(cuda, pool):
    """Two 16-channel Winograd layers on 56-pixel planes through fhip_conv_forward_chained (wino_chain_kernel writes the second layer's V from the
    first one's M, with a 2 x 2 max pooling between them in the pooled case): V and M of the first layer are 64 * 16 * 100 * 21000 = 2.15e9 floats
    each (> 2^31); without pooling so is the second layer's V.  Against the fp64 composition of the two layers."""
    import torch

    from feathercnn_amd import ConvLayer, ConvParam
    from feathercnn_amd.booster import can_chain_winograd, forward_chained, winograd_plan
    batch, side2 = 21000, 28 if pool else 56
    gen = torch.Generator(device=cuda).manual_seed(13)
    w0, w1 = ((torch.rand((16, 16, 3, 3), device=cuda, generator=gen) * 2 - 1) / 12.0 for _ in range(2))
    b0, b1 = ((torch.rand((16,), device=cuda, generator=gen) * 2 - 1) * 0.1 for _ in range(2))
    l0 = ConvLayer(ConvParam.make(16, 16, 56, 3, 1, 1, bias=True, act=1, batch=batch), w0, b0, algo=WINO)
    l1 = ConvLayer(ConvParam.make(16, 16, side2, 3, 1, 1, bias=True, act=1, batch=batch), w1, b1, algo=WINO)
    assert can_chain_winograd(l0, l1, pool)
    assert winograd_plan(l0.param).v_bytes // 4 > P31 and winograd_plan(l0.param).m_bytes // 4 > P31
    x = R.fill(torch.empty((batch, 16, 56, 56), device=cuda), 14)
    y = forward_chained([l0, l1], x, pools=[pool, False])
    _sync()
    assert tuple(y.shape) == (batch, 16, side2, side2)
    # V's columns run with the image index: the images beyond column 2^31 / (64 * 16) are the ones whose V and M offsets pass 2^31
    first_beyond = P31 // (64 * 16 * 100) + 1
    assert first_beyond < batch
    pos, _ = R.positions(tuple(y.shape), first_beyond * 16 * side2 * side2, cuda)
    want = R.two_layers_at(x, w0, b0, w1, b1, pos, pool)
    err = (y[pos].double() - want).abs()
    assert not bool(err.isnan().any()) and float(err.max()) <= TOL * float(y[:64].abs().max()), float(err.max())


# ---- layers of the main library ---------------------------------------------------------------------------------------------------------------

def _elementwise(cuda, count, aligned, op, inplace):
    """fhip_relu / fhip_add (+ ReLU) on `count` floats, 16-byte aligned or one float past that, against torch on whole slabs, bit for bit."""
    import torch
    lib, off = _main(), 0 if aligned else 1
    a = R.fill(torch.empty(count + off, device=cuda), 1)[off:]
    b = R.fill(torch.empty(count + off, device=cuda), 2)[off:] if op == "add" else None
    keep = [a[s].clone() for s in (slice(0, R.SLAB), slice(count - R.SLAB, count), slice(count % 7, count, count // R.SLAB))] if inplace else None
    y = a if inplace else R.nans(count + off, cuda)[off:]
    assert (y.data_ptr() % 16 == 0) == aligned and (a.data_ptr() % 16 == 0) == aligned
    rc = lib.fhip_relu(_p(y), _p(a), count, _stream()) if op == "relu" else lib.fhip_add(_p(y), _p(a), _p(b), count, 1, _stream())
    assert rc == 0, lib.fhip_last_error()
    _sync()
    slabs = iter(keep) if inplace else None

    def want(s):
        src = next(slabs) if inplace else a[s]
        return torch.relu(src) if op == "relu" else torch.relu(src + b[s])
    R.assert_equal_slabs(y, want, count)


def test_relu_aligned_2_32_plus_3(cuda):
    """2^32 + 3 floats, 16-byte aligned: float4 lanes past 2^30 and the three leftover floats past an unsigned index."""
    assert P32 + 3 > P32
    _elementwise(cuda, P32 + 3, True, "relu", False)


def test_relu_unaligned_2_31_plus_3_in_place(cuda):
    """2^31 + 3 floats, 4-byte aligned (a lane per float: 2^31 lanes), in place."""
    assert P31 + 3 > P31
    _elementwise(cuda, P31 + 3, False, "relu", True)


def test_add_aligned_2_32_plus_3_in_place(cuda):
    """y = relu(a + b) into a, 2^32 + 3 floats, 16-byte aligned."""
    _elementwise(cuda, P32 + 3, True, "add", True)


def test_add_unaligned_2_31_plus_3(cuda):
    """y = relu(a + b), 2^31 + 3 floats, 4-byte aligned."""
    _elementwise(cuda, P31 + 3, False, "add", False)


def _affine(cuda, batch, c, hw):
    import torch
    lib = _main()
    assert batch * c * hw > P31
    x = R.fill(torch.empty((batch, c, hw), device=cuda), 3)
    mul = torch.tensor([1.5, -0.75, 0.3, 2.0][:c], device=cuda)
    add = torch.tensor([0.1, 7.0, -3.0, 0.0][:c], device=cuda)
    y = R.nans((batch, c, hw), cuda)
    assert lib.fhip_affine(_p(y), _p(x), _p(mul), _p(add), batch, c, hw, 1, _stream()) == 0, lib.fhip_last_error()
    _sync()
    pos, _ = R.positions((batch, c, hw), P31, cuda)
    xs = x[pos].double() * mul.double()[pos[1]]
    _check_mag(y[pos], (xs + add.double()[pos[1]]).clamp_min(0), xs.abs() + add.double()[pos[1]].abs(), "affine")


def test_affine_float4_past_2_31(cuda):
    """8193 * 4 * 65536 = 2^31 + 262144 floats in float4 lanes (hw % 4 == 0)."""
    _affine(cuda, 8193, 4, 65536)


def test_affine_scalar_past_2_31(cuda):
    """8193 * 4 * 65535 floats (> 2^31), a float per lane (hw % 4 != 0)."""
    _affine(cuda, 8193, 4, 65535)


def _pooling(cuda, batch, c, h, w, k, s, pad, avg, glob):
    import torch

    from feathercnn_amd import _lib as L
    lib = _main()
    q = L.fhip_pool_param(c, h, w, k, k, s, s, pad, pad, pad, pad, avg, glob)
    oh, ow = ctypes.c_int(), ctypes.c_int()
    assert lib.fhip_pooling_output_dim(ctypes.byref(q), ctypes.byref(oh), ctypes.byref(ow)) == 0
    oh, ow = oh.value, ow.value
    assert batch * c * h * w > P31  # planes * H * W
    x = R.fill(torch.empty((batch, c, h, w), device=cuda), 4)
    y = R.nans((batch, c, oh, ow), cuda)
    assert lib.fhip_pooling(ctypes.byref(q), batch, _p(y), _p(x), _stream()) == 0, lib.fhip_last_error()
    _sync()
    first_beyond = P31 // (c * h * w) + 1  # images whose input lies beyond 2^31 elements
    assert first_beyond < batch
    if not avg:  # exact: whole images against torch, the first, the last and a strided sample beyond the threshold
        for imgs in R.units(batch, c * max(h * w, oh * ow), first_beyond):
            imgs = imgs.to(cuda)
            xi = x[imgs]
            want = xi.amax((2, 3), keepdim=True) if glob else torch.nn.functional.max_pool2d(xi, k, s, 0, ceil_mode=True)
            assert pad == 0 and torch.equal(y[imgs], want)
        return
    pos, _ = R.positions((batch, c, oh, ow), first_beyond * c * oh * ow, cuda)
    want, mag = R.pool_at(x, pos, h if glob else k, 1 if glob else s, 0 if glob else pad, True)
    _check_mag(y[pos], want, mag, "average pooling")


def test_pooling_generic_max_input_past_2_31(cuda):
    """pooling_kernel, 2 x 2 / stride 2 max on 126-pixel rows (no 16-byte rows): 45100 * 3 * 126 * 126 = 2.148e9 input floats."""
    _pooling(cuda, 45100, 3, 126, 126, 2, 2, 0, 0, 0)


def test_pooling_generic_average_past_2_31(cuda):
    """pooling_kernel, 3 x 3 / stride 1 average with padding (clipped windows): 43700 * 3 * 128 * 128 = 2.148e9 input floats, as many outputs."""
    _pooling(cuda, 43700, 3, 128, 128, 3, 1, 1, 1, 0)


def test_pooling_3x3_stride2_fast_input_past_2_31(cuda):
    """maxpool3s2_kernel: 43700 * 3 * 128 * 128 = 2.148e9 input floats."""
    _pooling(cuda, 43700, 3, 128, 128, 3, 2, 0, 0, 0)


def test_pooling_global_small_planes_input_past_2_31(cuda):
    """plane_reduce_small_kernel (7 x 7 planes through the LDS): 10956600 * 4 * 49 = 2.1475e9 input floats."""
    _pooling(cuda, 10956600, 4, 7, 7, 7, 1, 0, 1, 1)


def test_pooling_global_wave_per_plane_input_past_2_31(cuda):
    """plane_reduce_kernel (14 x 14 planes, a wave each), max: 2739200 * 4 * 196 = 2.1475e9 input floats."""
    _pooling(cuda, 2739200, 4, 14, 14, 14, 1, 0, 0, 1)


def test_softmax_rows_past_2_31(cuda):
    """2145400 rows of 1001 values: 2.1475e9 floats (> 2^31) in and out."""
    import torch
    lib, batch, cols = _main(), 2145400, 1001
    assert batch * cols > P31
    x = R.fill(torch.empty((batch, cols), device=cuda), 5, -4.0, 4.0)
    y = R.nans((batch, cols), cuda)
    assert lib.fhip_softmax(_p(y), _p(x), batch, cols, _stream()) == 0, lib.fhip_last_error()
    _sync()
    (rows, _), _ = R.positions((batch, cols), P31, cuda)
    xs = x[rows].double()
    e = torch.exp(xs - xs.amax(1, keepdim=True))
    want = e / e.sum(1, keepdim=True)
    _check_mag(y[rows], want, want, "softmax")  # an output's magnitude is itself: every term of the normalising sum is positive


def test_pixels_to_float_output_past_2_31(cuda):
    """2049 GRAY images of 1024 x 1024 pixels: 2^31 + 2^20 output floats; without mean / norm the conversion is exact."""
    import torch

    from feathercnn_amd import pixels as PX
    px = R.fill_bytes(torch.empty((2049, 1024, 1024, 1), dtype=torch.uint8, device=cuda), 6)
    y = R.nans((2049, 1, 1024, 1024), cuda)
    assert y.numel() > P31
    PX.pixels_to_float(px, PX.PIXEL_GRAY, out=y)
    _sync()
    flat = px.view(-1)
    R.assert_equal_slabs(y.view(-1), lambda s: flat[s].float(), y.numel())


def test_float_to_pixels_input_past_2_31(cuda):
    """2049 single-channel images of 1024 x 1024 whole numbers 0 .. 255: 2^31 + 2^20 input floats; every rounding mode gives the same bytes."""
    import torch

    from feathercnn_amd import pixels as PX
    x = R.fill_bytes(torch.empty((2049, 1, 1024, 1024), dtype=torch.float32, device=cuda), 7)
    assert x.numel() > P31
    out = torch.full((2049, 1024, 1024, 1), 7, dtype=torch.uint8, device=cuda)
    x.view(-1)[-1] = 200.0  # the last byte differs from the pre-fill whatever the draw
    PX.float_to_pixels(x, PX.PIXEL_GRAY, out=out)
    _sync()
    flat = x.view(-1)
    R.assert_equal_slabs(out.view(-1), lambda s: flat[s].to(torch.uint8), x.numel())


# ---- side libraries, just below 2^31 elements -------------------------------------------------------------------------------------------------

def _below_limit(shape):
    n = 1
    for d in shape:
        n *= d
    per = n // shape[0]
    assert P30 < n < P31 and n + per >= P31, (shape, n)  # one more image would reach the limit
    return n


def _gate_apply(cuda, shape, vec):
    import torch

    from feathercnn_amd import gate
    n, c, h, w = shape
    _below_limit(shape)
    x, res = R.fill(torch.empty(shape, device=cuda), 1), R.fill(torch.empty(shape, device=cuda), 2)
    g = R.fill(torch.empty((n, c, 1, 1), device=cuda), 3, 0.0, 1.0)
    y = R.nans(shape, cuda)
    assert gate.gate_route("apply", x, y, res) == f"fhip::gate_apply_kernel<{'true' if vec else 'false'}>"
    gate.channel_gate(x, g, residual=res, relu=True, out=y)
    _sync()
    pos, _ = R.positions(shape, P30, cuda)
    want = (x[pos].double() * g[pos[0], pos[1], 0, 0].double() + res[pos].double()).clamp_min(0)
    assert R.nerr(y[pos], want) <= TOL


def test_gate_apply_float4_with_residual_below_2_31(cuda):
    """32767 x 4 x 128 x 128 = 2^31 - 65536 floats: float4 units past 2^29, i * 4u past 2^30, byte offsets past 2^32."""
    _gate_apply(cuda, (32767, 4, 128, 128), True)


def test_gate_apply_scalar_with_residual_below_2_31(cuda):
    """33286 x 4 x 127 x 127 floats (odd planes: a float per unit, units past 2^30)."""
    _gate_apply(cuda, (33286, 4, 127, 127), False)


def _squeeze(cuda, shape, kernel, scratch):
    import torch

    from feathercnn_amd import gate
    _below_limit(shape)
    x = R.fill(torch.empty(shape, device=cuda), 4, 0.0, 1.0)
    assert gate.gate_route("squeeze", x) == f"fhip::squeeze_{kernel}_kernel<true>" and (gate.squeeze_scratch_bytes(shape) > 0) == scratch
    planes = shape[0] * shape[1]
    y = R.nans((shape[0], shape[1], 1, 1), cuda)
    gate.squeeze(x, out=y)
    _sync()
    first_beyond = P30 // (shape[2] * shape[3]) + 1
    sel = R.flat_positions(planes, shape[1], first_beyond).to(cuda)
    want = x.view(planes, -1)[sel].double().mean(1)
    assert not bool(y.isnan().any()) and R.nerr(y.view(-1)[sel], want) <= TOL


def test_gate_squeeze_group_below_2_31(cuda):
    """squeeze_group_kernel: 524287 planes of 64 x 64 (2^31 - 4096 floats)."""
    _squeeze(cuda, (524287, 1, 64, 64), "group", False)


def test_gate_squeeze_block_below_2_31(cuda):
    """squeeze_block_kernel, a block per plane: 131071 planes of 128 x 128."""
    _squeeze(cuda, (131071, 1, 128, 128), "block", False)


def test_gate_squeeze_split_below_2_31(cuda):
    """squeeze_block_kernel over chunks + squeeze_merge_kernel: 32767 planes of 256 x 256."""
    _squeeze(cuda, (32767, 1, 256, 256), "block", True)


def test_gate_activation_below_2_31(cuda):
    """Swish on 256999 x 2089 x 4 = 2^31 - 4 floats in float4 units."""
    import torch

    from feathercnn_amd import gate
    shape = (256999, 2089, 4)
    assert _below_limit(shape) == P31 - 4
    x = R.fill(torch.empty(shape, device=cuda), 5, -6.0, 6.0)
    y = R.nans(shape, cuda)
    assert gate.gate_route("activation", x, y) == "fhip::gate_activation_kernel<true>"
    gate.gate_activation(x, "swish", out=y)
    _sync()
    pos, _ = R.positions(shape, P30, cuda)
    xs = x[pos].double()
    assert R.nerr(y[pos], xs / (1 + torch.exp(-xs))) <= TOL


def _inorm(cuda, shape, kernel):
    import torch

    from feathercnn_amd import inorm
    n, c, h, w = shape
    _below_limit(shape)
    x = R.fill(torch.empty(shape, device=cuda), 6, -1.0, 3.0)
    gamma = torch.linspace(0.5, 1.5, c, device=cuda)
    beta = torch.linspace(-0.2, 0.3, c, device=cuda)
    y = R.nans(shape, cuda)
    assert inorm.instance_norm_route(x, y) == kernel
    inorm.instance_norm(x, gamma, beta, 1e-3, "leaky_relu", 0.2, out=y)
    _sync()
    # whole planes: the first two, the last two and 60 more, half of them beyond 2^30 elements
    planes, hw = n * c, h * w
    g = torch.Generator().manual_seed(3)
    beyond = P30 // hw + 1
    sel = torch.cat([torch.tensor([0, 1, planes - 2, planes - 1]), torch.randint(0, planes, (28,), generator=g),
                     torch.randint(beyond, planes, (32,), generator=g)]).to(cuda)
    assert int((sel >= beyond).sum()) * 2 >= sel.numel()
    want = R.instance_norm_planes(x, sel, gamma, beta, 1e-3, "leaky_relu", 0.2)
    got = y.view(planes, hw)[sel].double()
    assert not bool(got.isnan().any())
    per_plane = ((got - want).abs().amax(1) / want.abs().amax(1)).max()
    assert float(per_plane) <= TOL, float(per_plane)


def test_inorm_wave_route_below_2_31(cuda):
    """inorm_plane_kernel<256, 64>: 299593 x 7 planes of 32 x 32 (2^31 - 1024 floats): (size_t)plane * hw past 2^30."""
    _inorm(cuda, (299593, 7, 32, 32), "fhip::inorm_plane_kernel<256, 64, true>")


def test_inorm_block256_route_below_2_31(cuda):
    """inorm_plane_kernel<256, 256>: 524287 planes of 64 x 64."""
    _inorm(cuda, (524287, 1, 64, 64), "fhip::inorm_plane_kernel<256, 256, true>")


def test_inorm_block1024_route_below_2_31(cuda):
    """inorm_plane_kernel<1024, 1024>: 131071 planes of 128 x 128."""
    _inorm(cuda, (131071, 1, 128, 128), "fhip::inorm_plane_kernel<1024, 1024, true>")


def test_inorm_split_route_below_2_31(cuda):
    """inorm_partial_kernel + inorm_apply_kernel: 4681 x 7 planes of 256 x 256 in chunks of 4096 floats."""
    _inorm(cuda, (4681, 7, 256, 256), "fhip::inorm_partial_kernel<true>")


def test_inorm_prelu_per_channel_slopes_below_2_31(cuda):
    """activation_kernel<true> with a slope per channel: 299593 x 7 x 1024 floats; the channel comes from (i * 4u) / hw."""
    import torch

    from feathercnn_amd import inorm
    shape = (299593, 7, 1024)
    _below_limit(shape)
    x = R.fill(torch.empty(shape, device=cuda), 7)
    slopes = torch.linspace(0.05, 0.65, 7, device=cuda)
    y = R.nans(shape, cuda)
    inorm.activation(x, "prelu", slopes=slopes, out=y)
    _sync()
    pos, _ = R.positions(shape, P30, cuda)
    xs = x[pos].double()
    assert R.nerr(y[pos], torch.where(xs > 0, xs, xs * slopes.double()[pos[1]])) <= 1e-7  # one fp32 product


def _images_equal(got, want_of, batch, per_image, cuda):
    import torch
    for imgs in R.units(batch, per_image, P30 // per_image + 1):
        imgs = imgs.to(cuda)
        assert torch.equal(got[imgs], want_of(imgs))


def _shuffle(cuda, shape, vec):
    import torch

    from feathercnn_amd import shuffle
    n, c, h, w = shape
    _below_limit(shape)
    x = R.fill(torch.empty(shape, device=cuda), 8)
    y = R.nans(shape, cuda)
    assert shuffle.channel_route("shuffle", h, w, [y, x]) == f"fhip::channel_map_kernel<1, {'true' if vec else 'false'}>"
    shuffle.channel_shuffle(x, 2, out=y)
    _sync()
    _images_equal(y, lambda i: x[i].view(-1, 2, c // 2, h, w).transpose(1, 2).reshape(-1, c, h, w), n, c * h * w, cuda)


def test_channel_shuffle_16_byte_below_2_31(cuda):
    """ShuffleChannel, float4 accesses: 131071 x 4 x 64 x 64 = 2^31 - 16384 floats."""
    _shuffle(cuda, (131071, 4, 64, 64), True)


def test_channel_shuffle_4_byte_below_2_31(cuda):
    """ShuffleChannel on odd planes, a float per access: 135266 x 4 x 63 x 63 floats; base + 3 * stride passes 2^31."""
    _shuffle(cuda, (135266, 4, 63, 63), False)


def test_channel_slice_below_2_31(cuda):
    """Slice 4 channels into 1 + 3: 131071 x 4 x 64 x 64 input floats, one launch."""
    import torch

    from feathercnn_amd import shuffle
    shape = (131071, 4, 64, 64)
    _below_limit(shape)
    x = R.fill(torch.empty(shape, device=cuda), 9)
    outs = [R.nans((shape[0], k, 64, 64), cuda) for k in (1, 3)]
    assert shuffle.channel_route("slice", 64, 64, outs + [x]) == "fhip::channel_map_kernel<2, true>"
    shuffle.channel_slice(x, [1, -233], outs=outs)
    _sync()
    _images_equal(outs[0], lambda i: x[i][:, :1], shape[0], 4 * 4096, cuda)
    _images_equal(outs[1], lambda i: x[i][:, 1:], shape[0], 4 * 4096, cuda)


@pytest.mark.parametrize("side,route", [(64, "16b"), (63, "4b")])
def test_channel_map_table_two_in_two_out_below_2_31(cuda, side, route):
    """The fused Concat -> ShuffleChannel -> Slice form: two sources and two outputs of 2 channels, 4 rows in all, n * 4 * h * w just below
    2^31 units of the launch (each tensor holds half of them)."""
    import torch

    from feathercnn_amd import shuffle
    n = (P31 - 1) // (4 * side * side)
    assert P30 < n * 4 * side * side < P31
    srcs = [R.fill(torch.empty((n, 2, side, side), device=cuda), 10 + i) for i in range(2)]
    outs = [R.nans((n, 2, side, side), cuda) for _ in range(2)]
    tables = [[(0, 0), (1, 0)], [(0, 1), (1, 1)]]  # the shuffle of the concatenation, sliced in two
    assert shuffle.channel_route("map", side, side, outs + srcs) == f"fhip::channel_map_kernel<0, {'true' if route == '16b' else 'false'}>"
    shuffle.channel_map(srcs, tables, outs=outs, route=route)
    _sync()
    for j in range(2):
        for imgs in R.units(n, 2 * side * side, n // 2):
            imgs = imgs.to(cuda)
            assert torch.equal(outs[j][imgs], torch.stack([srcs[0][imgs][:, j], srcs[1][imgs][:, j]], 1))


def _side_conv(cuda, kind, prm, route_word, group, stride, pad, dil, crosses_output=True):
    """One layer of libfeather_deconv / gconv / atrous against the sampled fp64 definition."""
    import torch

    from feathercnn_amd import atrous, deconv, gconv
    batch, c, k = prm.batch, prm.input_channels, prm.output_channels
    gen = torch.Generator(device=cuda).manual_seed(5)
    cpg = c // group
    ks = prm.kernel_h
    wt = (torch.rand((k, cpg, ks, ks), device=cuda, generator=gen) * 2 - 1) / (cpg * ks * ks) ** 0.5
    b = (torch.rand((k,), device=cuda, generator=gen) * 2 - 1) * 0.1
    x = R.fill(torch.empty((batch, c, prm.input_h, prm.input_w), device=cuda), 6)
    shape = (batch, k, prm.output_h, prm.output_w)
    y = R.nans(shape, cuda)
    if kind == "deconv":
        lyr = deconv.DeconvLayer(prm, wt, b)
        route = deconv.Deconv().Route(prm)
    elif kind == "gconv":
        lyr = gconv.GroupedConvLayer(prm, wt, b)
        route = gconv.GroupedConv().Route(prm, y, x)
    else:
        lyr = atrous.AtrousLayer(prm, wt, b)
        route = atrous.AtrousConv().Route(prm)
    assert route_word in route, route
    lyr.Forward(x, out=y)
    _sync()
    pos, _ = R.positions(shape, P30, cuda)
    want = R.deconv_at(x, wt, b, pos, stride, pad, group) if kind == "deconv" else R.conv_at(x, wt, b, pos, stride, pad, dil, group)[0]
    err = (y[pos].double() - want).abs()
    assert not bool(err.isnan().any()) and float(err.max()) <= TOL * float(y[:64].abs().max()), float(err.max())


def test_deconv_mfma_route_output_below_2_31(cuda):
    """4 x 4 / stride 2 transposed convolution 16 -> 48 on 8-pixel planes, paired phases on the MFMA route: 174762 x 48 x 16 x 16 = 2^31 - 12288
    output floats."""
    from feathercnn_amd.deconv import DeconvParam
    prm = DeconvParam.make(16, 48, 8, batch=174762)
    _below_limit((174762, 48, 16, 16))
    _side_conv(cuda, "deconv", prm, "DeconvGemmPolicy<true>", 1, 2, 1, 1)


def test_deconv_generic_route_output_below_2_31(cuda):
    """4 -> 4 channels (no MFMA k-tile) on 16-pixel planes: 524287 x 4 x 32 x 32 = 2^31 - 4096 output floats."""
    from feathercnn_amd.deconv import DeconvParam
    prm = DeconvParam.make(4, 4, 16, batch=524287)
    _below_limit((524287, 4, 32, 32))
    _side_conv(cuda, "deconv", prm, "deconv_generic_kernel", 1, 2, 1, 1)


def test_gconv_tuned_route_past_2_31(cuda):
    """Grouped 3 x 3 (8 -> 8 in 2 groups) on 64-pixel planes: 65600 x 8 x 4096 = 2.1496e9 floats in and out (> 2^31: the library's limit is on
    lanes, not elements, and 2^31 lanes need an output of 2^33 floats)."""
    from feathercnn_amd import ConvParam
    prm = ConvParam.make(8, 8, 64, 3, 1, 1, group=2, batch=65600)
    assert 65600 * 8 * 4096 > P31
    _side_conv(cuda, "gconv", prm, "gconv3x3_kernel", 2, 1, 1, 1)


def test_gconv_generic_route_past_2_31(cuda):
    """Grouped 3 x 3 with 3 channels per group (no tuned form): 87400 x 6 x 4096 = 2.148e9 floats in and out (> 2^31)."""
    from feathercnn_amd import ConvParam
    prm = ConvParam.make(6, 6, 64, 3, 1, 1, group=2, batch=87400)
    assert 87400 * 6 * 4096 > P31
    _side_conv(cuda, "gconv", prm, "gconv_generic_kernel", 2, 1, 1, 1)


def test_atrous_mfma_route_output_below_2_31(cuda):
    """Dilation 2, 16 -> 48 channels on 32-pixel planes, MFMA route: 43690 x 48 x 1024 = 2^31 - 32768 output floats."""
    from feathercnn_amd.atrous import AtrousParam
    prm = AtrousParam.make(16, 48, 32, batch=43690)
    _below_limit((43690, 48, 32, 32))
    _side_conv(cuda, "atrous", prm, "AtrousGemmPolicy", 1, 1, 2, 2)


def test_atrous_depthwise_route_below_2_31(cuda):
    """Dilated depthwise 3 x 3 (8 channels, 64-pixel planes): 65535 x 8 x 4096 = 2^31 - 32768 floats in and out."""
    from feathercnn_amd.atrous import AtrousParam
    prm = AtrousParam.make(8, 8, 64, group=8, batch=65535)
    _below_limit((65535, 8, 64, 64))
    _side_conv(cuda, "atrous", prm, "atrous_dw3x3_kernel", 8, 1, 2, 2)


# ---- the Net runtime ----------------------------------------------------------------------------------------------------------------------------

def test_net_of_main_library_layers_with_a_blob_past_2_31(cuda):
    """model_zoo.tiny_plain (Convolution 3x3 / 1x1 / depthwise, Pooling, ReLU, Split, Eltwise, Concat, InnerProduct, Softmax) fed 1048600 images of
    8 x 8 on the device: conv1's blob holds 1048600 * 32 * 64 = 2.1475e9 floats (> 2^31), the blobs behind the pooling a quarter of that each.
    The outputs of the first two and the last two images equal a batch-4 run of those four images on a fresh net, and the CPU restatement
    (oracle.netcheck.PortNet) within the 1e-4 of the net tests."""
    import numpy as np
    import torch

    from feathercnn_amd import model_zoo
    from feathercnn_amd.net import Net
    from oracle import netcheck, nerr
    p, b, i, o = model_zoo.tiny_plain()
    batch = 1048600
    assert batch * 32 * 8 * 8 > P31
    x = R.fill(torch.empty((batch, 3, 8, 8), device=cuda), 25)
    four = torch.cat([x[:2], x[-2:]]).cpu().numpy()
    net = Net(fusion=2)
    net.LoadParam(p)
    net.LoadWeights(b)
    net.FeedInput(i, x)
    del x
    net.Forward()
    got = net.Extract(o).reshape(batch, -1)
    assert np.isfinite(got).all() and np.abs(got.sum(1) - 1).max() <= 1e-5  # every image of the batch came out as a distribution
    ends = np.concatenate([got[:2], got[-2:]])
    net.close()
    small = Net(fusion=2)
    small.LoadParam(p)
    small.LoadWeights(b)
    small.FeedInput(i, four)
    small.Forward()
    same = small.Extract(o).reshape(4, -1)
    assert nerr(ends, same) <= TOL, nerr(ends, same)  # (a route may depend on the batch -- split-K at batch 4 -- so not bit for bit)
    assert nerr(ends, netcheck.PortNet(p, b).run(i, four, o).reshape(4, -1)) <= TOL


def test_net_returns_the_side_library_refusal_with_the_layer_name_and_runs_again_at_a_small_batch(cuda):
    """model_zoo.tiny_generative (InstanceNorm, libfeather_inorm.so) fed 233100 images of 24 x 24 on the device: the blob in front of its first
    InstanceNorm holds 233100 * 16 * 576 = 2.148e9 floats (> 2^31), which that library refuses.  Forward returns the refusal at planning, before
    any layer runs, with the layer's name in the text; the same net object then runs two images correctly."""
    import numpy as np
    import torch

    import inorm_ref
    from feathercnn_amd import FeatherHipError, model_zoo
    from feathercnn_amd.net import Net
    p, b, i, o = model_zoo.tiny_generative()
    net = Net(fusion=2)
    net.LoadParam(p)
    net.LoadWeights(b)
    norms = [name for type_, name, _ in net.layers() if type_ == "InstanceNorm"]
    batch = 233100
    assert batch * 16 * 24 * 24 > P31 and norms
    big = R.fill(torch.empty((batch, 3, 24, 24), device=cuda), 15)
    net.FeedInput(i, big)
    del big
    with pytest.raises(FeatherHipError) as e:
        net.Forward()
    text = str(e.value)
    assert "2^31 elements" in text and any(f"layer {n}:" in text for n in norms), text
    x = np.random.default_rng(8).uniform(-1, 1, (2, 3, 24, 24)).astype(np.float32)
    net.FeedInput(i, x)
    net.Forward()
    assert inorm_ref.nerr(net.Extract(o), inorm_ref.Net(p, b).run(i, x, o)) <= TOL
