"""tests/large_ref.py alone, on the CPU at small batches of the geometries tests/test_large_routes_gpu.py runs: the sampled fp64 references equal
torch's float64 operators to 1e-12 (far inside the bounds the GPU cases assert), and the samplers keep their promises -- half of the positions at
or beyond the threshold, a quarter in the first image, the last element always among them."""
import pytest
import torch

import large_ref as R

F = torch.nn.functional


def _all_positions(shape):
    n = 1
    for d in shape:
        n *= d
    return R.unravel(torch.arange(n), shape)


@pytest.mark.parametrize("c,k,h,w,ks,s,p,d,g", [(16, 16, 20, 20, 3, 1, 1, 1, 1), (64, 128, 28, 28, 1, 2, 0, 1, 1), (48, 40, 7, 7, 1, 1, 0, 1, 1),
                                                (8, 8, 7, 7, 3, 2, 1, 1, 8), (4, 4, 16, 16, 5, 1, 2, 1, 4), (8, 8, 12, 12, 3, 1, 1, 1, 2),
                                                (6, 6, 12, 12, 3, 1, 1, 1, 2), (16, 48, 12, 12, 3, 1, 2, 2, 1), (8, 8, 12, 12, 3, 1, 2, 2, 8),
                                                (16, 16, 4, 30, 3, 1, 1, 1, 1)])
def test_conv_at_equals_torch_conv2d_in_fp64(c, k, h, w, ks, s, p, d, g):
    gen = torch.Generator().manual_seed(1)
    x = torch.rand((3, c, h, w), generator=gen) * 2 - 1
    wt = torch.rand((k, c // g, ks, ks), generator=gen) * 2 - 1
    b = torch.rand((k,), generator=gen) - 0.5
    want = F.conv2d(x.double(), wt.double(), b.double(), stride=s, padding=p, dilation=d, groups=g).relu()
    got, mag = R.conv_at(x, wt, b, _all_positions(tuple(want.shape)), s, p, d, g)
    assert float((got - want.reshape(-1)).abs().max()) <= 1e-12 and bool((mag + 1e-12 >= got.abs()).all())


@pytest.mark.parametrize("c,k,h,g", [(16, 48, 8, 1), (4, 4, 16, 1), (4, 6, 5, 2)])
def test_deconv_at_equals_torch_conv_transpose2d_in_fp64(c, k, h, g):
    gen = torch.Generator().manual_seed(2)
    x = torch.rand((2, c, h, h), generator=gen) * 2 - 1
    wt = torch.rand((k, c // g, 4, 4), generator=gen) * 2 - 1  # [K][C / group][kh][kw]
    b = torch.rand((k,), generator=gen) - 0.5
    kg = k // g
    wt_torch = torch.cat([wt[j * kg:(j + 1) * kg].transpose(0, 1) for j in range(g)], 0)  # per group [C / group][K / group]
    want = F.conv_transpose2d(x.double(), wt_torch.double(), b.double(), stride=2, padding=1, groups=g).relu()
    got = R.deconv_at(x, wt, b, _all_positions(tuple(want.shape)), 2, 1, g)
    assert float((got - want.reshape(-1)).abs().max()) <= 1e-12


@pytest.mark.parametrize("pool", [False, True])
def test_two_layers_at_equals_the_torch_composition_in_fp64(pool):
    g = torch.Generator().manual_seed(5)
    x = torch.rand((2, 4, 12, 12), generator=g) * 2 - 1
    w0, w1 = ((torch.rand((4, 4, 3, 3), generator=g) * 2 - 1) / 6 for _ in range(2))
    b0, b1 = (torch.rand((4,), generator=g) - 0.5 for _ in range(2))
    mid = F.conv2d(x.double(), w0.double(), b0.double(), padding=1).relu()
    want = F.conv2d(F.max_pool2d(mid, 2, 2) if pool else mid, w1.double(), b1.double(), padding=1).relu()
    got = R.two_layers_at(x, w0, b0, w1, b1, _all_positions(tuple(want.shape)), pool)
    assert float((got - want.reshape(-1)).abs().max()) <= 1e-12


def test_pool_at_equals_torch_pooling_in_fp64():
    x = torch.rand((2, 3, 12, 12), generator=torch.Generator().manual_seed(3)) * 2 - 1
    # 3 x 3 / stride 1 with padding 1: the reference starts its windows at o - 2 (both pads) and divides by the taps inside the image
    pos = _all_positions((2, 3, 12, 12))
    got, mag = R.pool_at(x, pos, 3, 1, 1, True)
    xp = F.pad(x.double(), (2, 0, 2, 0), value=float("nan"))
    win = xp.unfold(2, 3, 1).unfold(3, 3, 1).reshape(2, 3, 12, 12, 9)
    want = win.nanmean(-1)
    assert float((got - want.reshape(-1)).abs().max()) <= 1e-12 and bool((mag + 1e-12 >= got.abs()).all())
    got, _ = R.pool_at(x, _all_positions((2, 3, 6, 6)), 2, 2, 0, False)
    assert torch.equal(got, F.max_pool2d(x.double(), 2, 2).reshape(-1))
    got, _ = R.pool_at(x, _all_positions((2, 3, 1, 1)), 12, 1, 0, True)
    assert float((got - x.double().mean((2, 3)).reshape(-1)).abs().max()) <= 1e-12


def test_instance_norm_planes_equals_torch_in_fp64():
    x = torch.rand((3, 7, 8, 8), generator=torch.Generator().manual_seed(4)) * 4 - 1
    gamma, beta = torch.linspace(0.5, 1.5, 7), torch.linspace(-0.2, 0.3, 7)
    want = F.leaky_relu(F.instance_norm(x.double(), weight=gamma.double(), bias=beta.double(), eps=1e-3), 0.2)
    got = R.instance_norm_planes(x, torch.arange(21), gamma, beta, 1e-3, "leaky_relu", 0.2)
    assert float((got - want.reshape(21, 64)).abs().max()) <= 1e-12


def test_the_samplers_keep_their_promises():
    shape = (40, 3, 5, 7)
    numel, first = 40 * 105, 105
    flat = R.flat_positions(numel, first, 3000)
    assert flat.numel() == R.S and int((flat >= 3000).sum()) * 2 >= R.S and int((flat < first).sum()) >= R.S // 4 and int(flat.max()) == numel - 1
    idx = R.unravel(flat, shape)
    assert torch.equal(((idx[0] * 3 + idx[1]) * 5 + idx[2]) * 7 + idx[3], flat)
    pos, f2 = R.positions(shape, 3000, torch.device("cpu"))
    assert torch.equal(f2, flat) and all(int(i.max()) < d for i, d in zip(pos, shape))
    first_u, last_u, mid_u = R.units(1000, 2 ** 20, 600)
    assert first_u.tolist() == list(range(16)) and last_u.tolist() == list(range(984, 1000)) and int(mid_u.min()) >= 600 and mid_u.numel() == 16
    a = torch.arange(5000.0)
    R.assert_equal_slabs(a, lambda s: a[s].clone(), 5000)
    with pytest.raises(AssertionError):
        R.assert_equal_slabs(a, lambda s: torch.where(a[s] == 4999, torch.zeros(()), a[s]), 5000)  # the last element alone is wrong
    assert R.nerr(torch.tensor([1.0, float("nan")]), torch.tensor([1.0, 2.0], dtype=torch.float64)) == float("inf")
