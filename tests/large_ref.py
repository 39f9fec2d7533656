"""References for tensors of more than 2^30 / 2^31 / 2^32 elements (tests/test_large_routes_gpu.py): everything is computed on the device, in
float64, from the same inputs, with torch indexing -- independent code whose indices are 64-bit.

  * exact-class operations (ReLU, add, max pooling, channel moves, pixel conversion without mean / norm) are compared bit for bit with torch on
    whole slabs: the first and the last 16 M elements (or the images / planes that hold them) and a strided sample between them;
  * everything else at S = 4000 sampled output positions: a quarter anywhere, a quarter in the first image (a wrapped index lands there), half
    at element offsets at or above the threshold the case names.

Inputs are generated on the device in pieces (torch.rand materialises temporaries); outputs start as NaN, so an unwritten element is seen.
Nothing here drops a position: where a reference needs a whole plane or row, the sampled position selects that plane or row."""
from __future__ import annotations

S = 4000
SLAB = 1 << 24


def fill(t, seed, lo=-1.0, hi=1.0, piece=1 << 28):
    """uniform(lo, hi) into the contiguous tensor t, in pieces."""
    import torch
    gen = torch.Generator(device=t.device).manual_seed(seed)
    flat = t.view(-1)
    for i in range(0, flat.numel(), piece):
        flat[i:i + piece].uniform_(lo, hi, generator=gen)
    return t


def fill_bytes(t, seed, piece=1 << 26, dtype_max=256):
    """integers 0 .. 255 into t (uint8, or float32 holding whole numbers), in pieces."""
    import torch
    gen = torch.Generator(device=t.device).manual_seed(seed)
    flat = t.view(-1)
    for i in range(0, flat.numel(), piece):
        n = min(piece, flat.numel() - i)
        flat[i:i + n] = torch.randint(0, dtype_max, (n,), device=t.device, generator=gen, dtype=torch.int32).to(t.dtype)
    return t


def nans(shape, device):
    import torch
    return torch.full(shape if isinstance(shape, (tuple, list)) else (shape,), float("nan"), dtype=torch.float32, device=device)


def flat_positions(numel, first, threshold, seed=9):
    """S flat offsets into a tensor of `numel` elements whose first image holds `first`: S/4 anywhere, S/4 in the first image, S/2 at or above
    `threshold`.  The condition the cases rely on is asserted here."""
    import torch
    assert 0 < threshold < numel, (threshold, numel)
    g = torch.Generator().manual_seed(seed)
    q = S // 4
    flat = torch.cat([torch.randint(0, numel, (q,), generator=g), torch.randint(0, min(first, numel), (q,), generator=g),
                      torch.randint(threshold, numel, (S - 2 * q - 1,), generator=g), torch.tensor([numel - 1])])
    assert int((flat >= threshold).sum()) * 2 >= S
    return flat


def unravel(flat, shape):
    idx = []
    for d in reversed(shape):
        idx.append(flat % d)
        flat = flat // d
    return tuple(reversed(idx))


def positions(shape, threshold, device, seed=9):
    """Index tensors (one per dimension, on `device`) of S sampled positions of a tensor of `shape` ([N][...]): see flat_positions."""
    numel = 1
    for d in shape:
        numel *= d
    flat = flat_positions(numel, numel // shape[0], threshold, seed)
    return tuple(i.to(device) for i in unravel(flat, shape)), flat.to(device)


def units(count, per_unit, threshold_unit=0):
    """Indices of whole units (images, planes, rows) for slab comparisons: the first and the last units that hold SLAB elements, and a strided
    sample of as many between them (all of them beyond `threshold_unit` where that leaves enough)."""
    import torch
    k = max(1, min(count, SLAB // max(per_unit, 1)))
    stride = max(1, (count - max(threshold_unit, 0)) // k)
    return [torch.arange(0, k), torch.arange(count - k, count), torch.arange(max(threshold_unit, 0), count, stride)[:k]]


def assert_equal_slabs(got_flat, want_of, numel):
    """got_flat[s] == want_of(s) bit for bit on the first SLAB, the last SLAB and a strided sample of SLAB elements across the whole tensor."""
    import torch
    for s in (slice(0, min(SLAB, numel)), slice(max(numel - SLAB, 0), numel)):
        assert torch.equal(got_flat[s], want_of(s)), f"elements {s.start} .. {s.stop} differ"
    s = slice(numel % 7, numel, max(1, numel // SLAB))
    assert torch.equal(got_flat[s], want_of(s)), "the strided sample differs"


def conv_at(x, w, b, pos, stride=1, pad=0, dil=1, group=1, relu=True):
    """fp64 direct convolution at the sampled output positions pos = (n, k, oy, ox): x [N][C][H][W], w [K][C / group][kh][kw], b [K] or None."""
    import torch
    n_, k_, oy, ox = pos
    h, wd = x.shape[2], x.shape[3]
    kk, cpg, kh, kw = w.shape
    kpg = kk // group
    cc = torch.arange(cpg, device=x.device)
    c_idx = (k_ // kpg * cpg)[:, None] + cc[None, :]
    wd64 = w.double()
    acc = b.double()[k_].clone() if b is not None else torch.zeros(k_.shape, dtype=torch.float64, device=x.device)
    mag = acc.abs()
    for u in range(kh):
        for v in range(kw):
            yy, xx = oy * stride - pad + u * dil, ox * stride - pad + v * dil
            ok = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < wd)
            taps = x[n_[:, None], c_idx, yy.clamp(0, h - 1)[:, None], xx.clamp(0, wd - 1)[:, None]].double()  # [S][cpg]
            prod = taps * wd64[k_, :, u, v]
            acc += torch.where(ok, prod.sum(1), torch.zeros_like(acc))
            mag += torch.where(ok, prod.abs().sum(1), torch.zeros_like(acc))
    return (acc.clamp_min(0) if relu else acc), mag


def two_layers_at(x, w0, b0, w1, b1, pos, pool):
    """fp64 relu(conv3x3(pool?(relu(conv3x3(x))))) (pad 1 each) at pos: the first layer is evaluated at the taps the second one reads."""
    import torch
    n_, k_, oy, ox = pos
    mid_c = w0.shape[0]
    hh, ww = (x.shape[2] // 2, x.shape[3] // 2) if pool else (x.shape[2], x.shape[3])
    want = b1.double()[k_].clone()
    w164 = w1.double()
    for u in range(3):
        for v in range(3):
            yy, xx = oy - 1 + u, ox - 1 + v
            ok = (yy >= 0) & (yy < hh) & (xx >= 0) & (xx < ww)
            yc, xc = yy.clamp(0, hh - 1), xx.clamp(0, ww - 1)
            cols = []
            for c in range(mid_c):
                kc = torch.full_like(k_, c)
                if pool:
                    cols.append(torch.stack([conv_at(x, w0, b0, (n_, kc, 2 * yc + dy, 2 * xc + dx), 1, 1)[0] for dy in (0, 1) for dx in (0, 1)]).amax(0))
                else:
                    cols.append(conv_at(x, w0, b0, (n_, kc, yc, xc), 1, 1)[0])
            mid = torch.stack(cols, 1)
            want += torch.where(ok, (mid * w164[k_, :, u, v]).sum(1), torch.zeros_like(want))
    return want.clamp_min(0)


def deconv_at(x, w, b, pos, stride, pad, group=1, relu=True):
    """fp64 transposed convolution at pos = (n, k, oy, ox): x [N][C][H][W], w [K][C / group][kh][kw] (include/feather_hip/feather_deconv.h), b [K]
    or None; y[oy] collects x[iy] * w[u] where oy = iy * stride - pad + u."""
    import torch
    n_, k_, oy, ox = pos
    h, wd = x.shape[2], x.shape[3]
    kk, cpg, kh, kw = w.shape
    kpg = kk // group
    cc = torch.arange(cpg, device=x.device)
    c_idx = (k_ // kpg * cpg)[:, None] + cc[None, :]
    w64 = w.double()
    acc = b.double()[k_].clone() if b is not None else torch.zeros(k_.shape, dtype=torch.float64, device=x.device)
    for u in range(kh):
        for v in range(kw):
            ty, tx = oy + pad - u, ox + pad - v
            iy, ix = torch.div(ty, stride, rounding_mode="floor"), torch.div(tx, stride, rounding_mode="floor")
            ok = (ty % stride == 0) & (tx % stride == 0) & (iy >= 0) & (iy < h) & (ix >= 0) & (ix < wd)
            taps = x[n_[:, None], c_idx, iy.clamp(0, h - 1)[:, None], ix.clamp(0, wd - 1)[:, None]].double()
            acc += torch.where(ok, (taps * w64[k_, :, u, v]).sum(1), torch.zeros_like(acc))
    return acc.clamp_min(0) if relu else acc


def pool_at(x, pos, k, s, pad, avg):
    """fp64 PoolingLayer::Forward at pos = (n, c, oy, ox): the window starts at o * s - 2 * pad (both pads, as the reference), is clipped to the
    image, and the average divides by the taps inside.  -> (value, mean |tap|)."""
    import torch
    n_, c_, oy, ox = pos
    h, wd = x.shape[2], x.shape[3]
    val = torch.zeros(n_.shape, dtype=torch.float64, device=x.device) if avg else torch.full(n_.shape, -float("inf"), dtype=torch.float64, device=x.device)
    mag, cnt = torch.zeros_like(val), torch.zeros_like(val)
    for u in range(k):
        for v in range(k):
            yy, xx = oy * s - 2 * pad + u, ox * s - 2 * pad + v
            ok = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < wd)
            t = x[n_, c_, yy.clamp(0, h - 1), xx.clamp(0, wd - 1)].double()
            if avg:
                val += torch.where(ok, t, torch.zeros_like(t))
                mag += torch.where(ok, t.abs(), torch.zeros_like(t))
                cnt += ok.double()
            else:
                val = torch.where(ok, torch.maximum(val, t), val)
    return (val / cnt, mag / cnt) if avg else (val, val.abs())


def instance_norm_planes(x, planes, gamma, beta, eps, act=None, slope=0.0):
    """fp64 InstanceNorm (+ activation) of the planes (n * C + c indices) of x [N][C][H][W] -> [len(planes)][H * W]."""
    import torch
    c = x.shape[1]
    v = x.view(x.shape[0] * c, -1)[planes].double()
    y = (v - v.mean(1, keepdim=True)) / torch.sqrt(v.var(1, unbiased=False, keepdim=True) + eps)
    ch = planes % c
    if gamma is not None:
        y = y * gamma.double()[ch][:, None]
    if beta is not None:
        y = y + beta.double()[ch][:, None]
    if act == "relu":
        y = y.clamp_min(0)
    elif act == "leaky_relu":
        y = torch.where(y > 0, y, y * slope)
    return y


def nerr(got, want):
    """max |got - want| / max |want|, NaN-proof: a NaN in got is an infinite error."""
    d = (got.double() - want).abs()
    if bool(d.isnan().any()):
        return float("inf")
    return float(d.max()) / max(float(want.abs().max()), 1e-30)
