"""The instantiation sweep (tests/instance_cases.py): build a case with scaled inputs, run it, compare it with an fp64 reference.

Inputs are synth() data with a power-of-two scale per image, 2^-6 ... 2^6 (13 distinct scales; larger batches cycle through them): the
scaling adds no rounding, and a kernel that is wrong on a low-magnitude image can no longer hide behind a large one.  Biases are non-zero and
differ per channel.  In ReLU cases one output channel of every activated layer gets a bias below -(sum|w| * max|x|) - 1: its whole plane must
come back exactly 0.

Comparisons:
  * convolutions and fused forms: an fp64 composition (port.direct_f64 + numpy fp64 for ReLU, residual add, pooling and the second layer),
    per output plane: max|err| over the plane / the plane's max|ref| <= 1e-4.  Behind a ReLU the plane's scale is that of its pre-activation
    values (a plane whose positive part is a sliver near 0 would otherwise measure fp32 rounding against the sliver); a plane the ReLU clips
    entirely must be exactly 0;
  * ReLU, add, max pooling: bit-equal to numpy fp32;  pixels: bit-equal to tests/pixels_ref.py;
  * average / global pooling, softmax, affine: fp64 numpy, |err| <= 1e-6 x the output's magnitude (the fp64 sum of the |terms| entering it).

Run as a script (`python tests/instance_sweep.py [--check]`) it runs every case once, in table order; between cases it synchronises the device
and launches one separator, fhip_relu on 1024 * (i + 1) floats (a grid of i + 1 blocks), so that a kernel trace can be cut into one window per
case.  The relu case itself runs 2^20 + 3 floats: a grid no separator has.
"""
from __future__ import annotations

import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import oracle  # noqa: E402
import test_contract_gpu as TC  # noqa: E402
from instance_cases import CASES, DEPTHWISE, IM2COL, NAIVE, WINO  # noqa: E402
from oracle import Geom, synth  # noqa: E402

TOL = 1e-4
MAG_TOL = 1e-6
SCALE_EXP = list(range(-6, 7))
MAX_CHECKED = 6  # images compared in big batches: the first three and the last three


def image_scales(batch):
    """One power of two per image: evenly over 2^-6 .. 2^6 for up to 13 images, cycling beyond."""
    if batch <= len(SCALE_EXP):
        idx = np.round(np.linspace(0, len(SCALE_EXP) - 1, batch)).astype(int) if batch > 1 else np.array([0])
        return np.array([2.0 ** SCALE_EXP[i] for i in idx], np.float32)
    return np.array([2.0 ** SCALE_EXP[(7 * i) % len(SCALE_EXP)] for i in range(batch)], np.float32)


def scaled(x):
    s = image_scales(x.shape[0])
    return (x * s.reshape(-1, *([1] * (x.ndim - 1)))).astype(np.float32)


def checked_images(batch):
    return list(range(batch)) if batch <= MAX_CHECKED else [0, 1, 2, batch - 3, batch - 2, batch - 1]


def distinct_bias(k, seed):
    """Non-zero, different per channel, both signs."""
    rng = np.random.default_rng(seed)
    mag = 0.02 + 0.18 * (np.arange(k) + 1) / (k + 1)
    return (rng.permutation(mag) * np.where(np.arange(k) % 2, 1.0, -1.0)).astype(np.float32)


def clip_channel(k):
    return k // 2


def kill_bias(b, w, xmax, k):
    """Give channel k a bias that keeps its whole pre-activation plane below -1."""
    b = b.copy()
    b[k] = -(float(np.abs(w[k].astype(np.float64)).sum()) * xmax) - 1.0
    return b


def conv64(g, x, w, b):
    """fp64-accumulated convolution without activation (bias None = zeros)."""
    return oracle.port().direct_f64(g, np.ascontiguousarray(x, np.float32), w, np.zeros(g.oc, np.float32) if b is None else b).astype(np.float64)


def pool2(a):
    n, c, h, w = a.shape
    return a[:, :, :h // 2 * 2, :w // 2 * 2].reshape(n, c, h // 2, 2, w // 2, 2).max(axis=(3, 5))


def pool2_scale(pre):
    """the per-plane scale of a pooled output: its producer plane's max |pre-activation|."""
    return np.abs(pre).max(axis=(2, 3))


class Plane:
    """A per-plane comparison: ref (fp64, [n][k][h][w] over the checked images), scale [n][k] (the plane's max|ref| or its pre-activation's)."""

    def __init__(self, ref, scale, images):
        self.ref, self.scale, self.images = ref, scale, images


class Exact:
    def __init__(self, ref32):
        self.ref = ref32


class Mag:
    def __init__(self, ref, mag):
        self.ref, self.mag = ref, mag


def plane_ref(pre, relu, images):
    y = np.maximum(pre, 0) if relu else pre
    return Plane(y, np.abs(pre).max(axis=(2, 3)), images)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# builders: args -> (contract Case with call / buffers, {output: comparison})

def _weights(g, batch, seed):
    x, w, _ = synth(g, batch, seed=seed)
    return scaled(x), w


def _conv(a):
    lib = TC._lib()
    c, k, h, wd, ks, s, p, group, batch, algo = (a[n] for n in ("c", "k", "h", "w", "ks", "s", "p", "group", "batch", "algo"))
    relu = bool(a["relu"]) and algo != NAIVE
    prm = TC._param(c, k, h, wd, ks, s, p, group, batch, a["bias"], 1 if a["relu"] else 0)
    g = Geom(c, k, h, wd, ks, ks, s, s, p, p, p, p, group, 1, 0)
    x, w = _weights(g, batch, c + k + h)
    b = distinct_bias(k, k + h) if a["bias"] else None
    if relu and b is not None:
        b = kill_bias(b, w, float(np.abs(x).max()), clip_channel(k))
    nbuf, npk = TC._sizes(prm, algo, batch)
    nout = batch * prm.output_channels * prm.output_h * prm.output_w
    im = checked_images(batch)

    def call(P, st):
        cc = prm._c()
        return lib.fhip_conv_forward(ctypes.byref(cc), algo, batch, P["y"], P["x"], P["packed"], P["scratch"], P["b"], st)

    def ref():
        return {"y": plane_ref(conv64(g, x[im], w, b), relu, im)}

    bb = b if b is not None else np.full(k, np.nan, np.float32)
    return TC.Case(inputs={"x": x, "w": w, "b": bb}, outputs={"y": nout}, scratch={"scratch": nbuf},
                   packed={"packed": (npk, TC._init(prm, algo, "w", "packed"))}, call=call, bias_keys=("b",), batch=batch), ref, b is None


def _residual(a):
    lib = TC._lib()
    c, k, h, wd, batch = a["c"], a["k"], a["h"], a["w"], a["batch"]
    prm = TC._param(c, k, h, wd, 1, 1, 0, 1, batch, True, 1)
    g = Geom(c, k, h, wd, 1, 1, 1, 1, 0, 0, 0, 0, 1, 1, 0)
    x, w = _weights(g, batch, k)
    r = scaled(np.random.default_rng(7).uniform(-1, 1, (batch, k, h, wd)).astype(np.float32))
    b = distinct_bias(k, 3)
    b[clip_channel(k)] = -(float(np.abs(w[clip_channel(k)]).sum()) * float(np.abs(x).max())) - float(np.abs(r).max()) - 1.0
    nbuf, npk = TC._sizes(prm, IM2COL, batch)
    im = checked_images(batch)

    def call(P, st):
        cc = prm._c()
        return lib.fhip_conv_forward_residual(ctypes.byref(cc), IM2COL, batch, P["y"], P["x"], P["packed"], P["scratch"], P["b"], P["r"], st)

    def ref():
        return {"y": plane_ref(conv64(g, x[im], w, b) + r[im], True, im)}

    return TC.Case(inputs={"x": x, "w": w, "b": b, "r": r}, outputs={"y": r.size}, scratch={"scratch": nbuf},
                   packed={"packed": (npk, TC._init(prm, IM2COL, "w", "packed"))}, call=call, bias_keys=("b",), batch=batch), ref, False


def _maxpool2(a):
    lib = TC._lib()
    c, k, h, wd, batch, bias, relu = a["c"], a["k"], a["h"], a["w"], a["batch"], a["bias"], a["relu"]
    prm = TC._param(c, k, h, wd, 3, 1, 1, 1, batch, bias, 1 if relu else 0)
    g = Geom(c, k, h, wd, 3, 3, 1, 1, 1, 1, 1, 1, 1, 1, 0)
    x, w = _weights(g, batch, 5 + k)
    b = distinct_bias(k, 11) if bias else None
    if relu and bias:
        b = kill_bias(b, w, float(np.abs(x).max()), clip_channel(k))
    nbuf, npk = TC._sizes(prm, WINO, batch)
    nout = batch * k * (prm.output_h // 2) * (prm.output_w // 2)
    im = checked_images(batch)

    def call(P, st):
        cc = prm._c()
        return lib.fhip_conv_forward_maxpool2(ctypes.byref(cc), WINO, batch, P["y"], P["x"], P["packed"], P["scratch"], P["b"], st)

    def ref():
        pre = conv64(g, x[im], w, b)
        y = np.maximum(pre, 0) if relu else pre
        return {"y": Plane(pool2(y), pool2_scale(pre), im)}

    bb = b if b is not None else np.full(k, np.nan, np.float32)
    return TC.Case(inputs={"x": x, "w": w, "b": bb}, outputs={"y": nout}, scratch={"scratch": nbuf},
                   packed={"packed": (npk, TC._init(prm, WINO, "w", "packed"))}, call=call, bias_keys=("b",), batch=batch), ref, not bias


def _dw_pw(a):
    lib = TC._lib()
    c, k, h, wd, s, batch = a["c"], a["k"], a["h"], a["w"], a["s"], a["batch"]
    pd = TC._param(c, c, h, wd, 3, s, 1, c, batch, True, 1)
    pp = TC._param(c, k, pd.output_h, pd.output_w, 1, 1, 0, 1, batch, True, 1)
    gd = Geom(c, c, h, wd, 3, 3, s, s, 1, 1, 1, 1, c, 1, 0)
    gp = Geom(c, k, pd.output_h, pd.output_w, 1, 1, 1, 1, 0, 0, 0, 0, 1, 1, 0)
    rng = np.random.default_rng(h * wd + c)
    wdw = (rng.uniform(-1, 1, (c, 1, 3, 3)) / 3).astype(np.float32)
    wpw = (rng.uniform(-1, 1, (k, c, 1, 1)) / np.sqrt(c)).astype(np.float32)
    x = scaled(rng.uniform(-1, 1, (batch, c, h, wd)).astype(np.float32))
    bd = kill_bias(distinct_bias(c, 1), wdw, float(np.abs(x).max()), clip_channel(c))
    im = checked_images(batch)
    mid = np.maximum(conv64(gd, x, wdw, bd), 0)
    bp = kill_bias(distinct_bias(k, 2), wpw, float(np.abs(mid).max()) * 1.001 + 1e-3, clip_channel(k))
    _, nd = TC._sizes(pd, DEPTHWISE, batch)
    _, np_ = TC._sizes(pp, IM2COL, batch)

    def call(P, st):
        cd, cp = pd._c(), pp._c()
        return lib.fhip_conv_forward_dw_pw(ctypes.byref(cd), ctypes.byref(cp), batch, P["y"], P["x"], P["pd"], P["bd"], P["pp"], P["bp"], st)

    def ref():
        return {"y": plane_ref(conv64(gp, mid[im].astype(np.float32), wpw, bp), True, im)}

    return TC.Case(inputs={"x": x, "wd": wdw, "bd": bd, "wp": wpw, "bp": bp}, outputs={"y": batch * k * pp.output_h * pp.output_w},
                   packed={"pd": (nd, TC._init(pd, DEPTHWISE, "wd", "pd")), "pp": (np_, TC._init(pp, IM2COL, "wp", "pp"))}, call=call,
                   bias_keys=("bd", "bp"), batch=batch), ref, False


def _siblings(a):
    from feathercnn_amd import _lib as L
    from feathercnn_amd.booster import ConvParam
    lib = TC._lib()
    c, ka, kb, h, s, batch = a["c"], a["ka"], a["kb"], a["h"], a["s"], a["batch"]
    pa = TC._param(c, ka, h, h, 1, s, 0, 1, batch, True, 0)
    pb = TC._param(c, kb, h, h, 1, s, 0, 1, batch, True, 1)
    ca, cb, both = pa._c(), pb._c(), L.fhip_conv_param()
    assert lib.fhip_conv_siblings_geometry(ctypes.byref(ca), ctypes.byref(cb), ctypes.byref(both)) == 0
    pboth = ConvParam(output_channels=both.output_channels, input_channels=c, input_h=h, input_w=h, kernel_h=1, kernel_w=1, stride_h=s, stride_w=s,
                      group=1, bias_term=bool(both.bias_term), activation=0, batch=batch)
    pboth.AssignOutputDim()
    rng = np.random.default_rng(31)
    wa = (rng.standard_normal((ka, c, 1, 1)) / np.sqrt(c)).astype(np.float32)
    wb = (rng.standard_normal((kb, c, 1, 1)) / np.sqrt(c)).astype(np.float32)
    x = scaled(rng.uniform(-1, 1, (batch, c, h, h)).astype(np.float32))
    ba = distinct_bias(ka, 4)
    bb = kill_bias(distinct_bias(kb, 5), wb, float(np.abs(x).max()), clip_channel(kb))
    _, npk = TC._sizes(pboth, IM2COL, batch)
    plane = pa.output_h * pa.output_w
    ga = Geom(c, ka, h, h, 1, 1, s, s, 0, 0, 0, 0, 1, 1, 0)
    gb = Geom(c, kb, h, h, 1, 1, s, s, 0, 0, 0, 0, 1, 1, 0)
    im = checked_images(batch)

    def call(P, st):
        ca, cb = pa._c(), pb._c()
        return lib.fhip_conv_forward_siblings(ctypes.byref(ca), ctypes.byref(cb), batch, P["ya"], P["yb"], P["x"], P["packed"], P["b"], st)

    def ref():
        return {"ya": plane_ref(conv64(ga, x[im], wa, ba), False, im), "yb": plane_ref(conv64(gb, x[im], wb, bb), True, im)}

    return TC.Case(inputs={"x": x, "w": np.concatenate([wa, wb]), "b": np.concatenate([ba, bb])}, outputs={"ya": batch * ka * plane, "yb": batch * kb * plane},
                   packed={"packed": (npk, TC._init(pboth, IM2COL, "w", "packed"))}, call=call, bias_keys=("b",), batch=batch), ref, False


def _chained(a):
    lib = TC._lib()
    batch, ic, h, wd, layers, pad0 = a["batch"], a["c"], a["h"], a["w"], a["layers"], a["pad0"]
    rng = np.random.default_rng(100 + h)
    prms, inputs, packed, scratch, geoms, flags = [], {}, {}, {}, [], []
    x = scaled(rng.uniform(-1, 1, (batch, ic, h, wd)).astype(np.float32))
    inputs["x"] = x
    c, hh, ww, act = ic, h, wd, x.astype(np.float64)
    im = checked_images(batch)
    act = act[im]
    xmax = float(np.abs(x).max())
    pres = []
    for i, (oc, pool, bias, relu) in enumerate(layers):
        pd_ = pad0 if i == 0 else 1
        prm = TC._param(c, oc, hh, ww, 3, 1, pd_, 1, batch, bias, 1 if relu else 0)
        g = Geom(c, oc, hh, ww, 3, 3, 1, 1, pd_, pd_, pd_, pd_, 1, 1, 0)
        w = (rng.standard_normal((oc, c, 3, 3)) / np.sqrt(9 * c)).astype(np.float32)
        b = distinct_bias(oc, 20 + i) if bias else None
        if relu and bias:
            b = kill_bias(b, w, xmax * 1.001 + 1e-3, clip_channel(oc))
        inputs[f"w{i}"], inputs[f"b{i}"] = w, (b if b is not None else np.full(oc, np.nan, np.float32))
        pl = TC._plan(prm, batch)
        packed[f"u{i}"] = (pl.u_bytes // 4, TC._init(prm, WINO, f"w{i}", f"u{i}"))
        scratch[f"v{i}"], scratch[f"m{i}"] = pl.v_bytes // 4, pl.m_bytes // 4
        pre = conv64(g, act.astype(np.float32), w, b)
        y = np.maximum(pre, 0) if relu else pre
        pres.append(pool2_scale(pre) if pool else np.abs(pre).max(axis=(2, 3)))
        act = pool2(y) if pool else y
        xmax = float(np.abs(act).max())
        prms.append(prm)
        flags.append(pool)
        c, hh, ww = oc, prm.output_h // (2 if pool else 1), prm.output_w // (2 if pool else 1)
    final = Plane(act, pres[-1], im)
    n = len(prms)

    def call(P, st):
        for i, prm in enumerate(prms):
            cc = prm._c()
            nxt = prms[i + 1]._c() if i + 1 < n else None
            rc = lib.fhip_conv_forward_chained(ctypes.byref(cc), batch, P["y"] if nxt is None else None, P["x"] if i == 0 else None, P[f"u{i}"],
                                               P[f"v{i}"], P[f"m{i}"], P[f"b{i}"], ctypes.byref(nxt) if nxt is not None else None,
                                               P[f"v{i + 1}"] if nxt is not None else None, int(flags[i]), st)
            if rc:
                return rc
        return 0

    null = tuple(f"b{i}" for i, l in enumerate(layers) if not l[2])
    return TC.Case(inputs=inputs, outputs={"y": batch * c * hh * ww}, scratch=scratch, packed=packed, call=call,
                   bias_keys=null, batch=batch), (lambda: {"y": final}), bool(null)


def _first(a):
    lib = TC._lib()
    batch, ic, h, wd, oc, bias, relu, pool = (a[n] for n in ("batch", "c", "h", "w", "k", "bias", "relu", "pool"))
    rng = np.random.default_rng(11 + ic)
    pf = TC._param(ic, oc, h, wd, 3, 1, 1, 1, batch, bias, 1 if relu else 0)
    pn = TC._param(oc, 12, h, wd, 3, 1, 1, 1, batch, True, 1)
    gf = Geom(ic, oc, h, wd, 3, 3, 1, 1, 1, 1, 1, 1, 1, 1, 0)
    gn = Geom(oc, 12, h, wd, 3, 3, 1, 1, 1, 1, 1, 1, 1, 1, 0)
    wf = (rng.standard_normal((oc, ic, 3, 3)) / np.sqrt(9 * ic)).astype(np.float32)
    wn = (rng.standard_normal((12, oc, 3, 3)) / np.sqrt(9 * oc)).astype(np.float32)
    x = scaled(rng.uniform(-1, 1, (batch, ic, h, wd)).astype(np.float32))
    bf = distinct_bias(oc, 8) if bias else None
    if bias and relu:
        bf = kill_bias(bf, wf, float(np.abs(x).max()), clip_channel(oc))
    im = checked_images(batch)
    pre1 = conv64(gf, x[im], wf, bf)
    mid = np.maximum(pre1, 0) if relu else pre1
    bn = kill_bias(distinct_bias(12, 9), wn, float(np.abs(mid).max()) * 1.001 + 1e-3, clip_channel(12))
    pl = TC._plan(pn, batch)
    oh, ow = (h // 2, wd // 2) if pool else (h, wd)

    def call(P, st):
        cf, cn = pf._c(), pn._c()
        rc = lib.fhip_winograd_f63_input_from_first(ctypes.byref(cf), ctypes.byref(cn), batch, P["v"], P["x"], P["wf"], P["bf"], st)
        return rc or lib.fhip_conv_forward_chained(ctypes.byref(cn), batch, P["y"], None, P["u"], P["v"], P["m"], P["bn"], None, None, int(pool), st)

    def ref():
        pre = conv64(gn, mid.astype(np.float32), wn, bn)
        y = np.maximum(pre, 0)
        return {"y": Plane(pool2(y), pool2_scale(pre), im) if pool else Plane(y, np.abs(pre).max(axis=(2, 3)), im)}

    return TC.Case(inputs={"x": x, "wf": wf, "bf": bf if bf is not None else np.full(oc, np.nan, np.float32), "wn": wn, "bn": bn},
                   outputs={"y": batch * 12 * oh * ow}, scratch={"v": pl.v_bytes // 4, "m": pl.m_bytes // 4},
                   packed={"u": (pl.u_bytes // 4, TC._init(pn, WINO, "wn", "u"))}, call=call, bias_keys=("bf",) if not bias else (),
                   batch=batch), ref, not bias


def _relu(a):
    lib = TC._lib()
    n = a["n"]
    x = np.random.default_rng(1).uniform(-1, 1, n).astype(np.float32) * np.float32(2.0 ** -6)
    return TC.Case(inputs={"x": x}, outputs={"y": n}, call=lambda P, st: lib.fhip_relu(P["y"], P["x"], n, st)), \
        (lambda: {"y": Exact(np.maximum(x, np.float32(0)))}), False


def _add(a):
    lib = TC._lib()
    n, relu = a["n"], a["relu"]
    rng = np.random.default_rng(2)
    x1 = rng.uniform(-1, 1, n).astype(np.float32) * np.float32(64)
    x2 = rng.uniform(-1, 1, n).astype(np.float32) * np.float32(2.0 ** -6)
    want = x1 + x2
    want = np.maximum(want, np.float32(0)) if relu else want
    return TC.Case(inputs={"a": x1, "b": x2}, outputs={"y": n}, call=lambda P, st: lib.fhip_add(P["y"], P["a"], P["b"], n, relu, st)), \
        (lambda: {"y": Exact(want)}), False


def _affine(a):
    lib = TC._lib()
    nb, c, hw, relu = a["batch"], a["c"], a["hw"], a["relu"]
    rng = np.random.default_rng(3)
    x = scaled(rng.uniform(-1, 1, (nb, c, hw)).astype(np.float32)).reshape(-1)
    mul, add = rng.uniform(-2, 2, c).astype(np.float32), distinct_bias(c, 6)
    xs = x.reshape(nb, c, hw).astype(np.float64)
    y = xs * mul[None, :, None] + add[None, :, None]
    mag = np.abs(xs * mul[None, :, None]) + np.abs(add[None, :, None])
    y = np.maximum(y, 0) if relu else y
    return TC.Case(inputs={"x": x, "mul": mul, "add": add}, outputs={"y": x.size},
                   call=lambda P, st: lib.fhip_affine(P["y"], P["x"], P["mul"], P["add"], nb, c, hw, relu, st)), \
        (lambda: {"y": Mag(y.reshape(-1), mag.reshape(-1))}), False


def _pool_ref(x, a, oh, ow):
    """(value, magnitude) of PoolingLayer::Forward in fp64 (tests/test_contract_gpu._pool_ref's window rules)."""
    nb, c, h, w = x.shape
    y, m = np.empty((nb, c, oh, ow)), np.empty((nb, c, oh, ow))
    off = 2 * a["pad"]
    kh, kw, s = (h, w, 1) if a["glob"] else (a["k"], a["k"], a["s"])
    for i in range(oh):
        for j in range(ow):
            y0, x0 = max(i * s - off, 0), max(j * s - off, 0)
            y1, x1 = min(i * s - off + kh, h), min(j * s - off + kw, w)
            win = x[:, :, y0:y1, x0:x1].astype(np.float64)
            y[:, :, i, j] = win.mean(axis=(2, 3)) if a["avg"] else win.max(axis=(2, 3))
            m[:, :, i, j] = np.abs(win).mean(axis=(2, 3))
    return y, m


def _pooling(a):
    from feathercnn_amd import _lib as L
    lib = TC._lib()
    nb, c, h, w = a["batch"], a["c"], a["h"], a["w"]
    q = L.fhip_pool_param(c, h, w, a["k"], a["k"], a["s"], a["s"], a["pad"], a["pad"], a["pad"], a["pad"], a["avg"], a["glob"])
    oh, ow = ctypes.c_int(), ctypes.c_int()
    assert lib.fhip_pooling_output_dim(ctypes.byref(q), ctypes.byref(oh), ctypes.byref(ow)) == 0
    x = scaled(np.random.default_rng(4).uniform(-1, 1, (nb, c, h, w)).astype(np.float32))
    y, m = _pool_ref(x, a, oh.value, ow.value)
    cmp = Mag(y.reshape(-1), m.reshape(-1)) if a["avg"] else Exact(y.astype(np.float32).reshape(-1))
    return TC.Case(inputs={"x": x}, outputs={"y": nb * c * oh.value * ow.value},
                   call=lambda P, st: lib.fhip_pooling(ctypes.byref(q), nb, P["y"], P["x"], st)), (lambda: {"y": cmp}), False


def _softmax(a):
    lib = TC._lib()
    nb, n = a["batch"], a["n"]
    x = np.random.default_rng(5).uniform(-4, 4, (nb, n)).astype(np.float32) * image_scales(nb)[:, None]
    xs = x.astype(np.float64)
    e = np.exp(xs - xs.max(axis=1, keepdims=True))
    want = e / e.sum(axis=1, keepdims=True)
    # magnitude of an output: itself (every term of the normalising sum is positive)
    return TC.Case(inputs={"x": x.reshape(-1)}, outputs={"y": x.size}, call=lambda P, st: lib.fhip_softmax(P["y"], P["x"], nb, n, st)), \
        (lambda: {"y": Mag(want.reshape(-1), want.reshape(-1))}), False


def _pixels(a):
    import torch

    import pixels_ref
    from feathercnn_amd import pixels as PX
    lib = TC._lib()
    nb, ptype, w, h, tw, th = a["batch"], getattr(PX, "PIXEL_" + a["type"]), a["w"], a["h"], a["tw"], a["th"]
    cin, cout = pixels_ref.channels(ptype)
    px = np.random.default_rng(12).integers(0, 256, (nb, h, w, cin), dtype=np.uint8)
    mean = np.array([100.5, 17.25, 250.0][:cout], np.float32)
    norm = np.array([1 / 255, 0.5, 2.0][:cout], np.float32)
    want = np.stack([pixels_ref.from_pixels_resize(px[i], ptype, tw, th, mean, norm) for i in range(nb)]).astype(np.float32)
    dpx = torch.from_numpy(px.reshape(-1)).to("cuda")
    dm, dn = torch.from_numpy(mean).to("cuda"), torch.from_numpy(norm).to("cuda")
    keep = (dpx, dm, dn)

    def call(P, st, keep=keep):
        fp = ctypes.POINTER(ctypes.c_float)
        return lib.fhip_pixels_to_float(P["y"], ctypes.c_void_p(keep[0].data_ptr()), nb, ptype, w, h, tw, th,
                                        ctypes.cast(keep[1].data_ptr(), fp), ctypes.cast(keep[2].data_ptr(), fp), st)

    return TC.Case(inputs={}, outputs={"y": want.size}, call=call), (lambda: {"y": Exact(want.reshape(-1))}), False


BUILD = {"conv": _conv, "residual": _residual, "maxpool2": _maxpool2, "dw_pw": _dw_pw, "siblings": _siblings, "chained": _chained, "first": _first,
         "relu": _relu, "add": _add, "affine": _affine, "pooling": _pooling, "softmax": _softmax, "pixels": _pixels}


# ---------------------------------------------------------------------------------------------------------------------------------------------

def build(case):
    """-> (contract Case, ref() -> {output: comparison}, null_bias)"""
    return BUILD[case.kind](case.args)


def run(case):
    """Build and run one case on plain allocations (16-byte aligned): -> (outputs {name: float32 array}, ref callable)."""
    import torch
    c, ref, null = build(case)
    r = TC.Run(c, 0, guarded=False, null_bias=null)
    r.init()
    r.forward()
    torch.cuda.synchronize()
    return r.out_values(), ref


def compare(case, got, refs):
    """-> list of failure messages (empty: the case passed)."""
    bad = []
    for k, cmp in refs.items():
        y = got[k]
        if isinstance(cmp, Exact):
            if not np.array_equal(y.view(np.int32), np.ascontiguousarray(cmp.ref, np.float32).reshape(-1).view(np.int32)):
                i = int(np.argmax(y.view(np.int32) != cmp.ref.reshape(-1).view(np.int32)))
                bad.append(f"{case.name}: '{k}' is not bit-equal (first difference at {i}: {y[i]!r} vs {cmp.ref.reshape(-1)[i]!r})")
        elif isinstance(cmp, Mag):
            err = np.abs(y.astype(np.float64) - cmp.ref)
            lim = MAG_TOL * cmp.mag + 1e-30
            if not np.isfinite(y).all() or (err > lim).any():
                i = int(np.argmax(err / lim))
                bad.append(f"{case.name}: '{k}'[{i}] = {y[i]!r}, fp64 {cmp.ref[i]!r}: error {err[i]:.3e} > {MAG_TOL} x magnitude {cmp.mag[i]:.3e}")
        else:
            ref = cmp.ref
            y = y.reshape(-1, *ref.shape[1:])[cmp.images].astype(np.float64)
            if not np.isfinite(y).all():
                bad.append(f"{case.name}: '{k}' has non-finite values")
                continue
            err = np.abs(y - ref).max(axis=(2, 3))
            top = np.abs(ref).max(axis=(2, 3))
            for n, kk in zip(*np.nonzero(top == 0)):
                if err[n, kk] != 0:
                    bad.append(f"{case.name}: '{k}' image {cmp.images[n]} channel {kk}: the activation clips this plane, got max |y| = {err[n, kk]:.3e}")
            with np.errstate(divide="ignore", invalid="ignore"):
                e = np.where(top > 0, err / np.maximum(cmp.scale, 1e-300), 0.0)
            if (e > TOL).any():
                n, kk = np.unravel_index(int(np.argmax(e)), e.shape)
                bad.append(f"{case.name}: '{k}' image {cmp.images[n]} channel {kk}: "
                           f"per-plane error {e[n, kk]:.3e} > {TOL} ({int((e > TOL).sum())} planes)")
    return bad


def separator(i):
    """fhip_relu over 1024 * (i + 1) floats: a grid of exactly i + 1 blocks, on the current stream, after a device synchronisation."""
    import torch
    torch.cuda.synchronize()
    t = _SEP[0]
    rc = TC._lib().fhip_relu(ctypes.c_void_p(t.data_ptr()), ctypes.c_void_p(t.data_ptr()), 1024 * (i + 1),
                             ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()


_SEP = []


def main(argv):
    import json

    import torch
    check = "--check" in argv
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    _SEP.append(torch.zeros(1024 * (len(CASES) + 1), dtype=torch.float32, device="cuda"))
    failures, log = [], []
    for i, case in enumerate(CASES):
        separator(i)
        got, ref = run(case)
        log.append(case.name)
        if check:
            f = compare(case, got, ref())
            failures += f
            print(("FAIL " if f else "ok   ") + case.name, flush=True)
            for m in f:
                print("   ", m, flush=True)
    separator(len(CASES))
    print(json.dumps({"cases": len(log), "cus": cus, "failures": len(failures)}), flush=True)
    return 1 if failures else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
