"""The buffer and stream contract of the C-ABI (include/feather_hip/feather_hip.h, feather_net.h), route by route (tests/contract_routes.py).

Every tensor the library sees is the body of a guarded region (tests/guarded.py): canary guards of 1 MiB on both sides, outputs / scratch /
packed weights poisoned with a quiet NaN, inputs holding data between quiet-NaN guards.  Packed weights, outputs and scratch are allocated at
EXACTLY the sizes the library reports.  Checks, at body offsets 0 and 1 float (16- and 4-byte-aligned):

  * Init: guards intact, every packed word written, a second Init bit-identical (the header: Init is idempotent);
  * Forward: rc 0, every guard intact (outputs, scratch, inputs), no poison left in an output, inputs bitwise unchanged, the output bit-identical
    to the same call on plain torch allocations, parity <= 1e-4 against the CPU checker and the fp64 direct convolution (numpy fp64 for the
    layers; the same-order element-wise layers exact), and where GetBufferSize reports 0 bytes, the empty-body scratch region untouched;
  * bias_term = 0 with a bias pointer to an all-NaN array: bit-identical to the documented NULL bias;
  * the call on a non-default stream, captured into a torch.cuda.graph (global capture mode: no allocation, synchronisation or null-stream
    launch may happen inside), replayed twice over re-poisoned outputs and scratch: bit-identical, guards intact.

Nothing here passes NULL where the library needs a buffer: a missing check shows as a failed assertion, never as a fault.
"""
from __future__ import annotations

import ctypes
import functools
from dataclasses import dataclass, field
from typing import Callable

import numpy as np
import pytest

import oracle
from contract_routes import DEPTHWISE, IM2COL, NAIVE, ROUTES, WINO
from guarded import Guarded, describe
from oracle import Geom, nerr, synth

pytestmark = pytest.mark.gpu
TOL = 1e-4
PARITY_IMAGES = 2  # parity on the first images of a batch: the CPU checkers are slow, the GPU already ran the whole batch


# ---------------------------------------------------------------------------------------------------------------------------------------------
# a case: named buffers and the calls that use them

@dataclass
class Case:
    inputs: dict                      # name -> float32 array (data the library reads)
    outputs: dict                     # name -> float count (the library writes every word)
    scratch: dict = field(default_factory=dict)   # name -> float count (the library may write; never read back)
    packed: dict = field(default_factory=dict)    # name -> (float count, init(P, stream) -> rc): written by Init, read by Forward
    call: Callable = None             # call(P, stream) -> rc; P maps every buffer name to a device address (or None for a NULL bias)
    ref: Callable = None              # ref() -> {output: (checker result or None, fp64 result, tolerance or "exact")}
    bias_keys: tuple = ()             # inputs that are biases (the bias checks replace them)
    inplace: dict = field(default_factory=dict)   # output -> input whose buffer it shares
    confirm: Callable = None          # confirm() -> (ok, message): the host-side predicate of the route
    batch: int = 1


class _Plain:
    """A plain torch allocation of n floats, `offset` floats past its start (the same alignment as the guarded run: kernels that take
    dword forms on 4-byte-aligned tensors may sum in another order)."""

    def __init__(self, n, fill, offset=0):
        import torch
        self.n = n
        self.t = torch.empty(max(n, 1) + offset, dtype=torch.float32, device="cuda")
        self.body = self.t[offset:offset + n]
        if not isinstance(fill, str) and n:
            self.body.copy_(torch.from_numpy(np.ascontiguousarray(fill, np.float32).reshape(-1)))
        self._ptr = self.t.data_ptr() + 4 * offset

    @property
    def ptr(self):
        return self._ptr


def _lib():
    from feathercnn_amd import _lib as L
    return L.load_library()


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _param(c, k, h, w, ks, s, p, group, batch, bias, act):
    from feathercnn_amd import ConvParam
    prm = ConvParam(output_channels=k, input_channels=c, input_h=h, input_w=w, kernel_h=ks, kernel_w=ks, stride_h=s, stride_w=s, pad_left=p,
                    pad_right=p, pad_top=p, pad_bottom=p, group=group, bias_term=bool(bias), activation=act, batch=batch)
    prm.AssignOutputDim()
    return prm


def _geom(prm) -> Geom:
    return Geom(prm.input_channels, prm.output_channels, prm.input_h, prm.input_w, prm.kernel_h, prm.kernel_w, prm.stride_h, prm.stride_w,
                prm.pad_left, prm.pad_right, prm.pad_top, prm.pad_bottom, prm.group, int(bool(prm.bias_term)), int(prm.activation))


def _sizes(prm, algo, batch):
    b, k = ctypes.c_size_t(), ctypes.c_size_t()
    c = prm._c()
    assert _lib().fhip_conv_get_buffer_size(ctypes.byref(c), algo, batch, ctypes.byref(b), ctypes.byref(k)) == 0
    assert b.value % 4 == 0 and k.value % 4 == 0
    return b.value // 4, k.value // 4


def _plan(prm, batch):
    from feathercnn_amd import booster
    prm.batch = batch
    return booster.winograd_plan(prm)


def _init(prm, algo, wkey, pkey):
    def f(P, st):
        c = prm._c()
        return _lib().fhip_conv_init(ctypes.byref(c), algo, P[pkey], P[wkey], st)
    return f


def _refconv(prm, x, w, b, algo=-1):
    """(checker, fp64) outputs of one convolution on the first PARITY_IMAGES images.  The checker runs its IM2COL route for every group-1
    layer: the operation is what is checked, and the reference's Winograd crashes on some geometries the library takes (C % 8 == 4 with
    ragged tiles, tests/test_parity_gpu.py)."""
    g = _geom(prm)
    x = x[:PARITY_IMAGES]
    if algo < 0 and g.group == 1:
        algo = IM2COL
    chk = oracle.best().forward(g, x, w, b if prm.bias_term else None, algo=algo)
    if algo == NAIVE:  # NAIVE ignores the activation (avx/booster.cpp:41-61)
        g = Geom(*(list(g.__dict__.values())[:14] + [0]))
    f64 = oracle.port().direct_f64(g, x, w, b if prm.bias_term else np.zeros(g.oc, np.float32))
    return chk, f64


def _pool2(a):
    n, c, h, w = a.shape
    return a[:, :, :h // 2 * 2, :w // 2 * 2].reshape(n, c, h // 2, 2, w // 2, 2).max(axis=(3, 5))


def _bias(n, mode, rng):
    """The bias array of a case: real values, or NaN for the bias-ignored checks."""
    return rng.uniform(-0.1, 0.1, n).astype(np.float32) if mode == "real" else np.full(n, np.nan, np.float32)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# builders, one per kind of entry point.  mode: "real" (bias_term as the route says), "nan" / "null" (bias_term = 0; the bias pointer is an
# all-NaN array or NULL)

def _conv_case(a, mode):
    lib = _lib()
    bias = a["bias"] and mode == "real"
    prm = _param(a["c"], a["k"], a["h"], a["w"], a["ks"], a["s"], a["p"], a["group"], a["batch"], bias, a["act"])
    algo, batch = a["algo"], a["batch"]
    g = _geom(prm)
    x, w, b = synth(g, batch, seed=a["c"] + a["k"] + a["h"])
    if mode != "real":
        b = np.full_like(b, np.nan)
    nbuf, npk = _sizes(prm, algo, batch)
    nout = batch * prm.output_channels * prm.output_h * prm.output_w

    def call(P, st):
        c = prm._c()
        return lib.fhip_conv_forward(ctypes.byref(c), algo, batch, P["y"], P["x"], P["packed"], P["scratch"], P["b"], st)

    def ref():
        chk, f64 = _refconv(prm, x, w, b, algo=NAIVE if algo == NAIVE else -1)
        return {"y": (chk, f64, TOL)}

    def confirm():
        return _confirm(a, prm, algo, batch, nbuf)

    return Case(inputs={"x": x, "w": w, "b": b}, outputs={"y": nout}, scratch={"scratch": nbuf}, packed={"packed": (npk, _init(prm, algo, "w", "packed"))},
                call=call, ref=ref, bias_keys=("b",), confirm=confirm, batch=batch)


def _confirm(a, prm, algo, batch, nbuf):
    lib = _lib()
    c = prm._c()
    what = ROUTE_OF[id(a)].confirm
    sel = ctypes.c_int(-1)
    if what.startswith("dw"):
        lib.fhip_conv_select_algo(ctypes.byref(c), ctypes.byref(sel))
        return sel.value == DEPTHWISE and nbuf == 0, f"select_algo = {sel.value}, buffer_bytes = {4 * nbuf}"
    if what == "igemm_no_scratch":
        st = lib.fhip_conv_streams_1x1(ctypes.byref(c), algo, batch)
        return nbuf == 0 and not st, f"buffer_bytes = {4 * nbuf}, streams_1x1 = {st}"
    if what == "smallc":
        return nbuf == 0, f"buffer_bytes = {4 * nbuf}"
    if what == "scratch":
        return nbuf > 0, f"buffer_bytes = {4 * nbuf} (the route keeps partial sums in the scratch)"
    if what == "streams_1x1":
        st = lib.fhip_conv_streams_1x1(ctypes.byref(c), algo, batch)
        return st == 1 and nbuf == 0, f"streams_1x1 = {st}, buffer_bytes = {4 * nbuf}"
    pl = _plan(prm, batch)
    if what == "f63":
        return pl.frequency_points == 64, f"frequency_points = {pl.frequency_points}"
    if what == "f43":
        return pl.frequency_points == 36, f"frequency_points = {pl.frequency_points}"
    if what == "column_blocks":
        return pl.column_block < pl.columns_padded, f"column_block = {pl.column_block}, columns_padded = {pl.columns_padded}"
    raise AssertionError(f"unknown predicate {what}")


def _residual_case(a, mode):
    lib = _lib()
    batch = a["batch"]
    prm = _param(a["c"], a["k"], a["h"], a["w"], 1, 1, 0, 1, batch, mode == "real", 1)
    g = _geom(prm)
    x, w, b = synth(g, batch, seed=a["k"])
    if mode != "real":
        b = np.full_like(b, np.nan)
    nout = batch * prm.output_channels * prm.output_h * prm.output_w
    r = np.random.default_rng(7).uniform(-1, 1, nout).astype(np.float32)
    nbuf, npk = _sizes(prm, IM2COL, batch)

    def call(P, st):
        c = prm._c()
        return lib.fhip_conv_forward_residual(ctypes.byref(c), IM2COL, batch, P["y"], P["x"], P["packed"], P["scratch"], P["b"], P["r"], st)

    def ref():
        p0 = _param(a["c"], a["k"], a["h"], a["w"], 1, 1, 0, 1, batch, mode == "real", 0)
        chk, f64 = _refconv(p0, x, w, b, IM2COL)
        rr = r.reshape(batch, *chk.shape[1:])[:PARITY_IMAGES]
        return {"y": (np.maximum(chk + rr, 0), np.maximum(f64 + rr, 0), TOL)}

    def confirm():
        c = prm._c()
        ok = lib.fhip_conv_can_fuse_residual(ctypes.byref(c), IM2COL) == 1
        if ROUTE_OF[id(a)].confirm.endswith("+scratch"):
            ok = ok and nbuf > 0
        return ok, f"can_fuse_residual, buffer_bytes = {4 * nbuf}"

    return Case(inputs={"x": x, "w": w, "b": b, "r": r}, outputs={"y": nout}, scratch={"scratch": nbuf},
                packed={"packed": (npk, _init(prm, IM2COL, "w", "packed"))}, call=call, ref=ref, bias_keys=("b",), confirm=confirm, batch=batch)


def _maxpool2_case(a, mode):
    lib = _lib()
    batch = a["batch"]
    prm = _param(a["c"], a["k"], a["h"], a["w"], 3, 1, 1, 1, batch, mode == "real", 1)
    x, w, b = synth(_geom(prm), batch, seed=5)
    if mode != "real":
        b = np.full_like(b, np.nan)
    nbuf, npk = _sizes(prm, WINO, batch)
    nout = batch * prm.output_channels * (prm.output_h // 2) * (prm.output_w // 2)

    def call(P, st):
        c = prm._c()
        return lib.fhip_conv_forward_maxpool2(ctypes.byref(c), WINO, batch, P["y"], P["x"], P["packed"], P["scratch"], P["b"], st)

    def ref():
        chk, f64 = _refconv(prm, x, w, b)
        return {"y": (_pool2(chk), _pool2(f64), TOL)}

    def confirm():
        c = prm._c()
        return lib.fhip_conv_can_fuse_maxpool2(ctypes.byref(c), WINO) == 1, "can_fuse_maxpool2"

    return Case(inputs={"x": x, "w": w, "b": b}, outputs={"y": nout}, scratch={"scratch": nbuf}, packed={"packed": (npk, _init(prm, WINO, "w", "packed"))},
                call=call, ref=ref, bias_keys=("b",), confirm=confirm, batch=batch)


def _dw_pw_case(a, mode):
    lib = _lib()
    c, k, h, w, s, batch = a["c"], a["k"], a["h"], a["w"], a["s"], a["batch"]
    real = mode == "real"
    pd = _param(c, c, h, w, 3, s, 1, c, batch, real, 1)
    pp = _param(c, k, pd.output_h, pd.output_w, 1, 1, 0, 1, batch, real, 1)
    rng = np.random.default_rng(h * w + c)
    wd = (rng.uniform(-1, 1, (c, 1, 3, 3)) / 3).astype(np.float32)
    wp = (rng.uniform(-1, 1, (k, c, 1, 1)) / np.sqrt(c)).astype(np.float32)
    bd, bp = _bias(c, mode, rng), _bias(k, mode, rng)
    x = rng.uniform(-1, 1, (batch, c, h, w)).astype(np.float32)
    _, nd = _sizes(pd, DEPTHWISE, batch)
    _, np_ = _sizes(pp, IM2COL, batch)
    nout = batch * k * pp.output_h * pp.output_w

    def call(P, st):
        cd, cp = pd._c(), pp._c()
        return lib.fhip_conv_forward_dw_pw(ctypes.byref(cd), ctypes.byref(cp), batch, P["y"], P["x"], P["pd"], P["bd"], P["pp"], P["bp"], st)

    def ref():
        m1, m2 = _refconv(pd, x, wd, bd)
        out1 = oracle.best().forward(_geom(pp), m1, wp, bp if real else None)
        out2 = oracle.port().direct_f64(_geom(pp), m2.astype(np.float32), wp, bp if real else np.zeros(k, np.float32))
        return {"y": (out1, out2, TOL)}

    def confirm():
        cd, cp = pd._c(), pp._c()
        return lib.fhip_conv_can_fuse_dw_pw(ctypes.byref(cd), ctypes.byref(cp), batch) == 1, "can_fuse_dw_pw"

    return Case(inputs={"x": x, "wd": wd, "bd": bd, "wp": wp, "bp": bp}, outputs={"y": nout},
                packed={"pd": (nd, _init(pd, DEPTHWISE, "wd", "pd")), "pp": (np_, _init(pp, IM2COL, "wp", "pp"))}, call=call, ref=ref,
                bias_keys=("bd", "bp"), confirm=confirm, batch=batch)


def _siblings_case(a, mode):
    from feathercnn_amd import _lib as L
    from feathercnn_amd.booster import ConvParam
    lib = _lib()
    c, ka, kb, h, s, batch = a["c"], a["ka"], a["kb"], a["h"], a["s"], a["batch"]
    real = mode == "real"
    pa = _param(c, ka, h, h, 1, s, 0, 1, batch, real, 0)
    pb = _param(c, kb, h, h, 1, s, 0, 1, batch, real, 1)
    ca, cb, both = pa._c(), pb._c(), L.fhip_conv_param()
    assert lib.fhip_conv_siblings_geometry(ctypes.byref(ca), ctypes.byref(cb), ctypes.byref(both)) == 0
    pboth = ConvParam(output_channels=both.output_channels, input_channels=c, input_h=h, input_w=h, kernel_h=1, kernel_w=1, stride_h=s, stride_w=s,
                      group=1, bias_term=bool(both.bias_term), activation=0, batch=batch)
    pboth.AssignOutputDim()
    rng = np.random.default_rng(31)
    wa = (rng.standard_normal((ka, c, 1, 1)) / np.sqrt(c)).astype(np.float32)
    wb = (rng.standard_normal((kb, c, 1, 1)) / np.sqrt(c)).astype(np.float32)
    bb = _bias(ka + kb, mode, rng)
    x = rng.uniform(-1, 1, (batch, c, h, h)).astype(np.float32)
    _, npk = _sizes(pboth, IM2COL, batch)
    plane = pa.output_h * pa.output_w

    def call(P, st):
        ca, cb = pa._c(), pb._c()
        return lib.fhip_conv_forward_siblings(ctypes.byref(ca), ctypes.byref(cb), batch, P["ya"], P["yb"], P["x"], P["packed"], P["b"], st)

    def ref():
        ra = _refconv(pa, x, wa, bb[:ka])
        rb = _refconv(pb, x, wb, bb[ka:])
        return {"ya": (ra[0], ra[1], TOL), "yb": (rb[0], rb[1], TOL)}

    def confirm():
        ca, cb = pa._c(), pb._c()
        return lib.fhip_conv_can_fuse_siblings(ctypes.byref(ca), IM2COL, ctypes.byref(cb), IM2COL, batch) == 1, "can_fuse_siblings"

    return Case(inputs={"x": x, "w": np.concatenate([wa, wb]), "b": bb}, outputs={"ya": batch * ka * plane, "yb": batch * kb * plane},
                packed={"packed": (npk, _init(pboth, IM2COL, "w", "packed"))}, call=call, ref=ref, bias_keys=("b",), confirm=confirm, batch=batch)


def _chained_case(a, mode):
    lib = _lib()
    _, batch, ic, h, w, spec, pad0, bias, relu = a["run"]
    bias = bias and mode == "real"
    rng = np.random.default_rng(100)
    prms, pools, inputs, packed, scratch = [], [], {}, {}, {}
    c, hh, ww = ic, h, w
    for i, (oc, pool) in enumerate(spec):
        prm = _param(c, oc, hh, ww, 3, 1, pad0 if i == 0 else 1, 1, batch, bias, 1 if relu else 0)
        inputs[f"w{i}"] = (rng.standard_normal((oc, c, 3, 3)) / np.sqrt(9 * c)).astype(np.float32)
        inputs[f"b{i}"] = _bias(oc, mode, rng)
        pl = _plan(prm, batch)
        packed[f"u{i}"] = (pl.u_bytes // 4, _init(prm, WINO, f"w{i}", f"u{i}"))
        scratch[f"v{i}"], scratch[f"m{i}"] = pl.v_bytes // 4, pl.m_bytes // 4
        prms.append(prm)
        pools.append(pool)
        c, hh, ww = oc, prm.output_h, prm.output_w
        if pool:
            hh, ww = hh // 2, ww // 2
    x = rng.uniform(-1, 1, (batch, ic, h, w)).astype(np.float32)
    inputs["x"] = x
    n = len(prms)

    def call(P, st):
        for i, prm in enumerate(prms):
            cc = prm._c()
            nxt = prms[i + 1]._c() if i + 1 < n else None
            rc = lib.fhip_conv_forward_chained(ctypes.byref(cc), batch, P["y"] if nxt is None else None, P["x"] if i == 0 else None, P[f"u{i}"],
                                               P[f"v{i}"], P[f"m{i}"], P[f"b{i}"], ctypes.byref(nxt) if nxt is not None else None,
                                               P[f"v{i + 1}"] if nxt is not None else None, int(pools[i]), st)
            if rc:
                return rc
        return 0

    def ref():
        r1 = r2 = x[:PARITY_IMAGES]
        for i, prm in enumerate(prms):
            b = inputs[f"b{i}"] if bias else None
            r1 = oracle.best().forward(_geom(prm), r1, inputs[f"w{i}"], b)
            r2 = oracle.port().direct_f64(_geom(prm), np.asarray(r2, np.float32), inputs[f"w{i}"], b if bias else np.zeros(prm.output_channels, np.float32))
            if pools[i]:
                r1, r2 = _pool2(r1), _pool2(r2)
        return {"y": (r1, r2, TOL)}

    def confirm():
        ok = all(lib.fhip_conv_can_chain_winograd(ctypes.byref(prms[i]._c()), WINO, ctypes.byref(prms[i + 1]._c()), WINO, int(pools[i])) == 1
                 for i in range(n - 1))
        return ok, "can_chain_winograd for every adjacent pair"

    return Case(inputs=inputs, outputs={"y": batch * c * hh * ww}, scratch=scratch, packed=packed, call=call, ref=ref,
                bias_keys=tuple(f"b{i}" for i in range(n)), confirm=confirm, batch=batch)


def _first_case(a, mode):
    lib = _lib()
    _, batch, ic, h, w, oc, bias, relu, pool = a["case"]
    real = mode == "real"
    rng = np.random.default_rng(11)
    pf = _param(ic, oc, h, w, 3, 1, 1, 1, batch, bias and real, 1 if relu else 0)
    pn = _param(oc, 12, h, w, 3, 1, 1, 1, batch, real, 1)
    wf = (rng.standard_normal((oc, ic, 3, 3)) / np.sqrt(9 * ic)).astype(np.float32)
    wn = (rng.standard_normal((12, oc, 3, 3)) / np.sqrt(9 * oc)).astype(np.float32)
    bf, bn = _bias(oc, mode, rng), _bias(12, mode, rng)
    x = rng.uniform(-1, 1, (batch, ic, h, w)).astype(np.float32)
    pl = _plan(pn, batch)
    oh, ow = (h // 2, w // 2) if pool else (h, w)

    def call(P, st):
        cf, cn = pf._c(), pn._c()
        rc = lib.fhip_winograd_f63_input_from_first(ctypes.byref(cf), ctypes.byref(cn), batch, P["v"], P["x"], P["wf"], P["bf"], st)
        return rc or lib.fhip_conv_forward_chained(ctypes.byref(cn), batch, P["y"], None, P["u"], P["v"], P["m"], P["bn"], None, None, int(pool), st)

    def ref():
        m1, m2 = _refconv(pf, x, wf, bf)
        y1 = oracle.best().forward(_geom(pn), m1, wn, bn if real else None)
        y2 = oracle.port().direct_f64(_geom(pn), m2.astype(np.float32), wn, bn if real else np.zeros(12, np.float32))
        return {"y": ((_pool2(y1), _pool2(y2)) if pool else (y1, y2)) + (TOL,)}

    def confirm():
        cf, cn = pf._c(), pn._c()
        return lib.fhip_conv_can_fuse_first_winograd(ctypes.byref(cf), ctypes.byref(cn), WINO, batch) == 1, "can_fuse_first_winograd"

    return Case(inputs={"x": x, "wf": wf, "bf": bf, "wn": wn, "bn": bn}, outputs={"y": batch * 12 * oh * ow},
                scratch={"v": pl.v_bytes // 4, "m": pl.m_bytes // 4}, packed={"u": (pl.u_bytes // 4, _init(pn, WINO, "wn", "u"))}, call=call, ref=ref,
                bias_keys=("bf", "bn"), confirm=confirm, batch=batch)


def _out_to_next_case(a, mode):
    lib = _lib()
    batch, c, k, k2, h, w, pool = a["batch"], a["c"], a["k"], a["k2"], a["h"], a["w"], a["pool"]
    real = mode == "real"
    rng = np.random.default_rng(17)
    p1 = _param(c, k, h, w, 3, 1, 1, 1, batch, real, 1)
    h2, w2 = (h // 2, w // 2) if pool else (h, w)
    p2 = _param(k, k2, h2, w2, 3, 1, 1, 1, batch, real, 1)
    w1 = (rng.standard_normal((k, c, 3, 3)) / np.sqrt(9 * c)).astype(np.float32)
    wn = (rng.standard_normal((k2, k, 3, 3)) / np.sqrt(9 * k)).astype(np.float32)
    b1, b2 = _bias(k, mode, rng), _bias(k2, mode, rng)
    x = rng.uniform(-1, 1, (batch, c, h, w)).astype(np.float32)
    l1, l2 = _plan(p1, batch), _plan(p2, batch)

    def call(P, st):
        c1, c2 = p1._c(), p2._c()
        for rc in (lambda: lib.fhip_winograd_f63_input_transform(ctypes.byref(c1), batch, P["v1"], P["x"], st),
                   lambda: lib.fhip_winograd_f63_tile_gemm(ctypes.byref(c1), batch, P["m1"], P["u1"], P["v1"], st),
                   lambda: lib.fhip_winograd_f63_output_to_next_input(ctypes.byref(c1), ctypes.byref(c2), batch, P["vn"], P["m1"], P["b1"], pool, st),
                   lambda: lib.fhip_conv_forward_chained(ctypes.byref(c2), batch, P["y"], None, P["u2"], P["vn"], P["m2"], P["b2"], None, None, 0, st)):
            r = rc()
            if r:
                return r
        return 0

    def ref():
        m1, m2 = _refconv(p1, x, w1, b1)
        if pool:
            m1, m2 = _pool2(m1), _pool2(m2)
        y1 = oracle.best().forward(_geom(p2), m1, wn, b2 if real else None)
        y2 = oracle.port().direct_f64(_geom(p2), m2.astype(np.float32), wn, b2 if real else np.zeros(k2, np.float32))
        return {"y": (y1, y2, TOL)}

    def confirm():
        c1, c2 = p1._c(), p2._c()
        return lib.fhip_conv_can_chain_winograd(ctypes.byref(c1), WINO, ctypes.byref(c2), WINO, pool) == 1, "can_chain_winograd"

    return Case(inputs={"x": x, "w1": w1, "b1": b1, "w2": wn, "b2": b2}, outputs={"y": batch * k2 * h2 * w2},
                scratch={"v1": l1.v_bytes // 4, "m1": l1.m_bytes // 4, "vn": l2.v_bytes // 4, "m2": l2.m_bytes // 4},
                packed={"u1": (l1.u_bytes // 4, _init(p1, WINO, "w1", "u1")), "u2": (l2.u_bytes // 4, _init(p2, WINO, "w2", "u2"))}, call=call, ref=ref,
                bias_keys=("b1", "b2"), confirm=confirm, batch=batch)


def _wino_stages_case(a, mode):
    lib = _lib()
    batch = a["batch"]
    prm = _param(a["c"], a["k"], a["h"], a["w"], 3, 1, 1, 1, batch, mode == "real", 1)
    x, w, b = synth(_geom(prm), batch, seed=5)
    if mode != "real":
        b = np.full_like(b, np.nan)
    pl = _plan(prm, batch)

    def u_init(P, st):
        c = prm._c()
        return lib.fhip_winograd_f63_transform_kernel(ctypes.byref(c), P["u"], P["w"], st)

    def call(P, st):
        c = prm._c()
        return (lib.fhip_winograd_f63_input_transform(ctypes.byref(c), batch, P["v"], P["x"], st)
                or lib.fhip_winograd_f63_tile_gemm(ctypes.byref(c), batch, P["m"], P["u"], P["v"], st)
                or lib.fhip_winograd_f63_output_transform(ctypes.byref(c), batch, P["y"], P["m"], P["b"], st))

    def ref():
        chk, f64 = _refconv(prm, x, w, b)
        return {"y": (chk, f64, TOL)}

    def confirm():
        if ROUTE_OF[id(a)].confirm == "column_blocks":
            return pl.column_block < pl.columns_padded, f"column_block = {pl.column_block}, columns_padded = {pl.columns_padded}"
        return pl.frequency_points == 64, f"frequency_points = {pl.frequency_points}"

    return Case(inputs={"x": x, "w": w, "b": b}, outputs={"y": batch * prm.output_channels * prm.output_h * prm.output_w},
                scratch={"v": pl.v_bytes // 4, "m": pl.m_bytes // 4}, packed={"u": (pl.u_bytes // 4, u_init)}, call=call, ref=ref, bias_keys=("b",),
                confirm=confirm, batch=batch)


def _layer_confirm():
    return True, "layer"


def _relu_case(a, mode):
    lib = _lib()
    n = a["n"]
    x = np.random.default_rng(1).uniform(-1, 1, n).astype(np.float32)
    return Case(inputs={"x": x}, outputs={"y": n}, call=lambda P, st: lib.fhip_relu(P["y"], P["x"], n, st),
                ref=lambda: {"y": (None, np.maximum(x, 0), "exact")}, confirm=_layer_confirm)


def _add_case(a, mode):
    lib = _lib()
    n, relu = a["n"], a["relu"]
    rng = np.random.default_rng(2)
    x1, x2 = rng.uniform(-1, 1, n).astype(np.float32), rng.uniform(-1, 1, n).astype(np.float32)
    want = (x1 + x2) if not relu else np.maximum(x1 + x2, 0)
    if a["inplace"]:  # y == a, the way the Net runtime calls it (net.hip)
        return Case(inputs={"a": x1, "b": x2}, outputs={"y": n}, inplace={"y": "a"}, call=lambda P, st: lib.fhip_add(P["y"], P["y"], P["b"], n, relu, st),
                    ref=lambda: {"y": (None, want, "exact")}, confirm=_layer_confirm)
    return Case(inputs={"a": x1, "b": x2}, outputs={"y": n}, call=lambda P, st: lib.fhip_add(P["y"], P["a"], P["b"], n, relu, st),
                ref=lambda: {"y": (None, want, "exact")}, confirm=_layer_confirm)


def _affine_case(a, mode):
    lib = _lib()
    nb, c, hw, relu = a["batch"], a["c"], a["hw"], a["relu"]
    rng = np.random.default_rng(3)
    x = rng.uniform(-1, 1, nb * c * hw).astype(np.float32)
    mul, add = rng.uniform(-2, 2, c).astype(np.float32), rng.uniform(-1, 1, c).astype(np.float32)
    y = x.reshape(nb, c, hw).astype(np.float64) * mul[None, :, None] + add[None, :, None]
    y = np.maximum(y, 0) if relu else y
    return Case(inputs={"x": x, "mul": mul, "add": add}, outputs={"y": x.size},
                call=lambda P, st: lib.fhip_affine(P["y"], P["x"], P["mul"], P["add"], nb, c, hw, relu, st),
                ref=lambda: {"y": (None, y.reshape(-1), 1e-6)}, confirm=_layer_confirm)


def _pool_ref(x, a, oh, ow):
    """PoolingLayer::Forward restated in fp64 (feather_net.h): window origin j*stride - pad_top - pad_bottom, windows clipped to the image,
    the average over the in-range taps."""
    nb, c, h, w = x.shape
    y = np.empty((nb, c, oh, ow))
    off = 2 * a["pad"]
    kh, kw, s = (h, w, 1) if a["glob"] else (a["k"], a["k"], a["s"])
    for i in range(oh):
        for j in range(ow):
            y0, x0 = max(i * s - off, 0), max(j * s - off, 0)
            y1, x1 = min(i * s - off + kh, h), min(j * s - off + kw, w)
            win = x[:, :, y0:y1, x0:x1].astype(np.float64)
            y[:, :, i, j] = win.mean(axis=(2, 3)) if a["avg"] else win.max(axis=(2, 3))
    return y


def _pooling_case(a, mode):
    from feathercnn_amd import _lib as L
    lib = _lib()
    nb, c, h, w = a["batch"], a["c"], a["h"], a["w"]
    q = L.fhip_pool_param(c, h, w, a["k"], a["k"], a["s"], a["s"], a["pad"], a["pad"], a["pad"], a["pad"], a["avg"], a["glob"])
    oh, ow = ctypes.c_int(), ctypes.c_int()
    assert lib.fhip_pooling_output_dim(ctypes.byref(q), ctypes.byref(oh), ctypes.byref(ow)) == 0
    x = np.random.default_rng(4).uniform(-1, 1, (nb, c, h, w)).astype(np.float32)
    want = _pool_ref(x, a, oh.value, ow.value).reshape(-1)
    return Case(inputs={"x": x}, outputs={"y": nb * c * oh.value * ow.value}, call=lambda P, st: lib.fhip_pooling(ctypes.byref(q), nb, P["y"], P["x"], st),
                ref=lambda: {"y": (None, want, 1e-6 if a["avg"] else "exact")}, confirm=_layer_confirm)


def _softmax_case(a, mode):
    lib = _lib()
    nb, n = a["batch"], a["n"]
    x = np.random.default_rng(5).uniform(-4, 4, nb * n).astype(np.float32)
    e = np.exp(x.reshape(nb, n).astype(np.float64) - x.reshape(nb, n).max(axis=1, keepdims=True))
    want = (e / e.sum(axis=1, keepdims=True)).reshape(-1)
    return Case(inputs={"x": x}, outputs={"y": x.size}, call=lambda P, st: lib.fhip_softmax(P["y"], P["x"], nb, n, st),
                ref=lambda: {"y": (None, want, 1e-5)}, confirm=_layer_confirm)


BUILD = {"conv": _conv_case, "residual": _residual_case, "maxpool2": _maxpool2_case, "dw_pw": _dw_pw_case, "siblings": _siblings_case,
         "chained": _chained_case, "first": _first_case, "out_to_next": _out_to_next_case, "wino_stages": _wino_stages_case, "relu": _relu_case,
         "add": _add_case, "affine": _affine_case, "pooling": _pooling_case, "softmax": _softmax_case}
BIASED = ("conv", "residual", "maxpool2", "dw_pw", "siblings", "chained", "first", "out_to_next", "wino_stages")
ROUTE_OF = {id(r.args): r for r in ROUTES}


# ---------------------------------------------------------------------------------------------------------------------------------------------
# running a case

class Run:
    """The buffers of one case, guarded (at a body offset) or plain, with Init done."""

    def __init__(self, case: Case, offset=0, guarded=True, null_bias=False, stream=None):
        mk = (lambda n, fill: Guarded(n, fill, offset)) if guarded else (lambda n, fill: _Plain(n, fill, offset))
        self.case, self.null_bias = case, null_bias
        self.inputs = {k: mk(v.size, v) for k, v in case.inputs.items() if not (null_bias and k in case.bias_keys)}
        self.packed = {k: mk(n, "poison") for k, (n, _) in case.packed.items()}
        self.outputs = {k: (self.inputs[case.inplace[k]] if k in case.inplace else mk(n, "poison")) for k, n in case.outputs.items()}
        self.scratch = {k: mk(n, "poison") for k, n in case.scratch.items()}
        self.P = {k: b.ptr for d in (self.inputs, self.packed, self.outputs, self.scratch) for k, b in d.items()}
        for k in case.bias_keys:
            if null_bias:
                self.P[k] = None
        self.st = stream

    def stream_handle(self):
        import torch
        return ctypes.c_void_p((self.st or torch.cuda.current_stream()).cuda_stream)

    def init(self):
        for k, (_, f) in self.case.packed.items():
            rc = f(self.P, self.stream_handle())
            assert rc == 0, f"Init of {k} returned {rc}: {_lib().fhip_last_error().decode()}"

    def forward(self):
        rc = self.case.call(self.P, self.stream_handle())
        assert rc == 0, f"forward returned {rc}: {_lib().fhip_last_error().decode()}"

    def all_guarded(self):
        return {**{"input " + k: b for k, b in self.inputs.items()}, **{"packed " + k: b for k, b in self.packed.items()},
                **{"output " + k: b for k, b in self.outputs.items()}, **{"scratch " + k: b for k, b in self.scratch.items()}}

    def out_values(self):
        return {k: b.body.detach().cpu().numpy().copy() for k, b in self.outputs.items()}


def _skip_if_not_256(route):
    if route.cus256 and _cus() != 256:
        pytest.skip(f"{route.name}: geometry cut for 256 CUs, this device has {_cus()} (the route would be a different one here)")


@functools.lru_cache(maxsize=None)
def _case(name, mode="real") -> Case:
    r = next(r for r in ROUTES if r.name == name)
    return BUILD[r.kind](r.args, mode)


@functools.lru_cache(maxsize=None)
def _plain_outputs(name, offset):
    import torch
    run = Run(_case(name), offset, guarded=False)
    run.init()
    run.forward()
    torch.cuda.synchronize()
    return run.out_values()


@functools.lru_cache(maxsize=None)
def _reference(name):
    return _case(name).ref()


IDS = [r.name for r in ROUTES]
CONV_ROUTES = [r for r in ROUTES if r.kind not in ("relu", "add", "affine", "pooling", "softmax")]


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("route", CONV_ROUTES, ids=[r.name for r in CONV_ROUTES])
def test_init_footprint(cuda, route, offset):
    import torch
    _skip_if_not_256(route)
    case = _case(route.name)
    run = Run(case, offset)
    weights = {k: b.snapshot() for k, b in run.inputs.items()}
    run.init()
    torch.cuda.synchronize()
    for k, b in run.packed.items():
        assert b.guards_intact() is None, f"{route.name}: Init wrote outside packed '{k}' ({b.n} floats): {describe(b.guards_intact())}"
        assert b.unwritten() == 0, f"{route.name}: Init left {b.unwritten()} of {b.n} words of packed '{k}' unwritten (the sizes GetBufferSize reports)"
    for k, b in run.inputs.items():
        assert b.unchanged(weights[k]), f"{route.name}: Init changed its input '{k}' at {b.first_change(weights[k])}"
    first = {k: b.snapshot() for k, b in run.packed.items()}
    run.init()
    torch.cuda.synchronize()
    for k, b in run.packed.items():
        assert b.unchanged(first[k]), f"{route.name}: a second Init of '{k}' is not bit-identical (the header: Init is idempotent)"


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("route", ROUTES, ids=IDS)
def test_forward_footprint(cuda, route, offset):
    import torch
    _skip_if_not_256(route)
    case = _case(route.name)
    ok, why = case.confirm()
    assert ok, f"{route.name}: not on its route ({why})"
    run = Run(case, offset)
    run.init()
    torch.cuda.synchronize()
    before = {k: b.snapshot() for d in (run.inputs, run.packed) for k, b in d.items() if k not in case.inplace.values()}
    empty = {k: b.snapshot() for k, b in run.scratch.items() if b.n == 0}
    run.forward()
    torch.cuda.synchronize()
    for what, b in run.all_guarded().items():
        assert b.guards_intact() is None, f"{route.name} @ offset {offset}: {what} ({b.n} floats) written outside: {describe(b.guards_intact())}"
    for k, b in run.outputs.items():
        assert b.unwritten() == 0, f"{route.name} @ offset {offset}: {b.unwritten()} of {b.n} words of output '{k}' never written"
    for k, snap in before.items():
        b = run.inputs.get(k) or run.packed[k]
        assert b.unchanged(snap), f"{route.name} @ offset {offset}: input '{k}' changed at {b.first_change(snap)}"
    for k, snap in empty.items():
        assert run.scratch[k].unchanged(snap), (f"{route.name}: GetBufferSize reported 0 bytes for '{k}' but the forward wrote around the pointer "
                                                f"({run.scratch[k].first_change(snap)}); the Net runtime's plan_concurrency runs such layers on a second "
                                                "stream with the shared arena as their buffer")
    got = run.out_values()
    for k, v in _plain_outputs(route.name, offset).items():
        assert np.array_equal(got[k].view(np.int32), v.view(np.int32)), f"{route.name} @ offset {offset}: '{k}' differs from the plain-allocation run"
    for k, (chk, f64, tol) in _reference(route.name).items():
        y = got[k]
        if chk is not None:
            y = y.reshape(-1, *chk.shape[1:])[:chk.shape[0]]
            e = nerr(y, chk)
            assert np.isfinite(y).all() and e <= tol, f"{route.name}: '{k}' vs {type(oracle.best()).__name__}: {e:.3e}"
        y = y.reshape(np.shape(f64))
        if tol == "exact":
            assert np.array_equal(y, f64.astype(np.float32)), f"{route.name}: '{k}' is not exact"
        else:
            e = nerr(y, f64)
            assert np.isfinite(y).all() and e <= tol, f"{route.name}: '{k}' vs the fp64 restatement: {e:.3e}"


BIAS_ROUTES = [r for r in ROUTES if r.kind in BIASED]


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("route", BIAS_ROUTES, ids=[r.name for r in BIAS_ROUTES])
def test_bias_ignored_without_bias_term(cuda, route, offset):
    """feather_hip.h: bias_arr may be NULL when !bias_term -- so a route must never read it then."""
    import torch
    _skip_if_not_256(route)
    outs = []
    for null in (True, False):
        case = _case(route.name, "null" if null else "nan")
        run = Run(case, offset, null_bias=null)
        run.init()
        run.forward()
        torch.cuda.synchronize()
        for what, b in run.all_guarded().items():
            assert b.guards_intact() is None, f"{route.name}: {what} written outside: {describe(b.guards_intact())}"
        outs.append(run.out_values())
    for k in outs[0]:
        assert np.isfinite(outs[0][k]).all(), f"{route.name}: the NULL-bias run has non-finite '{k}'"
        assert np.array_equal(outs[0][k].view(np.int32), outs[1][k].view(np.int32)), \
            f"{route.name}: with bias_term = 0 the output '{k}' depends on the bias array (NaN bias changed {int(np.sum(outs[0][k] != outs[1][k]))} values)"


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("route", ROUTES, ids=IDS)
def test_stream_capture(cuda, route, offset):
    """feather_hip.h: Forward is asynchronous on `stream` and never allocates -- so it captures into a graph on a side stream."""
    import torch
    _skip_if_not_256(route)
    case = _case(route.name)
    side = torch.cuda.Stream()
    run = Run(case, offset, stream=side)
    with torch.cuda.stream(side):
        run.init()
        run.forward()  # eager warm-up (one-time attributes and the like)
    side.synchronize()
    eager = run.out_values()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        run.forward()
    torch.cuda.synchronize()
    for rep in range(2):
        for k, b in list(run.scratch.items()) + [(k, b) for k, b in run.outputs.items() if k not in case.inplace]:
            b.fill("poison")
        if case.inplace:  # in-place routes start again from their input values
            for k, src in case.inplace.items():
                run.outputs[k].fill(case.inputs[src])
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        for what, b in run.all_guarded().items():
            assert b.guards_intact() is None, f"{route.name}: replay {rep}: {what} written outside: {describe(b.guards_intact())}"
        got = run.out_values()
        for k in eager:
            assert np.array_equal(got[k].view(np.int32), eager[k].view(np.int32)), f"{route.name}: replay {rep} of '{k}' differs from the eager run"
    del graph


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the checks can fail: real kernels, buffers a little short (the missing words fall in the test's own guard, so nothing faults)

def _short_run(name, what, short_floats):
    import torch
    case = _case(name)
    sizes = dict(case.scratch) if what == "scratch" else dict(case.outputs)
    key = next(iter(sizes))
    shorter = Case(**{**case.__dict__, ("scratch" if what == "scratch" else "outputs"): {**sizes, key: sizes[key] - short_floats}})
    run = Run(shorter, 0)
    run.init()
    run.forward()
    torch.cuda.synchronize()
    return (run.scratch if what == "scratch" else run.outputs)[key]


def test_short_scratch_is_seen(cuda):
    r = next(r for r in ROUTES if r.name == "split-K mode 0 Big")
    assert _case(r.name).confirm()[0]
    b = _short_run(r.name, "scratch", 64)  # 256 bytes short of buffer_bytes
    assert b.guards_intact() is not None, "a split-K scratch 256 bytes short must show in its guard"


def test_short_output_is_seen(cuda):
    r = next(r for r in ROUTES if r.name == "mis: 1x1 ragged planes")  # pixel-slot mode: 16-byte stores at 4-byte-aligned ends
    a = r.args
    b = _short_run(r.name, "outputs", a["w"])  # one output row short
    assert b.guards_intact() is not None, "an output one row short must show in its guard"


def test_guard_write_is_seen(cuda):
    g = Guarded(100, np.arange(100, dtype=np.float32), 1)
    assert g.guards_intact() is None
    g.raw[g.lo + 100 + 5] = 0
    assert g.guards_intact() == (105, 0)
