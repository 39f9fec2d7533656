"""The zero-Padding fold (fold_zero_paddings, net_plan.h) against every plan kind of the Net runtime (tests/test_frame_seams_cpu.py,
tests/test_frame_seams_gpu.py).

The fold hands a convolution pads no .param could give it -- different on the two sides of an axis, larger than the kernel's reach -- and runs
before every other pass, so the algorithm, the epilogues, the pair, the chains and the first-layer fusion are all chosen on the folded
parameters.  Each net here is `Input [-> ...] -> zero Padding(M) -> convolution "k" [-> ...]`, the smallest shape its plan kind exists at
(tests/lifecycle_cases.py's docstring has the rules: 3-, 6-, 7/8-, 12- and 14-pixel planes, at most 72 channels), with M, as (top, bottom,
left, right), from

  (0, 1, 0, 1)  TensorFlow's SAME          (1, 0, 1, 0)  its mirror            (1, 1, 1, 1)  what turns a pad-0 layer into a pad-1 layer
  (2, 1, 3, 0)  four different sums        (3, 3, 3, 3)  beyond a 3x3's reach  (0, 2, 0, 0)  one side only

and, for the depthwise rows, (0, 0, 0, 2): with own pad 1 the layer keeps pad_left == 1, which selects depthwise3x3_direct_kernel, while the
output grows two columns past the input's right edge -- the one geometry in which that kernel's LEFT tap lies outside the row.

A row (one test id) is a list of nets; a net states its claim as `claim(level, tuned)`:
  folded     the Padding is gone from net.layers() and its top refuses Extract (level >= 2), or it stays (level 0, and the rows that exist to
             show a Padding that must stay: two readers, a reader behind a Split, a value of -0.0 whose bits are not zero)
  pads       the four pads layer "k" must report: own pads plus margins where folded
  algo       the route of layer "k", from the selection rule (fhip_conv_select_algo[_tuned]) on the input the layer sees
  gone       the layers its plan must have absorbed: the 2x2 max pooling (ConvLayer::Fuse: the fused-pool flag, visible as the missing
             Pooling layer), the residual Eltwise and ReLU, BatchNorm / Scale / ReLU, the 1x1 layer of a depthwise + pointwise pair
  pool_fast  where the pooling is fused: inside the Winograd output transform (even output, F(6,3)) or behind it (pre_pool).  The runtime
             does not report which; the column says which path the row was cut to reach (route and output parity are asserted) and the CPU
             test holds that the rows reach both
  residual   Net.residuals() of "k": 1 in the GEMM epilogue (IM2COL), 2 a launch of its own (Winograd), 0 none
  pair       Net.fused_pointwise() of "k": None, or whether the pair runs as ONE kernel (fhip_conv_can_fuse_dw_pw)
  chain      Net.chains(raw=True) of the named layers at fusion level 3
A plan the planner declines is claimed as declined, with the condition that declines it beside the row.
"""
from __future__ import annotations

import functools
import zlib

import numpy as np

from feathercnn_amd import model_zoo

MARGINS = ((0, 1, 0, 1), (1, 0, 1, 0), (1, 1, 1, 1), (2, 1, 3, 0), (3, 3, 3, 3), (0, 2, 0, 0))
LEFT_TAP = (0, 0, 0, 2)  # see the module docstring
SETTINGS = ((0, {}), (2, {}), (3, {"tuned": True}), (3, {"tuned": True, "graph": True}))
BATCHES = (4, 1)


def conv_out(size, k, s, lo, hi):
    return (size + lo + hi - k) // s + 1


def select_algo(k, s, group, cin, cout, h, w, tuned):
    """fhip_conv_select_algo / fhip_conv_select_algo_tuned and ConvLayer::LoadParam's routes, on the input plane (h, w) the layer reads."""
    if 1 < group < cin:
        return "GCONV"
    if group == cin and group > 1:
        return "DEPTHWISE"
    wino = k == 3 and s == 1 and cout % 4 == 0 and cin % 4 == 0
    if wino and h > 8 and w > 8:
        return "WINOGRADF63"
    if wino and tuned and h >= 4 and w >= 4 and 16 <= cin <= 1024:
        return "WINOGRADF63"
    return "IM2COL"


def wino_f43(oh, ow):
    """wino_f43 (winograd_f63.hip) on the output size of a 3x3 / stride-1 layer: F(4x4,3x3) on 7- and 8-pixel planes."""
    if oh < 1 or ow < 1 or oh > 8 or ow > 8 or (oh < 7 and ow < 7):
        return False
    return ((oh + 3) // 4) * ((ow + 3) // 4) * 36 < ((oh + 5) // 6) * ((ow + 5) // 6) * 64


class FoldNet:
    """Input (cin, plane) [-> head] -> Padding(M, value) -> "k" [-> tail]."""

    def __init__(self, row, plane, cin, m, k, s=1, p=0, group=1, cout=None, tail=None, head=None, folds=True, value=None, readers="one"):
        self.row, self.plane, self.cin, self.m = row, plane, cin, tuple(m)
        self.k, self.s, self.p, self.group, self.cout = k, s, p, group, cout or cin
        self.tail, self.head, self.folds, self.value, self.readers = tail, head, folds, value, readers
        self.id = f"{row}@{plane[0]}x{plane[1]}/M{''.join(map(str, m))}"

    # ---- geometry ----
    def padded(self):
        t, b, l, r = self.m
        return self.plane[0] + t + b, self.plane[1] + l + r

    def out_plane(self):
        t, b, l, r = self.m
        return conv_out(self.plane[0], self.k, self.s, self.p + t, self.p + b), conv_out(self.plane[1], self.k, self.s, self.p + l, self.p + r)

    def exists(self):
        oh, ow = self.out_plane()
        return oh >= 1 and ow >= 1

    # ---- the model ----
    @functools.lru_cache(maxsize=None)
    def model(self):
        """-> (param, weights, outputs)."""
        g = model_zoo.GraphBuilder(zlib.crc32(f"{self.id}/{SALT.get(self.id, 0)}".encode()) % (1 << 31))
        h, w = self.plane
        x = g.input("data", self.cin, h, w)
        other = None
        if self.tail == "residual":  # the other operand first: the residual rule adds an EARLIER blob
            x, y = g.split("tap", x)
            ph, pw = self.out_plane()
            assert (ph, pw) == (h, w), self.id
            other = g.conv("br", y, self.cin, self.cout, 1)
        if self.head == "conv3x3p1":
            x = g.conv("a", x, self.cin, self.cin, 3, 1, 1)
        t, b, l, r = self.m
        x = g.padding("pad", x, t, b, l, r, value=self.value)
        outputs = []
        if self.readers == "two":
            outputs.append(g.conv("k2", x, self.cin, self.cout, self.k, self.s, self.p, group=self.group))
        elif self.readers == "split":
            x, x2 = g.split("fork", x)
            outputs.append(g.conv("k2", x2, self.cin, self.cout, self.k, self.s, self.p, group=self.group))
        x = g.conv("k", x, self.cin, self.cin if self.group == self.cin and self.group > 1 else self.cout, self.k, self.s, self.p, group=self.group)
        kout = self.cin if self.group == self.cin and self.group > 1 else self.cout
        if self.tail == "pool":
            x = g.pool("pool", x, 2, 2, 0)
        elif self.tail == "residual":
            x = g.relu("relu", g.eltwise("sum", x, other))
        elif self.tail == "bn":
            x = g.relu("relu", g.scale("scale", g.bn("bn", x, kout), kout))
        elif self.tail == "pw72":
            x = g.conv("pw", x, kout, 72, 1)
        elif self.tail == "conv3x3p1":
            x = g.conv("b", x, kout, kout, 3, 1, 1)
        outputs.append(x)
        param, weights = g.finish()
        return param, weights, tuple(outputs)

    def input(self, batch):
        seed = zlib.crc32(f"{self.id}/x/{SALT.get(self.id, 0)}".encode())
        return np.random.default_rng(seed).normal(0, 1, (max(BATCHES), self.cin) + self.plane).astype(np.float32)[:batch]

    # ---- the claim ----
    def claim(self, level, tuned=False):
        t, b, l, r = self.m
        folded = self.folds and level >= 2
        own = (self.p,) * 4
        pads = (self.p + t, self.p + b, self.p + l, self.p + r) if folded else own
        seen = self.plane if folded else self.padded()  # the plane layer "k" reads
        kout = self.cin if self.group == self.cin and self.group > 1 else self.cout
        algo = select_algo(self.k, self.s, self.group, self.cin, kout, seen[0], seen[1], tuned)
        oh, ow = self.out_plane()
        c = dict(folded=folded, pads=pads, algo=algo, gone=[], pool_fast=None, residual=0, pair=None, chain={})
        main = algo not in ("GCONV",)  # the side routes take ReLU and affine epilogues only (side_epilogues_only)
        if self.tail == "pool" and level >= 2 and main:
            c["gone"] = ["pool"]
            c["pool_fast"] = algo == "WINOGRADF63" and not wino_f43(oh, ow) and oh % 2 == 0 and ow % 2 == 0  # fhip_conv_can_fuse_maxpool2
        if self.tail == "residual" and level >= 2:
            c["gone"] = ["sum", "relu"]
            c["residual"] = 1 if algo == "IM2COL" else 2  # fhip_conv_can_fuse_residual: the GEMM epilogue is IM2COL's
        if self.tail == "bn" and level >= 2:
            c["gone"] = ["bn", "scale", "relu"]
        if self.tail == "pw72" and level >= 2:
            # ConvLayer::Fuse: depthwise 3x3, stride 1 or 2, pad_left == 1 and pad_top == 1 (it looks at two of the four pads) and 64 < K < 160;
            # one kernel where dwpw_applicable holds: W % 4 == 0, OW % 4 == 0 and OW * s == W (which pins the right pad), any bottom pad
            if pads[0] == 1 and pads[2] == 1:
                c["gone"] = ["pw"]
                c["pair"] = self.plane[1] % 4 == 0 and ow % 4 == 0 and ow * self.s == self.plane[1]
        if level >= 3 and tuned:
            k_plain = algo == "WINOGRADF63" and not wino_f43(oh, ow)
            if self.head == "conv3x3p1" and k_plain and pads == (1, 1, 1, 1):
                c["chain"] = {"a": (0, 1), "k": (1, 0)}  # plan_chains: `next` must be pad 1 all round -- which the fold makes it
            if self.tail == "conv3x3p1":
                b_plain = select_algo(3, 1, 1, kout, kout, oh, ow, tuned) == "WINOGRADF63" and not wino_f43(oh, ow)
                if k_plain and b_plain:
                    c["chain"] = {"k": (0, 1), "b": (1, 0)}  # winograd_can_chain looks at the pads of `next` only: a folded head chains
                elif b_plain and 2 <= self.cin <= 4 and (self.k, self.s, self.group) == (3, 1, 1) and pads == (1, 1, 1, 1) and self.plane[1] % 2 == 0:
                    c["chain"] = {"k": (0, 2), "b": (2, 0)}  # first_candidate: pad 1 all round after the fold; winograd_can_fuse_first: an even width
        return c


def _all_m(row, plane, cin, margins=MARGINS, **kw):
    nets = [FoldNet(row, plane, cin, m, **kw) for m in margins]
    return [n for n in nets if n.exists()]


DW_M = MARGINS + (LEFT_TAP,)
ROWS = {
    # 3x3 stride 1, own pad 0 and 1: 12 x 14 is F(6,3) with or without tuned selection; 6 x 7 is IM2COL untuned and, tuned, F(4,3) or F(6,3) by
    # the folded output (7 .. 8 pixels: F(4,3)); a 3-pixel side keeps IM2COL under tuned selection (input_h >= 4)
    "c3s1p0_f63": _all_m("c3s1p0_f63", (12, 14), 16, k=3, p=0), "c3s1p1_f63": _all_m("c3s1p1_f63", (12, 14), 16, k=3, p=1),
    "c3s1p0_f43": _all_m("c3s1p0_f43", (6, 7), 16, k=3, p=0), "c3s1p1_f43": _all_m("c3s1p1_f43", (6, 7), 16, k=3, p=1),
    "c3s1p0_im2col": _all_m("c3s1p0_im2col", (3, 4), 16, k=3, p=0), "c3s1p1_im2col": _all_m("c3s1p1_im2col", (3, 4), 16, k=3, p=1),
    "c3s2p0": _all_m("c3s2p0", (12, 14), 16, k=3, s=2, p=0),
    "c5p2": _all_m("c5p2", (8, 7), 16, k=5, p=2),
    # 77 pixels per plane: ragged 1x1 columns (ragged_1x1: OHW % 4 != 0, 16 | C, 32 | K) -- which the folded layer, a 1x1 with pads, must leave
    "c1s1_ragged": _all_m("c1s1_ragged", (7, 11), 16, k=1, cout=32), "c1s2": _all_m("c1s2", (7, 11), 16, k=1, s=2, cout=32),
    # depthwise: 14 x 12 (W % 4 == 0: 16-byte vectors; unfolded and pad 1 the flat kernel) and 7 x 9 (odd: scalar lanes, the chunk kernel at stride 2)
    "dw3s1p1": _all_m("dw3s1p1", (14, 12), 16, DW_M, k=3, p=1, group=16) + _all_m("dw3s1p1", (7, 9), 16, DW_M, k=3, p=1, group=16),
    "dw3s1p0": _all_m("dw3s1p0", (14, 12), 16, DW_M, k=3, p=0, group=16) + _all_m("dw3s1p0", (7, 9), 16, DW_M, k=3, p=0, group=16),
    "dw3s2p1": _all_m("dw3s2p1", (14, 12), 16, DW_M, k=3, s=2, p=1, group=16) + _all_m("dw3s2p1", (7, 9), 16, DW_M, k=3, s=2, p=1, group=16),
    "dw3s2p0": _all_m("dw3s2p0", (14, 12), 16, DW_M, k=3, s=2, p=0, group=16) + _all_m("dw3s2p0", (7, 9), 16, DW_M, k=3, s=2, p=0, group=16),
    "g4c3p1": _all_m("g4c3p1", (7, 9), 16, k=3, p=1, group=4),
    # the pair: (0, 2, 0, 0) keeps OW * s == W while the bottom pad is 3 (one kernel); (0, 1, 0, 1) on stride 2 makes pad_right 2, OW * 2 != W
    # (two kernels); (1, 1, 1, 1) on an own pad of 0 MAKES a pair; (1, 0, 1, 0) on own pad 1 gives pad_left 2: no pair
    "dwpw": [FoldNet("dwpw_s1", (6, 8), 16, (0, 2, 0, 0), k=3, p=1, group=16, tail="pw72"), FoldNet("dwpw_s2", (6, 8), 16, (0, 1, 0, 1), k=3, s=2, p=1, group=16, tail="pw72"),
             FoldNet("dwpw_made", (6, 8), 16, (1, 1, 1, 1), k=3, p=0, group=16, tail="pw72"), FoldNet("dwpw_lost", (6, 8), 16, (1, 0, 1, 0), k=3, p=1, group=16, tail="pw72")],
    # 12 x 12 and own pad 1: (0, 1, 0, 1) gives a 13-pixel output (odd: pre_pool and fhip_pooling), (1, 1, 1, 1) a 14-pixel one (inside the transform),
    # (0, 2, 0, 1) 14 x 13; on 6 x 6 the layer is IM2COL, or F(4,3) under tuned selection: neither has a pooled transform
    "pool": [FoldNet("pool_odd", (12, 12), 16, (0, 1, 0, 1), k=3, p=1, tail="pool"), FoldNet("pool_even", (12, 12), 16, (1, 1, 1, 1), k=3, p=1, tail="pool"),
             FoldNet("pool_mixed", (12, 12), 16, (0, 2, 0, 1), k=3, p=1, tail="pool"), FoldNet("pool_im2col", (6, 6), 16, (0, 1, 0, 1), k=3, p=1, tail="pool")],
    "residual": [FoldNet("res", (7, 9), 16, (1, 1, 1, 1), k=3, p=0, tail="residual"), FoldNet("res", (12, 14), 16, (1, 1, 1, 1), k=3, p=0, tail="residual"),
                 FoldNet("res5", (7, 9), 16, (0, 2, 2, 0), k=5, p=1, tail="residual")],
    "bn_scale_relu": [FoldNet("bn", (7, 9), 16, m, k=3, p=0, tail="bn") for m in ((1, 1, 1, 1), (0, 1, 0, 1), (2, 1, 3, 0))],
    # conv3x3 p1 -> Padding (1, 1, 1, 1) -> conv3x3 p0 at level 3 tuned on a 12-pixel plane: the fold makes a chain; with (0, 1, 0, 1) it makes none
    "chain_made": [FoldNet("chain", (12, 12), 16, (1, 1, 1, 1), k=3, p=0, head="conv3x3p1"), FoldNet("chain", (12, 12), 16, (0, 1, 0, 1), k=3, p=0, head="conv3x3p1")],
    # Padding (0, 1, 0, 1) -> conv3x3 p1 -> conv3x3 p1: the head of a chain with pads (1, 2, 1, 2)
    "chain_head": [FoldNet("chain_head", (12, 12), 16, m, k=3, p=1, tail="conv3x3p1") for m in ((0, 1, 0, 1), (2, 1, 3, 0))],
    # Input (3 channels) -> Padding (1, 1, 1, 1) -> conv3x3 p0 (3 -> 16) -> conv3x3 p1: the fold makes a first-layer candidate; 12 x 13 has an odd
    # width, which winograd_can_fuse_first declines (float2 image reads)
    "first_layer": [FoldNet("first", (12, 12), 3, (1, 1, 1, 1), k=3, p=0, cout=16, tail="conv3x3p1"), FoldNet("first", (12, 13), 3, (1, 1, 1, 1), k=3, p=0, cout=16, tail="conv3x3p1"),
                    FoldNet("first", (12, 12), 3, (0, 1, 0, 1), k=3, p=0, cout=16, tail="conv3x3p1")],
    # a Padding that must stay: two readers of its top, one reader behind a Split, and a value of -0.0 (bits 0x80000000: zero_pad_margins compares bits)
    "kept": [FoldNet("two_readers", (7, 9), 16, (1, 1, 1, 1), k=3, p=0, folds=False, readers="two"), FoldNet("behind_split", (7, 9), 16, (1, 1, 1, 1), k=3, p=0, folds=False, readers="split"),
             FoldNet("minus_zero", (7, 9), 16, (1, 1, 1, 1), k=3, p=0, folds=False, value=-0.0), FoldNet("minus_zero", (12, 14), 16, (0, 1, 0, 1), k=3, s=2, p=0, folds=False, value=-0.0)],
}

# Nets whose first draw left an output plane below 1e-3 of the tensor's maximum in the float64 result (tests/seam_cases.py's SALT rule): drawn
# again with this salt, the first that lifts the smallest plane to 2e-2 of the maximum.
SALT = {}


def nets():
    return [n for row in ROWS.values() for n in row]
