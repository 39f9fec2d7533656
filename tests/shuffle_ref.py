"""Restatement of ncnn's ShuffleChannel and Slice, of the channel map that composes them with Concat, and of whole nets that hold such
layers: the yardstick of tests/test_shuffle_cpu.py and tests/test_shuffle_gpu.py.

`channel_shuffle`, `channel_slice` and `apply_map` are the definitions of include/feather_hip/feather_shuffle.h written with numpy indexing:
they only move values, so the GPU tests compare bit for bit.  `compose` builds a channel-map table from a list of steps the way the runtime
does at fusion level 2, independently of it.  `Net` runs every other layer as tests/inorm_ref.py's Net does (float64, rounded to float32
per blob).
"""
from __future__ import annotations

import re

import numpy as np

import inorm_ref
from gconv_ref import nerr  # noqa: F401  (the project's parity metric, re-exported)

SHARE = -233
MAP_TYPES = ("ShuffleChannel", "Slice")


def shuffle_order(c: int, group: int, reverse: bool = False) -> np.ndarray:
    """order[o] = the input channel that output channel o takes: o = i * group + k  <-  k * (c / group) + i; reverse: the inverse."""
    if group < 1 or c % group:
        raise ValueError(f"group {group} does not divide {c} channels")
    order = np.arange(c).reshape(group, c // group).T.reshape(-1)
    if reverse:
        inv = np.empty(c, np.int64)
        inv[order] = np.arange(c)
        return inv
    return order


def channel_shuffle(x, group: int, reverse: bool = False) -> np.ndarray:
    x = np.asarray(x)
    return np.ascontiguousarray(x[:, shuffle_order(x.shape[1], group, reverse)])


def slice_sizes(c: int, sizes) -> list:
    """ncnn's rule: -233 is an equal share of what is left, (c - used) / (entries left)."""
    out, used = [], 0
    if not len(sizes):
        raise ValueError("a slice needs at least one size")
    for j, s in enumerate(sizes):
        if s == SHARE:
            s = (c - used) // (len(sizes) - j)
        if s < 1:
            raise ValueError(f"slice size {s} of {list(sizes)} on {c} channels")
        used += s
        if used > c:
            raise ValueError(f"slice sizes {list(sizes)} need more than {c} channels")
        out.append(int(s))
    return out


def channel_slice(x, sizes) -> list:
    x = np.asarray(x)
    res, at = [], 0
    for s in slice_sizes(x.shape[1], sizes):
        res.append(np.ascontiguousarray(x[:, at:at + s]))
        at += s
    return res


def apply_map(srcs, tables) -> list:
    """tables[j][r] = (source index, source channel) of channel r of output j."""
    return [np.stack([np.asarray(srcs[s])[:, c] for s, c in t], axis=1) for t in tables]


def compose(src_channels, steps, outputs):
    """Channel-map tables of a chain.  Blobs are named: sources are "s0", "s1", ...; each step is ("concat", [bottoms], top),
    ("shuffle", bottom, top, group, reverse) or ("slice", bottom, [tops], sizes).  -> one table per name in `outputs`."""
    rows = {f"s{i}": [(i, ch) for ch in range(c)] for i, c in enumerate(src_channels)}
    for st in steps:
        if st[0] == "concat":
            rows[st[2]] = [e for b in st[1] for e in rows[b]]
        elif st[0] == "shuffle":
            src = rows[st[1]]
            rows[st[2]] = [src[i] for i in shuffle_order(len(src), st[3], st[4])]
        else:
            src, at = rows[st[1]], 0
            for top, s in zip(st[2], slice_sizes(len(src), st[3])):
                rows[top] = src[at:at + s]
                at += s
    return [rows[o] for o in outputs]


_ARRAY = re.compile(rb"(?<=\s)-233\d\d=\S+")


def parse_param(text: bytes):
    """oracle.netcheck.parse_param plus ncnn's array params: `-233xx=count,v0,v1,...` becomes pd[-233xx] = [v0, v1, ...]."""
    from oracle.netcheck import parse_param as scalar_params
    layers = scalar_params(_ARRAY.sub(b"", text))
    tok = text.decode().split()
    arrays, t = [], 3
    for type_, _, bottoms, tops, _ in layers:
        t += 4 + len(bottoms) + len(tops)
        found = {}
        while t < len(tok) and "=" in tok[t] and tok[t].split("=")[0].lstrip("-").isdigit():
            k, v = tok[t].split("=", 1)
            if int(k) <= -23300:
                parts = v.split(",")
                assert int(parts[0]) == len(parts) - 1, tok[t]
                found[int(k)] = [int(p) for p in parts[1:]]
            t += 1
        arrays.append(found)
    return [(ty, nm, b, tp, {**pd, **arr}) for (ty, nm, b, tp, pd), arr in zip(layers, arrays)]


class Net(inorm_ref.Net):
    """inorm_ref.Net plus ShuffleChannel and Slice."""

    def __init__(self, param: bytes, weights: bytes):
        super().__init__(_ARRAY.sub(b"", param), weights)  # neither layer has weights
        self.layers = parse_param(param)

    def run(self, input_name: str, x: np.ndarray, output_name: str, keep: bool = False):
        blobs = {input_name: np.ascontiguousarray(x, np.float32)}
        all_layers = self.layers
        try:
            for layer in all_layers:
                type_, _, bottoms, tops, pd = layer
                if type_ == "Input":
                    continue
                if type_ == "ShuffleChannel":
                    blobs[tops[0]] = channel_shuffle(blobs[bottoms[0]], pd.get(0, 1), bool(pd.get(1, 0)))
                elif type_ == "Slice":
                    assert pd.get(1, 0) == 0 and len(pd[-23300]) == len(tops)
                    for t, y in zip(tops, channel_slice(blobs[bottoms[0]], pd[-23300])):
                        blobs[t] = y
                else:
                    if len(bottoms) == 1 and type_ != "Split":
                        self.layers = [layer]
                        out = inorm_ref.Net.run(self, bottoms[0], blobs[bottoms[0]], tops[0], keep=True)
                    else:
                        out = self._many(layer, blobs)
                    for t in tops:
                        blobs[t] = out[t]
        finally:
            self.layers = all_layers
        return blobs if keep else blobs[output_name]

    def _many(self, layer, blobs):
        """A layer with several bottoms or tops (Concat, Eltwise, Split): inorm_ref.Net.run reads them from its own blob table, which
        starts from one input; restated here on ours."""
        type_, _, bottoms, tops, _ = layer
        if type_ == "Concat":
            return {tops[0]: np.ascontiguousarray(np.concatenate([blobs[b] for b in bottoms], axis=1), np.float32)}
        if type_ == "Eltwise":
            return {tops[0]: (blobs[bottoms[0]].astype(np.float64) + blobs[bottoms[1]]).astype(np.float32)}
        assert type_ == "Split", type_
        return {t: blobs[bottoms[0]] for t in tops}
