"""The float64 evaluator of nets that hold Padding, Crop and PixelShuffle next to any layer type create_layer accepts: the yardstick of
tests/test_frame_seams_cpu.py and tests/test_frame_seams_gpu.py.  Shaped like tests/resample_ref.Net:

  Padding, Crop, PixelShuffle   tests/frame_ref.pad / crop / pixel_shuffle (index maps that move float32 words: bit copies);
  every other layer             as tests/seam_ref.py evaluates it (float64, the blob rounded to float32).

The net is always evaluated AS WRITTEN -- Padding, then the convolution with its own pads -- never in the folded form the planner may run.

The .bin is read layer by layer: a Padding with 6=per_channel_pad_data_size holds that many raw floats where it stands in the layer list;
every other layer is read by tests/gate_ref.Net as a one-layer net from where the last one stopped (the way tests/seam_ref.py steps over
int8 layers).  `read` is the number of bytes consumed: a reader that is one float off shows there and in every layer behind it.
"""
from __future__ import annotations

import numpy as np

import frame_ref as FR
import gate_ref
import seam_ref
import shuffle_ref
from inorm_ref import plane_nerr  # noqa: F401  (the metric of the seam tests, re-exported)

FRAME_TYPES = ("Padding", "Crop", "PixelShuffle")


def frame_layer(layer, bottoms, per_channel=None):
    """One framing layer `(type, name, bottoms, tops, params)` applied to its bottoms' float32 blobs (a list): the restatement the device
    must equal bit for bit."""
    type_, _, _, _, pd = layer
    a = bottoms[0]
    if type_ == "Padding":
        return FR.pad(a, pd.get(0, 0), pd.get(1, 0), pd.get(2, 0), pd.get(3, 0), pd.get(4, 0), np.float32(pd.get(5, 0.0)), per_channel,
                      pd.get(7, 0), pd.get(8, 0))
    if type_ == "Crop":
        return FR.crop(a, pd.get(0, 0), pd.get(1, 0), pd.get(2, 0), pd.get(3, -233), pd.get(4, -233), pd.get(5, -233), pd.get(6, 0), pd.get(7, 0),
                       pd.get(8, 0), like=bottoms[1] if len(bottoms) > 1 else None)
    assert type_ == "PixelShuffle", type_
    return FR.pixel_shuffle(a, pd.get(0, 1), pd.get(1, 0))


class Net:
    def __init__(self, param: bytes, weights: bytes):
        self.layers = shuffle_ref.parse_param(param)
        rows = [r for r in param.decode().splitlines()[2:] if r.split()]
        assert len(rows) == len(self.layers)
        self.w, self.pc, self.read = {}, {}, 0
        for row, layer in zip(rows, self.layers):
            type_, name, _, _, pd = layer
            if type_ in FRAME_TYPES:
                n = pd.get(6, 0) if type_ == "Padding" else 0
                if n:
                    self.pc[name] = np.frombuffer(bytes(weights[self.read:self.read + 4 * n]), "<f4").astype(np.float32)
                    assert self.pc[name].size == n, (name, "the .bin ends inside the per-channel values")
                    self.read += 4 * n
                continue
            reader = gate_ref.Net(f"7767517\n1 1\n{row}\n".encode(), memoryview(weights)[self.read:])
            self.w.update(reader.w)
            self.read += reader.read

    def run(self, input_name, x, output_name=None, keep=False, inputs=None):
        blobs = {input_name: np.ascontiguousarray(x, np.float32)}
        for k, v in (inputs or {}).items():
            blobs[k] = np.ascontiguousarray(v, np.float32)
        for layer in self.layers:
            type_, name, bottoms, tops, pd = layer
            if type_ == "Input":
                continue
            a = blobs[bottoms[0]]
            if type_ in FRAME_TYPES:
                blobs[tops[0]] = frame_layer(layer, [blobs[b] for b in bottoms], self.pc.get(name))
            elif type_ == "Split":
                for t in tops:
                    blobs[t] = a
            elif type_ == "Slice":
                for t, y in zip(tops, shuffle_ref.channel_slice(a, pd[-23300])):
                    blobs[t] = y
            elif type_ == "Eltwise":
                assert len(bottoms) == 2 and a.shape == blobs[bottoms[1]].shape, name
                blobs[tops[0]] = a + blobs[bottoms[1]]  # float32, seam_ref's line
            elif type_ == "Concat":
                blobs[tops[0]] = np.ascontiguousarray(np.concatenate([blobs[b] for b in bottoms], axis=1))
            elif type_ == "BinaryOp" or seam_ref._gated(type_, bottoms, pd):
                b = blobs[bottoms[1]]
                gate_first = type_ == "BinaryOp" and a.shape[2:] == (1, 1) and b.shape[2:] != (1, 1)
                y = gate_ref.channel_gate(b, a) if gate_first else gate_ref.channel_gate(a, b)
                blobs[tops[0]] = np.ascontiguousarray(y, np.float32)
            else:  # one bottom, one top: seam_ref.Net.run on a net of that one layer
                assert len(bottoms) == 1 and len(tops) == 1, (type_, name)
                blobs[tops[0]] = seam_ref.Net.run(seam_ref._One(layer, self.w), bottoms[0], a, tops[0])
        return blobs if keep else blobs[output_name]
