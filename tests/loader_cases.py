"""Hostile-model cases for the .param / .bin readers (feathercnn_amd/csrc/net_model.h, net_layers.h, net.hip): a deterministic table, no test code.

``cases()`` returns a list of ``Case`` tuples ``(name, param, bin, expectation, code, dilated)``:

* ``expectation`` -- ``ACCEPT``: an unmodified base model, both loads return 0 (the control: the harness can load a model);
  ``REFUSE``: the param load or, after a param load that returned 0, the weight load returns a non-zero code and leaves a message in
  fhip_last_error(); ``EITHER``: the calls may refuse or load, the process has to return normally.
* ``code`` -- for a ``REFUSE`` case whose code the reference's source settles (paths relative to its src/, cited where the case is
  made): the code the refusing call must return.  ``None`` where the reference has no check of its own.
* ``dilated`` -- the net gets fhip_net_set_dilated before the param load (models that hold dilated convolutions).

A case is ``REFUSE`` only where the file is malformed whatever a later stage makes of it: a count that cannot be one, a size that no
file of that length can hold, a record whose declared length disagrees with its content, a value outside the layer's definition that is
known when the param is read.  What only the fed shape can decide (a slope count against the channels of the bottom, slice sizes against
the channel count, a pooling stride of 0, which Reshape refuses) is ``EITHER`` here: Reshape may allocate on a device and is not run.
"""
from __future__ import annotations

import copy
from typing import NamedTuple, Optional

from feathercnn_amd import model_zoo
from oracle import netcheck

ACCEPT, REFUSE, EITHER = "accept", "refuse", "either"
INT_VALUES = (0, -1, 2147483647, -2147483648)
FLOAT_VALUES = ("nan", "inf", "1e39")

# type -> (integer ids, float ids, array ids) its LoadParam reads; tests/test_loader_hostile_cpu.py holds this table against the LoadParam bodies of net_layers.h
_CONV = ((0, 1, 11, 2, 12, 3, 13, 4, 14, 5, 6, 7, 8), (), ())
_DECONV = ((0, 1, 11, 2, 12, 3, 13, 4, 14, 15, 16, 18, 19, 20, 21, 5, 6, 7, 8, 9), (), ())
PARAM_IDS = {
    "Input": ((), (), ()), "Convolution": _CONV, "ConvolutionDepthWise": _CONV, "Deconvolution": _DECONV, "DeconvolutionDepthWise": _DECONV,
    "ReLU": ((), (0,), ()), "InstanceNorm": ((0, 2), (1,), ()), "PReLU": ((0,), (), ()), "Sigmoid": ((), (), ()), "TanH": ((), (), ()),
    "Clip": ((), (0, 1), ()), "Pooling": ((0, 1, 11, 2, 12, 3, 13, 14, 15, 4), (), ()), "InnerProduct": ((0, 1, 2), (), ()),
    "Dropout": ((), (0,), ()), "Softmax": ((), (), ()), "BatchNorm": ((0,), (1,), ()), "Scale": ((0, 1), (), ()), "Split": ((), (), ()),
    "Eltwise": ((0,), (), (1,)), "Concat": ((0,), (), ()), "ShuffleChannel": ((0, 1), (), ()), "Slice": ((1,), (), (0,)),
    "BinaryOp": ((0, 1), (), ()), "Swish": ((), (), ()), "HardSigmoid": ((), (0, 1), ()),
}


class Case(NamedTuple):
    name: str
    param: bytes
    bin: bytes
    expectation: str
    code: Optional[int] = None
    dilated: bool = False


class Model(NamedTuple):
    tag: str
    param: bytes
    bin: bytes
    dilated: bool


class _Layer:
    def __init__(self, type_, name, nb, nt, bottoms, tops, pairs):
        self.type, self.name, self.nb, self.nt, self.bottoms, self.tops, self.pairs = type_, name, nb, nt, bottoms, tops, pairs

    def tokens(self):
        return [self.type, self.name, self.nb, self.nt] + self.bottoms + self.tops + self.pairs

    def set(self, key, value):
        """`key=value`, in place of the pair with that key if the layer has one."""
        pair = f"{key}={value}"
        for i, p in enumerate(self.pairs):
            if p.split("=")[0] == str(key):
                self.pairs[i] = pair
                return
        self.pairs.append(pair)


def _parse(param: bytes):
    tok = param.decode().split()
    header, t, layers = tok[:3], 3, []
    for _ in range(int(tok[1])):
        nb, nt = int(tok[t + 2]), int(tok[t + 3])
        e = t + 4 + nb + nt
        pairs = []
        while e < len(tok) and "=" in tok[e]:
            pairs.append(tok[e])
            e += 1
        layers.append(_Layer(tok[t], tok[t + 1], tok[t + 2], tok[t + 3], tok[t + 4:t + 4 + nb], tok[t + 4 + nb:t + 4 + nb + nt], pairs))
        t = e
    assert t == len(tok)
    return header, layers


def _render(header, layers) -> bytes:
    return (header[0] + "\n" + " ".join(header[1:]) + "\n" + "".join(" ".join(l.tokens()) + "\n" for l in layers)).encode()


def _extras():
    """The reader branches no zoo model takes: a leaky ReLU, InstanceNorm without affine, one shared PReLU slope, a reversed shuffle, a Slice
    with -233 shares, a Dropout without a scale, HardSigmoid and a two-bottom Scale outside an SE block."""
    g = model_zoo.GraphBuilder(31)
    x = g.input("data", 8, 6, 6)
    x = g.relu("leaky", x, slope=0.1)
    x = g.instance_norm("in_plain", x, 8, affine=False)
    x = g.prelu("prelu_shared", x, 1)
    x = g.shuffle("unshuffle", x, 2, reverse=True)
    a, b, c = g.slice("thirds", x, [2, -233, -233])
    b = g.dropout("drop_identity", b)
    x = g.concat("cat", [a, b, c])
    keep, sq = g.split("sp", x)
    gate = g.hard_sigmoid("hs", g.pool("gap", sq, 1, 1, avg=True, global_=True))
    x = g.scale_by("gated", keep, gate)
    x = g.clip("clip", x, -1.0, 1.0)
    return g.finish() + ("data", "clip")


def base_models():
    zoo = [("tiny_allsorts", model_zoo.tiny_allsorts, False), ("tiny_grouped", model_zoo.tiny_grouped, False), ("tiny_deconv", model_zoo.tiny_deconv, False),
           ("tiny_generative", model_zoo.tiny_generative, False), ("tiny_shuffle", model_zoo.tiny_shuffle, False),
           ("tiny_dilated", model_zoo.tiny_dilated, True), ("tiny_se", model_zoo.tiny_se, False), ("extras", _extras, False)]
    out = []
    for tag, fn, dilated in zoo:
        p, b, _, _ = fn()
        out.append(Model(tag, p, b, dilated))
    return out


def base_types(models=None):
    return {l.type for m in (models or base_models()) for l in _parse(m.param)[1]}


# ---- expectations of the value cases -----------------------------------------------------------------------------------------------------
def _value_rule(type_, layer, key, v, dilated):
    """(expectation, code) of `key=v` on a layer of `type_`; see the module docstring for what makes a REFUSE."""
    big = v == 2147483647
    if type_ in ("Convolution", "ConvolutionDepthWise"):
        if key in (0, 1, 11, 7) and v <= 0:
            return REFUSE, None                      # no outputs, an empty kernel, no groups
        if key == 7 and big:
            return REFUSE, None                      # a group that does not divide num_output
        if key == 6 and v != 0:
            return REFUSE, None                      # negative, or more weights than any file of this length holds
        if key == 8:
            return (REFUSE, -200) if v else (EITHER, None)   # conv_layer.h:49-54 (int8)
        if key in (2, 12):
            if big and not dilated:
                return REFUSE, -200                  # conv_layer.h:43-47
            return (REFUSE, None) if v <= 0 else (EITHER, None)
        return EITHER, None
    if type_ in ("Deconvolution", "DeconvolutionDepthWise"):
        if key in (0, 1, 11, 3, 13, 7, 6) and v <= 0:
            return REFUSE, None
        if key in (6, 7) and big:
            return REFUSE, None
        if key in (2, 12):
            return REFUSE, None                      # every value here is a dilation other than 1
        if key in (8, 9, 20, 21) and v:
            return REFUSE, None                      # int8, built-in activation, explicit output size: not this layer's definition
        if key in (4, 14, 15, 16, 18, 19) and v < 0:
            return REFUSE, None
        return EITHER, None
    if type_ == "InnerProduct":
        if key == 0 or (key == 2 and v != 0):
            return REFUSE, None                      # no rows; rows that do not divide the weights; weights the file cannot hold
        return EITHER, None
    if type_ == "InstanceNorm" and key == 0:
        return REFUSE, None                          # no channels, or (affine) more gammas than the file holds
    if type_ == "PReLU" and key == 0:
        return REFUSE, None
    if type_ == "BatchNorm" and key == 0 and v != 0:
        return REFUSE, None
    if type_ == "Scale" and key == 0 and v != 0:
        return (REFUSE, -100) if v < 0 else (REFUSE, None)   # scale_layer.h:37-41
    if type_ == "Eltwise" and key == 0:
        return REFUSE, -100                          # eltwise_layer.h:62-66: every value here is an op other than SUM
    if type_ == "Concat" and key == 0 and v != 0:
        return REFUSE, None                          # concat_layer.h:70-73 refuses the axis at Reshape; it is known here
    if type_ == "ShuffleChannel" and key == 0 and v <= 0:
        return REFUSE, None
    if type_ == "Slice" and key == 1 and v != 0:
        return REFUSE, None
    if type_ == "BinaryOp" and (key == 0 or v != 0):
        return REFUSE, None                          # only 0=2 (mul) without a scalar operand
    return EITHER, None


def _float_rule(type_, key, v):
    # "nan" and "inf" hold none of '.', 'e': ParamDict reads them as the integer 0 (paramdict.cpp:158-171); 1e39 overflows fp32 to +inf
    if v == "1e39" and (type_ == "HardSigmoid" or (type_ == "Clip" and key == 0)):
        return REFUSE, None                          # a non-finite HardSigmoid coefficient; Clip with min = +inf above its max
    return EITHER, None


# ---- the table -----------------------------------------------------------------------------------------------------------------------------
def cases():
    models = base_models()
    parsed = {m.tag: _parse(m.param) for m in models}
    out = []

    def add(name, param, bin_, expectation, code=None, dilated=False):
        out.append(Case(name, param, bin_, expectation, code, dilated))

    def mutated(m, index, fn):
        header, layers = parsed[m.tag]
        layers = copy.deepcopy(layers)
        fn(layers[index])
        return _render(header, layers)

    for m in models:
        assert _render(*parsed[m.tag]).split() == m.param.split()
        add(f"{m.tag}/accept", m.param, m.bin, ACCEPT, None, m.dilated)

    # one representative layer per type: its first appearance; Convolution also on the grouped and on the dilated route
    reps = {}
    for m in models:
        for i, l in enumerate(parsed[m.tag][1]):
            reps.setdefault(l.type, (m, i))
            pd = dict(p.split("=") for p in l.pairs)
            if l.type == "ConvolutionDepthWise" and m.tag == "tiny_grouped" and 1 < int(pd.get("7", 1)) < int(pd["0"]):
                reps.setdefault("ConvolutionDepthWise:grouped", (m, i))
            if l.type == "Convolution" and "2" in pd:
                reps.setdefault("Convolution:dilated", (m, i))

    # structural cases
    for key, (m, i) in reps.items():
        if ":" in key:
            continue
        layers = parsed[m.tag][1]
        l = layers[i]
        known = {t for k in layers[:i] for t in k.tops}
        is_input = l.type == "Input"
        tag = f"{m.tag}/{l.type}/{l.name}"

        def case(what, fn, expectation, code=None):
            add(f"{tag}/{what}", mutated(m, i, fn), m.bin, expectation, code, m.dilated)

        if not is_input:
            case("bottom_count_0", lambda x: setattr(x, "nb", "0"), REFUSE)
            case("unknown_bottom", lambda x: x.bottoms.__setitem__(0, "no_such_blob"), REFUSE, -300)                          # net.cpp:127-132
            fresh = l.tops[0] not in known
            case("own_top_as_bottom", lambda x: x.bottoms.__setitem__(0, x.tops[0]), REFUSE if fresh else EITHER, -300 if fresh else None)  # net.cpp:127-132
            # the first top is read as one more bottom
            case("bottom_count_plus_1", lambda x: setattr(x, "nb", str(len(x.bottoms) + 1)), REFUSE if fresh else EITHER, -300 if fresh else None)
            case("top_in_use", lambda x: x.tops.__setitem__(0, sorted(known)[0]), EITHER)                                     # net.cpp:149-150 replaces the map entry
        else:
            case("bottom_count_plus_1", lambda x: setattr(x, "nb", "1"), EITHER)                                              # net.cpp:128 exempts Input
        case("bottom_count_-1", lambda x: setattr(x, "nb", "-1"), REFUSE)
        case("bottom_count_text", lambda x: setattr(x, "nb", "two"), EITHER if is_input else REFUSE)                           # read as 0
        case("top_count_0", lambda x: setattr(x, "nt", "0"), REFUSE)
        case("top_count_text", lambda x: setattr(x, "nt", "one"), REFUSE)
    for m in models:
        header, layers = parsed[m.tag]
        n = len(layers)
        for what, h, expectation, code in (("layer_count_plus_1", [header[0], str(n + 1), header[2]], REFUSE, None),
                                           ("layer_count_minus_1", [header[0], str(n - 1), header[2]], EITHER, None),
                                           ("layer_count_0", [header[0], "0", header[2]], REFUSE, -1),                        # net.cpp:78-83
                                           ("layer_count_text", [header[0], "many", header[2]], REFUSE, -1),                  # net.cpp:78-83
                                           ("blob_count_0", [header[0], header[1], "0"], REFUSE, -1),                         # net.cpp:78-83
                                           ("blob_count_text", [header[0], header[1], "some"], REFUSE, -1),                   # net.cpp:78-83
                                           ("magic_old", ["7767516", header[1], header[2]], REFUSE, -1)):                     # utils.cpp:37-41
            add(f"{m.tag}/{what}", _render(h, layers), m.bin, expectation, code, m.dilated)

    # value cases
    for key, (m, i) in reps.items():
        l = parsed[m.tag][1][i]
        ints, floats, arrays = PARAM_IDS[l.type]
        tag = f"{m.tag}/{key}/{l.name}"
        for k in ints:
            for v in INT_VALUES:
                expectation, code = _value_rule(l.type, l, k, v, m.dilated)
                add(f"{tag}/{k}={v}", mutated(m, i, lambda x: x.set(k, v)), m.bin, expectation, code, m.dilated)
        for k in floats:
            for v in FLOAT_VALUES:
                expectation, code = _float_rule(l.type, k, v)
                add(f"{tag}/{k}={v}", mutated(m, i, lambda x: x.set(k, v)), m.bin, expectation, code, m.dilated)
        if ":" in key:
            continue
        for k in arrays:
            # paramdict.cpp:121-128 (an element that is not there) and :110-116 return -1 through net.cpp:154-159
            for what, value, code in (("len_larger", "4,2,3", -1), ("len_smaller", "1,2,3", None), ("len_negative", "-1,2,3", None),
                                      ("len_huge_no_values", "100000000", -1), ("len_int_max", "2147483647,1", -1)):
                add(f"{tag}/array{k}_{what}", mutated(m, i, lambda x: x.set(-23300 - k, value)), m.bin, REFUSE, code, m.dilated)
        add(f"{tag}/array_id_32", mutated(m, i, lambda x: x.pairs.append("-23332=1,2")), m.bin, REFUSE, None, m.dilated)
        if l.type in ("Input", "Slice", "Clip"):  # the id itself past int and past long long: the same parser for every layer type
            for what, pair in (("id_llong_min", "-9223372036854775808=1,2"), ("id_llong_max", "9223372036854775807=1"),
                               ("id_past_llong", "-99999999999999999999999=1,2"), ("id_int_min", "-2147483648=1,2"), ("id_negative", "-5=1")):
                add(f"{tag}/{what}", mutated(m, i, lambda x: x.pairs.append(pair)), m.bin, REFUSE, None, m.dilated)
        add(f"{tag}/empty_value", mutated(m, i, lambda x: x.pairs.append("5=")), m.bin, REFUSE, -1, m.dilated)              # paramdict.cpp:152-168

    # semantic cases
    def semantic(what, type_key, fn, expectation, code=None):
        m, i = reps[type_key]
        l = parsed[m.tag][1][i]
        add(f"{m.tag}/{type_key}/{l.name}/{what}", mutated(m, i, fn), m.bin, expectation, code, m.dilated)

    for t in ("Convolution", "ConvolutionDepthWise", "ConvolutionDepthWise:grouped", "Convolution:dilated", "Deconvolution", "DeconvolutionDepthWise"):
        deconv = t.startswith("Deconv")
        semantic("group_0", t, lambda x: x.set(7, 0), REFUSE)
        semantic("group_not_dividing", t, lambda x: x.set(7, 7), REFUSE)               # no representative has a multiple of 7 outputs
        semantic("kernel_0", t, lambda x: x.set(1, 0), REFUSE)
        semantic("dilation_0", t, lambda x: x.set(2, 0), REFUSE)
        semantic("stride_0", t, lambda x: x.set(3, 0), REFUSE if deconv else EITHER)   # a convolution's stride 0 means 1 (booster ConvParam default)
        semantic("weight_data_size_plus_1", t, lambda x: x.set(6, int(dict(p.split("=") for p in x.pairs)["6"]) + 1), REFUSE)
        semantic("weight_data_size_minus_1", t, lambda x: x.set(6, int(dict(p.split("=") for p in x.pairs)["6"]) - 1), REFUSE)
    semantic("weight_data_size_plus_1", "InnerProduct", lambda x: x.set(2, int(dict(p.split("=") for p in x.pairs)["2"]) + 1), REFUSE)
    semantic("kernel_0", "Pooling", lambda x: x.set(1, 0), EITHER)                      # shape stage
    semantic("stride_0", "Pooling", lambda x: x.set(2, 0), EITHER)                      # shape stage: fhip_pooling_output_dim refuses it
    semantic("sizes_past_channels", "Slice", lambda x: x.set(-23300, f"{len(x.tops)}," + ",".join(["1000000"] * len(x.tops))), EITHER)   # shape stage
    semantic("size_0", "Slice", lambda x: x.set(-23300, f"{len(x.tops)}," + ",".join(["0"] * len(x.tops))), REFUSE)
    semantic("size_infinite", "Slice", lambda x: x.set(-23300, f"{len(x.tops)}," + ",".join(["1e39"] * len(x.tops))), REFUSE)
    semantic("sizes_count_not_tops", "Slice", lambda x: x.set(-23300, f"{len(x.tops) + 1}," + ",".join(["1"] * (len(x.tops) + 1))), REFUSE)
    semantic("group_0", "ShuffleChannel", lambda x: x.set(0, 0), REFUSE)
    semantic("two_tops", "ShuffleChannel", lambda x: (setattr(x, "nt", "2"), x.tops.append("second_top")), REFUSE)
    semantic("min_above_max", "Clip", lambda x: (x.set(0, "1.000000"), x.set(1, "0.500000")), REFUSE)
    semantic("slopes_not_channels", "PReLU", lambda x: x.set(0, int(dict(p.split("=") for p in x.pairs)["0"]) + 1), EITHER)   # shape stage (and the .bin is then short)
    semantic("one_bottom", "Eltwise", lambda x: (setattr(x, "nb", "1"), x.bottoms.pop()), REFUSE)
    semantic("coeffs", "Eltwise", lambda x: x.set(-23301, "2,0.5,0.5"), REFUSE, -100)  # eltwise_layer.h:56-61

    def third_bottom(x):
        x.nb = "3"
        x.bottoms.append(x.bottoms[0])

    semantic("three_bottoms", "BinaryOp", third_bottom, REFUSE)
    m, i = next((m, i) for m in models for i, l in enumerate(parsed[m.tag][1]) if l.type == "Scale" and len(l.bottoms) == 2)
    add(f"{m.tag}/Scale/{parsed[m.tag][1][i].name}/two_bottoms_two_tops",
        mutated(m, i, lambda x: (setattr(x, "nt", "2"), x.tops.append("second_top"))), m.bin, REFUSE, None, m.dilated)
    add(f"{m.tag}/Scale/{parsed[m.tag][1][i].name}/two_bottoms_with_bias", mutated(m, i, lambda x: x.set(1, 1)), m.bin, REFUSE, None, m.dilated)
    semantic("axis_1", "Concat", lambda x: x.set(0, 1), REFUSE)
    semantic("axis_-1", "Concat", lambda x: x.set(0, -1), REFUSE)

    # weight-stream cases: a .bin that ends anywhere but at its end is refused by LoadWeights with -1 (net.cpp:211-217)
    for m in models:
        port = netcheck.PortNet(m.param, m.bin)
        assert port.consumed == len(m.bin), m.tag
        cuts = {0}
        for _, start, end in port.blocks:
            cuts.update((end - 4, end + 4))
        _, start, end = max(port.blocks, key=lambda b: b[2] - b[1])
        cuts.add((start + end) // 2 // 4 * 4 + 1)  # not even a whole float
        for c in sorted(cuts):
            if 0 <= c < len(m.bin):
                add(f"{m.tag}/bin_cut_at_{c}", m.param, m.bin[:c], REFUSE, -1, m.dilated)
        for extra in (4, 4096):
            add(f"{m.tag}/bin_{extra}_trailing_bytes", m.param, m.bin + b"\x7f" * extra, EITHER, None, m.dilated)  # the reference never looks past the last layer

    # the .param cut after every token of two models (the reference's layer types; the extras with arrays and the newer types), and, for the
    # other six, after every layer and after every token of the last layer: every token of all eight would alone be 2300 cases, past the
    # size the whole table is held to, and every type's line is still cut at its end and the tail of every file token by token.  Short of the
    # last layer's first pair the declared layer count is not met: refused.  Inside its pairs the missing ids take their defaults.
    for m in models:
        tok = m.param.split()
        header, layers = parsed[m.tag]
        last = layers[-1]
        head = len(tok) - len(last.pairs)  # tokens up to and including the last layer's names
        if m.tag in ("tiny_allsorts", "extras"):
            cuts = range(len(tok))
        else:
            ends, n = [], 3
            for l in layers:
                n += len(l.tokens())
                ends.append(n)
            cuts = sorted(set(ends[:-1]) | set(range(ends[-2], len(tok))))
        for n in cuts:
            add(f"{m.tag}/param_cut_after_{n}_tokens", b" ".join(tok[:n]) + b"\n", m.bin, REFUSE if n < head else EITHER, None, m.dilated)
    return out


def write_cases(table, directory):
    """The table as the NNNN.param / NNNN.bin (/ NNNN.dilated) files tests/cpp/net_loader_hostile_main.cpp reads."""
    import os
    written = {}
    for i, c in enumerate(table):
        with open(os.path.join(directory, f"{i:04d}.param"), "wb") as f:
            f.write(c.param)
        path = os.path.join(directory, f"{i:04d}.bin")
        if c.bin in written:  # most cases keep their model's .bin: one copy on disk
            os.link(written[c.bin], path)
        else:
            with open(path, "wb") as f:
                f.write(c.bin)
            written[c.bin] = path
        if c.dilated:
            open(os.path.join(directory, f"{i:04d}.dilated"), "wb").close()


if __name__ == "__main__":
    table = cases()
    print(len(table), "cases:", {e: sum(c.expectation == e for c in table) for e in (ACCEPT, REFUSE, EITHER)})
