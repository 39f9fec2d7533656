"""The decoder layers without a device: the constants, the description struct and the route names against feather_decoder.h, the split rule,
every refusal of the library (which comes before any device call), and the neighbours that must stay what they were."""
import ctypes
import os
import re

import pytest

import decoder_cases as C
import side_contract as SC
from feathercnn_amd import decoder as D

HEADER = open(os.path.join(SC.INCLUDE, "feather_hip", "feather_decoder.h")).read()
lib = SC.fixture("decoder")


def test_the_constants_and_the_struct_are_the_headers():
    define = lambda name: int(re.search(r"#define FHIP_DECODER_%s (\d+)" % name, HEADER).group(1))  # noqa: E731
    assert (D.NET_ROUTE, D.MAX_D, D.KEY_TILE, D.MAX_SPLITS, D.RMS_WAVE_MAX) == tuple(define(n) for n in ("NET_ROUTE", "MAX_D", "KEY_TILE", "MAX_SPLITS", "RMS_WAVE_MAX"))
    assert D.ROW_TILES == tuple(define("ROW_TILE_" + n) for n in ("FEW", "MID", "WIDE"))
    assert (D.SPLIT_BLOCKS, D.SPLIT_TARGET, D.SPLIT_MIN_TILES) == tuple(define("SPLIT_" + n) for n in ("BLOCKS", "TARGET", "MIN_TILES"))
    ops = re.findall(r"FHIP_DECODER_(\w+) = (\d)", HEADER)
    assert ops == [(n, str(getattr(D, n))) for n in ("SDPA", "COMBINE", "KV_CONCAT", "RMS_NORM", "ROTARY", "EMBED")] and (C.SDPA, C.EMBED) == (D.SDPA, D.EMBED)
    body = re.search(r"typedef struct\s*\{(.*?)\}\s*fhip_sdpa_desc;", HEADER, re.S).group(1)
    fields = [(kind, name.strip()) for kind, names in re.findall(r"^\s*(int|float) ([\w, ]+);", body, re.M) for name in names.split(",")]
    assert fields == [({ctypes.c_int: "int", ctypes.c_float: "float"}[t], n) for n, t in D.SdpaDesc._fields_]
    from feathercnn_amd import net as N
    assert D.NET_ROUTE == N.DECODER_ROUTE == max(N.ROUTE_NAMES) and N.ROUTE_NAMES[D.NET_ROUTE] == "DECODER"


@pytest.mark.parametrize("what,a,b,c", [(D.SDPA, d, r, t) for d in (4, 32, 36, 64, 68, 96, 100, 128) for r, t in ((1, 0), (32, 0), (33, 0), (64, 0), (65, 0), (5, 128), (500, 32), (5, 64))] +
                         [(D.COMBINE, 0, 0, 0), (D.KV_CONCAT, 0, 0, 0), (D.KV_CONCAT, 1, 0, 0), (D.RMS_NORM, 1, 0, 0), (D.RMS_NORM, 256, 0, 0), (D.RMS_NORM, 257, 0, 0),
                          (D.ROTARY, 0, 0, 0), (D.ROTARY, 1, 0, 0), (D.EMBED, 0, 0, 0)])
def test_the_route_is_the_rule(what, a, b, c):
    assert D.decoder_route(what, a, b, c) == D.route_rule(what, a, b, c) and D.decoder_route(what, a, b, c) in C.targets()


def _desc(**kw):
    base = dict(n=1, heads=4, kv_heads=2, tq=3, tk=40, d=8, q_row_stride=8, q_head_stride=24, k_row_stride=8, k_head_stride=320, v_row_stride=8, v_head_stride=320,
                out_row_stride=8, out_head_stride=24, scale=1.0)
    return D.SdpaDesc(**dict(base, **kw))


@pytest.mark.parametrize("kw,code,word", [
    (dict(n=0), -2, "< 1"), (dict(tk=0), -2, "< 1"), (dict(heads=3), -2, "heads % kv_heads"), (dict(causal=2), -2, "causal"), (dict(splits=-1), -2, "splits"),
    (dict(row_tile=48), -2, "row_tile"), (dict(scale=float("inf")), -2, "finite"), (dict(scale=float("nan")), -2, "finite"), (dict(k_row_stride=7), -2, "row stride"),
    (dict(q_head_stride=-1), -2, "negative"), (dict(mask_head_stride=-4), -2, "negative"), (dict(n=2, k_image_stride=2 ** 31 - 1), -2, "2^31"),
    (dict(tq=2 ** 28), -2, "2^31"), (dict(d=6), -1, "multiple of 4"), (dict(d=132), -1, "128"), (dict(d=0), -2, "d < 1"),
], ids=lambda v: str(v).replace(" ", ""))
def test_sdpa_refuses_before_any_device_call(lib, kw, code, word):
    desc, size = _desc(**kw), ctypes.c_size_t()
    for rc in (lib.fhip_sdpa_get_buffer_size(ctypes.byref(desc), ctypes.byref(size), None), lib.fhip_sdpa_forward(ctypes.byref(desc), 64, 64, 64, None, 64, None, None)):
        assert rc == code and word in lib.fhip_decoder_last_error().decode(), lib.fhip_decoder_last_error()


def test_pointers_and_the_split_rule(lib):
    fwd = lambda desc, q=64, out=64, scratch=None: lib.fhip_sdpa_forward(ctypes.byref(desc), q, 64, 64, None, out, scratch, None)  # noqa: E731
    assert fwd(_desc(), q=None) == -2 and fwd(_desc(), out=66) == -2 and b"aligned" in lib.fhip_decoder_last_error()
    assert fwd(_desc(splits=2)) == -2 and b"scratch" in lib.fhip_decoder_last_error() and fwd(_desc(splits=2), scratch=72) == -2
    assert D.sdpa_plan(_desc()) == (0, 1) and D.sdpa_plan(_desc(splits=9)) == (4 * 1 * 2 * 2 * 6 * (8 + 2), 2)  # forced, clamped to the two key tiles
    big = dict(heads=32, kv_heads=8, tq=1, d=128, q_head_stride=128, q_row_stride=128, out_head_stride=128, out_row_stride=128, k_row_stride=128, v_row_stride=128)
    for tk, n, want in ((1024, 1, 16), (4096, 1, 64), (16384, 1, 64), (16384, 4, 16), (16384, 16, 1), (100, 1, 2), (40, 1, 1)):  # ceil(512 / B) against KT / 2; B >= 128: none
        desc = _desc(**dict(big, tk=tk, n=n, k_head_stride=tk * 128, v_head_stride=tk * 128, k_image_stride=8 * tk * 128, v_image_stride=8 * tk * 128, q_image_stride=4096, out_image_stride=4096))
        assert D.sdpa_plan(desc)[1] == want, (tk, n)


@pytest.mark.parametrize("call,args,word", [
    ("fhip_kv_concat_forward", (1, 1, -1, 1, 4, 64, 64, 64, None), "tp < 0"), ("fhip_kv_concat_forward", (1, 1, 2, 1, 4, None, 64, 64, None), "null"),
    ("fhip_kv_concat_forward", (2 ** 10, 2 ** 10, 2 ** 10, 1, 4, 64, 64, 64, None), "2^31"), ("fhip_rms_norm_forward", (0, 4, None, 1e-6, 64, 64, None), "< 1"),
    ("fhip_rms_norm_forward", (1, 4, None, -1.0, 64, 64, None), "eps"), ("fhip_rms_norm_forward", (1, 4, None, 1e-6, 66, 64, None), "aligned"),
    ("fhip_rotary_forward", (1, 1, 1, 3, 0, 64, 64, 0, 64, 64, None), "even"), ("fhip_rotary_forward", (1, 1, 1, 4, 2, 64, 64, 0, 64, 64, None), "interleaved"),
    ("fhip_rotary_forward", (1, 1, 1, 4, 0, None, 64, 0, 64, 64, None), "null"), ("fhip_embed_forward", (1, 4, 0, 64, 64, None, 64, None), "< 1"),
    ("fhip_embed_forward", (1, 2 ** 16, 2 ** 15, 64, 64, None, 64, None), "2^31"), ("fhip_embed_forward", (1, 4, 5, None, 64, None, 64, None), "null"),
], ids=lambda v: str(v).replace(" ", ""))
def test_the_small_entries_refuse_before_any_device_call(lib, call, args, word):
    assert getattr(lib, call)(*args) == -2 and word in lib.fhip_decoder_last_error().decode(), lib.fhip_decoder_last_error()


def _net(decoder=True, detection=True):
    from feathercnn_amd.net import Net
    net = Net()
    net.SetDecoder(decoder)
    net.SetTransformer()
    net.SetDetection(detection)
    return net


def _param(*lines):
    return ("7767517\n%d %d\n" % (len(lines), sum(int(ln.split()[3]) for ln in lines)) + "\n".join(lines) + "\n").encode()


INPUTS = ["Input %s 0 1 %s" % (b, b) for b in "qkvmab"]
GOOD = {"SDPA": "SDPA l 3 1 q k v top", "SDPA_mask": "SDPA l 4 1 q k v m top 5=1 6=0.5", "SDPA_cache": "SDPA l 6 3 q k v m a b top pk pv 5=1 7=1", "SDPA_cache_only": "SDPA l 5 3 q k v a b top pk pv 7=1",
        "RMSNorm": "RMSNorm l 1 1 q top 0=8 1=1e-5 2=0", "RotaryEmbed": "RotaryEmbed l 3 1 q k v top 0=1", "Embed": "Embed l 1 1 q top 0=4 1=5 2=1 3=20"}
BAD = {"SDPA l 4 1 q k v m top": "4 and 1", "SDPA l 3 1 q k v top 5=1": "3 and 1", "SDPA l 4 1 q k v m top 5=1 7=1": "6 bottoms", "SDPA l 3 1 q k v top 5=2": "5=2", "SDPA l 3 1 q k v top 7=3": "7=3",
       "SDPA l 3 1 q k v top 6=1e39": "6=", "RMSNorm l 1 1 q top": "0=0", "RMSNorm l 1 1 q top 0=8 1=-1": "1=", "RMSNorm l 1 1 q top 0=8 2=2": "2=2", "RMSNorm l 2 1 q k top 0=8": "one bottom",
       "RotaryEmbed l 1 1 q top": "three bottoms", "RotaryEmbed l 3 1 q k v top 0=2": "0=2", "Embed l 1 1 q top 0=4 1=5 3=19": "3=19", "Embed l 1 1 q top 0=0 1=5": "0=0", "Embed l 1 1 q top 0=4 1=5 2=2 3=20": "2=2"}


@pytest.mark.parametrize("name", sorted(GOOD))
def test_loadparam_takes_the_good_forms(name):
    net = _net()
    net.LoadParam(_param(*INPUTS, GOOD[name]))
    assert [a for t, _, a in net.layers() if t != "Input"] == ["DECODER"]


@pytest.mark.parametrize("line", sorted(BAD), ids=lambda v: v.replace(" ", "_"))
def test_loadparam_refusals_name_the_layer(line):
    from feathercnn_amd import FeatherHipError
    with pytest.raises(FeatherHipError, match="code -100") as e:
        _net().LoadParam(_param(*INPUTS, line))
    assert "layer l" in str(e.value) and BAD[line] in str(e.value), str(e.value)


@pytest.mark.parametrize("name", ["SDPA", "RMSNorm", "RotaryEmbed", "Embed"])
def test_the_switch_the_hint_and_truncated_weights(name):
    from feathercnn_amd import FeatherHipError
    line = GOOD[name].replace("2=0", "2=1")
    for kw, word in ((dict(decoder=False), "(fhip_net_set_decoder lifts this)"), (dict(detection=False), "set both")):
        with pytest.raises(FeatherHipError, match="code -200") as e:
            _net(**kw).LoadParam(_param(*INPUTS, line))
        assert name in str(e.value) and word in str(e.value), str(e.value)
    if name in ("RMSNorm", "Embed"):  # the two with weights: a file that ends inside them names the layer
        net = _net()
        net.LoadParam(_param(*INPUTS, line))
        with pytest.raises(FeatherHipError) as e:
            net.LoadWeights(b"\0" * 12)
        assert "Layer l loading weights failed" in str(e.value), str(e.value)
    from feathercnn_amd import model_zoo
    net = _net()
    net.LoadParam(model_zoo.tiny_llama(dry=True)[1])
    assert {t for t, _, a in net.layers() if a == "DECODER"} == {"SDPA", "RMSNorm", "RotaryEmbed", "Embed"}


def test_the_neighbours_are_what_they_were():
    """MultiHeadAttention with a mask is still refused: masked attention is the SDPA layer's."""
    from feathercnn_amd import FeatherHipError
    from feathercnn_amd.net import Net
    net = Net()
    net.SetTransformer()
    net.SetDetection(True)
    with pytest.raises(FeatherHipError, match="code -100") as e:
        net.LoadParam(b"7767517\n2 2\nInput in0 0 1 in0 0=8 1=6\nMultiHeadAttention l 1 1 in0 top 0=8 1=2 2=64 5=1\n")
    assert "attention mask" in str(e.value)
