"""libfeather_q8.so and Net.SetRequantized without a GPU: the twin property on the restatement (tests/q8_ref.py), the loader (the switch, the
messages without it, the refusals with it), and the host side of the library over the case table of tests/q8_cases.py.  The layers run in
tests/test_q8_gpu.py and tests/test_q8_net_gpu.py; the contract of the library's row is tests/test_q8_contract_cpu.py.

What is NOT here: the NET_E_TOPOLOGY refusals of the layers that cannot read a q8 blob (average Pooling, Eltwise, Concat, InnerProduct, an fp32
Convolution, an unfused BatchNorm) and of Extract.  The Net refuses them in reshape_all, at the first Forward, behind FeedInput and the Reshape of
the layers in front, which allocate device memory: they need a device, and are tests/test_q8_net_gpu.py's.  And the Split, Eltwise and q8 paths
of tests/q8_ref.net_forward are checked here against that function alone (tests/qconv_ref.net_forward has no Split); their independent check is
the twin run on the device there."""
import ctypes

import numpy as np
import pytest

import q8_cases as QC
import q8_ref as Q
import qconv_ref as R
import side_contract

F = np.float32
lib = side_contract.fixture("q8")
HEAD = b"7767517\n2 2\nInput data 0 1 data 0=1 1=1 2=16\n"


def _x(n=3, seed=5):
    return np.random.default_rng(seed).uniform(-1, 1, (n, 3, 16, 16)).astype(F)


# ---- the property the tests stand on -------------------------------------------------------------------------------------------------
def test_the_restatement_of_nets_is_the_existing_one_where_that_one_applies():
    """tests/q8_ref.net_forward on tiny_quant (no q8 blob, no Split) is tests/qconv_ref.net_forward, blob for blob and level for level."""
    from feathercnn_amd import model_zoo
    model, x = model_zoo.tiny_quant(), _x()
    for level in (0, 1, 2):
        a, b = Q.net_forward(model, x, level), R.net_forward(model, x, level)
        assert a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a), level


@pytest.mark.parametrize("bn,levels", [(True, (2,)), (False, (0, 1, 2))], ids=["with_the_fold", "without_batchnorm"])
def test_tiny_requant_equals_its_twin_on_every_fp32_blob(bn, levels):
    from feathercnn_amd import model_zoo
    model, twin = model_zoo.tiny_requant(bn=bn), model_zoo.tiny_requant(bn=bn, twin=True)
    assert b"8=101" in model[0] and b"8=101" not in twin[0] and model[0].replace(b"8=101", b"8=1") == twin[0] and len(model[1]) == len(twin[1]) + 16
    for seed in (5, 6):
        x = _x(seed=seed)
        for level in levels:
            a, b = Q.net_forward(model, x, level), Q.net_forward(twin, x, level)
            q8 = {k for k in a if isinstance(a[k], Q.Q8Blob)}
            assert {"relu1", "relu2", "pool2", "conv3_relu", "split_0", "split_1", "relu_dw"} <= q8 and not any(isinstance(v, Q.Q8Blob) for v in b.values())
            for k in a.keys() - q8:
                assert np.array_equal(a[k], b[k]), (level, k)
            for k in q8:  # and a q8 blob holds the quantised twin blob: the scale is its reader's
                s = {"relu1": "conv2", "relu2": "conv3", "pool2": "conv3", "conv3_relu": "dw", "relu_dw": "pw"}.get(k)
                if s:
                    assert np.array_equal(a[k].q, R.quantise(b[k], _scale(twin, s))), k
            assert np.abs(a["fc"]).max() > 0.5


def _layer(model, layer):
    """An int8 convolution of a model as its .param and .bin state it, read the way the restatement reads them: a dict of the weights, the
    bias (or None), the weight scales, the input scale, the output scale (or None), the group, the stride and the pad."""
    rd = R._Bin(model[1])
    for type_, name, _, _, pd in R._layers(model[0]):
        if type_ in ("Convolution", "ConvolutionDepthWise"):
            k, kh, s, p, group = int(pd[0]), int(pd[1]), int(pd[3]), int(pd[4]), int(pd[7])
            c = int(pd[6]) * group // (k * kh * kh)
            wq = rd.int8(int(pd[6])).reshape(k, c // group, kh, kh)
            bias = rd.raw(k) if int(pd[5]) else None
            s_w, s_in = rd.raw(k), rd.raw(1)[0]
            s_out = rd.raw(1)[0] if int(pd[8]) > 100 else None
            if name == layer:
                return dict(wq=wq, b=bias, s_w=s_w, s_in=s_in, s_out=s_out, group=group, strides=(s, s), pads=(p, p, p, p))
        elif type_ in ("BatchNorm", "Scale"):
            rd.raw(int(pd[0]) * (4 if type_ == "BatchNorm" else 2))
    raise KeyError(layer)


def _scale(model, layer):
    """The input scale of an int8 layer of a model."""
    return _layer(model, layer)["s_in"]


@pytest.mark.parametrize("reader", ["conv2", "dw", "side"])
def test_a_reader_with_another_scale_equals_the_direct_restatement_and_differs_from_the_twin(reader):
    """With s_in != s_out the int8 blob is used as it is -- not quantised again, and dequantised with the READER's s_in, not its producer's
    s_out: the reader's top is the layer of feather_q8.h computed from the int8 blob it reads and the numbers of its own .bin entry, and
    the net is no longer its twin."""
    from feathercnn_amd import model_zoo
    model, twin, x = model_zoo.tiny_requant(mismatch=reader), model_zoo.tiny_requant(mismatch=reader, twin=True), _x()
    a, b = Q.net_forward(model, x, 2), Q.net_forward(twin, x, 2)
    assert not np.array_equal(a["fc"], b["fc"])
    bottom, producer = {"conv2": ("relu1", "conv1"), "dw": ("split_0", "conv3"), "side": ("split_1", "conv3")}[reader]
    l = _layer(model, reader)
    assert isinstance(a[bottom], Q.Q8Blob) and l["s_in"] != _scale(model_zoo.tiny_requant(), reader) and l["s_in"] != _layer(model, producer)["s_out"]
    want = Q.conv(a[bottom].q, l["wq"], R.dequant_scales(l["s_w"], l["s_in"]), l["b"], l["group"], l["strides"], l["pads"], False, s_in=None, s_out=l["s_out"])
    top = a[reader]  # the reader's own top: its ReLU, where it has one, is a layer behind it in the restatement
    assert (l["s_out"] is None) == (not isinstance(top, Q.Q8Blob))
    assert np.array_equal(top.q if isinstance(top, Q.Q8Blob) else top, want) and np.abs(want).max() > 0
    # and it is neither of the two wrong readings: the blob quantised again with the reader's scale, or the producer's scale in d[k]
    again = Q.conv(R.quantise(a[bottom].q, l["s_in"]), l["wq"], R.dequant_scales(l["s_w"], l["s_in"]), l["b"], l["group"], l["strides"], l["pads"], False, None, l["s_out"])
    theirs = Q.conv(a[bottom].q, l["wq"], R.dequant_scales(l["s_w"], _layer(model, producer)["s_out"]), l["b"], l["group"], l["strides"], l["pads"], False, None, l["s_out"])
    assert not np.array_equal(again, want) and not np.array_equal(theirs, want)


# ---- the loader ----------------------------------------------------------------------------------------------------------------------
def _net(requantized=True, quantized=True, fusion=2):
    from feathercnn_amd.net import Net
    net = Net(fusion=fusion)
    if quantized:
        net.SetQuantized(True)
    if requantized:
        net.SetRequantized(True)
    return net


def test_tiny_requant_loads_with_the_switch_and_every_int8_layer_reports_qconv():
    from feathercnn_amd import FeatherHipError, model_zoo
    p, b, i, o = model_zoo.tiny_requant()
    assert model_zoo.tiny_requant() == (p, b, i, o) and model_zoo.tiny_requant(dry=True) == (p, len(b), i, o)
    assert "tiny_requant" in model_zoo.REQUANTIZED_NETS and not set(model_zoo.REQUANTIZED_NETS) & set(model_zoo.QUANTIZED_NETS)
    assert all(n in model_zoo.MODELS for n in model_zoo.REQUANTIZED_NETS)
    net = _net()
    net.LoadParam(p)
    net.LoadWeights(b)
    routed = [nm for _, nm, a in net.layers() if a == "QCONV"]
    assert routed == list(model_zoo.QUANT_LAYERS["tiny_requant"]) and set(model_zoo.REQUANT_LAYERS["tiny_requant"]) <= set(routed)
    from feathercnn_amd import net as netmod
    assert not hasattr(netmod, "ROUTE_Q8")  # no route code of its own
    with pytest.raises(FeatherHipError, match="before LoadParam"):
        net.SetRequantized(False)


def test_without_the_switch_the_old_messages_come_back_word_for_word():
    from feathercnn_amd import FeatherHipError, model_zoo
    p = model_zoo.tiny_requant()[0]
    for net, want in ((_net(requantized=False), "layer conv1: int8_scale_term 101 (requantised int8 output) is not supported"),
                      (_net(quantized=False), "layer conv1: int8 convolution is not supported"),  # the switch needs SetQuantized
                      (_net(requantized=False, quantized=False), "layer conv1: int8 convolution is not supported")):
        with pytest.raises(FeatherHipError) as e:
            net.LoadParam(p)
        assert "code -200" in str(e.value) and str(e.value).endswith(want) and "fhip_net_set_" not in str(e.value), str(e.value)


def test_what_stays_refused_with_the_switch():
    from feathercnn_amd import FeatherHipError
    for line, word in (("Convolution c 1 1 data c 0=4 1=1 6=64 8=201", "0 .. 200"), ("InnerProduct c 1 1 data c 0=4 2=64 8=101", "requantised"),
                       ("Convolution c 1 1 data c 0=4 1=1 6=64 8=-1", "requantised")):
        with pytest.raises(FeatherHipError) as e:
            _net().LoadParam(HEAD + line.encode() + b"\n")
        assert "code -200" in str(e.value) and word in str(e.value) and "fhip_net_set_" not in str(e.value), (line, str(e.value))


@pytest.mark.parametrize("s_out,word", [(0.0, "output scale"), (float("nan"), "output scale"), (float("inf"), "output scale"), (-2.0, "output scale"), (None, None)])
def test_a_bad_or_missing_output_scale_is_refused_at_load_weights(s_out, word):
    from feathercnn_amd import FeatherHipError, model_zoo
    g = model_zoo.GraphBuilder(1, quant={})
    g.conv("c", g.input("data", 16, 4, 4), 16, 4, 1, requant=3.0)
    text, blob = g.finish()
    blob = blob[:-4] + (b"" if s_out is None else np.array([s_out], "<f4").tobytes())
    net = _net()
    net.LoadParam(text)
    with pytest.raises(FeatherHipError) as e:
        net.LoadWeights(blob)
    if word:
        assert "layer c: the int8 " + word in str(e.value), str(e.value)  # (LoadWeights reports every layer's failure as -1)
    good = _net()
    good.LoadParam(text)
    good.LoadWeights(g.finish()[1])


# ---- the host side of the library ----------------------------------------------------------------------------------------------------
def test_supported_buffer_size_and_route_over_the_case_table(lib):
    told = ctypes.create_string_buffer(160)
    for case in QC.CASES:
        _, c, k, group, h, w, kh, kw, s, pads, batch, forms = case
        for form in forms:
            p = QC.param(case, form)
            assert lib.fhip_q8_supported(ctypes.byref(p)) == 1, (case[0], lib.fhip_q8_last_error())
            assert lib.fhip_q8_route(ctypes.byref(p), told, 160) == 0 and told.value.decode() == QC.routes(case, form)[0]
            for route in QC.all_routes():
                sb, pk = ctypes.c_size_t(7), ctypes.c_size_t(7)
                rc = lib.fhip_q8_get_buffer_size_route(ctypes.byref(p), batch, route.encode(), ctypes.byref(sb), ctypes.byref(pk))
                if route in QC.routes(case, form):
                    assert rc == 0 and sb.value == 0 and pk.value % 16 == 0 and pk.value >= k * (c // group) * kh * kw, (case[0], route)
                else:
                    assert rc == -1 and b"cannot run this layer" in lib.fhip_q8_last_error(), (case[0], form, route, rc)  # FHIP_E_UNSUPPORTED
            assert lib.fhip_q8_get_buffer_size_route(ctypes.byref(p), batch, b"fhip::no_such_kernel", ctypes.byref(sb), ctypes.byref(pk)) == -2
        both = QC.param(case, QC.II, input_int8=0, output_int8=0)
        assert lib.fhip_q8_supported(ctypes.byref(both)) == 0 and b"libfeather_qconv" in lib.fhip_q8_last_error()  # fp32 in and out: not this library


def test_supported_refuses_what_the_definition_lists(lib):
    case = QC.CASES[0]
    for over, word in ((dict(int8_scale_term=201), "int8_scale_term"), (dict(int8_scale_term=-1), "int8_scale_term"), (dict(dilation_h=2), "dilation"),
                       (dict(group=2), "partial group"), (dict(pad_left=-1), "negative"), (dict(activation=2), "activation"), (dict(output_h=3), "output_h"),
                       (dict(input_int8=2), "input_int8"), (dict(kernel_h=60), "larger than the padded"), (dict(input_channels=0), "channels")):
        p = QC.param(case, QC.II, **over)
        assert lib.fhip_q8_supported(ctypes.byref(p)) == 0 and word.encode() in lib.fhip_q8_last_error(), (over, lib.fhip_q8_last_error())
    assert lib.fhip_q8_supported(ctypes.byref(QC.param(case, QC.II, int8_scale_term=200))) == 1
    huge = QC.param(case, QC.II, input_channels=16, input_h=20000, input_w=20000, output_h=20000, output_w=20000, output_channels=1)
    assert lib.fhip_q8_supported(ctypes.byref(huge)) == 0 and b"2^31" in lib.fhip_q8_last_error()  # 6.4e9 bytes of q8 input
    n = ctypes.c_size_t()
    assert lib.fhip_q8_tensor_bytes(2, 20, 3, 5, ctypes.byref(n)) == 0 and n.value == 2 * 2 * 3 * 5 * 16
    assert lib.fhip_q8_tensor_bytes(1, 16, 1 << 14, 1 << 13, ctypes.byref(n)) == -2  # exactly 2^31 bytes
    assert lib.fhip_q8_tensor_bytes(1, 16, (1 << 14) - 1, 1 << 13, ctypes.byref(n)) == 0 and n.value == ((1 << 14) - 1) * (1 << 13) * 16


def test_dequant_scales_are_those_of_the_qconv_library(lib):
    s_w = np.array([0.0, 0.5, 3.0000002, 77.7, 1e-20], F)
    d = np.empty_like(s_w)
    v = ctypes.c_void_p
    assert lib.fhip_q8_dequant_scales(v(d.ctypes.data), v(s_w.ctypes.data), 5, 0.3333333) == 0
    assert np.array_equal(d.view(np.int32), R.dequant_scales(s_w, 0.3333333).view(np.int32))
    assert lib.fhip_q8_dequant_scales(v(d.ctypes.data), v(s_w.ctypes.data), 5, 0.0) == -2
