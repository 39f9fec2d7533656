"""The audio front end without a device: tests/stft_ref.py against torch.stft in float64, the host basis against the float64 formula, the
shapes and the route rule, every refusal of the library and of the Net runtime with its word, and the zoo nets."""
import ctypes

import numpy as np
import pytest

import stft_cases as C
import stft_ref as R

TORCH_PAD = ("constant", "replicate", "reflect")


@pytest.mark.parametrize("case", [c for c in C.CASES if c[9] != 2], ids=C.case_id)  # torch.stft has no (sum window^2)^-1/2 normalisation
def test_the_restatement_is_torch_stft(case):
    import torch
    n, l, n_fft, power, hop, winlen, wt, center, pad, norm, ones, _ = case
    x = C.spectrogram_case(case)[0].astype(np.float64)
    t = torch.stft(torch.from_numpy(x), n_fft, hop, winlen, window=torch.from_numpy(R.window(winlen, None, wt)), center=bool(center), pad_mode=TORCH_PAD[pad],
                   normalized=bool(norm), onesided=bool(ones), return_complex=True)
    want = torch.view_as_real(t).numpy()
    got = R.spectrogram(x, **dict(C.case_kwargs(case), power=0))
    assert got.shape == want.shape and np.abs(got - want).max() <= 1e-11 * max(1.0, np.abs(want).max())


@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_the_host_basis_is_the_formula_rounded_once_and_the_shapes_agree(case):
    from feathercnn_amd import stft as M
    n, l, n_fft, power, hop, winlen, wt, center, pad, norm, ones, _ = case
    want = R.basis(n_fft, winlen, wt, norm, ones)
    got = M.basis(n_fft, winlen, wt, norm, bool(ones))
    assert got.shape == want.shape and np.abs(got - want).max() <= 2.0 ** -24 * np.abs(want).max()  # half an ulp of the largest entry
    assert M.output_shape(n, l, n_fft, power, hop, center, pad, ones) == C.spectrogram_case(case)[1].shape
    assert M.stft_route(0, n_fft, hop) == M.route_rule(0, n_fft, hop) == C.MFMA


def test_the_route_rule_names_every_instantiation():
    from feathercnn_amd import stft as M
    assert {M.stft_route(0, 400, 160)} | {M.stft_route(1, op, v) for op in C.UNARY_OPS for v in (0, 1)} == C.targets()
    assert all(M.stft_route(1, op, v) == M.route_rule(1, op, v) for op in C.UNARY_OPS for v in (0, 1))
    assert M.output_shape(2, 16000, 400, 2, 160) == (2, 201, 101) and M.output_shape(2, 16000, 400) == (2, 201, 161, 2)  # hoplen: n_fft / 4


def _forward(l=100, n_fft=16, power=0, hop=4, center=1, pad=2, ones=1, n=1, frames=None, x=64, y=4096):
    """fhip_stft_forward on pointers that are never followed: every refusal comes before any device call."""
    from feathercnn_amd import _lib
    lib = _lib.load_stft_library()
    frames = (l + (2 * (n_fft // 2) if center else 0) - n_fft) // max(hop, 1) + 1 if frames is None else frames
    rc = lib.fhip_stft_forward(n, l, n_fft, power, hop, center, pad, ones, ctypes.c_void_p(x), ctypes.c_void_p(128), ctypes.c_void_p(y), frames, None)
    return rc, lib.fhip_stft_last_error().decode()


@pytest.mark.parametrize("kw,word", [
    (dict(l=10, n_fft=16, center=0), "shorter than n_fft"), (dict(l=8, n_fft=16), "reflect"), (dict(n_fft=4098), "4096"), (dict(n_fft=1), "n_fft"),
    (dict(hop=0), "hoplen"), (dict(pad=3), "pad_type"), (dict(power=3), "power"), (dict(frames=7), "frames"), (dict(l=2 ** 20, n=2 ** 11), "2^31"),
    (dict(l=2 ** 20, n=2 ** 10, hop=1), "2^31"), (dict(x=0), "null"), (dict(x=66), "aligned"), (dict(x=4096 + 64), "overlap"),
], ids=lambda v: str(v).replace(" ", ""))
def test_the_library_refuses_before_any_device_call(kw, word):
    rc, msg = _forward(**kw)
    assert rc == -2 and word in msg, msg


@pytest.mark.parametrize("args,word", [((16, 0, 0, 0, 1), "winlen"), ((16, 17, 0, 0, 1), "winlen"), ((16, 16, 3, 0, 1), "window_type"), ((16, 16, 0, 3, 1), "normalized"),
                                       ((5000, 16, 0, 0, 1), "4096")])
def test_the_basis_refuses(args, word):
    from feathercnn_amd import FeatherHipError, stft as M
    with pytest.raises(FeatherHipError, match=word):
        M.basis(*args)


def test_unary_refuses():
    from feathercnn_amd import _lib
    lib = _lib.load_stft_library()
    for op in (2, 3, 9, 16, 18, -1):
        assert lib.fhip_unary_forward(op, ctypes.c_void_p(64), ctypes.c_void_p(64), 4, None) == -2 and "op must be" in lib.fhip_stft_last_error().decode()
    assert lib.fhip_unary_forward(8, ctypes.c_void_p(64), ctypes.c_void_p(72), 4, None) == -2 and "overlap" in lib.fhip_stft_last_error().decode()
    assert lib.fhip_unary_forward(8, ctypes.c_void_p(64), ctypes.c_void_p(64), 2 ** 31, None) == -2 and "2^31" in lib.fhip_stft_last_error().decode()


# ---- the Net runtime ---------------------------------------------------------------------------------------------------------------------
TYPES = {"Spectrogram": "0=16", "UnaryOp": "0=8"}


def _one(type_, params, extra_bottom=False):
    lines = ["Input in0 0 1 in0 0=100 1=1 2=1"] + (["Input in1 0 1 in1 0=100 1=1 2=1"] if extra_bottom else [])
    lines.append(f"{type_} l {2 if extra_bottom else 1} 1 in0 {'in1 ' if extra_bottom else ''}top {params}")
    return ("7767517\n%d %d\n" % (len(lines), len(lines)) + "\n".join(lines) + "\n").encode()


def _net(param, audio=True, detection=True):
    from feathercnn_amd.net import Net
    net = Net()
    if audio:
        net.SetAudio()
    if detection:
        net.SetDetection(True)
    net.LoadParam(param)
    return net


def _refused(param, code, word, **kw):
    from feathercnn_amd import FeatherHipError
    with pytest.raises(FeatherHipError, match=f"code {code}") as e:
        _net(param, **kw)
    assert word in str(e.value), str(e.value)
    return str(e.value)


@pytest.mark.parametrize("type_", sorted(TYPES))
def test_the_switch(type_):
    from feathercnn_amd import FeatherHipError
    from feathercnn_amd.net import Net
    p = _one(type_, TYPES[type_])
    assert "(fhip_net_set_audio lifts this)" in _refused(p, -200, type_, audio=False)  # a default net refuses both
    msg = _refused(p, -200, "fhip_net_set_detection", detection=False)
    assert type_ in msg and "set both" in msg
    net = _net(p)
    assert (type_, "l", "STFT") in net.layers()
    with pytest.raises(FeatherHipError, match="before LoadParam"):
        net.SetAudio(False)
    net = Net()
    net.SetAudio()
    net.SetAudio(False)  # on-then-off equals the default
    net.SetDetection(True)
    with pytest.raises(FeatherHipError, match="code -200"):
        net.LoadParam(p)


@pytest.mark.parametrize("type_,params,word", [
    ("Spectrogram", "", "0=0"), ("Spectrogram", "0=1", "0=1"), ("Spectrogram", "0=4097", "0=4097"), ("Spectrogram", "0=16 1=3", "1=3"), ("Spectrogram", "0=16 2=0", "2=0"),
    ("Spectrogram", "0=16 3=17", "3=17"), ("Spectrogram", "0=16 3=0", "3=0"), ("Spectrogram", "0=16 4=3", "4=3"), ("Spectrogram", "0=16 5=2", "5=2"),
    ("Spectrogram", "0=16 6=3", "6=3"), ("Spectrogram", "0=16 7=3", "7=3"), ("Spectrogram", "0=16 8=2", "8=2"), ("Spectrogram", "0=2 2=0", "2=0"),  # the default hop of n_fft 2
    ("UnaryOp", "0=2", "0=2"), ("UnaryOp", "0=3", "0=3"), ("UnaryOp", "0=9", "0=9"), ("UnaryOp", "0=16", "0=16"), ("UnaryOp", "0=18", "0=18"),
], ids=lambda v: str(v).replace(" ", "_"))
def test_loadparam_refusals_name_the_layer_and_the_param(type_, params, word):
    msg = _refused(_one(type_, params), -100, word)
    assert "layer l" in msg and type_ in msg


def test_a_second_bottom_is_refused_and_the_defaults_are_the_tables():
    assert "second bottom" in _refused(_one("Spectrogram", "0=16", extra_bottom=True), -100, "layer l")
    assert _net(_one("Spectrogram", "0=16")).layers()[-1] == ("Spectrogram", "l", "STFT")  # power 0, hoplen 4, winlen 16, ones, centred, reflect, one-sided


def test_the_zoo_nets_dry_load():
    from feathercnn_amd import model_zoo
    from feathercnn_amd.net import Net
    for build, count in ((model_zoo.tiny_audio, 9), (model_zoo.quartznet_5x5_wave, 61)):
        net = Net()
        for switch in (net.SetAudio, net.SetConv1d, net.SetTransformer):
            switch()
        net.SetDetection(True)
        net.LoadParam(build(dry=True)[0])
        layers = net.layers()
        assert len(layers) == count and [a for t, _, a in layers if t in ("Spectrogram", "UnaryOp")] == ["STFT"] * (6 if count == 9 else 2)
    assert model_zoo.quartznet_5x5_wave(dry=True)[1] == model_zoo.quartznet_5x5(dry=True)[1] + 4 + 4 * 64 * 257  # the body's weights and the mel bank
