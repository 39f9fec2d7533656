"""InverseSpectrogram without a device: the restatement against torch.istft, the host arrays, the round trip, the route rule and every refusal."""
import ctypes

import numpy as np
import pytest

import istft_cases as C
import istft_ref as R
import stft_ref as S


@pytest.mark.parametrize("case", [c for c in C.CASES if c[7] != 2], ids=C.case_id)  # torch.istft has no (sum window^2)^1/2 normalisation
def test_the_restatement_is_torch_istft(case):
    import torch
    n, frames, n_fft, hop, winlen, wt, center, norm, ones = case
    x, want = C.case_data(case)
    # two-sided: the real part of the complex inverse (with return_complex=False torch reads only the first half of the frequencies)
    got = torch.istft(torch.view_as_complex(torch.from_numpy(x.astype(np.float64))), n_fft, hop, winlen, window=torch.from_numpy(S.window(winlen, None, wt)),
                      center=bool(center), normalized=bool(norm), onesided=bool(ones), return_complex=not ones)
    got = (got if ones else got.real).numpy()
    assert got.shape == want.shape and np.abs(got - want).max() <= 1e-10


@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_the_host_arrays_are_the_formulas_rounded_once(case):
    from feathercnn_amd import istft as M
    n, frames, n_fft, hop, winlen, wt, center, norm, ones = case
    want = R.basis(n_fft, winlen, wt, norm, ones)
    got = M.basis(n_fft, winlen, wt, norm, bool(ones))
    assert got.shape == want.shape and np.abs(got - want).max() <= 2.0 ** -24 * np.abs(want).max()  # half an ulp of the largest entry
    if ones:
        assert not got[:, 1].any() and (n_fft % 2 or not got[:, n_fft + 1].any())  # the ignored imaginary columns are zeros
    want = 1 / R.envelope(frames, n_fft, hop, winlen, wt, center)
    got = M.envelope(frames, n_fft, hop, winlen, wt, bool(center))
    assert got.shape == want.shape == (M.output_length(frames, n_fft, hop, bool(center)),) == C.case_data(case)[1].shape[1:]
    assert (np.abs(got - want) <= 2.0 ** -24 * want * (1 + 1e-6)).all()  # half an ulp of each entry (and the order of the double sum)
    assert M.istft_route(n_fft, hop) == M.route_rule(n_fft, hop) == C.MFMA == "fhip::istft_mfma_kernel"


def test_spectrogram_then_inverse_returns_the_waveform():
    x = np.random.default_rng(19100).uniform(-1, 1, (2, 800))
    back = R.inverse_spectrogram(S.spectrogram(x, 400, 0, 160, 400, 1), 400, 160, 400, 1)
    assert back.shape == x.shape and np.abs(back - x).max() <= 1e-12  # float64: a sum of 400 terms of size 1


def _forward(frames=10, n_fft=16, hop=4, center=1, ones=1, n=1, out_len=None, x=4096, basis=128, env=256, y=64):
    """fhip_istft_forward on pointers that are never followed: every refusal comes before any device call."""
    from feathercnn_amd import _lib
    lib = _lib.load_istft_library()
    out_len = (frames - 1) * hop + n_fft - (2 * (n_fft // 2) if center else 0) if out_len is None else out_len
    rc = lib.fhip_istft_forward(n, frames, n_fft, hop, center, ones, ctypes.c_void_p(x), ctypes.c_void_p(basis), ctypes.c_void_p(env), ctypes.c_void_p(y), out_len, None)
    return rc, lib.fhip_istft_last_error().decode()


@pytest.mark.parametrize("kw,word", [
    (dict(n_fft=1), "n_fft"), (dict(n_fft=4098), "4096"), (dict(hop=0), "hoplen"), (dict(frames=0), "frames"), (dict(frames=1), "out_len < 1"), (dict(out_len=7), "out_len"),
    (dict(n=0), "n < 1"), (dict(frames=2 ** 20, n=2 ** 7), "2^31"), (dict(frames=2 ** 20, hop=2 ** 12), "2^31"), (dict(frames=2 ** 17, hop=2 ** 10, n=2 ** 5), "2^31"),
    (dict(x=0), "null"), (dict(env=0), "null"), (dict(y=66), "aligned"), (dict(x=4098), "aligned"), (dict(y=4096 + 64), "overlap"),
], ids=lambda v: str(v).replace(" ", ""))
def test_the_library_refuses_before_any_device_call(kw, word):
    rc, msg = _forward(**kw)
    assert rc == -2 and word in msg, msg


@pytest.mark.parametrize("call,args,word", [
    ("basis", (16, 0), "winlen"), ("basis", (16, 17), "winlen"), ("basis", (16, 16, 3), "window_type"), ("basis", (16, 16, 0, 3), "normalized"), ("basis", (5000,), "4096"),
    ("envelope", (4, 16, 8, 7), "sample 3"), ("envelope", (4, 16, 4, 16, 1, False), "sample 0"),  # hoplen above winlen: the first gap; Hann without center starts at zero
    ("envelope", (4, 16, 4, 16, 3), "window_type"), ("envelope", (1, 16, 4), "out_len < 1"), ("output_length", (0, 16), "frames"),
])
def test_the_host_functions_refuse(call, args, word):
    from feathercnn_amd import FeatherHipError, istft as M
    with pytest.raises(FeatherHipError, match=word):
        getattr(M, call)(*args)


def _one(params):
    return f"7767517\n2 2\nInput in0 0 1 in0 0=2 1=10 2=9\nInverseSpectrogram l 1 1 in0 top {params}\n".encode()


def _net(audio=True, detection=True):
    from feathercnn_amd.net import Net
    net = Net()
    net.SetAudio(audio)
    net.SetDetection(detection)
    return net


def _refused(param, code, word, **kw):
    from feathercnn_amd import FeatherHipError
    with pytest.raises(FeatherHipError, match=f"code {code}") as e:
        _net(**kw).LoadParam(param)
    assert word in str(e.value), str(e.value)
    return str(e.value)


def test_the_switch_and_the_route():
    from feathercnn_amd import ISTFT_NET_ROUTE, model_zoo, net as N
    p = _one("0=16")
    assert "(fhip_net_set_audio lifts this)" in _refused(p, -200, "InverseSpectrogram", audio=False)  # a default net refuses it, as it refuses Spectrogram
    msg = _refused(p, -200, "fhip_net_set_detection", detection=False)
    assert "InverseSpectrogram" in msg and "set both" in msg
    assert N.ISTFT_ROUTE == ISTFT_NET_ROUTE == 119 and N.ROUTE_NAMES[119] == "ISTFT"
    for param, want in ((p, ["ISTFT"]), (model_zoo.tiny_resynth(dry=True)[0], ["STFT", "ISTFT", "STFT"])):
        net = _net()
        net.LoadParam(param)
        assert [a for t, _, a in net.layers() if t != "Input"] == want


@pytest.mark.parametrize("params,word", [("", "0=0"), ("0=1", "0=1"), ("0=4097", "0=4097"), ("0=16 1=0", "1=0"), ("0=16 1=2", "1=2"), ("0=16 2=0", "2=0"), ("0=2", "2=0"),
                                         ("0=16 3=17", "3=17"), ("0=16 3=0", "3=0"), ("0=16 4=3", "4=3"), ("0=16 5=2", "5=2"), ("0=16 7=3", "7=3")],
                         ids=lambda v: str(v).replace(" ", "_"))
def test_loadparam_refusals_name_the_layer_and_the_param(params, word):
    msg = _refused(_one(params), -100, word)
    assert "layer l" in msg and "InverseSpectrogram" in msg
