"""The numpy restatement of include/feather_hip/feather_rnn.h, line by line: the recurrent core of ncnn's LSTM, GRU and RNN.  Sums run in the
dtype asked for (float64 by default: what the tests compare the device's float32 with, by the project's normalised error; float32 to show
that a case's conditioning leaves float32 room).  model_zoo.numpy_forward's recurrent layers are this text, not a second one."""
import numpy as np

LSTM, GRU, RNN = range(3)  # FHIP_RNN_LSTM, FHIP_RNN_GRU, FHIP_RNN_RNN
GATES = {LSTM: 4, GRU: 3, RNN: 1}
AUTO, STEP, SEQUENCE = range(3)  # FHIP_RNN_ROUTE_*
NET_ROUTE = 114  # FHIP_RNN_NET_ROUTE
UNIT_TILE, SEQ_TILE, MFMA_MULTIPLE, SEQUENCE_TILE = 32, 32, 4, 4  # FHIP_RNN_UNIT_TILE, _SEQ_TILE, _MFMA_MULTIPLE, _SEQUENCE_TILE
SEQUENCE_LDS_FLOATS = 40960  # FHIP_RNN_SEQUENCE_LDS_FLOATS
SEQUENCE_MAX_H = {LSTM: 100, GRU: 115, RNN: 198}  # FHIP_RNN_SEQUENCE_MAX_H_*
SEQUENCE_MAX_N = 256  # FHIP_RNN_SEQUENCE_MAX_N


def sequence_fits(cell, h):
    return GATES[cell] * h * h + 2 * SEQUENCE_TILE * h <= SEQUENCE_LDS_FLOATS


def route(cell, h, n, t, forced=AUTO):
    """The rule of the header: the kernel instantiation a call launches."""
    seq = forced == SEQUENCE or (forced == AUTO and sequence_fits(cell, h) and n <= SEQUENCE_MAX_N)
    kernel = "sequence" if seq else ("step_mfma" if h % MFMA_MULTIPLE == 0 else "step_direct")
    return "fhip::rnn_%s_kernel<%d>" % (kernel, cell)


def _sigmoid(x):
    with np.errstate(over="ignore"):
        return 1 / (1 + np.exp(-x))


def recurrent(cell, direction, xp, wh, bn=None, h0=None, c0=None, dtype=np.float64):
    """xp [n][T][nd * G * H] (the input projections with the bias), wh [nd][G * H][H], bn [nd][H] (GRU), h0 / c0 None or [n][nd][H]
    -> (out [n][T][nd * H], hn [n][nd][H], cn [n][nd][H] or None)."""
    xp, wh = np.asarray(xp, dtype), np.asarray(wh, dtype)
    nd, G = (2 if direction == 2 else 1), GATES[cell]
    n, T = xp.shape[:2]
    H = wh.shape[2]
    assert wh.shape == (nd, G * H, H) and xp.shape[2] == nd * G * H
    out = np.zeros((n, T, nd * H), dtype)
    hn = np.zeros((n, nd, H), dtype)
    cn = np.zeros((n, nd, H), dtype) if cell == LSTM else None
    for d in range(nd):
        reverse = direction == 1 or (direction == 2 and d == 1)
        h = np.zeros((n, H), dtype) if h0 is None else np.asarray(h0, dtype)[:, d].copy()
        c = np.zeros((n, H), dtype) if c0 is None or cell != LSTM else np.asarray(c0, dtype)[:, d].copy()
        w = wh[d].reshape(G, H, H)
        for t in (range(T - 1, -1, -1) if reverse else range(T)):
            x = xp[:, t, d * G * H:(d + 1) * G * H].reshape(n, G, H)
            dot = np.einsum("gjk,ik->igj", w, h)  # Wh[d][g * H + j] . h_prev
            if cell == LSTM:
                a = x + dot
                I, F, O, Gt = _sigmoid(a[:, 0]), _sigmoid(a[:, 1]), _sigmoid(a[:, 2]), np.tanh(a[:, 3])
                c = F * c + I * Gt
                h = O * np.tanh(c)
            elif cell == GRU:
                R, U = _sigmoid(x[:, 0] + dot[:, 0]), _sigmoid(x[:, 1] + dot[:, 1])
                N = np.tanh(x[:, 2] + R * (dot[:, 2] + np.asarray(bn, dtype)[d]))
                h = (1 - U) * N + U * h
            else:
                h = np.tanh(x[:, 0] + dot[:, 0])
            out[:, t, d * H:(d + 1) * H] = h
        hn[:, d] = h
        if cell == LSTM:
            cn[:, d] = c
    return out, hn, cn


def project(cell, direction, x, wx, bias, dtype=np.float64):
    """The caller's part: x [n][T][size], wx [nd][G * H][size], bias as ncnn stores it ([nd][4][H] for LSTM and GRU, [nd][H] for RNN)
    -> (xp [n][T][nd * G * H], bn [nd][H] or None)."""
    x, wx, bias = np.asarray(x, dtype), np.asarray(wx, dtype), np.asarray(bias, dtype)
    nd, G = wx.shape[0], GATES[cell]
    H = wx.shape[1] // G
    b = bias.reshape(nd, -1, H)
    xp = np.concatenate([x @ wx[d].T + b[d, :G].reshape(-1) for d in range(nd)], axis=2)
    return xp, (b[:, 3] if cell == GRU else None)


def layer(cell, direction, x, wx, bias, wh, h0=None, c0=None, dtype=np.float64):
    """ncnn's LSTM / GRU / RNN layer on x [n][T][size] -> (out, hn, cn)."""
    xp, bn = project(cell, direction, x, wx, bias, dtype)
    return recurrent(cell, direction, xp, wh, bn, h0, c0, dtype)


def normalised_error(got, want):
    """The project's error measure (tests/test_net_gpu.py): the largest difference over the largest magnitude of the reference."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-30))
