"""The numpy restatement of include/feather_hip/feather_frame.h: the window (ncnn's Padding and Crop as one operation) and PixelShuffle, written
from the header's formulas as index maps -- no np.pad, no reshape tricks -- so that tests/test_frame_cpu.py can hold it against np.pad,
torch.nn.functional.pad, torch.nn.functional.pixel_shuffle, plain slicing and tests/yolo_ref.reorg, which are independent of it.

Every function moves float32 words: the result of window() and of pixel_shuffle() without a ReLU is a bit copy of input elements and of the
constant, which the tests compare as int32 views (NaN payloads and -0.0 count).  feathercnn_amd.model_zoo.numpy_forward takes its Padding,
Crop and PixelShuffle layers from here."""
import numpy as np

F = np.float32
CONSTANT, REPLICATE, REFLECT = 0, 1, 2
RELU_NONE, RELU_SLOPE, RELU_PLAIN = 0, 1, 2
TILE = 4096  # FHIP_FRAME_TILE
NET_ROUTE = 112  # FHIP_FRAME_NET_ROUTE


def window_output_dim(c, h, w, front=0, behind=0, top=0, bottom=0, left=0, right=0):
    oc, oh, ow = c + front + behind, h + top + bottom, w + left + right
    if min(c, h, w) < 1 or min(oc, oh, ow) < 1:
        raise ValueError("a dimension < 1")
    return oc, oh, ow


def source_index(type_, i, d):
    """map(i, d) of the header for an array of output-minus-margin indices: the source index, -1 where a constant window has none."""
    i = np.asarray(i, np.int64)
    if type_ == REPLICATE:
        return np.minimum(np.maximum(i, 0), d - 1)
    if type_ == REFLECT:
        return np.where(i < 0, -i, np.where(i >= d, 2 * (d - 1) - i, i))
    return np.where((i < 0) | (i >= d), -1, i)


def window(x, type_=CONSTANT, value=0.0, per_channel=None, front=0, behind=0, top=0, bottom=0, left=0, right=0):
    """The window of x[n][c][h][w] (feather_frame.h): positive margins pad, negative ones crop."""
    x = np.ascontiguousarray(x, F)
    n, c, h, w = x.shape
    oc, oh, ow = window_output_dim(c, h, w, front, behind, top, bottom, left, right)
    if type_ not in (CONSTANT, REPLICATE, REFLECT):
        raise ValueError("type")
    if type_ != CONSTANT and (front > 0 or behind > 0 or per_channel is not None):
        raise ValueError("channel pads and per-channel values are defined for type 0 only")
    if type_ == REFLECT and (top >= h or bottom >= h or left >= w or right >= w):
        raise ValueError("a reflect pad must be smaller than the dimension")
    sq = np.arange(oc, dtype=np.int64) - front
    sq = np.where((sq < 0) | (sq >= c), -1, sq)  # channels are never replicated or reflected
    sy = source_index(type_, np.arange(oh) - top, h)
    sx = source_index(type_, np.arange(ow) - left, w)
    fill = np.full(oc, np.asarray(value, F).view(np.uint32), np.uint32)
    if per_channel is not None:
        pc = np.ascontiguousarray(per_channel, F).reshape(c).view(np.uint32)
        fill = np.where(sq >= 0, pc[np.maximum(sq, 0)], fill)
    bits = x.view(np.uint32)
    out = np.empty((n, oc, oh, ow), np.uint32)
    out[:] = fill.reshape(1, oc, 1, 1)
    q = np.nonzero(sq >= 0)[0]
    y = np.nonzero(sy >= 0)[0]
    xs = np.nonzero(sx >= 0)[0]
    if len(q) and len(y) and len(xs):
        out[np.ix_(np.arange(n), q, y, xs)] = bits[np.ix_(np.arange(n), sq[q], sy[y], sx[xs])]
    return out.view(F)


def pad(x, top=0, bottom=0, left=0, right=0, type_=CONSTANT, value=0.0, per_channel=None, front=0, behind=0):
    """ncnn's Padding: the window with margins >= 0."""
    if min(top, bottom, left, right, front, behind) < 0:
        raise ValueError("Padding margins are >= 0")
    return window(x, type_, value, per_channel, front, behind, top, bottom, left, right)


def crop_margins(c, h, w, woffset=0, hoffset=0, coffset=0, outw=-233, outh=-233, outc=-233, woffset2=0, hoffset2=0, coffset2=0):
    """ncnn's Crop parameters as the six margins of the window (front, behind, top, bottom, left, right), all <= 0."""
    def axis(dim, off, out, off2):
        if off < 0 or off2 < 0:
            raise ValueError("negative offset")
        size = dim - off - off2 if out == -233 else out
        if size < 1 or off + size > dim:
            raise ValueError("the window leaves the blob")
        return -off, off + size - dim
    f, b = axis(c, coffset, outc, coffset2)
    t, bo = axis(h, hoffset, outh, hoffset2)
    l, r = axis(w, woffset, outw, woffset2)
    return f, b, t, bo, l, r


def crop(x, woffset=0, hoffset=0, coffset=0, outw=-233, outh=-233, outc=-233, woffset2=0, hoffset2=0, coffset2=0, like=None):
    """ncnn's Crop; `like`: the reference blob of the two-bottom form, whose (c, h, w) are (outc, outh, outw)."""
    if like is not None:
        outc, outh, outw = like.shape[1:]
    f, b, t, bo, l, r = crop_margins(*x.shape[1:], woffset, hoffset, coffset, outw, outh, outc, woffset2, hoffset2, coffset2)
    return window(x, CONSTANT, 0.0, None, f, b, t, bo, l, r)


def pixel_shuffle_output_dim(r, c, h, w):
    if r < 1 or min(c, h, w) < 1 or c % (r * r):
        raise ValueError("PixelShuffle needs r >= 1 and a multiple of r * r channels")
    return c // (r * r), h * r, w * r


def activation(x, relu=RELU_NONE, slope=0.0):
    x = np.asarray(x, F)
    if relu == RELU_SLOPE:
        with np.errstate(invalid="ignore", over="ignore"):
            return np.where(x > 0, x, x * F(slope)).astype(F)
    if relu == RELU_PLAIN:
        return np.where(x > 0, x, F(0)).astype(F)  # fmaxf(x, 0.f): -0.0 and NaN become +0.0
    return x


def pixel_shuffle(x, r, mode=0, relu=RELU_NONE, slope=0.0):
    """PixelShuffle of x[n][C * r * r][h][w] (feather_frame.h): out[q][i * r + sh][j * r + sw] = in[channel(q, sh, sw)][i][j]."""
    x = np.ascontiguousarray(x, F)
    n, c, h, w = x.shape
    C, oh, ow = pixel_shuffle_output_dim(r, c, h, w)
    bits = x.view(np.uint32)
    out = np.empty((n, C, oh, ow), np.uint32)
    for q in range(C):
        for sh in range(r):
            for sw in range(r):
                ch = (sh * r + sw) * C + q if mode else q * r * r + sh * r + sw
                out[:, q, sh::r, sw::r] = bits[:, ch]
    return activation(out.view(F), relu, slope)


# ---- the .param reader the tests share ---------------------------------------------------------------------------------------------------
def parse_param(text):
    """-> [(type, name, bottoms, tops, {id: value})] of a .param text (bytes or str); array ids (-233xx) keep their list."""
    if isinstance(text, bytes):
        text = text.decode()
    out = []
    for line in text.splitlines()[2:]:
        tok = line.split()
        if not tok:
            continue
        nb, nt = int(tok[2]), int(tok[3])
        pd = {}
        for kv in tok[4 + nb + nt:]:
            k, v = kv.split("=")
            if int(k) <= -23300:
                pd[int(k)] = [float(e) for e in v.split(",")[1:]]
            else:
                pd[int(k)] = float(v) if any(ch in v for ch in ".eE") else int(v)
        out.append((tok[0], tok[1], tok[4:4 + nb], tok[4 + nb:4 + nb + nt], pd))
    return out
