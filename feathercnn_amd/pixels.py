"""uint8 images to the fp32 input tensor on the device: ncnn's ``Mat::from_pixels_resize`` (+ ``substract_mean_normalize``) for a
batch, over ``fhip_pixels_to_float`` (include/feather_hip/feather_net.h), and back: ``Mat::to_pixels_resize`` for a batch, over
``fhip_float_to_pixels`` (include/feather_hip/feather_pixout.h).  ``PIXEL_*`` are ncnn's codes (reference src/ncnn/mat.h:125-146)."""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from .booster import FeatherHipError, _check, _stream

PIXEL_CONVERT_SHIFT = 16
PIXEL_RGB = 1
PIXEL_BGR = 1 << 1
PIXEL_GRAY = 1 << 2
PIXEL_RGBA = 1 << 3
PIXEL_RGB2BGR = PIXEL_RGB | (PIXEL_BGR << PIXEL_CONVERT_SHIFT)
PIXEL_RGB2GRAY = PIXEL_RGB | (PIXEL_GRAY << PIXEL_CONVERT_SHIFT)
PIXEL_BGR2RGB = PIXEL_BGR | (PIXEL_RGB << PIXEL_CONVERT_SHIFT)
PIXEL_BGR2GRAY = PIXEL_BGR | (PIXEL_GRAY << PIXEL_CONVERT_SHIFT)
PIXEL_GRAY2RGB = PIXEL_GRAY | (PIXEL_RGB << PIXEL_CONVERT_SHIFT)
PIXEL_GRAY2BGR = PIXEL_GRAY | (PIXEL_BGR << PIXEL_CONVERT_SHIFT)
PIXEL_RGBA2RGB = PIXEL_RGBA | (PIXEL_RGB << PIXEL_CONVERT_SHIFT)
PIXEL_RGBA2BGR = PIXEL_RGBA | (PIXEL_BGR << PIXEL_CONVERT_SHIFT)
PIXEL_RGBA2GRAY = PIXEL_RGBA | (PIXEL_GRAY << PIXEL_CONVERT_SHIFT)

_CHANNELS = {PIXEL_RGB: 3, PIXEL_BGR: 3, PIXEL_GRAY: 1, PIXEL_RGBA: 4}
_TYPES = (PIXEL_RGB, PIXEL_BGR, PIXEL_GRAY, PIXEL_RGBA, PIXEL_RGB2BGR, PIXEL_RGB2GRAY, PIXEL_BGR2RGB, PIXEL_BGR2GRAY, PIXEL_GRAY2RGB,
          PIXEL_GRAY2BGR, PIXEL_RGBA2RGB, PIXEL_RGBA2BGR, PIXEL_RGBA2GRAY)


def pixel_channels(ptype: int):
    """(source channels, output channels) of a pixel type."""
    if ptype not in _TYPES:
        raise FeatherHipError(f"unknown pixel type {ptype:#x}")
    return _CHANNELS[ptype & 0xFFFF], _CHANNELS[(ptype >> 16) or (ptype & 0xFFFF)]


def _per_channel(v, cout, what):
    """A host float32 array of cout values (kept alive by the caller) and its pointer, or (None, None)."""
    if v is None:
        return None, None
    a = np.ascontiguousarray(np.asarray(v, dtype=np.float32).reshape(-1))
    if a.size != cout:
        raise FeatherHipError(f"{what} needs {cout} values (one per output channel), got {a.size}")
    return a, a.ctypes.data_as(ctypes.c_void_p)


def _images(pixels, ptype):
    """(n, h, w, pointer, on_device, keep-alive) of a uint8 [N][H][W][C] / [H][W][C] numpy array or CUDA tensor."""
    import torch
    cin, _ = pixel_channels(ptype)
    if isinstance(pixels, torch.Tensor):
        if not pixels.is_cuda or pixels.dtype != torch.uint8:
            raise FeatherHipError("pixels: a uint8 CUDA tensor or a uint8 numpy array")
        t = pixels.contiguous()
        shape, ptr, dev = tuple(t.shape), t.data_ptr(), 1
    else:
        t = np.ascontiguousarray(pixels)
        if t.dtype != np.uint8:
            raise FeatherHipError("pixels: a uint8 CUDA tensor or a uint8 numpy array")
        shape, ptr, dev = t.shape, t.ctypes.data, 0
    if len(shape) == 3:
        shape = (1,) + tuple(shape)
    if len(shape) != 4 or shape[3] != cin:
        raise FeatherHipError(f"pixels: [N][H][W][{cin}] or [H][W][{cin}] for pixel type {ptype:#x}, got {tuple(shape)}")
    n, h, w, _ = (int(v) for v in shape)
    return n, h, w, ctypes.c_void_p(ptr), dev, t


def pixels_to_float(pixels, ptype: int, target=None, mean=None, norm=None, out=None):
    """ncnn's from_pixels_resize (+ substract_mean_normalize) of a batch on the current stream: uint8 CUDA tensor [N][H][W][C] (or
    [H][W][C]) -> fp32 CUDA tensor [N][cout][target_h][target_w].  target = (w, h), default the source size; mean / norm: cout values
    or None.  `out` may be given (a contiguous fp32 CUDA tensor of that shape)."""
    import torch
    if not (isinstance(pixels, torch.Tensor) and pixels.is_cuda):
        raise FeatherHipError("pixels_to_float wants a uint8 CUDA tensor (Net.FeedPixels takes host arrays too)")
    n, h, w, ptr, _, keep = _images(pixels, ptype)
    tw, th = (w, h) if target is None else (int(target[0]), int(target[1]))
    _, cout = pixel_channels(ptype)
    m, mp = _per_channel(mean, cout, "mean")
    s, sp = _per_channel(norm, cout, "norm")
    if out is None:
        out = torch.empty((n, cout, th, tw), dtype=torch.float32, device=keep.device)
    elif tuple(out.shape) != (n, cout, th, tw) or out.dtype != torch.float32 or not out.is_contiguous():
        raise FeatherHipError(f"out must be a contiguous fp32 tensor of shape {(n, cout, th, tw)}")
    _check(_lib.load_library().fhip_pixels_to_float(ctypes.c_void_p(out.data_ptr()), ptr, n, int(ptype), w, h, tw, th, mp, sp, _stream()),
           "fhip_pixels_to_float")
    del m, s  # read by value at the call
    return out


# ---- NV21 (yuv420sp) frames ----------------------------------------------------------------------------------------------------------
_YUV_TYPES = (PIXEL_RGB, PIXEL_RGB2BGR, PIXEL_RGB2GRAY)


def _frames(frames, ptype):
    """(n, w, h, cout, pointer, on_device, keep-alive) of uint8 NV21 frames [N][h*3/2][w] / [h*3/2][w], numpy array or CUDA tensor."""
    import torch
    if ptype not in _YUV_TYPES:
        raise FeatherHipError(f"pixel type {ptype:#x}: an NV21 frame converts as PIXEL_RGB, PIXEL_RGB2BGR or PIXEL_RGB2GRAY")
    if isinstance(frames, torch.Tensor):
        if not frames.is_cuda or frames.dtype != torch.uint8:
            raise FeatherHipError("frames: a uint8 CUDA tensor or a uint8 numpy array")
        t = frames.contiguous()
        shape, ptr, dev = tuple(t.shape), t.data_ptr(), 1
    else:
        t = np.ascontiguousarray(frames)
        if t.dtype != np.uint8:
            raise FeatherHipError("frames: a uint8 CUDA tensor or a uint8 numpy array")
        shape, ptr, dev = t.shape, t.ctypes.data, 0
    if len(shape) == 2:
        shape = (1,) + tuple(shape)
    if len(shape) != 3 or shape[1] % 3:
        raise FeatherHipError(f"frames: NV21 [N][h*3/2][w] or [h*3/2][w], got {tuple(shape)}")
    n, rows, w = (int(v) for v in shape)
    return n, w, rows * 2 // 3, 1 if ptype == PIXEL_RGB2GRAY else 3, ctypes.c_void_p(ptr), dev, t


def yuv420sp_to_float(frames, ptype: int = PIXEL_RGB, target=None, resize_first: bool = True, mean=None, norm=None, out=None):
    """NV21 camera frames to the fp32 tensor on the current stream (fhip_yuv420sp_to_float): uint8 CUDA tensor [N][h*3/2][w] (or
    [h*3/2][w]) -> fp32 CUDA tensor [N][cout][target_h][target_w], bit-identical to the reference's chain
    resize_bilinear_yuv420sp -> yuv420sp2rgb -> from_pixels (resize_first) or yuv420sp2rgb -> from_pixels_resize (not resize_first).
    ptype: PIXEL_RGB, PIXEL_RGB2BGR or PIXEL_RGB2GRAY; target = (w, h), default the frame size; mean / norm: cout values or None."""
    import torch
    if not (isinstance(frames, torch.Tensor) and frames.is_cuda):
        raise FeatherHipError("yuv420sp_to_float wants a uint8 CUDA tensor (Net.FeedYUV420sp takes host arrays too)")
    n, w, h, cout, ptr, _, keep = _frames(frames, ptype)
    tw, th = (w, h) if target is None else (int(target[0]), int(target[1]))
    m, mp = _per_channel(mean, cout, "mean")
    s, sp = _per_channel(norm, cout, "norm")
    if out is None:
        out = torch.empty((n, cout, th, tw), dtype=torch.float32, device=keep.device)
    elif tuple(out.shape) != (n, cout, th, tw) or out.dtype != torch.float32 or not out.is_contiguous():
        raise FeatherHipError(f"out must be a contiguous fp32 tensor of shape {(n, cout, th, tw)}")
    _check(_lib.load_library().fhip_yuv420sp_to_float(ctypes.c_void_p(out.data_ptr()), ptr, n, int(ptype), w, h, tw, th, int(bool(resize_first)),
                                                      mp, sp, _stream()), "fhip_yuv420sp_to_float")
    del m, s  # read by value at the call
    return out


# ---- mixed-size batches: per-image size, pitch and ROI ----------------------------------------------------------------------------
def _image_descs(images, ptype, rois):
    """(ctypes array of fhip_pixel_image, on_device, keep-alive) of a list of uint8 [H][W][C] numpy arrays or CUDA tensors, all of one
    kind.  A view whose pixels are contiguous within a row (img[y0:y1, x0:x1] included) is passed as it is, its row stride as the pitch;
    anything else is copied.  rois: None, or one (x, y, w, h) or None per image."""
    import torch
    cin, _ = pixel_channels(ptype)
    images = list(images)
    if not images:
        raise FeatherHipError("images: an empty list")
    if rois is not None and len(rois) != len(images):
        raise FeatherHipError(f"rois: {len(rois)} entries for {len(images)} images")
    on_device = isinstance(images[0], torch.Tensor)
    descs = (_lib.fhip_pixel_image * len(images))()
    keep = []
    for i, img in enumerate(images):
        if on_device:
            if not (isinstance(img, torch.Tensor) and img.is_cuda and img.dtype == torch.uint8):
                raise FeatherHipError(f"images[{i}]: every image a uint8 CUDA tensor, or every image a uint8 numpy array")
            if img.dim() != 3 or img.stride(2) != 1 or img.stride(1) != img.shape[2] or img.stride(0) < img.shape[1] * img.shape[2]:
                img = img.contiguous()
            shape, pitch, ptr = tuple(img.shape), img.stride(0), img.data_ptr()
        else:
            if isinstance(img, torch.Tensor) or not isinstance(img, np.ndarray) or img.dtype != np.uint8:
                raise FeatherHipError(f"images[{i}]: every image a uint8 CUDA tensor, or every image a uint8 numpy array")
            if img.ndim != 3 or img.strides[2] != 1 or img.strides[1] != img.shape[2] or img.strides[0] < img.shape[1] * img.shape[2]:
                img = np.ascontiguousarray(img)
            shape, pitch, ptr = img.shape, img.strides[0], img.ctypes.data
        if len(shape) != 3 or shape[2] != cin:
            raise FeatherHipError(f"images[{i}]: [H][W][{cin}] for pixel type {ptype:#x}, got {tuple(shape)}")
        keep.append(img)
        d = descs[i]
        d.data, d.h, d.w, d.stride = ptr, int(shape[0]), int(shape[1]), int(pitch)
        if rois is not None and rois[i] is not None:
            d.roi_x, d.roi_y, d.roi_w, d.roi_h = (int(v) for v in rois[i])
    return descs, int(on_device), keep


def _plan(descs, ptype, tw, th):
    """The host plan of fhip_pixel_images_plan as a uint8 numpy array (8-byte aligned)."""
    lib = _lib.load_library()
    size = ctypes.c_size_t(0)
    _check(lib.fhip_pixel_images_plan(descs, len(descs), int(ptype), tw, th, None, ctypes.byref(size)), "fhip_pixel_images_plan")
    buf = np.zeros((size.value + 7) // 8, np.uint64).view(np.uint8)[:size.value]
    _check(lib.fhip_pixel_images_plan(descs, len(descs), int(ptype), tw, th, buf.ctypes.data_as(ctypes.c_void_p), ctypes.byref(size)),
           "fhip_pixel_images_plan")
    return buf


def pixels_images_to_float(images, ptype: int, target, rois=None, mean=None, norm=None, out=None):
    """A mixed-size batch on the current stream (fhip_pixels_to_float_images): `images` a list of uint8 CUDA tensors [H][W][C] (row-strided
    views are read in place), rois None or one (x, y, w, h) / None per image -> fp32 CUDA tensor [N][cout][target_h][target_w], image i
    bit-identical to from_pixels_resize of a dense copy of its ROI.  The plan is uploaded as a CUDA tensor on the current stream."""
    import torch
    descs, dev, keep = _image_descs(images, ptype, rois)
    if not dev:
        raise FeatherHipError("pixels_images_to_float wants uint8 CUDA tensors (Net.FeedPixelImages takes host arrays too)")
    tw, th = int(target[0]), int(target[1])
    _, cout = pixel_channels(ptype)
    m, mp = _per_channel(mean, cout, "mean")
    s, sp = _per_channel(norm, cout, "norm")
    plan = _plan(descs, ptype, tw, th)
    n = len(descs)
    device = keep[0].device
    plan_dev = torch.from_numpy(plan).to(device)  # on the current stream; freed into the caching allocator after the launch below
    if out is None:
        out = torch.empty((n, cout, th, tw), dtype=torch.float32, device=device)
    elif tuple(out.shape) != (n, cout, th, tw) or out.dtype != torch.float32 or not out.is_contiguous():
        raise FeatherHipError(f"out must be a contiguous fp32 tensor of shape {(n, cout, th, tw)}")
    _check(_lib.load_library().fhip_pixels_to_float_images(ctypes.c_void_p(out.data_ptr()), plan.ctypes.data_as(ctypes.c_void_p),
                                                           ctypes.c_void_p(plan_dev.data_ptr()), mp, sp, _stream()),
           "fhip_pixels_to_float_images")
    del m, s, keep  # read at the call (the plan's bytes are on the device)
    return out


# ---- the output side: fp32 tensors to uint8 images (libfeather_pixout.so) -------------------------------------------------------------
_OUT_CHANNELS = {PIXEL_RGB: 3, PIXEL_BGR: 3, PIXEL_GRAY: 1, PIXEL_RGBA: 4, PIXEL_RGB2BGR: 3, PIXEL_BGR2RGB: 3}


def output_channels(ptype: int) -> int:
    """Channels of an OUTPUT pixel type (the six Mat::to_pixels writes anything for); every other type is refused."""
    if ptype not in _OUT_CHANNELS:
        raise FeatherHipError(f"pixel type {ptype:#x} is not an output type: PIXEL_RGB, PIXEL_BGR, PIXEL_GRAY, PIXEL_RGBA, PIXEL_RGB2BGR "
                              "or PIXEL_BGR2RGB")
    return _OUT_CHANNELS[ptype]


_check_pixout = _lib.checker(_lib.load_pixout_library, "fhip_pixout_last_error")


def float_to_pixels(x, ptype: int, target=None, mean=None, norm=None, out=None):
    """ncnn's Mat::to_pixels_resize (after substract_mean_normalize when mean / norm are given) of a batch on the current stream
    (fhip_float_to_pixels): fp32 CUDA tensor [N][C][h][w] (or [C][h][w]) -> uint8 CUDA tensor [N][target_h][target_w][C], bit-identical
    to the reference per image.  ptype: PIXEL_RGB, PIXEL_BGR, PIXEL_GRAY, PIXEL_RGBA, PIXEL_RGB2BGR or PIXEL_BGR2RGB, whose channels must
    be C; target = (w, h), default the source size; mean / norm: C values (per plane of x) or None.  `out` may be given: a uint8 CUDA
    tensor of that shape whose pixels and rows are contiguous -- a view into a padded frame works, its row stride is the pitch and the
    bytes between its rows are not touched."""
    import torch
    cn = output_channels(ptype)
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float32:
        raise FeatherHipError("float_to_pixels wants an fp32 CUDA tensor")
    shape = tuple(x.shape)
    if len(shape) == 3:
        shape = (1,) + shape
    if len(shape) != 4 or shape[1] != cn:
        raise FeatherHipError(f"x: [N][{cn}][h][w] or [{cn}][h][w] for pixel type {ptype:#x}, got {tuple(x.shape)}")
    if not x.is_cuda:
        raise FeatherHipError("float_to_pixels wants an fp32 CUDA tensor")
    x = x.contiguous()
    n, _, h, w = (int(v) for v in shape)
    tw, th = (w, h) if target is None else (int(target[0]), int(target[1]))
    m, mp = _per_channel(mean, cn, "mean")
    s, sp = _per_channel(norm, cn, "norm")
    pitch = 0
    if out is None:
        out = torch.empty((n, th, tw, cn), dtype=torch.uint8, device=x.device)
    else:
        if not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == (n, th, tw, cn)):
            raise FeatherHipError(f"out must be a uint8 CUDA tensor of shape {(n, th, tw, cn)}")
        pitch = out.stride(1)
        if out.stride(3) != 1 or out.stride(2) != cn or pitch < tw * cn or out.stride(0) != th * pitch:
            raise FeatherHipError("out: pixels and rows must be contiguous, rows `pitch` bytes apart and images target_h * pitch apart")
    _check_pixout(_lib.load_pixout_library().fhip_float_to_pixels(ctypes.c_void_p(out.data_ptr()), pitch, ctypes.c_void_p(x.data_ptr()), n,
                                                                  int(ptype), w, h, tw, th, mp, sp, _stream()), "fhip_float_to_pixels")
    del m, s  # read by value at the call
    return out
