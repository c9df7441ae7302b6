"""Camera frames -> backbone input on the GPU -- what the reference does on the CPU in two places: offline in
``preprocess.py`` (``cv2.warpAffine(image, trans, image_size, flags=INTER_LINEAR)`` with the matrix of
``get_resize_transform``) and per item in its loader (``lib/dataset/JointsDataset.py:129-133`` imread / BGR->RGB /
transform, ``run/validate.py:44-52`` ToTensor + Normalize).

Host side (this file): the inverse of the 2x3 ``resize_transform`` (float64, rounded once to fp32) and the launch.
Device side: ``fvp_ingest_frames`` (csrc/fvp_heatmap.hip) - bilinear warp with zero border, channel swap, / 255,
mean / std, written as fp32 ``[N,3,H,W]`` and / or straight into the bf16 input buffer of the HIP backbone
(``PoseResNet.forward_frames``).  The arithmetic is spelled out in ``include/fvp.h``; it is NOT bit-compatible with
OpenCV's fixed-point INTER_LINEAR.

NV12 surfaces - what a hardware decoder or a capture card leaves in device memory - go in without an RGB frame in
between: ``Nv12Frames`` describes the two planes (pitch and frame stride are the tensors' strides), ``ingest_nv12`` /
``launch_nv12`` call ``fvp_ingest_nv12``, whose outputs equal ``fvp_ingest_frames`` on the frame converted pixel by
pixel with the integer formula of ``include/fvp.h``.

Bayer raw frames - the 8-bit mosaic a machine-vision camera delivers, one byte per pixel - are the third input:
``BayerFrames`` describes them, ``ingest_bayer`` / ``launch_bayer`` call ``fvp_ingest_bayer`` (no RGB frame in between),
``demosaic_bayer`` / ``BayerFrames.to_rgb`` call ``fvp_demosaic_bayer`` for the stages that work on an RGB frame.  The
outputs of the first equal ``fvp_ingest_frames`` on the output of the second, bit for bit.
"""
import ctypes as C
import math

import numpy as np
import torch

from .. import _capi as capi
from .._args import f3, load_lib, ptr, require_gpu, stream_ptr, tensor_arg

IMAGENET_MEAN = (0.485, 0.456, 0.406)        # run/validate.py:44-45
IMAGENET_STD = (0.229, 0.224, 0.225)


def invert_affine(resize_transform):
    """Forward 2x3 (camera -> network pixels) -> fp32[6] destination -> source matrix: inverted in float64, rounded once."""
    t = np.asarray(resize_transform.detach().cpu() if isinstance(resize_transform, torch.Tensor) else resize_transform,
                   dtype=np.float64).reshape(2, 3)
    det = t[0, 0] * t[1, 1] - t[0, 1] * t[1, 0]
    if not np.isfinite(det) or det == 0.0:
        raise capi.FvpError("resize_transform is singular")
    a = np.array([[t[1, 1], -t[0, 1]], [-t[1, 0], t[0, 0]]]) / det
    b = -a @ t[:, 2]
    return np.concatenate([a, b[:, None]], axis=1).reshape(6).astype(np.float32)


class _InverseCache:
    """The inverse of the last ``resize_transform`` tensor seen, keyed by identity / address / version like the engine's
    geometry (engine.HotPath.geom): reading a GPU tensor costs one host synchronisation, which a steady-state or
    captured forward must not have."""

    def __init__(self):
        self.key, self.ref, self.inv = None, None, None

    def get(self, resize_transform):
        if not isinstance(resize_transform, torch.Tensor):
            return invert_affine(resize_transform)
        key = (id(resize_transform), resize_transform.data_ptr(), resize_transform._version)
        if key != self.key:
            self.inv = invert_affine(resize_transform)
            self.key, self.ref = key, resize_transform      # pin the tensor so id / address cannot be recycled
        return self.inv


_inverse = _InverseCache()


def launch(lib, frames, resize_transform, image_size, swap_rb, mean, std, nhwc8, nchw, general=False):
    """One ``fvp_ingest_frames`` call on the current stream.  ``frames`` uint8 ``[N,Hs,Ws,3]`` contiguous;
    ``image_size`` = (W, H) like ``cfg.DATASET.IMAGE_SIZE``; ``nhwc8`` / ``nchw``: output tensors or None."""
    N, Hs, Ws, _ = tensor_arg("frames", frames, torch.uint8, ("N", "Hs", "Ws", 3), hint="HWC").shape
    W, H = int(image_size[0]), int(image_size[1])
    inv = _inverse.get(resize_transform)
    flags = (capi.INGEST_SWAP_RB if swap_rb else 0) | (capi.INGEST_GENERAL if general else 0)
    rc = lib.fvp_ingest_frames(ptr(frames), N, Hs, Ws, (C.c_float * 6)(*[float(v) for v in inv]), f3(mean), f3(std), H, W,
                               flags, ptr(nhwc8), ptr(nchw), stream_ptr(frames.device))
    capi.check(lib, rc, "fvp_ingest_frames")


def _out_arg(out, shape, device):
    """The fp32 output of an ingest call: a new tensor, or the caller's - held to its element count, not to a shape."""
    if out is None:
        return torch.empty(shape, dtype=torch.float32, device=device)
    if out.dtype != torch.float32 or out.numel() != math.prod(shape) or not out.is_contiguous() or out.device != device:
        raise capi.FvpError(f"out must be a contiguous float32 tensor of {shape} on {device}")
    return out


def ingest_frames(frames, resize_transform, image_size, swap_rb=True, mean=IMAGENET_MEAN, std=IMAGENET_STD, out=None,
                  _lib=None):
    """``frames``: uint8 GPU tensor ``[N,Hs,Ws,3]`` (or ``[B,V,Hs,Ws,3]``) of camera frames at their native resolution,
    HWC; ``resize_transform``: the forward 2x3 (camera -> network pixels, ``get_resize_transform``) as a tensor or
    array - the object the model gets; ``image_size`` = (W, H).  ``swap_rb`` turns BGR frames (cv2.imread) into the RGB
    order the ImageNet constants are in.  Returns fp32 ``[N,3,H,W]`` (``[B,V,3,H,W]``): the tensor the reference's
    loader hands to the backbone."""
    require_gpu("ingest_frames", frames.device, _lib is not None)
    lib, _ = load_lib(_lib)
    lead = tuple(frames.shape[:-3])
    flat = frames.reshape(-1, *frames.shape[-3:]) if frames.dim() == 5 else frames
    W, H = int(image_size[0]), int(image_size[1])
    out = _out_arg(out, (flat.shape[0], 3, H, W), frames.device)
    launch(lib, flat, resize_transform, (W, H), swap_rb, mean, std, None, out)
    return out.view(*lead, 3, H, W)


YUV_STANDARDS = {("bt601", False): capi.YUV_BT601_LIMITED, ("bt709", False): capi.YUV_BT709_LIMITED,
                 ("bt601", True): capi.YUV_BT601_FULL, ("bt709", True): capi.YUV_BT709_FULL}


def _frame_stride(t, nlead, what):
    """Element stride from frame to frame of ``t`` whose first ``nlead`` dimensions count frames: they must flatten to
    one constant stride (None when there is a single frame: any stride does)."""
    dims = [(n, st) for n, st in zip(t.shape[:nlead], t.stride()[:nlead]) if n != 1]
    for (_, outer), (n, inner) in zip(dims, dims[1:]):
        if outer != n * inner:
            raise capi.FvpError(f"{what}: the leading dimensions {tuple(t.shape[:nlead])} with strides "
                                f"{tuple(t.stride()[:nlead])} do not flatten to one constant frame stride")
    return dims[-1][1] if dims else None


class Nv12Frames:
    """NV12 camera frames in device memory, as two views of the decoder's surface (no copy):

    ``y``   uint8 ``[..., Hs, Ws]``: the luma plane; ``uv`` uint8 ``[..., Hs/2, Ws/2, 2]``: the interleaved (U, V) plane,
    same leading dimensions.  The last dimension of ``y`` and the last two of ``uv`` are dense; the row stride is the
    surface's pitch and the stride between frames is free, as long as the leading dimensions flatten to one constant
    frame stride.  ``standard``: ``"bt601"`` or ``"bt709"``; ``full_range``: 0..255 luma instead of 16..235."""

    def __init__(self, y, uv, standard="bt601", full_range=False):
        key = (str(standard).lower(), bool(full_range))
        if key not in YUV_STANDARDS:
            raise capi.FvpError(f"unknown colour standard {standard!r} (bt601 or bt709)")
        for name, t in (("y", y), ("uv", uv)):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8:
                raise capi.FvpError(f"{name} must be a uint8 tensor")
        if y.dim() < 2 or uv.dim() != y.dim() + 1 or uv.shape[-1] != 2:
            raise capi.FvpError(f"y must be [...,Hs,Ws] and uv [...,Hs/2,Ws/2,2], got {tuple(y.shape)} and {tuple(uv.shape)}")
        Hs, Ws = int(y.shape[-2]), int(y.shape[-1])
        if Hs < 2 or Ws < 2 or Hs % 2 or Ws % 2:
            raise capi.FvpError(f"NV12 frames have even, non-zero height and width, got {Hs} x {Ws}")
        if tuple(uv.shape[-3:-1]) != (Hs // 2, Ws // 2):
            raise capi.FvpError(f"uv must be [...,{Hs // 2},{Ws // 2},2] for y [...,{Hs},{Ws}], got {tuple(uv.shape)}")
        if tuple(y.shape[:-2]) != tuple(uv.shape[:-3]):
            raise capi.FvpError(f"y and uv differ in their leading dimensions: {tuple(y.shape[:-2])} and {tuple(uv.shape[:-3])}")
        if y.device != uv.device:
            raise capi.FvpError("y and uv are on different devices")
        if y.stride(-1) != 1 or uv.stride(-1) != 1 or uv.stride(-2) != 2:
            raise capi.FvpError("the last dimension of y and the last two of uv must be dense (a row is Ws bytes in a "
                                "row, only the pitch between rows is free)")
        self.y, self.uv, self.standard = y, uv, YUV_STANDARDS[key]
        self.lead = tuple(y.shape[:-2])
        self.N = 1
        for n in self.lead:
            self.N *= int(n)
        self.Hs, self.Ws = Hs, Ws
        self.y_pitch, self.uv_pitch = int(y.stride(-2)), int(uv.stride(-3))
        nlead = len(self.lead)
        ys, us = _frame_stride(y, nlead, "y"), _frame_stride(uv, nlead, "uv")
        self.y_frame_stride = int(ys) if ys is not None else Hs * self.y_pitch
        self.uv_frame_stride = int(us) if us is not None else (Hs // 2) * self.uv_pitch
        self.device, self.is_cuda = y.device, y.is_cuda

    @classmethod
    def from_buffer(cls, buf, height, width, pitch=None, standard="bt601", full_range=False):
        """The layout a decoder hands out: ``buf`` uint8 ``[..., Hs*3/2, pitch]`` - Hs rows of luma, then Hs/2 rows of
        interleaved chroma, ``pitch >= Ws`` bytes per row (``pitch`` defaults to the last dimension; with ``pitch``
        given, a flat ``[..., Hs*3/2 * pitch]`` buffer is accepted too).  The two planes are views of ``buf``."""
        Hs, Ws = int(height), int(width)
        if Hs < 2 or Ws < 2 or Hs % 2 or Ws % 2:
            raise capi.FvpError(f"NV12 frames have even, non-zero height and width, got {Hs} x {Ws}")
        rows = Hs * 3 // 2
        if not isinstance(buf, torch.Tensor) or buf.dtype != torch.uint8 or buf.dim() < 1:
            raise capi.FvpError("buf must be a uint8 tensor")
        if pitch is not None and (buf.dim() < 2 or buf.shape[-1] != int(pitch) or buf.shape[-2] != rows):
            if buf.shape[-1] != rows * int(pitch) or buf.stride(-1) != 1:
                raise capi.FvpError(f"buf {tuple(buf.shape)} is neither [...,{rows},{pitch}] nor [...,{rows * int(pitch)}]")
            buf = buf.unflatten(-1, (rows, int(pitch)))
        if buf.dim() < 2 or buf.shape[-2] != rows or buf.shape[-1] < Ws:
            raise capi.FvpError(f"buf must be [...,{rows},pitch >= {Ws}] for {Hs} x {Ws} frames, got {tuple(buf.shape)}")
        if buf.stride(-1) != 1:
            raise capi.FvpError("the rows of buf must be dense")
        y = buf[..., :Hs, :Ws]
        uv = buf[..., Hs:, :Ws].unflatten(-1, (Ws // 2, 2))
        return cls(y, uv, standard, full_range)


def launch_nv12(lib, frames, resize_transform, image_size, mean, std, nhwc8, nchw):
    """One ``fvp_ingest_nv12`` call on the current stream: the NV12 counterpart of ``launch`` (same cached inverse)."""
    if not isinstance(frames, Nv12Frames):
        raise capi.FvpError(f"frames must be Nv12Frames, got {type(frames).__name__}")
    W, H = int(image_size[0]), int(image_size[1])
    inv = _inverse.get(resize_transform)
    rc = lib.fvp_ingest_nv12(ptr(frames.y), ptr(frames.uv), frames.N, frames.Hs, frames.Ws, frames.y_pitch, frames.uv_pitch,
                             frames.y_frame_stride, frames.uv_frame_stride, frames.standard,
                             (C.c_float * 6)(*[float(v) for v in inv]), f3(mean), f3(std), H, W, ptr(nhwc8), ptr(nchw),
                             stream_ptr(frames.device))
    capi.check(lib, rc, "fvp_ingest_nv12")


def ingest_nv12(frames, resize_transform, image_size, mean=IMAGENET_MEAN, std=IMAGENET_STD, out=None, _lib=None):
    """``frames``: ``Nv12Frames`` on the GPU with leading dimensions ``[...]``; ``resize_transform`` and ``image_size``
    as for ``ingest_frames``.  Returns fp32 ``[...,3,H,W]``, RGB order: bit for bit what ``ingest_frames(...,
    swap_rb=False)`` returns for the frames converted to RGB with the integer formula of ``include/fvp.h``."""
    if not isinstance(frames, Nv12Frames):
        raise capi.FvpError(f"frames must be Nv12Frames, got {type(frames).__name__}")
    require_gpu("ingest_nv12", frames.device, _lib is not None)
    lib, _ = load_lib(_lib)
    W, H = int(image_size[0]), int(image_size[1])
    out = _out_arg(out, (frames.N, 3, H, W), frames.device)
    launch_nv12(lib, frames, resize_transform, (W, H), mean, std, None, out)
    return out.view(*frames.lead, 3, H, W)


BAYER_PATTERNS = {"rggb": capi.BAYER_RGGB, "grbg": capi.BAYER_GRBG, "gbrg": capi.BAYER_GBRG, "bggr": capi.BAYER_BGGR}


class BayerFrames:
    """8-bit Bayer raw camera frames in device memory (no copy):

    ``raw``  uint8 ``[..., Hs, Ws]``, Hs and Ws even and >= 4.  The last dimension is dense, the row stride is the pitch
    (any value >= Ws, odd ones included) and the leading dimensions flatten to one constant frame stride.  ``pattern``:
    the 2 x 2 cell at the top-left corner, ``"rggb"`` (BayerRG8), ``"grbg"`` (GR8), ``"gbrg"`` (GB8) or ``"bggr"`` (BG8).
    ``tone``: uint8 ``[3,256]`` on the frames' device, applied per channel after the demosaic (``tone_table``), or None."""

    def __init__(self, raw, pattern="rggb", tone=None):
        key = str(pattern).lower()
        if key not in BAYER_PATTERNS:
            raise capi.FvpError(f"unknown Bayer pattern {pattern!r} (rggb, grbg, gbrg or bggr)")
        if not isinstance(raw, torch.Tensor) or raw.dtype != torch.uint8 or raw.dim() < 2:
            raise capi.FvpError("raw must be a uint8 tensor [...,Hs,Ws]")
        Hs, Ws = int(raw.shape[-2]), int(raw.shape[-1])
        if Hs < 4 or Ws < 4 or Hs % 2 or Ws % 2:
            raise capi.FvpError(f"Bayer frames have even height and width of at least 4, got {Hs} x {Ws}")
        if raw.stride(-1) != 1 or raw.stride(-2) < Ws:
            raise capi.FvpError("the last dimension of raw must be dense and its rows must not overlap (a row is Ws bytes "
                                "in a row, only the pitch between rows is free)")
        if tone is not None:
            if not isinstance(tone, torch.Tensor) or tone.dtype != torch.uint8 or tuple(tone.shape) != (3, 256) \
                    or not tone.is_contiguous():
                raise capi.FvpError("tone must be a contiguous uint8 tensor [3,256]")
            if tone.device != raw.device:
                raise capi.FvpError(f"tone is on {tone.device}, the frames are on {raw.device}")
        self.raw, self.pattern, self.tone = raw, BAYER_PATTERNS[key], tone
        self.lead = tuple(raw.shape[:-2])
        self.N = 1
        for n in self.lead:
            self.N *= int(n)
        self.Hs, self.Ws, self.pitch = Hs, Ws, int(raw.stride(-2))
        fs = _frame_stride(raw, len(self.lead), "raw")
        self.frame_stride = int(fs) if fs is not None else Hs * self.pitch
        self.device, self.is_cuda = raw.device, raw.is_cuda

    @staticmethod
    def tone_table(gains=(1.0, 1.0, 1.0), gamma=1.0, black=0, device=None):
        """uint8 ``[3,256]``: black level, white-balance gains (R, G, B) and gamma in one table, in float64:
        ``lut[c][v] = clip(rint(255 * clip((v - black) * gains[c] / (255 - black), 0, 1) ** (1 / gamma)), 0, 255)``."""
        if not 0 <= float(black) < 255 or not float(gamma) > 0 or len(gains) != 3:
            raise capi.FvpError("tone_table: 0 <= black < 255, gamma > 0 and three gains")
        v = np.arange(256, dtype=np.float64)
        lut = np.empty((3, 256), np.float64)
        for c in range(3):
            lin = np.clip((v - float(black)) * float(gains[c]) / (255.0 - float(black)), 0.0, 1.0)
            lut[c] = np.clip(np.rint(255.0 * lin ** (1.0 / float(gamma))), 0, 255)
        return torch.from_numpy(lut.astype(np.uint8)).to(device if device is not None else "cpu")

    def to_rgb(self, out=None, _lib=None):
        """The demosaiced frames, uint8 ``[...,Hs,Ws,3]`` in R, G, B order (``demosaic_bayer``)."""
        return demosaic_bayer(self, out=out, _lib=_lib)


def _bayer_arg(frames):
    if not isinstance(frames, BayerFrames):
        raise capi.FvpError(f"frames must be BayerFrames, got {type(frames).__name__}")


def launch_bayer(lib, frames, resize_transform, image_size, mean, std, nhwc8, nchw):
    """One ``fvp_ingest_bayer`` call on the current stream: the Bayer counterpart of ``launch`` (same cached inverse)."""
    _bayer_arg(frames)
    W, H = int(image_size[0]), int(image_size[1])
    inv = _inverse.get(resize_transform)
    rc = lib.fvp_ingest_bayer(ptr(frames.raw), frames.N, frames.Hs, frames.Ws, frames.pitch, frames.frame_stride,
                              frames.pattern, ptr(frames.tone), (C.c_float * 6)(*[float(v) for v in inv]), f3(mean), f3(std),
                              H, W, ptr(nhwc8), ptr(nchw), stream_ptr(frames.device))
    capi.check(lib, rc, "fvp_ingest_bayer")


def ingest_bayer(frames, resize_transform, image_size, mean=IMAGENET_MEAN, std=IMAGENET_STD, out=None, _lib=None):
    """``frames``: ``BayerFrames`` on the GPU with leading dimensions ``[...]``; ``resize_transform`` and ``image_size``
    as for ``ingest_frames``.  Returns fp32 ``[...,3,H,W]``, RGB order: bit for bit what ``ingest_frames(...,
    swap_rb=False)`` returns for ``demosaic_bayer(frames)``."""
    _bayer_arg(frames)
    require_gpu("ingest_bayer", frames.device, _lib is not None)
    lib, _ = load_lib(_lib)
    W, H = int(image_size[0]), int(image_size[1])
    out = _out_arg(out, (frames.N, 3, H, W), frames.device)
    launch_bayer(lib, frames, resize_transform, (W, H), mean, std, None, out)
    return out.view(*frames.lead, 3, H, W)


def demosaic_bayer(frames, out=None, _lib=None):
    """``frames``: ``BayerFrames`` on the GPU -> uint8 ``[...,Hs,Ws,3]`` in R, G, B order (one ``fvp_demosaic_bayer`` call
    on the current stream): the frames overlay, crops, re-ID and anonymiser take.  ``out``: a contiguous uint8 tensor of
    that many elements to write into."""
    _bayer_arg(frames)
    require_gpu("demosaic_bayer", frames.device, _lib is not None)
    lib, _ = load_lib(_lib)
    shape = (*frames.lead, frames.Hs, frames.Ws, 3)
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=frames.device)
    elif out.dtype != torch.uint8 or out.numel() != math.prod(shape) or not out.is_contiguous() or out.device != frames.device:
        raise capi.FvpError(f"out must be a contiguous uint8 tensor of {shape} on {frames.device}")
    rc = lib.fvp_demosaic_bayer(ptr(frames.raw), frames.N, frames.Hs, frames.Ws, frames.pitch, frames.frame_stride,
                                frames.pattern, ptr(frames.tone), 0, ptr(out), stream_ptr(frames.device))
    capi.check(lib, rc, "fvp_demosaic_bayer")
    return out.view(shape)
