"""Camera frames -> backbone input on the GPU -- what the reference does on the CPU in two places: offline in
``preprocess.py`` (``cv2.warpAffine(image, trans, image_size, flags=INTER_LINEAR)`` with the matrix of
``get_resize_transform``) and per item in its loader (``lib/dataset/JointsDataset.py:129-133`` imread / BGR->RGB /
transform, ``run/validate.py:44-52`` ToTensor + Normalize).

Host side (this file): the inverse of the 2x3 ``resize_transform`` (float64, rounded once to fp32) and the launch.
Device side: ``fvp_ingest_frames`` (csrc/fvp_heatmap.hip) - bilinear warp with zero border, channel swap, / 255,
mean / std, written as fp32 ``[N,3,H,W]`` and / or straight into the bf16 input buffer of the HIP backbone
(``PoseResNet.forward_frames``).  The arithmetic is spelled out in ``include/fvp.h``; it is NOT bit-compatible with
OpenCV's fixed-point INTER_LINEAR.
"""
import ctypes as C

import numpy as np
import torch

from .. import _capi as capi

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


def _f3(v):
    v = [float(x) for x in v]
    assert len(v) == 3
    return (C.c_float * 3)(*v)


def launch(lib, frames, resize_transform, image_size, swap_rb, mean, std, nhwc8, nchw, general=False):
    """One ``fvp_ingest_frames`` call on the current stream.  ``frames`` uint8 ``[N,Hs,Ws,3]`` contiguous;
    ``image_size`` = (W, H) like ``cfg.DATASET.IMAGE_SIZE``; ``nhwc8`` / ``nchw``: output tensors or None."""
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[-1] != 3:
        raise capi.FvpError(f"frames must be uint8 [N,Hs,Ws,3], got {frames.dtype} {tuple(frames.shape)}")
    if not frames.is_contiguous():
        raise capi.FvpError("frames must be contiguous (HWC)")
    N, Hs, Ws, _ = frames.shape
    W, H = int(image_size[0]), int(image_size[1])
    inv = _inverse.get(resize_transform)
    flags = (capi.INGEST_SWAP_RB if swap_rb else 0) | (capi.INGEST_GENERAL if general else 0)
    stream = C.c_void_p(torch.cuda.current_stream(frames.device).cuda_stream) if frames.is_cuda else None
    rc = lib.fvp_ingest_frames(C.c_void_p(frames.data_ptr()), N, Hs, Ws, (C.c_float * 6)(*[float(v) for v in inv]),
                               _f3(mean), _f3(std), H, W, flags,
                               C.c_void_p(nhwc8.data_ptr()) if nhwc8 is not None else None,
                               C.c_void_p(nchw.data_ptr()) if nchw is not None else None, stream)
    capi.check(lib, rc, "fvp_ingest_frames")


def ingest_frames(frames, resize_transform, image_size, swap_rb=True, mean=IMAGENET_MEAN, std=IMAGENET_STD, out=None,
                  _lib=None):
    """``frames``: uint8 GPU tensor ``[N,Hs,Ws,3]`` (or ``[B,V,Hs,Ws,3]``) of camera frames at their native resolution,
    HWC; ``resize_transform``: the forward 2x3 (camera -> network pixels, ``get_resize_transform``) as a tensor or
    array - the object the model gets; ``image_size`` = (W, H).  ``swap_rb`` turns BGR frames (cv2.imread) into the RGB
    order the ImageNet constants are in.  Returns fp32 ``[N,3,H,W]`` (``[B,V,3,H,W]``): the tensor the reference's
    loader hands to the backbone."""
    if _lib is None and not frames.is_cuda:
        raise capi.FvpError("ingest_frames runs on the GPU only (no CPU fallback)")
    lib = _lib if _lib is not None else capi.load()
    lead = tuple(frames.shape[:-3])
    flat = frames.reshape(-1, *frames.shape[-3:]) if frames.dim() == 5 else frames
    W, H = int(image_size[0]), int(image_size[1])
    shape = (flat.shape[0], 3, H, W)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=frames.device)
    elif out.dtype != torch.float32 or out.numel() != flat.shape[0] * 3 * H * W or not out.is_contiguous() \
            or out.device != frames.device:
        raise capi.FvpError(f"out must be a contiguous float32 tensor of {shape} on {frames.device}")
    launch(lib, flat, resize_transform, (W, H), swap_rb, mean, std, None, out)
    return out.view(*lead, 3, H, W)
