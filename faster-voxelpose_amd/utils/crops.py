"""Person crops out: ``PersonCrops`` turns the per-view pixels of ``fvp_joint_evidence`` (``views``) into one box per (frame,
view, person) and cuts fixed-size, normalised patches of those boxes out of the camera frames, on the device
(``fvp_person_rois``, ``fvp_crop_rois``, ``fvp_crop_rois_nv12``; include/fvp.h, ABI 16) - what appearance features, a
top-down 2-D refiner, face blurring or an action classifier start from.  The crop is the ingest's arithmetic: patch r equals
``fvp_ingest_frames`` / ``fvp_ingest_nv12`` on its frame with the box's matrix, bit for bit.  A decoder's NV12 surface
(``dataset.images.Nv12Frames``) is read directly, with its own pitches and frame strides.  Two launches on the caller's
current HIP stream; no arithmetic on tensors happens here and nothing synchronises with the host: PyTorch is used for device
memory and streams only.

Not built: rotated boxes, anti-aliased down-scaling (a crop that shrinks by more than 2 x aliases as the ingest does),
I420 / P010 surfaces, compaction of the valid crops into a dense list, any appearance model.
"""
import math

import torch

from .. import _capi as capi
from .._args import f3, load_lib, require_gpu, stream_ptr, tensor_arg
from .._args import ptr as _ptr
from ..dataset.images import IMAGENET_MEAN, IMAGENET_STD, Nv12Frames

MAX_PEOPLE = 32                                          # the limit of fvp_person_rois


class PersonCrops:
    """``PersonCrops(num_joints_or_cfg, size=(256, 192), scale=1.25, pad_px=0.0, min_joints=2, joints=None, conf_min=0.0,
    mean=IMAGENET_MEAN, std=IMAGENET_STD, bf16=False, swap_rb=False)``

    ``num_joints_or_cfg``  J, or a config (``DATASET.NUM_JOINTS``);
    ``size``               (h, w) of a patch, w even; the box takes the aspect w / h;
    ``scale``              the joints' extent is multiplied by it (> 0), then ``pad_px`` (>= 0) pixels are added on each side;
    ``min_joints``         a box needs that many usable joints (>= 1) in the view; with fewer it is all zero, and so is its patch;
    ``joints``             the joint indices the box is built from (for example the head's); None: all J;
    ``conf_min``           with ``joint_conf`` given, a joint below it is not usable;
    ``mean``, ``std``      of the normalisation, in output channel order;
    ``bf16``               False: patches fp32 ``[B,V,N,3,h,w]``; True: ``[B,V,N,h,w/2,8]`` bfloat16, the pixel-pair input layout of
                           the bf16 backbone (channel 3 = 0);
    ``swap_rb``            RGB frames only: output channel c reads source channel 2 - c (BGR frames of cv2.imread).
    The defaults are API defaults, not tuned values."""

    def __init__(self, num_joints_or_cfg, size=(256, 192), scale=1.25, pad_px=0.0, min_joints=2, joints=None, conf_min=0.0,
                 mean=IMAGENET_MEAN, std=IMAGENET_STD, bf16=False, swap_rb=False, _lib=None):
        self.lib, self._injected = load_lib(_lib)
        J = num_joints_or_cfg if isinstance(num_joints_or_cfg, int) else num_joints_or_cfg.DATASET.NUM_JOINTS
        self.J = int(J)
        if not 1 <= self.J <= capi.FVP_MAX_JOINTS:
            raise capi.FvpError(f"PersonCrops needs 1 <= J <= {capi.FVP_MAX_JOINTS}, got {self.J}")
        try:
            self.h, self.w = (int(v) for v in size)
        except (TypeError, ValueError):
            raise capi.FvpError(f"size must be (h, w), got {size!r}") from None
        if self.h < 1 or self.w < 2 or self.w % 2:
            raise capi.FvpError(f"PersonCrops needs a patch of h >= 1 rows and an even w >= 2, got size = {size}")
        self.joints = list(range(self.J)) if joints is None else [int(j) for j in joints]
        if any(not (0 <= j < self.J) for j in self.joints):
            raise capi.FvpError(f"joints: indices in [0, {self.J}), got {joints}")
        self.joint_mask = 0
        for j in self.joints:
            self.joint_mask |= 1 << j
        self.scale, self.pad_px, self.conf_min = float(scale), float(pad_px), float(conf_min)
        self.min_joints = int(min_joints)
        if not (self.scale > 0 and math.isfinite(self.scale) and self.pad_px >= 0 and math.isfinite(self.pad_px)
                and self.min_joints >= 1) or self.conf_min != self.conf_min:
            raise capi.FvpError(f"PersonCrops needs a finite scale > 0, a finite pad_px >= 0, min_joints >= 1 and a conf_min "
                                f"that is not NaN (scale = {scale}, pad_px = {pad_px}, min_joints = {min_joints}, conf_min = "
                                f"{conf_min})")
        self.aspect = self.w / self.h
        self.mean, self.std = tuple(float(v) for v in mean), tuple(float(v) for v in std)
        if len(self.mean) != 3 or len(self.std) != 3 or not all(math.isfinite(v) for v in self.mean + self.std) \
                or any(v == 0 for v in self.std):
            raise capi.FvpError(f"mean and std: three finite values each, std non-zero (mean = {mean}, std = {std})")
        self.bf16, self.swap_rb = bool(bf16), bool(swap_rb)
        self._mean, self._std = f3(self.mean), f3(self.std)

    def rois(self, views, ids=None, joint_conf=None):
        """``views [B,V,N,J,4]`` (``last_evidence[0]``, or ``joint_evidence(...)[0]`` of any poses) -> ``(rois [B,V,N,4]``
        fp32 (x0, y0, x1, y1) in pixels of the original frame, not clipped; ``count [B,V,N]`` int32, the usable joints;
        ``score [B,V,N]`` fp32, their mean heatmap support in that view``)``.  ``ids [B,N]`` int32 (``last_tracks[0]``):
        slots with a negative id get no box; ``joint_conf [B,N,J]`` (``last_evidence[1]``): joints below ``conf_min`` are
        not usable.  A box without ``min_joints`` usable joints is zeros in all three.  One launch on the current stream."""
        v = tensor_arg("views", views, torch.float32, ("B", "V", "N", self.J, 4), hint="what joint_evidence returns")
        require_gpu("the box computation", v.device, self._injected)
        B, V, N = v.shape[:3]
        if not 1 <= N <= MAX_PEOPLE or V > capi.FVP_MAX_VIEWS:
            raise capi.FvpError(f"PersonCrops.rois limits: 1 <= N <= {MAX_PEOPLE}, V <= {capi.FVP_MAX_VIEWS} (N = {N}, V = {V})")
        tensor_arg("ids", ids, torch.int32, (B, N), v.device, hint="what PoseTracker.update returns", optional=True)
        c = tensor_arg("joint_conf", joint_conf, torch.float32, (B, N, self.J), v.device, optional=True)
        rois = torch.empty((B, V, N, 4), dtype=torch.float32, device=v.device)
        count = torch.empty((B, V, N), dtype=torch.int32, device=v.device)
        score = torch.empty((B, V, N), dtype=torch.float32, device=v.device)
        rc = self.lib.fvp_person_rois(_ptr(v), _ptr(ids), _ptr(c), B, V, N, self.J, self.joint_mask, self.min_joints,
                                      self.scale, self.pad_px, self.aspect, self.conf_min, _ptr(rois), _ptr(count),
                                      _ptr(score), stream_ptr(v.device))
        capi.check(self.lib, rc, "fvp_person_rois")
        return rois, count, score

    def crop(self, frames, rois):
        """Cut ``rois [B,V,K,4]`` fp32 (x0, y0, x1, y1; ``rois()``'s, or any caller-made boxes) out of ``frames`` - ``uint8
        [B,V,Hs,Ws,3]`` or an ``Nv12Frames`` with leading dimensions ``[B,V]`` - and return the patches: fp32
        ``[B,V,K,3,h,w]``, or with ``bf16=True`` bfloat16 ``[B,V,K,h,w/2,8]``.  A box that is not finite or has no area
        (an invalid box of ``rois()`` is zeros) gives an all-zero patch; pixels of a box outside the frame are the
        normalised 0.  One launch on the current stream."""
        f, r = frames, rois
        nv12 = isinstance(f, Nv12Frames)
        if nv12:
            if len(f.lead) != 2:
                raise capi.FvpError(f"an NV12 surface to crop from must have leading dimensions [B,V], got {f.lead}")
            B, V, Hs, Ws = f.lead[0], f.lead[1], f.Hs, f.Ws
        else:
            B, V, Hs, Ws = tensor_arg("frames", f, torch.uint8, ("B", "V", "Hs", "Ws", 3),
                                      hint="HWC camera frames; or Nv12Frames").shape[:4]
        require_gpu("the crop", f.device, self._injected)
        r = tensor_arg("rois", r, torch.float32, (B, V, "K", 4), f.device, hint="what rois() returns")
        if r.shape[2] < 1:
            raise capi.FvpError(f"rois must hold K >= 1 boxes per frame and view, got {tuple(r.shape)}")
        if nv12 and self.swap_rb:
            raise capi.FvpError("swap_rb is for RGB frames: an NV12 surface converts to R, G, B in that order")
        K = r.shape[2]
        R = B * V * K
        if self.bf16:
            out = torch.empty((B, V, K, self.h, self.w // 2, 8), dtype=torch.bfloat16, device=f.device)
            o16, o32 = _ptr(out), None
        else:
            out = torch.empty((B, V, K, 3, self.h, self.w), dtype=torch.float32, device=f.device)
            o16, o32 = None, _ptr(out)
        if nv12:
            rc = self.lib.fvp_crop_rois_nv12(_ptr(f.y), _ptr(f.uv), B * V, Hs, Ws, f.y_pitch, f.uv_pitch, f.y_frame_stride,
                                             f.uv_frame_stride, f.standard, _ptr(r), R, K, self._mean, self._std, self.h,
                                             self.w, o16, o32, stream_ptr(f.device))
            capi.check(self.lib, rc, "fvp_crop_rois_nv12")
            return out
        rc = self.lib.fvp_crop_rois(_ptr(f), B * V, Hs, Ws, _ptr(r), R, K, self._mean, self._std, self.h, self.w,
                                    capi.INGEST_SWAP_RB if self.swap_rb else 0, o16, o32, stream_ptr(f.device))
        capi.check(self.lib, rc, "fvp_crop_rois")
        return out

    def __call__(self, frames, views, ids=None, joint_conf=None):
        """``rois()`` then ``crop()``: returns ``(patches, rois, count, score)``."""
        rois, count, score = self.rois(views, ids=ids, joint_conf=joint_conf)
        return self.crop(frames, rois), rois, count, score
