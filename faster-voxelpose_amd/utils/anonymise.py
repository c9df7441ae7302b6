"""Faces out of the camera frames: ``FaceAnonymiser`` makes one head box per (frame, view, person) from the per-view pixels of
``fvp_joint_evidence`` (``views``) and replaces what the boxes cover in the camera frames, on the device and in place, by a
frame-anchored mosaic or by one colour (``fvp_person_rois`` with a head joint mask, then ``fvp_anonymise_rois`` /
``fvp_anonymise_rois_nv12``; include/fvp.h, ABI 23).  A decoder's NV12 surface (``dataset.images.Nv12Frames``) is written
directly, luma and chroma, with its own pitches and frame strides.  Two launches on the caller's current HIP stream; no
arithmetic on tensors happens here and nothing synchronises with the host: PyTorch is used for device memory and streams
only, so both launches can be captured into a hipGraph.

It is not a stage of the forward: call it behind the forward, after everything that reads clean pixels (``model.crops``,
``PersonReId``'s signature) and before ``PoseOverlay.draw``.

Not built: Gaussian blur, rotated boxes, a face detector (the box comes from the skeleton's head joints), I420 / P010
surfaces, pitched RGB frames.
"""
import ctypes as C
import math

import torch

from .. import _capi as capi
from .._args import load_lib, require_gpu, stream_ptr, tensor_arg
from .._args import ptr as _ptr
from ..dataset.images import Nv12Frames

MAX_PEOPLE, MAX_ROIS = 32, 64                            # the limits of fvp_person_rois and fvp_anonymise_rois
CELLS = (2, 4, 8, 16, 32)
SHAPES = {"rect": capi.ANON_RECT, "ellipse": capi.ANON_ELLIPSE}
MODES = {"mosaic": capi.ANON_MOSAIC, "fill": capi.ANON_FILL}
# joints of the head in the two joint sets with a default: Panoptic's 15 (neck 0, nose 1: LIMBS15 of utils.vis starts with
# the neck-nose limb) and COCO-17 (nose 0, eyes 1 2, ears 3 4: the five joints LIMBS17 ties to the shoulders 5 6 through the ears)
_HEAD_JOINTS = {15: (0, 1), 17: (0, 1, 2, 3, 4)}


class FaceAnonymiser:
    """``FaceAnonymiser(num_joints_or_cfg, joints=None, scale=3.0, pad_px=2.0, min_joints=1, aspect=1.0, conf_min=0.0,
    cell=8, shape="ellipse", mode="mosaic", colour=(0, 0, 0))``

    ``num_joints_or_cfg``  J, or a config (``DATASET.NUM_JOINTS``);
    ``joints``             the joint indices the head box is built from; None: neck and nose for J = 15 (Panoptic), nose,
                           eyes and ears for J = 17 (COCO); any other J needs them given;
    ``scale``              the head joints' extent is multiplied by it (> 0), then ``pad_px`` (>= 0) pixels are added on each side;
    ``min_joints``         a box needs that many usable head joints (>= 1) in the view; with fewer nothing is hidden there;
    ``aspect``             width / height of the box (> 0);
    ``conf_min``           with ``joint_conf`` given, a joint below it is not usable;
    ``cell``               side of a mosaic cell in pixels: 2, 4, 8, 16 or 32; cells are anchored at the frame's origin;
    ``shape``              ``"ellipse"`` (inscribed in the box) or ``"rect"``;
    ``mode``               ``"mosaic"`` (a covered pixel takes the mean of its cell) or ``"fill"`` (it takes ``colour``);
    ``colour``             R, G, B of ``"fill"``, in the frames' channel order (an NV12 surface converts it by its standard).
    The defaults are API defaults, not tuned values: how far a head reaches beyond its joints depends on the joint set and
    on the camera, and is the caller's to choose."""

    def __init__(self, num_joints_or_cfg, joints=None, scale=3.0, pad_px=2.0, min_joints=1, aspect=1.0, conf_min=0.0, cell=8,
                 shape="ellipse", mode="mosaic", colour=(0, 0, 0), _lib=None):
        self.lib, self._injected = load_lib(_lib)
        J = num_joints_or_cfg if isinstance(num_joints_or_cfg, int) else num_joints_or_cfg.DATASET.NUM_JOINTS
        self.J = int(J)
        if not 1 <= self.J <= capi.FVP_MAX_JOINTS:
            raise capi.FvpError(f"FaceAnonymiser needs 1 <= J <= {capi.FVP_MAX_JOINTS}, got {self.J}")
        if joints is None:
            if self.J not in _HEAD_JOINTS:
                raise capi.FvpError(f"no default head joints for {self.J} joints (known: {sorted(_HEAD_JOINTS)}): pass joints")
            joints = _HEAD_JOINTS[self.J]
        self.joints = [int(j) for j in joints]
        if not self.joints or any(not (0 <= j < self.J) for j in self.joints):
            raise capi.FvpError(f"joints: at least one index in [0, {self.J}), got {joints}")
        self.joint_mask = 0
        for j in self.joints:
            self.joint_mask |= 1 << j
        self.scale, self.pad_px, self.aspect, self.conf_min = float(scale), float(pad_px), float(aspect), float(conf_min)
        self.min_joints = int(min_joints)
        if not (self.scale > 0 and math.isfinite(self.scale) and self.pad_px >= 0 and math.isfinite(self.pad_px)
                and self.aspect > 0 and math.isfinite(self.aspect) and self.min_joints >= 1) or self.conf_min != self.conf_min:
            raise capi.FvpError(f"FaceAnonymiser needs a finite scale > 0, a finite pad_px >= 0, a finite aspect > 0, min_joints "
                                f">= 1 and a conf_min that is not NaN (scale = {scale}, pad_px = {pad_px}, aspect = {aspect}, "
                                f"min_joints = {min_joints}, conf_min = {conf_min})")
        if cell not in CELLS:
            raise capi.FvpError(f"cell must be one of {CELLS}, got {cell!r}")
        if shape not in SHAPES or mode not in MODES:
            raise capi.FvpError(f"shape is one of {sorted(SHAPES)} and mode one of {sorted(MODES)}, got {shape!r} and {mode!r}")
        self.cell, self.shape, self.mode = int(cell), shape, mode
        try:
            self.colour = tuple(int(c) for c in colour)
        except (TypeError, ValueError):
            raise capi.FvpError(f"colour must be three integers in 0 .. 255, got {colour!r}") from None
        if len(self.colour) != 3 or not all(0 <= c <= 255 for c in self.colour):
            raise capi.FvpError(f"colour must be three integers in 0 .. 255, got {colour!r}")
        self._colour = (C.c_uint8 * 3)(*self.colour)

    def rois(self, views, ids=None, joint_conf=None):
        """``views [B,V,N,J,4]`` (``last_evidence[0]``, or ``joint_evidence(...)[0]`` of any poses) -> ``(rois [B,V,N,4]``
        fp32 (x0, y0, x1, y1), the head boxes in pixels of the original frame, not clipped; ``count [B,V,N]`` int32, the
        usable head joints; ``score [B,V,N]`` fp32, their mean heatmap support in that view``)``.  ``ids [B,N]`` int32
        (``last_tracks[0]``): slots with a negative id get no box; ``joint_conf [B,N,J]`` (``last_evidence[1]``): joints
        below ``conf_min`` are not usable.  A box without ``min_joints`` usable joints is zeros, which hides nothing.  One
        ``fvp_person_rois`` launch on the current stream."""
        v = tensor_arg("views", views, torch.float32, ("B", "V", "N", self.J, 4), hint="what joint_evidence returns")
        require_gpu("the head boxes", v.device, self._injected)
        B, V, N = v.shape[:3]
        if not 1 <= N <= MAX_PEOPLE or V > capi.FVP_MAX_VIEWS:
            raise capi.FvpError(f"FaceAnonymiser.rois limits: 1 <= N <= {MAX_PEOPLE}, V <= {capi.FVP_MAX_VIEWS} (N = {N}, V = {V})")
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

    def apply(self, frames, rois):
        """Hide what ``rois [B,V,K,4]`` fp32 (x0, y0, x1, y1; ``rois()``'s, or any caller-made boxes, K <= 64) cover in
        ``frames`` - ``uint8 [B,V,Hs,Ws,3]`` or an ``Nv12Frames`` with leading dimensions ``[B,V]`` - in place, and return
        ``frames``.  A box that is not finite, reaches beyond +-65536 or has no area hides nothing.  One launch on the
        current stream."""
        f, r = frames, rois
        nv12 = isinstance(f, Nv12Frames)
        if nv12:
            if len(f.lead) != 2:
                raise capi.FvpError(f"an NV12 surface to anonymise must have leading dimensions [B,V], got {f.lead}")
            B, V, Hs, Ws = f.lead[0], f.lead[1], f.Hs, f.Ws
        else:
            B, V, Hs, Ws = tensor_arg("frames", f, torch.uint8, ("B", "V", "Hs", "Ws", 3),
                                      hint="HWC camera frames; or Nv12Frames").shape[:4]
        require_gpu("the anonymiser", f.device, self._injected)
        r = tensor_arg("rois", r, torch.float32, (B, V, "K", 4), f.device, hint="what rois() returns")
        K = r.shape[2]
        if not 1 <= K <= MAX_ROIS:
            raise capi.FvpError(f"rois must hold 1 <= K <= {MAX_ROIS} boxes per frame and view, got {tuple(r.shape)}")
        tail = (_ptr(r), B * V * K, K, self.cell, SHAPES[self.shape], MODES[self.mode], self._colour, stream_ptr(f.device))
        if nv12:
            rc = self.lib.fvp_anonymise_rois_nv12(_ptr(f.y), _ptr(f.uv), B * V, Hs, Ws, f.y_pitch, f.uv_pitch,
                                                  f.y_frame_stride, f.uv_frame_stride, f.standard, *tail)
            capi.check(self.lib, rc, "fvp_anonymise_rois_nv12")
            return frames
        rc = self.lib.fvp_anonymise_rois(_ptr(f), B * V, Hs, Ws, *tail)
        capi.check(self.lib, rc, "fvp_anonymise_rois")
        return frames

    def __call__(self, frames, views, ids=None, joint_conf=None):
        """``rois()`` then ``apply()``: returns ``frames``."""
        return self.apply(frames, self.rois(views, ids=ids, joint_conf=joint_conf)[0])
