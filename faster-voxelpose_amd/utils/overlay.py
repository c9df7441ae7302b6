"""Poses back onto the camera frames: ``PoseOverlay`` draws the skeletons of ``fvp_joint_evidence``'s ``views`` into the
``uint8`` frames they were computed from, on the device and in place (``fvp_draw_poses``, include/fvp.h, ABI 14) - the
device-side counterpart of ``utils/vis.py::save_image_with_poses``, which copies frames and poses to the host and draws
with matplotlib.  A decoder's NV12 surface (``dataset.images.Nv12Frames``) is drawn on directly, luma and chroma, with its
own pitches and frame strides (``fvp_draw_poses_nv12``, ABI 15).  One launch on the caller's current HIP stream; no
arithmetic on tensors happens here and nothing synchronises with the host: PyTorch is used for device memory and streams
only.

Not built: text labels, anti-aliasing, pitched RGB frames.
"""
import ctypes as C

import torch

from .. import _capi as capi
from .._args import load_lib, require_gpu, stream_ptr, tensor_arg
from .._args import ptr as _ptr
from ..dataset.images import Nv12Frames

# person colours, RGB, indexed by track id (or by slot without ids) modulo the length
PALETTE = [(230, 25, 75), (60, 180, 75), (255, 225, 25), (0, 130, 200), (245, 130, 48), (145, 30, 180), (70, 240, 240),
           (240, 50, 230), (210, 245, 60), (250, 190, 212), (0, 128, 128), (220, 190, 255), (170, 110, 40), (255, 250, 200),
           (128, 0, 0), (170, 255, 195)]
MAX_PEOPLE, MAX_LIMBS, MAX_COLOURS, MAX_Q4 = 32, 64, 64, 1024          # the limits of fvp_draw_poses


class PoseOverlay:
    """``PoseOverlay(num_joints_or_cfg, limbs=None, palette=None, joint_radius=8.0, limb_width=4.0, alpha=1.0,
    conf_min=0.0, nv12=False)``

    ``num_joints_or_cfg``  J, or a config (``DATASET.NUM_JOINTS``);
    ``limbs``              joint index pairs [L,2]; default: the table of ``utils.vis`` for J in {14, 15, 17};
    ``palette``            RGB triples [P,3] in the frames' channel order; default: ``PALETTE`` (16 colours);
    ``joint_radius``       radius of a joint's disc, pixels (the reference draws cv2.circle of radius 8);
    ``limb_width``         width of a limb, pixels (cv2.line of thickness 4 there);
    ``alpha``              opacity in (0, 1]: 1 paints, lower values blend with the frame;
    ``conf_min``           with ``joint_conf`` given, a joint below it - and every limb ending in it - is left out.
    ``nv12``               True: ``model.overlay`` may draw into ``Nv12Frames`` views.  In place means into the
                           decoder's own surface, which the decoder may still hold as a reference picture: the flag is
                           the caller's statement that the surface is theirs to paint.  ``draw()``
                           itself takes an ``Nv12Frames`` either way.
    Radius and half width are rounded to sixteenths of a pixel, ``alpha`` to 1/256."""

    def __init__(self, num_joints_or_cfg, limbs=None, palette=None, joint_radius=8.0, limb_width=4.0, alpha=1.0,
                 conf_min=0.0, nv12=False, _lib=None):
        self.lib, self._injected = load_lib(_lib)
        J = num_joints_or_cfg if isinstance(num_joints_or_cfg, int) else num_joints_or_cfg.DATASET.NUM_JOINTS
        self.J = int(J)
        if not 1 <= self.J <= capi.FVP_MAX_JOINTS:
            raise capi.FvpError(f"PoseOverlay needs 1 <= J <= {capi.FVP_MAX_JOINTS}, got {self.J}")
        if limbs is None:
            from .vis import _LIMBS                      # (imports matplotlib: only for the default table)
            if self.J not in _LIMBS:
                raise capi.FvpError(f"no default skeleton for {self.J} joints (known: {sorted(_LIMBS)}): pass limbs")
            limbs = _LIMBS[self.J]
        self.limbs = [(int(a), int(b)) for a, b in limbs]
        self.palette = [tuple(int(c) for c in rgb) for rgb in (PALETTE if palette is None else palette)]
        if len(self.limbs) > MAX_LIMBS or any(not (0 <= j < self.J) for ab in self.limbs for j in ab):
            raise capi.FvpError(f"limbs: at most {MAX_LIMBS} pairs of joint indices in [0, {self.J})")
        if not 1 <= len(self.palette) <= MAX_COLOURS or any(len(c) != 3 or not all(0 <= v <= 255 for v in c)
                                                            for c in self.palette):
            raise capi.FvpError(f"palette: 1 to {MAX_COLOURS} RGB triples of bytes")
        self.conf_min = float(conf_min)
        self.nv12 = bool(nv12)
        if self.conf_min != self.conf_min or not (joint_radius >= 0 and limb_width >= 0 and 0 < alpha <= 1):
            raise capi.FvpError(f"PoseOverlay needs joint_radius, limb_width >= 0, alpha in (0, 1] and a conf_min that is "
                                f"not NaN (joint_radius = {joint_radius}, limb_width = {limb_width}, alpha = {alpha}, "
                                f"conf_min = {conf_min})")
        self.joint_radius_q4 = round(float(joint_radius) * 16)
        self.limb_half_q4 = round(float(limb_width) / 2 * 16)
        self.alpha = round(float(alpha) * 256)
        if self.joint_radius_q4 > MAX_Q4 or self.limb_half_q4 > MAX_Q4 or self.alpha < 1:
            raise capi.FvpError(f"PoseOverlay limits: joint_radius and limb_width / 2 <= {MAX_Q4 // 16} pixels, alpha >= "
                                f"1/512 (joint_radius = {joint_radius}, limb_width = {limb_width}, alpha = {alpha})")
        L, P = len(self.limbs), len(self.palette)
        self._limbs = (C.c_int32 * max(2 * L, 1))(*[j for ab in self.limbs for j in ab])
        self._palette = (C.c_uint8 * (3 * P))(*[v for c in self.palette for v in c])

    def draw(self, frames, views, ids=None, joint_conf=None):
        """Draw ``views [B,V,N,J,4]`` (``last_evidence[0]``, or ``joint_evidence(...)[0]`` of any poses) into ``frames``
        ``uint8 [B,V,Hs,Ws,3]`` in place and return ``frames``.  ``ids [B,N]`` int32 (``last_tracks[0]``): the colour
        follows the track and slots with a negative id are left out; None: the colour follows the slot.  ``joint_conf
        [B,N,J]`` (``last_evidence[1]``): joints below ``conf_min`` are left out.  One launch on the current stream.
        ``frames`` may also be an ``Nv12Frames`` with leading dimensions ``[B,V]``: both planes are drawn on in place,
        with the surface's pitches, frame strides and colour standard (the palette stays RGB)."""
        f, v = frames, views
        nv12 = isinstance(f, Nv12Frames)
        if nv12:
            if len(f.lead) != 2:
                raise capi.FvpError(f"an NV12 surface to draw on must have leading dimensions [B,V], got {f.lead}")
            B, V, Hs, Ws = f.lead[0], f.lead[1], f.Hs, f.Ws
        else:
            B, V, Hs, Ws = tensor_arg("frames", f, torch.uint8, ("B", "V", "Hs", "Ws", 3), hint="HWC camera frames").shape[:4]
        require_gpu("the overlay", f.device, self._injected)
        v = tensor_arg("views", v, torch.float32, (B, V, "N", self.J, 4), f.device, hint="what joint_evidence returns")
        N = v.shape[2]
        if not 1 <= N <= MAX_PEOPLE or V > capi.FVP_MAX_VIEWS or min(Hs, Ws) < 1:
            raise capi.FvpError(f"PoseOverlay.draw limits: 1 <= N <= {MAX_PEOPLE}, V <= {capi.FVP_MAX_VIEWS}, Hs, Ws >= 1 "
                                f"(N = {N}, V = {V}, Hs = {Hs}, Ws = {Ws})")
        tensor_arg("ids", ids, torch.int32, (B, N), f.device, hint="what PoseTracker.update returns", optional=True)
        c = tensor_arg("joint_conf", joint_conf, torch.float32, (B, N, self.J), f.device, optional=True)
        stream = stream_ptr(f.device)
        if nv12:
            rc = self.lib.fvp_draw_poses_nv12(_ptr(f.y), _ptr(f.uv), B, V, Hs, Ws, f.y_pitch, f.uv_pitch, f.y_frame_stride,
                                              f.uv_frame_stride, f.standard, _ptr(v), _ptr(ids), _ptr(c), N, self.J,
                                              self._limbs, len(self.limbs), self._palette, len(self.palette),
                                              self.joint_radius_q4, self.limb_half_q4, self.alpha, self.conf_min, stream)
            capi.check(self.lib, rc, "fvp_draw_poses_nv12")
            return frames
        rc = self.lib.fvp_draw_poses(_ptr(f), B, V, Hs, Ws, _ptr(v), _ptr(ids), _ptr(c), N, self.J, self._limbs,
                                     len(self.limbs), self._palette, len(self.palette), self.joint_radius_q4,
                                     self.limb_half_q4, self.alpha, self.conf_min, stream)
        capi.check(self.lib, rc, "fvp_draw_poses")
        return frames
