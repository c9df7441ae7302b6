"""Joint visibility per view: ``JointVisibility`` answers, for every fused joint and every camera, whether the camera can see
the joint at all - the ray from the camera centre to the joint against a capsule model of every present person of the frame,
on the device (``fvp_joint_visibility``, include/fvp.h, ABI 17).  ``fvp_joint_evidence`` gives a joint's pixel, depth and
heatmap sample in every view whether or not another person's torso stands in between; ``occluder`` says who does, and
``vis_conf`` is the joint's confidence over the views that see it instead of over all of them.  One launch on the caller's
current HIP stream; no arithmetic on tensors happens here and nothing synchronises with the host: PyTorch is used for device
memory and streams only.

Not built: occlusion by scene objects, soft visibility, a per-view mask inside ``PoseOverlay`` / ``PersonCrops`` (they take
``[B,N,J]`` confidences).
"""
import ctypes as C
import math

import numpy as np
import torch

from .. import _capi as capi

MAX_PEOPLE, MAX_PRIMS = capi.FVP_VIS_MAX_PEOPLE, capi.FVP_VIS_MAX_PRIMS      # the limits of fvp_joint_visibility


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


class JointVisibility:
    """``JointVisibility(num_joints_or_cfg, prims=None, radius=50.0, spheres=None, guard=60.0, feeds_conf=True)``

    ``num_joints_or_cfg``  J, or a config (``DATASET.NUM_JOINTS``; its ``ORI_IMAGE_SIZE`` is then the default frame size);
    ``prims``              joint index pairs [L,2], one capsule around each 3-D segment; default: the limb table of
                           ``utils.vis`` for J in {14, 15, 17};
    ``radius``             capsule radius in mm: one value, or one per pair;
    ``spheres``            ``{joint: radius_mm}``: spheres around single joints (a head), appended behind the capsules;
    ``guard``              mm of the ray before the joint that are never tested, so that the joint's own flesh does not hide
                           it; a camera closer than that to a joint does not evaluate it;
    ``feeds_conf``         read by ``model.visibility``: ``vis_conf`` replaces ``last_evidence[1]`` as the ``joint_conf`` handed
                           to the smoother, the overlay and the crops.
    The default radii and the guard are anthropometric guesses (a limb of 10 cm across, a guard just above the radius): no
    dataset was on hand to tune them, and nothing here measures how often the verdict matches a labelled occlusion."""

    def __init__(self, num_joints_or_cfg, prims=None, radius=50.0, spheres=None, guard=60.0, feeds_conf=True, _lib=None):
        # `_lib` is a test seam (tests/hipemu); the product always loads libfvp_hip.so
        self._injected = _lib is not None
        self.lib = _lib if _lib is not None else capi.load()
        self.frame_size = None
        if isinstance(num_joints_or_cfg, int):
            J = num_joints_or_cfg
        else:
            J = num_joints_or_cfg.DATASET.NUM_JOINTS
            ws, hs = num_joints_or_cfg.DATASET.ORI_IMAGE_SIZE
            self.frame_size = (int(hs), int(ws))
        self.J = int(J)
        if not 1 <= self.J <= capi.FVP_MAX_JOINTS:
            raise capi.FvpError(f"JointVisibility needs 1 <= J <= {capi.FVP_MAX_JOINTS}, got {self.J}")
        if prims is None:
            from .vis import _LIMBS                      # (imports matplotlib: only for the default table)
            if self.J not in _LIMBS:
                raise capi.FvpError(f"no default skeleton for {self.J} joints (known: {sorted(_LIMBS)}): pass prims")
            prims = _LIMBS[self.J]
        pairs = [(int(a), int(b)) for a, b in prims]
        try:
            radii = [float(r) for r in radius]
        except TypeError:
            radii = [float(radius)] * len(pairs)
        if len(radii) != len(pairs):
            raise capi.FvpError(f"radius: one value, or one per pair ({len(pairs)}), got {len(radii)}")
        for j, r in (spheres or {}).items():
            pairs.append((int(j), int(j)))
            radii.append(float(r))
        self.prims, self.radius = pairs, radii
        if len(pairs) > MAX_PRIMS or any(not (0 <= j < self.J) for ab in pairs for j in ab):
            raise capi.FvpError(f"prims and spheres: at most {MAX_PRIMS} primitives of joint indices in [0, {self.J})")
        if any(not (r > 0 and math.isfinite(r)) for r in radii):
            raise capi.FvpError(f"radius and spheres: finite values > 0 (mm), got {radii}")
        self.guard = float(guard)
        if not (self.guard >= 0 and math.isfinite(self.guard)):
            raise capi.FvpError(f"guard: a finite value >= 0 (mm), got {guard}")
        self.feeds_conf = bool(feeds_conf)
        L = len(pairs)
        self._prims = (C.c_int32 * max(2 * L, 1))(*[j for ab in pairs for j in ab])
        self._radius = (C.c_float * max(L, 1))(*radii)
        self._seq_ids, self._cams, self._frame_sets = {}, None, {}

    def _tables(self, cameras, seqs, V, device):
        """Camera dicts and sequence names -> (cams [nsets,V,24], frame_set [B]), uploaded once per new sequence / list."""
        from ..engine import HotPath
        seqs = tuple(seqs)
        for s in dict.fromkeys(seqs):
            if s not in self._seq_ids:
                if s not in cameras or len(cameras[s]) != V:
                    raise capi.FvpError(f"cameras holds no {V} cameras for sequence {s!r}")
                rows = np.stack([HotPath._cam_row(cameras[s][c]) for c in range(V)])
                t = torch.from_numpy(rows).to(device)[None]
                self._cams = t if self._cams is None else torch.cat([self._cams, t], dim=0)
                self._seq_ids[s] = self._cams.shape[0] - 1
                self._frame_sets.clear()
        if seqs not in self._frame_sets:
            if len(self._frame_sets) >= 256:            # bounded, as in the engine
                self._frame_sets.pop(next(iter(self._frame_sets)))
            self._frame_sets[seqs] = torch.tensor([self._seq_ids[s] for s in seqs], dtype=torch.int32, device=device)
        return self._cams, self._frame_sets[seqs]

    def __call__(self, fused_poses, cameras_or_cams, frame_set_or_meta, views=None, ids=None, frame_size=None):
        """``fused_poses [B,N,J,5]`` (the forward's, a smoother's, ground truth) -> ``(occluder [B,V,N,J] int32, vis_conf
        [B,N,J] fp32, vis_count [B,N,J] int32)``.  ``occluder``: -2 the joint is not evaluated (absent person, a joint that
        is not finite, a camera within ``guard``), -1 a free line of sight, else the slot of the person nearest the camera
        whose body crosses the ray (the joint's own slot: self-occlusion).  With ``views [B,V,N,J,4]``
        (``last_evidence[0]``) a view sees a joint when the line of sight is free, the joint lies in front of the camera and
        its pixel inside the frame of ``frame_size = (Hs, Ws)``; ``vis_count`` counts those views and ``vis_conf`` is the
        clamped mean of their heatmap samples (0 with none).  Without ``views`` both are None.

        The cameras: a float32 tensor ``[nsets,V,24]`` of camera records with an int32 tensor ``[B]`` of set rows (the
        engine's own tables: what ``model.visibility`` passes), or the ``cameras`` dict of the forward with its ``meta``
        (``meta['seq']`` names the sequence of each frame; a sequence's cameras are uploaded when it is first seen, V is
        then taken from ``views`` or the dict).  ``ids [B,N]`` int32 (``last_tracks[0]``): a slot with a negative id is
        neither evaluated nor an occluder.  One launch on the current stream."""
        p = fused_poses
        if not torch.is_tensor(p) or p.dtype != torch.float32 or p.dim() != 4 or tuple(p.shape[2:]) != (self.J, 5) \
                or not p.is_contiguous():
            raise capi.FvpError(f"fused_poses must be a contiguous float32 tensor [B,N,{self.J},5], got "
                                f"{getattr(p, 'dtype', type(p))} {tuple(getattr(p, 'shape', ()))}")
        if not self._injected and p.device.type != "cuda":
            raise capi.FvpError(f"fused_poses live on {p.device}: the visibility test runs on a ROCm GPU device (spelled "
                                "'cuda:N' in PyTorch-ROCm); there is no CPU fallback")
        B, N = p.shape[:2]
        v = views
        if v is not None and (not torch.is_tensor(v) or v.dtype != torch.float32 or v.device != p.device or v.dim() != 5
                              or v.shape[0] != B or tuple(v.shape[2:]) != (N, self.J, 4) or not v.is_contiguous()):
            raise capi.FvpError(f"views must be a contiguous float32 tensor [{B},V,{N},{self.J},4] on {p.device} (what "
                                f"joint_evidence returns), got {getattr(v, 'dtype', type(v))} {tuple(getattr(v, 'shape', ()))}")
        if torch.is_tensor(cameras_or_cams):
            cams, fs = cameras_or_cams, frame_set_or_meta
            if cams.dtype != torch.float32 or cams.device != p.device or cams.dim() != 3 or cams.shape[0] < 1 \
                    or cams.shape[2] != capi.FVP_CAM_FLOATS or not cams.is_contiguous():
                raise capi.FvpError(f"cams must be a contiguous float32 tensor [nsets,V,{capi.FVP_CAM_FLOATS}] on {p.device}, "
                                    f"got {cams.dtype} {tuple(cams.shape)}")
            if not torch.is_tensor(fs) or fs.dtype != torch.int32 or fs.device != p.device or tuple(fs.shape) != (B,) \
                    or not fs.is_contiguous():
                raise capi.FvpError(f"with a cams tensor, the frames' camera sets must be a contiguous int32 tensor [{B}] on "
                                    f"{p.device}")
            V = cams.shape[1]
        else:
            seqs = frame_set_or_meta["seq"] if isinstance(frame_set_or_meta, dict) else frame_set_or_meta
            if len(seqs) != B:
                raise capi.FvpError(f"{len(seqs)} sequence names for {B} frames")
            V = v.shape[1] if v is not None else (len(cameras_or_cams[seqs[0]]) if B else 1)
            cams, fs = self._tables(cameras_or_cams, seqs, V, p.device)
        if v is not None and v.shape[1] != V:
            raise capi.FvpError(f"views hold {v.shape[1]} views, the camera table {V}")
        if not 1 <= N <= MAX_PEOPLE or not 1 <= V <= capi.FVP_MAX_VIEWS:
            raise capi.FvpError(f"JointVisibility limits: 1 <= N <= {MAX_PEOPLE}, 1 <= V <= {capi.FVP_MAX_VIEWS} (N = {N}, "
                                f"V = {V})")
        if ids is not None and (not torch.is_tensor(ids) or ids.dtype != torch.int32 or ids.device != p.device
                                or tuple(ids.shape) != (B, N) or not ids.is_contiguous()):
            raise capi.FvpError(f"ids must be a contiguous int32 tensor [{B},{N}] on {p.device} (what PoseTracker.update "
                                "returns)")
        Hs, Ws = 1, 1
        if v is not None:
            size = self.frame_size if frame_size is None else frame_size
            try:
                Hs, Ws = (int(x) for x in size)
            except (TypeError, ValueError):
                raise capi.FvpError(f"with views, frame_size must be (Hs, Ws) of the camera frames, got {size!r}") from None
            if Hs < 1 or Ws < 1:
                raise capi.FvpError(f"frame_size must be (Hs, Ws) with both >= 1, got {size!r}")
        occluder = torch.empty((B, V, N, self.J), dtype=torch.int32, device=p.device)
        vis_conf = vis_count = None
        if v is not None:
            vis_conf = torch.empty((B, N, self.J), dtype=torch.float32, device=p.device)
            vis_count = torch.empty((B, N, self.J), dtype=torch.int32, device=p.device)
        if B == 0:
            return occluder, vis_conf, vis_count        # all empty (an empty tensor has no address to pass)
        stream = C.c_void_p(torch.cuda.current_stream(p.device).cuda_stream) if p.device.type == "cuda" else None
        rc = self.lib.fvp_joint_visibility(_ptr(p), _ptr(cams), _ptr(fs), _ptr(ids), _ptr(v), B, V, N, self.J, self._prims,
                                           self._radius, len(self.prims), self.guard, Hs, Ws, _ptr(occluder), _ptr(vis_conf),
                                           _ptr(vis_count), stream)
        capi.check(self.lib, rc, "fvp_joint_visibility")
        return occluder, vis_conf, vis_count
