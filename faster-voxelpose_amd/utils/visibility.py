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

import torch

from .. import _capi as capi
from .._args import CameraTables, load_lib, require_gpu, resolve_cameras, stream_ptr, tensor_arg
from .._args import ptr as _ptr

MAX_PEOPLE, MAX_PRIMS = capi.FVP_VIS_MAX_PEOPLE, capi.FVP_VIS_MAX_PRIMS      # the limits of fvp_joint_visibility


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
        self.lib, self._injected = load_lib(_lib)
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
        self._cameras = CameraTables()                 # of the sequences handed in as camera dicts
        self._seq_ids = self._cameras.ids

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
        p = tensor_arg("fused_poses", fused_poses, torch.float32, ("B", "N", self.J, 5))
        require_gpu("the visibility test", p.device, self._injected)
        B, N = p.shape[:2]
        v = tensor_arg("views", views, torch.float32, (B, "V", N, self.J, 4), p.device, hint="what joint_evidence returns",
                       optional=True)
        # a cameras dict says nothing about V: the views do, else the dict's first sequence
        known_V = v.shape[1] if v is not None and not torch.is_tensor(cameras_or_cams) else None
        cams, fs, V = resolve_cameras(self._cameras, cameras_or_cams, frame_set_or_meta, B, known_V, p.device)
        if v is not None and v.shape[1] != V:
            raise capi.FvpError(f"views hold {v.shape[1]} views, the camera table {V}")
        if not 1 <= N <= MAX_PEOPLE or not 1 <= V <= capi.FVP_MAX_VIEWS:
            raise capi.FvpError(f"JointVisibility limits: 1 <= N <= {MAX_PEOPLE}, 1 <= V <= {capi.FVP_MAX_VIEWS} (N = {N}, "
                                f"V = {V})")
        tensor_arg("ids", ids, torch.int32, (B, N), p.device, hint="what PoseTracker.update returns", optional=True)
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
        stream = stream_ptr(p.device)
        rc = self.lib.fvp_joint_visibility(_ptr(p), _ptr(cams), _ptr(fs), _ptr(ids), _ptr(v), B, V, N, self.J, self._prims,
                                           self._radius, len(self.prims), self.guard, Hs, Ws, _ptr(occluder), _ptr(vis_conf),
                                           _ptr(vis_count), stream)
        capi.check(self.lib, rc, "fvp_joint_visibility")
        return occluder, vis_conf, vis_count
