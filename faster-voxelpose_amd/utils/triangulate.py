"""Triangulated joints from the views: ``JointTriangulator`` gives every fused joint a geometric second opinion - the point the
rays through the 2-D heat-map peaks of the usable views agree on - with the reprojection residual per joint and view and the
residual per camera and frame, on the device (``fvp_triangulate_joints``, include/fvp.h, ABI 18).  The distance of the
triangulated joint from the fused one says how much the network's answer leans on its prior; a camera whose residual stands
apart from the others has been bumped.  One launch (two with the per-camera residual) on the caller's current HIP stream;
no arithmetic on tensors happens here and nothing synchronises with the host: PyTorch is used for device memory and streams
only.

Re-calibration of a camera that has moved: ``utils/recalibrate.py::CameraRefiner`` reads ``obs`` and ``view_state``.
Not built: an iterated rejection, triangulated poses fed into tracker or smoother.
"""
import ctypes as C
import math

import numpy as np
import torch

from .. import _capi as capi
from .._args import CameraTables, load_lib, require_gpu, resolve_cameras, stream_ptr, tensor_arg
from .._args import ptr as _ptr

MAX_RADIUS = capi.FVP_TRI_MAX_RADIUS
OUTPUTS = ("tri_poses", "tri_count", "tri_stats", "obs", "view_state", "cam_resid", "cam_count")


class JointTriangulator:
    """``JointTriangulator(cfg, radius=3, min_peak=0.3, undistort_iters=8, min_views=2, min_det=1e-3, reject_px=0.0,
    per_camera=True, resize_transform=None)``

    ``cfg``              the model's config: ``DATASET.NUM_JOINTS``, ``HEATMAP_SIZE``, ``IMAGE_SIZE``, ``ORI_IMAGE_SIZE``;
    ``radius``           half-size, in heat-map cells, of the window searched around the reprojected fused joint, 1..8;
    ``min_peak``         a view whose window maximum is below it is set aside;
    ``undistort_iters``  fixed-point rounds that take the observed pixel back through the lens polynomial, 0..16;
    ``min_views``        views needed to triangulate a joint, >= 2;
    ``min_det``          a joint whose normal matrix has det <= min_det * (trace / 3)^3 is degenerate (rays nearly parallel);
    ``reject_px``        > 0: views whose residual exceeds it are dropped once and the joint is solved again; <= 0: off;
    ``per_camera``       also reduce the residual per camera and frame (``cam_resid``, ``cam_count``): one more launch;
    ``resize_transform`` the 2x3 camera -> network pixel transform; default: the dataset constant of ``cfg``.
    The defaults are guesses: no dataset was on hand to tune them."""

    def __init__(self, cfg, radius=3, min_peak=0.3, undistort_iters=8, min_views=2, min_det=1e-3, reject_px=0.0,
                 per_camera=True, resize_transform=None, _lib=None):
        self.lib, self._injected = load_lib(_lib)
        ds = cfg.DATASET
        self.J = int(ds.NUM_JOINTS)
        if not 1 <= self.J <= capi.FVP_MAX_JOINTS:
            raise capi.FvpError(f"JointTriangulator needs 1 <= J <= {capi.FVP_MAX_JOINTS}, got {self.J}")
        self.radius, self.undistort_iters, self.min_views = int(radius), int(undistort_iters), int(min_views)
        self.min_peak, self.min_det, self.reject_px = float(min_peak), float(min_det), float(reject_px)
        if not 1 <= self.radius <= MAX_RADIUS or not 0 <= self.undistort_iters <= 16 or self.min_views < 2:
            raise capi.FvpError(f"JointTriangulator needs 1 <= radius <= {MAX_RADIUS}, 0 <= undistort_iters <= 16 and "
                                f"min_views >= 2, got {radius}, {undistort_iters}, {min_views}")
        if not all(math.isfinite(x) for x in (self.min_peak, self.min_det, self.reject_px)):
            raise capi.FvpError(f"min_peak, min_det and reject_px must be finite, got {min_peak}, {min_det}, {reject_px}")
        self.per_camera = bool(per_camera)
        if resize_transform is None:
            from .transforms import get_resize_transform
            resize_transform = get_resize_transform(ds.ORI_IMAGE_SIZE, ds.IMAGE_SIZE)
        if torch.is_tensor(resize_transform):
            resize_transform = resize_transform.detach().cpu()
        self.geom = capi.make_geom(ds, np.asarray(resize_transform, np.float32).reshape(6), self.J)
        self._cameras = CameraTables()                 # of the sequences handed in as camera dicts
        self._out = {}

    def outputs(self, B, V, N, device):
        """The preallocated outputs of one shape on one device: rewritten by every call of that shape."""
        key = (B, V, N, str(device))
        if key not in self._out:
            J, f, i = self.J, torch.float32, torch.int32
            mk = lambda shape, dt: torch.empty(shape, dtype=dt, device=device)      # noqa: E731
            out = [mk((B, N, J, 5), f), mk((B, N, J), i), mk((B, N, J, 2), f), mk((B, V, N, J, 4), f), mk((B, V, N, J), i)]
            out += [mk((B, V), f), mk((B, V), i)] if self.per_camera else [None, None]
            self._out[key] = tuple(out)
        return self._out[key]

    def __call__(self, fused_poses, cameras_or_cams, frame_set_or_meta, heat_cl, occluder=None, ids=None, geom=None):
        """``fused_poses [B,N,J,5]`` and the channels-last heat maps ``heat_cl [B,V,H,W,JP]`` of the same frames (the engine's
        staging copy) -> ``(tri_poses [B,N,J,5], tri_count [B,N,J] int32, tri_stats [B,N,J,2], obs [B,V,N,J,4], view_state
        [B,V,N,J] int32, cam_resid [B,V], cam_count [B,V] int32)``, the last two None without ``per_camera``.  ``tri_poses``:
        the triangulated xyz where ``tri_count >= min_views``, else the fused one, elements 3 and 4 copied - it drops in
        wherever ``fused_poses`` goes.  ``tri_count``: the views of the final solve; below ``min_views``: that many usable
        views; -1 degenerate; -2 not evaluated.  ``tri_stats``: (distance from the fused joint in mm, weighted rms
        reprojection residual in pixels).  ``obs``: (observed pixel x, y in the original image, peak, residual or -1).
        ``view_state``: 1 used, 0 not evaluated, -1 behind the camera or outside the map, -2 peak low, -3 peak on the window's
        border, -4 occluded, -5 rejected, -6 usable but the joint was not triangulated.  ``cam_resid``, ``cam_count``: the
        mean residual and the number of used joint-views per camera and frame.  The tensors are preallocated per shape and
        rewritten by the next call of that shape.

        The cameras: a float32 tensor ``[nsets,V,24]`` of camera records with an int32 tensor ``[B]`` of set rows (the
        engine's own tables: what ``model.triangulator`` passes), or the ``cameras`` dict of the forward with its ``meta``.
        ``occluder [B,V,N,J]`` int32 (``last_visibility[0]``): only views with -1 are used.  ``ids [B,N]`` int32
        (``last_tracks[0]``): a slot with a negative id is not evaluated.  ``geom``: an ``FvpGeom`` to use instead of the one
        built from ``cfg`` (the engine's, with the forward's resize transform)."""
        p = tensor_arg("fused_poses", fused_poses, torch.float32, ("B", "N", self.J, 5))
        require_gpu("the triangulation", p.device, self._injected)
        B, N = p.shape[:2]
        g = self.geom if geom is None else geom
        h = tensor_arg("heat_cl", heat_cl, torch.float32, (B, "V", g.H, g.W, g.JP), p.device,
                       hint="the channels-last staging copy")
        cams, fs, V = resolve_cameras(self._cameras, cameras_or_cams, frame_set_or_meta, B, h.shape[1], p.device)
        if not 1 <= V <= capi.FVP_MAX_VIEWS or N < 1:
            raise capi.FvpError(f"JointTriangulator limits: N >= 1, 1 <= V <= {capi.FVP_MAX_VIEWS} (N = {N}, V = {V})")
        tensor_arg("occluder", occluder, torch.int32, (B, V, N, self.J), p.device, optional=True)
        tensor_arg("ids", ids, torch.int32, (B, N), p.device, optional=True)
        out = self.outputs(B, V, N, p.device)
        if B == 0:
            return out                                  # all empty (an empty tensor has no address to pass)
        g.V = V
        stream = stream_ptr(p.device)
        rc = self.lib.fvp_triangulate_joints(_ptr(h), _ptr(cams), cams.shape[0], _ptr(fs), _ptr(p), _ptr(ids), _ptr(occluder),
                                             B, N, C.byref(g), self.radius, self.min_peak, self.undistort_iters,
                                             self.min_views, self.min_det, self.reject_px, *[_ptr(t) for t in out], stream)
        capi.check(self.lib, rc, "fvp_triangulate_joints")
        return out
