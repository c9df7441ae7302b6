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
from .visibility import JointVisibility

MAX_RADIUS = capi.FVP_TRI_MAX_RADIUS
OUTPUTS = ("tri_poses", "tri_count", "tri_stats", "obs", "view_state", "cam_resid", "cam_count")


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


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

    _tables = JointVisibility._tables      # the same upload-once camera tables (reads _seq_ids, _cams, _frame_sets)

    def __init__(self, cfg, radius=3, min_peak=0.3, undistort_iters=8, min_views=2, min_det=1e-3, reject_px=0.0,
                 per_camera=True, resize_transform=None, _lib=None):
        # `_lib` is a test seam (tests/hipemu); the product always loads libfvp_hip.so
        self._injected = _lib is not None
        self.lib = _lib if _lib is not None else capi.load()
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
        rt = np.asarray(resize_transform, np.float32).reshape(6)
        g = capi.FvpGeom()
        g.clamp_max = float(max(ds.ORI_IMAGE_SIZE[0], ds.ORI_IMAGE_SIZE[1]))
        for i in range(6):
            g.rt[i] = float(rt[i])
        g.W, g.H = int(ds.HEATMAP_SIZE[0]), int(ds.HEATMAP_SIZE[1])
        g.hm_w, g.hm_h = float(g.W), float(g.H)
        g.img_w, g.img_h = float(ds.IMAGE_SIZE[0]), float(ds.IMAGE_SIZE[1])
        g.V, g.J, g.JP = 0, self.J, 4 * ((self.J + 3) // 4)
        self.geom = g
        self._seq_ids, self._cams, self._frame_sets = {}, None, {}
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
        p, h = fused_poses, heat_cl
        if not torch.is_tensor(p) or p.dtype != torch.float32 or p.dim() != 4 or tuple(p.shape[2:]) != (self.J, 5) \
                or not p.is_contiguous():
            raise capi.FvpError(f"fused_poses must be a contiguous float32 tensor [B,N,{self.J},5], got "
                                f"{getattr(p, 'dtype', type(p))} {tuple(getattr(p, 'shape', ()))}")
        if not self._injected and p.device.type != "cuda":
            raise capi.FvpError(f"fused_poses live on {p.device}: the triangulation runs on a ROCm GPU device (spelled "
                                "'cuda:N' in PyTorch-ROCm); there is no CPU fallback")
        B, N = p.shape[:2]
        g = self.geom if geom is None else geom
        if not torch.is_tensor(h) or h.dtype != torch.float32 or h.device != p.device or h.dim() != 5 or h.shape[0] != B \
                or tuple(h.shape[2:]) != (g.H, g.W, g.JP) or not h.is_contiguous():
            raise capi.FvpError(f"heat_cl must be a contiguous float32 tensor [{B},V,{g.H},{g.W},{g.JP}] on {p.device} (the "
                                f"channels-last staging copy), got {getattr(h, 'dtype', type(h))} {tuple(getattr(h, 'shape', ()))}")
        V = h.shape[1]
        if torch.is_tensor(cameras_or_cams):
            cams, fs = cameras_or_cams, frame_set_or_meta
            if cams.dtype != torch.float32 or cams.device != p.device or cams.dim() != 3 or cams.shape[0] < 1 \
                    or tuple(cams.shape[1:]) != (V, capi.FVP_CAM_FLOATS) or not cams.is_contiguous():
                raise capi.FvpError(f"cams must be a contiguous float32 tensor [nsets,{V},{capi.FVP_CAM_FLOATS}] on {p.device}, "
                                    f"got {cams.dtype} {tuple(cams.shape)}")
            if not torch.is_tensor(fs) or fs.dtype != torch.int32 or fs.device != p.device or tuple(fs.shape) != (B,) \
                    or not fs.is_contiguous():
                raise capi.FvpError(f"with a cams tensor, the frames' camera sets must be a contiguous int32 tensor [{B}] on "
                                    f"{p.device}")
        else:
            seqs = frame_set_or_meta["seq"] if isinstance(frame_set_or_meta, dict) else frame_set_or_meta
            if len(seqs) != B:
                raise capi.FvpError(f"{len(seqs)} sequence names for {B} frames")
            cams, fs = self._tables(cameras_or_cams, seqs, V, p.device)
        if not 1 <= V <= capi.FVP_MAX_VIEWS or N < 1:
            raise capi.FvpError(f"JointTriangulator limits: N >= 1, 1 <= V <= {capi.FVP_MAX_VIEWS} (N = {N}, V = {V})")
        for name, t, shape in (("occluder", occluder, (B, V, N, self.J)), ("ids", ids, (B, N))):
            if t is not None and (not torch.is_tensor(t) or t.dtype != torch.int32 or t.device != p.device
                                  or tuple(t.shape) != shape or not t.is_contiguous()):
                raise capi.FvpError(f"{name} must be a contiguous int32 tensor {list(shape)} on {p.device}")
        out = self.outputs(B, V, N, p.device)
        if B == 0:
            return out                                  # all empty (an empty tensor has no address to pass)
        g.V = V
        stream = C.c_void_p(torch.cuda.current_stream(p.device).cuda_stream) if p.device.type == "cuda" else None
        rc = self.lib.fvp_triangulate_joints(_ptr(h), _ptr(cams), cams.shape[0], _ptr(fs), _ptr(p), _ptr(ids), _ptr(occluder),
                                             B, N, C.byref(g), self.radius, self.min_peak, self.undistort_iters,
                                             self.min_views, self.min_det, self.reject_px, *[_ptr(t) for t in out], stream)
        capi.check(self.lib, rc, "fvp_triangulate_joints")
        return out
