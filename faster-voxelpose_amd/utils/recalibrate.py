"""Bumped cameras re-fitted on the device: ``CameraRefiner`` takes what ``JointTriangulator`` leaves behind - the observed pixel
per joint and view, which observations were used, the 3-D joints - and corrects the cameras' extrinsic parameters against
them (``fvp_camera_refit_accumulate`` + ``fvp_camera_refit_solve``, include/fvp.h, ABI 19): a robust resection per camera,
one Gauss-Newton step on its rotation and centre in fp64, accumulated over as many batches as the caller likes, the result a
camera table in the layout every projection call reads.  The 3-D joints are held fixed: that is what pulls one bumped camera
back to the consensus of the others.  This is not bundle adjustment, and when every camera of a rig has moved nothing fixes
the gauge.  One launch per call on the caller's current HIP stream; no arithmetic on tensors happens here and nothing
synchronises with the host: PyTorch is used for device memory and streams only.

Not built: intrinsics or lens re-fit, joint refinement of points and cameras (bundle adjustment), gauge fixing when every
camera is re-fitted at once, swapping the corrected tables into a running engine (its fine-grid cache depends on them: pass
``camera_dicts(...)`` into the forward under a new sequence name instead).
"""
import math

import torch

from .. import _capi as capi
from .._args import load_lib, require_gpu, stream_ptr, tensor_arg
from .._args import ptr as _ptr

ACC = capi.FVP_CAL_ACC
OK, CLAMPED, FEW, DEGENERATE = capi.FVP_CAL_OK, capi.FVP_CAL_CLAMPED, capi.FVP_CAL_FEW, capi.FVP_CAL_DEGENERATE


class CameraRefiner:
    """``CameraRefiner(cfg, nseq=1, undistort_iters=8, huber_px=0.0, decay=1.0, min_obs=60, lam=0.0, min_pivot=1e-9,
    max_angle_deg=5.0, max_shift_mm=200.0)``

    ``cfg``              the model's config: ``DATASET.NUM_JOINTS``;
    ``nseq``             camera sets (sequences) the accumulators are first sized for; they follow the table handed in;
    ``undistort_iters``  fixed-point rounds of the lens model, as the triangulator's, 0..16;
    ``huber_px``         > 0: residuals beyond it (pixels of the undistorted image) weigh huber_px / e; <= 0: off;
    ``decay``            what every ``accumulate`` multiplies the old sums by: 1 accumulates, < 1 forgets, 0 replaces;
    ``min_obs``          observations a camera needs before it is solved, >= 6;
    ``lam``              Levenberg damping added to the scaled normal matrix's diagonal, >= 0;
    ``min_pivot``        a scaled Cholesky pivot at or below it makes the camera degenerate, > 0;
    ``max_angle_deg``, ``max_shift_mm``  the trust region of one step: a longer step is scaled down (state CLAMPED).
    The defaults are guesses: no rig was on hand to tune them."""

    def __init__(self, cfg, nseq=1, undistort_iters=8, huber_px=0.0, decay=1.0, min_obs=60, lam=0.0, min_pivot=1e-9,
                 max_angle_deg=5.0, max_shift_mm=200.0, _lib=None):
        self.lib, self._injected = load_lib(_lib)
        self.J = int(cfg.DATASET.NUM_JOINTS)
        if not 1 <= self.J <= capi.FVP_MAX_JOINTS:
            raise capi.FvpError(f"CameraRefiner needs 1 <= J <= {capi.FVP_MAX_JOINTS}, got {self.J}")
        self.nseq, self.undistort_iters, self.min_obs = int(nseq), int(undistort_iters), int(min_obs)
        self.huber_px, self.decay, self.lam, self.min_pivot = float(huber_px), float(decay), float(lam), float(min_pivot)
        self.max_angle_rad, self.max_shift_mm = math.radians(float(max_angle_deg)), float(max_shift_mm)
        if self.nseq < 1 or not 0 <= self.undistort_iters <= 16 or self.min_obs < 6:
            raise capi.FvpError(f"CameraRefiner needs nseq >= 1, 0 <= undistort_iters <= 16 and min_obs >= 6, got {nseq}, "
                                f"{undistort_iters}, {min_obs}")
        if not math.isfinite(self.huber_px) or not 0.0 <= self.decay <= 1.0 or not (0.0 <= self.lam < math.inf):
            raise capi.FvpError(f"huber_px must be finite, decay in [0, 1] and lam >= 0, got {huber_px}, {decay}, {lam}")
        if not all(0.0 < x < math.inf for x in (self.min_pivot, self.max_angle_rad, self.max_shift_mm)):
            raise capi.FvpError(f"min_pivot, max_angle_deg and max_shift_mm must be positive and finite, got {min_pivot}, "
                                f"{max_angle_deg}, {max_shift_mm}")
        self.acc = None                    # [nsets, V, 32] float64: the accumulators, a linearisation at the table they saw
        self._store = None
        self._out = {}

    # ---- state ------------------------------------------------------------------------------------------------------
    def _state(self, nsets, V, device):
        """The accumulators of the first ``nsets`` camera sets: storage for max(nsets, nseq) sets, kept (and its address
        with it) until the table outgrows it or changes its view count or device."""
        st = self._store
        if st is None or st.shape[0] < nsets or st.shape[1] != V or st.device != device:
            new = torch.zeros((max(nsets, self.nseq), V, ACC), dtype=torch.float64, device=device)
            if st is not None and st.shape[1] == V and st.device == device:
                new[:st.shape[0]].copy_(st)
            self._store = new
        self.acc = self._store[:nsets]
        return self.acc

    def reset(self, sets=None):
        """Zero the accumulators (of the camera sets ``sets``; default: all).  To be called whenever the camera records they
        were accumulated against change - ``refine`` does it itself - and after a graph capture, whose capture pass does not
        run the launches."""
        if self._store is not None:
            if sets is None:
                self._store.zero_()
            else:
                for s in sets:
                    self._store[int(s)].zero_()

    def outputs(self, nsets, V, device):
        """Two preallocated output sets per shape, used in turn by ``solve`` (``refine`` ping-pongs between them)."""
        key = (nsets, V, str(device))
        if key not in self._out:
            mk = lambda shape, dt: torch.empty(shape, dtype=dt, device=device)      # noqa: E731
            self._out[key] = [[(mk((nsets, V, capi.FVP_CAM_FLOATS), torch.float32), mk((nsets, V, 6), torch.float32),
                                mk((nsets, V), torch.int32)) for _ in range(2)], 0]
        return self._out[key]

    def _check_cams(self, cams, device=None):
        tensor_arg("cams", cams, torch.float32, ("nsets", "V", capi.FVP_CAM_FLOATS), device)
        require_gpu("the re-fit", cams.device, self._injected)
        if cams.shape[0] < 1 or not 1 <= cams.shape[1] <= capi.FVP_MAX_VIEWS:
            raise capi.FvpError(f"CameraRefiner limits: nsets >= 1, 1 <= V <= {capi.FVP_MAX_VIEWS} (cams {tuple(cams.shape)})")

    # ---- the two calls ----------------------------------------------------------------------------------------------
    def accumulate(self, points, obs, view_state, cams, frame_set):
        """One launch: the observations of one batch into the accumulators.  ``points [B,N,J,5]`` (``fused_poses`` or
        ``tri_poses``), ``obs [B,V,N,J,4]`` and ``view_state [B,V,N,J]`` int32 as ``JointTriangulator`` left them for the
        same batch, ``cams [nsets,V,24]`` and ``frame_set [B]`` int32 (the engine's tables)."""
        p = tensor_arg("points", points, torch.float32, ("B", "N", self.J, 5))
        self._check_cams(cams, p.device)
        B, N = p.shape[:2]
        nsets, V = cams.shape[:2]
        if N < 1:
            raise capi.FvpError("CameraRefiner limits: N >= 1")
        for name, t, dt, shape in (("obs", obs, torch.float32, (B, V, N, self.J, 4)),
                                   ("view_state", view_state, torch.int32, (B, V, N, self.J)),
                                   ("frame_set", frame_set, torch.int32, (B,))):
            tensor_arg(name, t, dt, shape, p.device)
        acc = self._state(nsets, V, p.device)
        if B == 0:
            return acc                                  # (an empty tensor has no address to pass)
        rc = self.lib.fvp_camera_refit_accumulate(_ptr(p), _ptr(obs), _ptr(view_state), _ptr(cams), nsets, _ptr(frame_set), B,
                                                  V, N, self.J, self.undistort_iters, self.huber_px, self.decay, _ptr(acc),
                                                  stream_ptr(p.device))
        capi.check(self.lib, rc, "fvp_camera_refit_accumulate")
        return acc

    def solve(self, cams):
        """One launch: ``(cams_out [nsets,V,24], cal_stats [nsets,V,6], cal_state [nsets,V] int32)`` from the accumulators and
        the table they were accumulated against.  ``cal_state``: 1 solved, 2 solved and clamped to the trust region, 0 fewer
        than ``min_obs`` observations, -1 degenerate - in the last two the record is copied.  ``cal_stats``: (step angle in
        radians, step length in mm, rms residual before the step in pixels, the rms the linear model expects after it, the
        number of observations, the smallest scaled pivot).  Two preallocated output sets are used in turn: a result stays
        valid across the next ``solve``, not the one after."""
        self._check_cams(cams)
        nsets, V = cams.shape[:2]
        acc = self._state(nsets, V, cams.device)
        slot = self.outputs(nsets, V, cams.device)
        use = slot[1]
        if slot[0][use][0].data_ptr() == cams.data_ptr():   # the table handed in is an earlier result: write the other set
            use = 1 - use
        slot[1] = 1 - use
        out = slot[0][use]
        rc = self.lib.fvp_camera_refit_solve(_ptr(acc), _ptr(cams), nsets, V, self.min_obs, self.lam, self.min_pivot,
                                             self.max_angle_rad, self.max_shift_mm, *[_ptr(t) for t in out],
                                             stream_ptr(cams.device))
        capi.check(self.lib, rc, "fvp_camera_refit_solve")
        return out

    def refine(self, points, obs, view_state, cams, frame_set, iters=3):
        """``iters`` Gauss-Newton rounds on one batch: reset, accumulate, solve, each round against the round before's
        ``cams_out`` (the observations are pixels and do not depend on the camera table).  No host synchronisation.  The
        accumulators are left holding the last round's sums, linearised at the last round's input table."""
        if int(iters) < 1:
            raise capi.FvpError(f"refine needs iters >= 1, got {iters}")
        out = None
        for _ in range(int(iters)):
            self.reset()
            self.accumulate(points, obs, view_state, cams, frame_set)
            out = self.solve(cams)
            cams = out[0]
        return out

    @staticmethod
    def camera_dicts(cams_out, names):
        """``cams_out [nsets,V,24]`` -> the ``cameras`` dict of the forward, ``{name: [dict(R, T, fx, fy, cx, cy, k, p) per
        view]}`` for the set names ``names``: pass it to ``model(...)`` under a new sequence name to adopt the corrected
        rig.  Copies to the host (the one place here that synchronises)."""
        c = cams_out.detach().cpu().numpy()
        if c.ndim != 3 or c.shape[2] != capi.FVP_CAM_FLOATS or len(names) != c.shape[0]:
            raise capi.FvpError(f"camera_dicts needs [nsets,V,{capi.FVP_CAM_FLOATS}] records and one name per set")
        return {name: [dict(R=r[0:9].reshape(3, 3).copy(), T=r[9:12].reshape(3, 1).copy(), fx=float(r[12]), fy=float(r[13]),
                            cx=float(r[14]), cy=float(r[15]), k=r[16:19].reshape(3, 1).copy(), p=r[19:21].reshape(2, 1).copy())
                       for r in c[s]] for s, name in enumerate(names)}
