"""Steady poses per person: ``PoseSmoother`` owns the device-side state of ``fvp_track_smooth`` (include/fvp.h, ABI 13)
and issues one launch per batch on the caller's current HIP stream.

``PoseTracker.update`` gives every valid slot of ``fused_poses [B,N,J,5]`` a track id and a track slot; the poses
themselves are still the raw per-frame estimates.  ``update`` here runs a One-Euro filter (Casiez et al. 2012) per joint of
every track: a joint the cameras do not support (``joint_conf < conf_min``, NaN, Inf) is bridged by prediction, a track
that drops out coasts for up to ``max_age`` frames, and every track keeps its row of ``track_poses`` for its whole life.
All of it is defined bit for bit in include/fvp.h.  Not built: feeding the predictions back into the tracker's
association (the tracker still matches against the raw last pose), re-identification after ``max_age``.

No arithmetic happens here and nothing synchronises with the host: PyTorch is used for device memory and streams only.
"""
import ctypes as C

import torch

from .. import _capi as capi
from .tracking import PoseTracker


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


class PoseSmoother:
    """``PoseSmoother(tracker_or_shape, rate_hz=30.0, min_cutoff=1.0, beta=0.005, d_cutoff=1.0, conf_min=0.0, damp=0.8,
    max_age=None, device=None)``

    ``tracker_or_shape``  a ``PoseTracker`` - N, J, T, nseq, max_age, the device and the sequence numbering are the
                          tracker's - or the tuple ``(N, J, T, nseq)``;
    ``rate_hz``           frames per second of a sequence;
    ``min_cutoff``        cutoff (Hz) of the position filter at rest: lower is steadier and lags more;
    ``beta``              cutoff gained per mm/s of filtered speed: higher follows fast motion more closely;
    ``d_cutoff``          cutoff (Hz) of the velocity filter;
    ``conf_min``          with ``joint_conf`` given, a joint below it is predicted instead of measured;
    ``damp``              factor in [0, 1] on the velocity of every predicted frame;
    ``max_age``           a track unseen for more than max_age frames is dropped (default: the tracker's, else 15).
    The defaults are API defaults, not tuned values.

    State (device tensors, one row per sequence): ``flt_pose [nseq,T,J,3]``, ``flt_vel [nseq,T,J,3]`` (mm/s), ``flt_id
    [nseq,T]`` (-1 = free slot), ``flt_age [nseq,T]``."""

    _STATE = ("flt_pose", "flt_vel", "flt_id", "flt_age")

    def __init__(self, tracker_or_shape, rate_hz=30.0, min_cutoff=1.0, beta=0.005, d_cutoff=1.0, conf_min=0.0, damp=0.8,
                 max_age=None, device=None, _lib=None):
        # `_lib` is a test seam (tests/hipemu); the product always loads libfvp_hip.so
        self.tracker = tracker_or_shape if isinstance(tracker_or_shape, PoseTracker) else None
        if self.tracker is not None:
            tr = self.tracker
            N, J, T, nseq = tr.N, tr.J, tr.T, tr.nseq
            max_age = tr.max_age if max_age is None else max_age
            device = tr.device if device is None else device
            if _lib is None and tr._injected:
                _lib = tr.lib
        else:
            N, J, T, nseq = tracker_or_shape
        self._injected = _lib is not None
        self.lib = _lib if _lib is not None else capi.load()
        self.N, self.J, self.T, self.nseq = int(N), int(J), int(T), int(nseq)
        self.max_age = 15 if max_age is None else int(max_age)
        self.rate_hz, self.min_cutoff, self.beta = float(rate_hz), float(min_cutoff), float(beta)
        self.d_cutoff, self.conf_min, self.damp = float(d_cutoff), float(conf_min), float(damp)
        self.device = torch.device("cuda" if device is None else device)
        if not self._injected and self.device.type != "cuda":
            raise capi.FvpError(f"device={str(self.device)!r}: the smoother runs on a ROCm GPU device (spelled 'cuda:N' in "
                                "PyTorch-ROCm); there is no CPU fallback")
        if self.N < 1 or self.J < 1 or self.nseq < 1 or self.T < self.N or self.max_age < 0:
            raise capi.FvpError(f"PoseSmoother needs N, J, nseq >= 1, T >= N and max_age >= 0 (N = {self.N}, J = {self.J}, "
                                f"nseq = {self.nseq}, T = {self.T}, max_age = {self.max_age})")
        if self.N > capi.FVP_TRACK_MAX_DETS or self.T > capi.FVP_TRACK_MAX_TRACKS or self.J > capi.FVP_MAX_JOINTS:
            raise capi.FvpError(f"PoseSmoother limits: N <= {capi.FVP_TRACK_MAX_DETS}, T <= {capi.FVP_TRACK_MAX_TRACKS}, "
                                f"J <= {capi.FVP_MAX_JOINTS} (N = {self.N}, T = {self.T}, J = {self.J})")
        # (written so that a NaN fails, as in the library)
        if not (self.rate_hz > 0 and self.min_cutoff > 0 and self.d_cutoff > 0 and self.beta >= 0 and 0 <= self.damp <= 1):
            raise capi.FvpError(f"PoseSmoother needs rate_hz, min_cutoff, d_cutoff > 0, beta >= 0 and damp in [0, 1] "
                                f"(rate_hz = {self.rate_hz}, min_cutoff = {self.min_cutoff}, d_cutoff = {self.d_cutoff}, "
                                f"beta = {self.beta}, damp = {self.damp})")
        dev = self.device
        self.flt_pose = torch.zeros((self.nseq, self.T, self.J, 3), device=dev)
        self.flt_vel = torch.zeros((self.nseq, self.T, self.J, 3), device=dev)
        self.flt_id = torch.full((self.nseq, self.T), -1, dtype=torch.int32, device=dev)
        self.flt_age = torch.zeros((self.nseq, self.T), dtype=torch.int32, device=dev)
        # without a tracker to share the numbering with: sequence name -> state row in order of first appearance
        self.seq_ids = self.tracker.seq_ids if self.tracker is not None else {}
        self._frame_sets = {}

    # ---------------------------------------------------------------------------------------------
    def _stream(self):
        if self.device.type == "cuda":
            return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        return None

    def frame_sets(self, seqs):
        """[B] int32 device tensor of state rows for a list of sequence names: the tracker's numbering when built from one."""
        if self.tracker is not None:
            return self.tracker.frame_sets(seqs)
        seqs = tuple(seqs)
        for s in seqs:
            if s not in self.seq_ids:
                if len(self.seq_ids) >= self.nseq:
                    raise capi.FvpError(f"sequence {s!r} is one more than the nseq = {self.nseq} this smoother was built for "
                                        f"(known: {list(self.seq_ids)})")
                self.seq_ids[s] = len(self.seq_ids)
        if seqs not in self._frame_sets:
            if len(self._frame_sets) >= 256:            # bounded, as in the engine
                self._frame_sets.pop(next(iter(self._frame_sets)))
            self._frame_sets[seqs] = torch.tensor([self.seq_ids[s] for s in seqs], dtype=torch.int32, device=self.device)
        return self._frame_sets[seqs]

    def _same_device(self, t):
        return t.device == self.device or (self.device.index is None and t.device.type == self.device.type)

    def update(self, fused_poses, ids, slots, joint_conf=None, meta=None, sequences=None):
        """One batch ``fused_poses [B,N,J,5]`` with the ``ids [B,N]`` and ``slots [B,N]`` ``PoseTracker.update`` returned
        for it, frames in time order -> ``(smooth [B,N,J,5], track_poses [B,T,J,4], track_state [B,T,2] int32)``:
        ``smooth`` is ``fused_poses`` with the xyz of every valid slot replaced by its track's filtered ones (the layout
        core/metrics.py, utils/vis.py and ``joint_evidence`` take); ``track_poses[b,t]`` = (x, y, z, flag) of track slot t
        after frame b - a person keeps its row for the life of the track, flag 1 = measured in this frame, 0 = predicted
        (an unsupported joint, or the whole track coasting), a free slot is zeros; ``track_state[b,t]`` = (track id, frames
        since last seen), (-1, 0) for a free slot.  One launch on the current stream, no host synchronisation.

        ``joint_conf [B,N,J]`` (``last_evidence[1]``): joints below ``conf_min`` are predicted; None: every finite joint is
        measured.  ``sequences`` / ``meta`` as for ``PoseTracker.update``."""
        t = fused_poses
        if t.dtype != torch.float32:
            raise capi.FvpError(f"fused_poses must be float32, got {t.dtype}")
        if not self._same_device(t):
            raise capi.FvpError(f"fused_poses lives on {t.device}, the smoother was built for {self.device}")
        if t.dim() != 4 or tuple(t.shape[1:]) != (self.N, self.J, 5) or not t.is_contiguous():
            raise capi.FvpError(f"fused_poses must be contiguous [B,{self.N},{self.J},5], got {tuple(t.shape)}")
        B = t.shape[0]
        for name, x in (("ids", ids), ("slots", slots)):
            if not torch.is_tensor(x) or x.dtype != torch.int32 or x.device != t.device or tuple(x.shape) != (B, self.N) \
                    or not x.is_contiguous():
                raise capi.FvpError(f"{name} must be a contiguous int32 tensor [{B},{self.N}] on {t.device} (what "
                                    f"PoseTracker.update returned for this batch)")
        if joint_conf is not None:
            c = joint_conf
            if c.dtype != torch.float32 or c.device != t.device or tuple(c.shape) != (B, self.N, self.J) \
                    or not c.is_contiguous():
                raise capi.FvpError(f"joint_conf must be a contiguous float32 tensor [{B},{self.N},{self.J}] on {t.device}, "
                                    f"got {c.dtype} {tuple(c.shape)} on {c.device}")
        if sequences is None and meta is not None:
            sequences = meta["seq"]
        if sequences is None:
            fs = None
        elif torch.is_tensor(sequences):
            fs = sequences
            if fs.dtype != torch.int32 or fs.device != t.device or tuple(fs.shape) != (B,) or not fs.is_contiguous():
                raise capi.FvpError(f"sequences must be a contiguous int32 tensor [{B}] on {t.device}, got {fs.dtype} "
                                    f"{tuple(fs.shape)} on {fs.device}")
        else:
            if len(sequences) != B:
                raise capi.FvpError(f"{len(sequences)} sequence names for {B} frames")
            fs = self.frame_sets(sequences)
        smooth = torch.empty_like(t)
        track_poses = torch.empty((B, self.T, self.J, 4), device=self.device)
        track_state = torch.empty((B, self.T, 2), dtype=torch.int32, device=self.device)
        if B == 0:
            return smooth, track_poses, track_state
        rc = self.lib.fvp_track_smooth(_ptr(t), _ptr(fs), _ptr(ids), _ptr(slots), _ptr(joint_conf), _ptr(self.flt_pose),
                                       _ptr(self.flt_vel), _ptr(self.flt_id), _ptr(self.flt_age), _ptr(smooth),
                                       _ptr(track_poses), _ptr(track_state), B, self.N, self.J, self.nseq, self.T,
                                       self.rate_hz, self.min_cutoff, self.beta, self.d_cutoff, self.conf_min, self.damp,
                                       self.max_age, self._stream())
        capi.check(self.lib, rc, "fvp_track_smooth")
        return smooth, track_poses, track_state

    def reset(self, seq=None):
        """Back to the initial state (no tracks): every sequence, or one (a state row or a name)."""
        if seq is None:
            rows = slice(None)
        else:
            rows = self.seq_ids[seq] if not isinstance(seq, int) else seq
            if not 0 <= rows < self.nseq:
                raise capi.FvpError(f"sequence row {rows} outside [0, {self.nseq})")
        self.flt_pose[rows] = 0.0
        self.flt_vel[rows] = 0.0
        self.flt_id[rows] = -1
        self.flt_age[rows] = 0

    def state(self):
        """Clones of the four state tensors (checkpointing, tests)."""
        return {k: getattr(self, k).clone() for k in self._STATE}

    def load_state(self, state):
        """The inverse of ``state()``."""
        for k in self._STATE:
            getattr(self, k).copy_(state[k])
