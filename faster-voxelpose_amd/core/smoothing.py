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
import torch

from .. import _capi as capi
from .._args import (SequenceRows, device_matches, frame_rows, load_lib, require_gpu, stream_ptr, tensor_arg)
from .._args import ptr as _ptr
from .tracking import PoseTracker


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
        self.lib, self._injected = load_lib(_lib)
        self.N, self.J, self.T, self.nseq = int(N), int(J), int(T), int(nseq)
        self.max_age = 15 if max_age is None else int(max_age)
        self.rate_hz, self.min_cutoff, self.beta = float(rate_hz), float(min_cutoff), float(beta)
        self.d_cutoff, self.conf_min, self.damp = float(d_cutoff), float(conf_min), float(damp)
        self.device = torch.device("cuda" if device is None else device)
        require_gpu("the smoother", self.device, self._injected)
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
        # the tracker's numbering when built from one; else sequence name -> state row in order of first appearance
        self._rows = SequenceRows(limit=self.nseq)
        self.seq_ids = self.tracker.seq_ids if self.tracker is not None else self._rows.ids

    # ---------------------------------------------------------------------------------------------
    def frame_sets(self, seqs):
        """[B] int32 device tensor of state rows for a list of sequence names: the tracker's numbering when built from one."""
        if self.tracker is not None:
            return self.tracker.frame_sets(seqs)
        return self._rows.rows(seqs, self.device)

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
        t = tensor_arg("fused_poses", fused_poses, torch.float32, ("B", self.N, self.J, 5))
        if not device_matches(t.device, self.device):
            raise capi.FvpError(f"fused_poses lives on {t.device}, the smoother was built for {self.device}")
        B = t.shape[0]
        for name, x in (("ids", ids), ("slots", slots)):
            tensor_arg(name, x, torch.int32, (B, self.N), t.device, hint="what PoseTracker.update returned for this batch")
        tensor_arg("joint_conf", joint_conf, torch.float32, (B, self.N, self.J), t.device, optional=True)
        fs = frame_rows(self.frame_sets, sequences, meta, B, t.device)
        smooth = torch.empty_like(t)
        track_poses = torch.empty((B, self.T, self.J, 4), device=self.device)
        track_state = torch.empty((B, self.T, 2), dtype=torch.int32, device=self.device)
        if B == 0:
            return smooth, track_poses, track_state
        rc = self.lib.fvp_track_smooth(_ptr(t), _ptr(fs), _ptr(ids), _ptr(slots), _ptr(joint_conf), _ptr(self.flt_pose),
                                       _ptr(self.flt_vel), _ptr(self.flt_id), _ptr(self.flt_age), _ptr(smooth),
                                       _ptr(track_poses), _ptr(track_state), B, self.N, self.J, self.nseq, self.T,
                                       self.rate_hz, self.min_cutoff, self.beta, self.d_cutoff, self.conf_min, self.damp,
                                       self.max_age, stream_ptr(self.device))
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
