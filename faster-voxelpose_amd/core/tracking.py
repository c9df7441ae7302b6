"""Person identities across frames: ``PoseTracker`` owns the device-side state of ``fvp_track_update`` (include/fvp.h,
ABI 12) and issues one launch per batch on the caller's current HIP stream.

The forward returns ``fused_poses [B,N,J,5]`` ordered by NMS rank: the same person sits in slot 3 in one frame and in slot
0 in the next.  ``update`` gives every valid slot a track id that follows the person through the frames of its camera
sequence - nearest-pose greedy association with a distance gate, births, a maximum age and eviction from a full table, all
defined bit for bit in include/fvp.h.  Pose smoothing and coasting through gaps consume the ids: core/smoothing.py
(``PoseSmoother``).  Not built: motion prediction inside the association (it runs on the raw last pose, not on the smoother's
predictions), re-identification after ``max_age``, Hungarian (optimal) assignment.
Re-identification of a person who comes back after ``max_age`` is ``fvp_track_reid``: core/reid.py (``PersonReId``).

No arithmetic happens here and nothing synchronises with the host: PyTorch is used for device memory and streams only.
"""
import torch

from .. import _capi as capi
from .._args import (SequenceRows, device_matches, frame_rows, load_lib, require_gpu, stream_ptr, tensor_arg)
from .._args import ptr as _ptr


class PoseTracker:
    """``PoseTracker(cfg_or_N_J, nseq=1, max_tracks=None, gate_mm=500.0, max_age=15, device=None)``

    ``cfg_or_N_J``  a config (``CAPTURE_SPEC.MAX_PEOPLE`` slots per frame, ``DATASET.NUM_JOINTS`` joints, ``DEVICE``) or
                    the pair ``(N, J)``;
    ``nseq``        camera sequences tracked side by side, each with its own time line and its own ids from 0;
    ``max_tracks``  track slots per sequence, T >= N (default 2 N, at most ``FVP_TRACK_MAX_TRACKS``);
    ``gate_mm``     a detection and a track may be matched when their mean joint distance is <= gate_mm;
    ``max_age``     a track unmatched for more than max_age frames of its sequence is dropped.
    The three defaults are API defaults, not tuned values.

    State (device tensors, one row per sequence): ``trk_pose [nseq,T,J,3]``, ``trk_id [nseq,T]`` (-1 = free slot),
    ``trk_age [nseq,T]``, ``next_id [nseq]``."""

    def __init__(self, cfg_or_N_J, nseq=1, max_tracks=None, gate_mm=500.0, max_age=15, device=None, _lib=None):
        self.lib, self._injected = load_lib(_lib)
        if isinstance(cfg_or_N_J, (tuple, list)):
            N, J = cfg_or_N_J
        else:
            N, J = cfg_or_N_J.CAPTURE_SPEC.MAX_PEOPLE, cfg_or_N_J.DATASET.NUM_JOINTS
            device = cfg_or_N_J.DEVICE if device is None else device
        self.N, self.J, self.nseq = int(N), int(J), int(nseq)
        self.T = 2 * self.N if max_tracks is None else int(max_tracks)
        self.gate_mm, self.max_age = float(gate_mm), int(max_age)
        self.device = torch.device("cuda" if device is None else device)
        require_gpu("the tracker", self.device, self._injected)
        if self.N < 1 or self.J < 1 or self.nseq < 1 or self.T < self.N or self.max_age < 0:
            raise capi.FvpError(f"PoseTracker needs N, J, nseq >= 1, max_tracks >= N and max_age >= 0 (N = {self.N}, "
                                f"J = {self.J}, nseq = {self.nseq}, max_tracks = {self.T}, max_age = {self.max_age})")
        if self.N > capi.FVP_TRACK_MAX_DETS or self.T > capi.FVP_TRACK_MAX_TRACKS or self.J > capi.FVP_MAX_JOINTS:
            raise capi.FvpError(f"PoseTracker limits: N <= {capi.FVP_TRACK_MAX_DETS}, max_tracks <= "
                                f"{capi.FVP_TRACK_MAX_TRACKS}, J <= {capi.FVP_MAX_JOINTS} (N = {self.N}, max_tracks = "
                                f"{self.T}, J = {self.J})")
        dev = self.device
        self.trk_pose = torch.zeros((self.nseq, self.T, self.J, 3), device=dev)
        self.trk_id = torch.full((self.nseq, self.T), -1, dtype=torch.int32, device=dev)
        self.trk_age = torch.zeros((self.nseq, self.T), dtype=torch.int32, device=dev)
        self.next_id = torch.zeros((self.nseq,), dtype=torch.int32, device=dev)
        self._rows = SequenceRows(limit=self.nseq)
        self.seq_ids = self._rows.ids                  # sequence name -> row of the state, in order of first appearance

    # ---------------------------------------------------------------------------------------------
    def frame_sets(self, seqs):
        """[B] int32 device tensor of state rows for a list of sequence names (uploaded once per distinct list)."""
        return self._rows.rows(seqs, self.device)

    def update(self, fused_poses, meta=None, sequences=None):
        """One batch ``fused_poses [B,N,J,5]`` (the forward's first output, or any poses in that layout), frames in time
        order -> ``(ids [B,N] int32, slots [B,N] int32, costs [B,N] float32)``: the track id of every valid slot (-1 for
        an invalid one), the track slot that holds it, and the mean joint distance in mm to the track it was matched
        with (-1 for a new track and for invalid slots).  One launch on the current stream, no host synchronisation.

        The sequence of each frame: ``sequences`` - an int32 device tensor [B] of state rows (what
        ``engine.frame_sets()`` returns: the forward passes its own), or a list of B sequence names - else
        ``meta['seq']``, else sequence 0 for every frame.  A row outside [0, nseq) belongs to no sequence: the frame comes
        back all -1 and changes nothing."""
        t = tensor_arg("fused_poses", fused_poses, torch.float32, ("B", self.N, self.J, 5))
        if not device_matches(t.device, self.device):
            raise capi.FvpError(f"fused_poses lives on {t.device}, the tracker was built for {self.device}")
        B = t.shape[0]
        fs = frame_rows(self.frame_sets, sequences, meta, B, t.device)
        ids = torch.empty((B, self.N), dtype=torch.int32, device=self.device)
        slots = torch.empty((B, self.N), dtype=torch.int32, device=self.device)
        costs = torch.empty((B, self.N), device=self.device)
        if B == 0:
            return ids, slots, costs
        rc = self.lib.fvp_track_update(_ptr(t), _ptr(fs), _ptr(self.trk_pose), _ptr(self.trk_id), _ptr(self.trk_age),
                                       _ptr(self.next_id), _ptr(ids), _ptr(slots), _ptr(costs), B, self.N, self.J,
                                       self.nseq, self.T, self.gate_mm, self.max_age, stream_ptr(self.device))
        capi.check(self.lib, rc, "fvp_track_update")
        return ids, slots, costs

    def reset(self, seq=None):
        """Back to the initial state (no tracks, ids from 0 again): every sequence, or one (a state row or a name)."""
        if seq is None:
            rows = slice(None)
        else:
            rows = self.seq_ids[seq] if not isinstance(seq, int) else seq
            if not 0 <= rows < self.nseq:
                raise capi.FvpError(f"sequence row {rows} outside [0, {self.nseq})")
        self.trk_pose[rows] = 0.0
        self.trk_id[rows] = -1
        self.trk_age[rows] = 0
        self.next_id[rows] = 0

    def state(self):
        """Clones of the four state tensors (checkpointing, tests)."""
        return dict(trk_pose=self.trk_pose.clone(), trk_id=self.trk_id.clone(), trk_age=self.trk_age.clone(),
                    next_id=self.next_id.clone())

    def load_state(self, state):
        """The inverse of ``state()``."""
        for k in ("trk_pose", "trk_id", "trk_age", "next_id"):
            getattr(self, k).copy_(state[k])
