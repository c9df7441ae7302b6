"""Bone lengths per person: ``LimbModel`` owns the device-side state of ``fvp_limb_learn`` (include/fvp.h, ABI 22) and
issues ``fvp_limb_learn`` and ``fvp_limb_fit``, one launch each per batch, on the caller's current HIP stream.

The tracker gives every person an id and a track slot, the smoother steadies every joint on its own; neither knows that a
person is a rigid linkage, so a forearm breathes from frame to frame and an occluded wrist sits wherever the soft-argmax put
it.  ``update`` keeps a running, gated estimate of every limb's length per track, taken from the frames in which both ends
are supported (``joint_conf >= conf_min``, finite); ``fit`` moves a pose, as little as a few Gauss-Seidel sweeps allow, onto
those lengths - with both ends supported each takes half of a limb's correction, an unsupported end takes all of it.  All of
it is defined bit for bit in include/fvp.h.  Not built: carrying a person's lengths across re-identification, lengths as a
re-ID or association cue, joint-angle limits, left/right symmetry, a fit coupled into the One-Euro state.

``LimbModel`` is not a model attribute and not a row of the forward's stage table: it runs behind the forward
(INTEGRATION.md).  No arithmetic happens here and nothing synchronises with the host: PyTorch is used for device memory and
streams only.
"""
import ctypes as C

import torch

from .. import _capi as capi
from .._args import (SequenceRows, device_matches, frame_rows, load_lib, require_gpu, stream_ptr, tensor_arg)
from .._args import ptr as _ptr
from .tracking import PoseTracker


class LimbModel:
    """``LimbModel(tracker_or_shape, limbs=None, conf_min=0.0, min_frames=10, window=64, gate_sigma=3.0, gate_mm=20.0,
    relearn=15, stiffness=1.0, iters=4, device=None)``

    ``tracker_or_shape``  a ``PoseTracker`` - N, J, T, nseq, the device and the sequence numbering are the tracker's - or
                          the tuple ``(N, J, T, nseq)``;
    ``limbs``             joint index pairs [L,2], L <= 64, any list (cycles are fine); default: the table of ``utils.vis``
                          for J in {14, 15, 17};
    ``conf_min``          with ``joint_conf`` given, a joint below it is unsupported: its limbs are not measured, and the
                          fit moves it alone;
    ``min_frames``        accepted samples before a limb's length is used (``target`` is 0 until then) and gated;
    ``window``            samples the running mean and variance weigh equally; exponential forgetting after that;
    ``gate_sigma``, ``gate_mm``  a sample further from the length than max(gate_sigma * std, gate_mm) is an outlier;
    ``relearn``           more outliers in a row than this and the limb starts over from the sample;
    ``stiffness``         fraction in [0, 1] of a limb's length error one visit removes;
    ``iters``             Gauss-Seidel sweeps over the limb table, 1..32.
    The defaults are API defaults, not tuned values.

    State (device tensors, one row per sequence): ``limb_len [nseq,T,L]``, ``limb_var [nseq,T,L]``, ``limb_cnt [nseq,T,L]``,
    ``limb_out [nseq,T,L]`` (int32), ``limb_id [nseq,T]`` (-1 = never used)."""

    _STATE = ("limb_len", "limb_var", "limb_cnt", "limb_out", "limb_id")

    def __init__(self, tracker_or_shape, limbs=None, conf_min=0.0, min_frames=10, window=64, gate_sigma=3.0, gate_mm=20.0,
                 relearn=15, stiffness=1.0, iters=4, device=None, _lib=None):
        self.tracker = tracker_or_shape if isinstance(tracker_or_shape, PoseTracker) else None
        if self.tracker is not None:
            tr = self.tracker
            N, J, T, nseq = tr.N, tr.J, tr.T, tr.nseq
            device = tr.device if device is None else device
            if _lib is None and tr._injected:
                _lib = tr.lib
        else:
            N, J, T, nseq = tracker_or_shape
        self.lib, self._injected = load_lib(_lib)
        self.N, self.J, self.T, self.nseq = int(N), int(J), int(T), int(nseq)
        self.conf_min, self.gate_sigma, self.gate_mm = float(conf_min), float(gate_sigma), float(gate_mm)
        self.min_frames, self.window, self.relearn = int(min_frames), int(window), int(relearn)
        self.stiffness, self.iters = float(stiffness), int(iters)
        self.device = torch.device("cuda" if device is None else device)
        require_gpu("the limb model", self.device, self._injected)
        if limbs is None:
            from ..utils.vis import _LIMBS                # (imports matplotlib: only for the default table)
            if self.J not in _LIMBS:
                raise capi.FvpError(f"no default skeleton for {self.J} joints (known: {sorted(_LIMBS)}): pass limbs")
            limbs = _LIMBS[self.J]
        self.limbs = [(int(a), int(b)) for a, b in limbs]
        self.L = len(self.limbs)
        if self.N < 1 or self.J < 1 or self.nseq < 1 or self.T < self.N:
            raise capi.FvpError(f"LimbModel needs N, J, nseq >= 1 and T >= N (N = {self.N}, J = {self.J}, nseq = {self.nseq}, "
                                f"T = {self.T})")
        if self.N > capi.FVP_TRACK_MAX_DETS or self.T > capi.FVP_TRACK_MAX_TRACKS or self.J > capi.FVP_MAX_JOINTS:
            raise capi.FvpError(f"LimbModel limits: N <= {capi.FVP_TRACK_MAX_DETS}, T <= {capi.FVP_TRACK_MAX_TRACKS}, "
                                f"J <= {capi.FVP_MAX_JOINTS} (N = {self.N}, T = {self.T}, J = {self.J})")
        if not 1 <= self.L <= capi.FVP_LIMB_MAX or any(not (0 <= a < self.J and 0 <= b < self.J and a != b)
                                                        for a, b in self.limbs):
            raise capi.FvpError(f"limbs: 1 to {capi.FVP_LIMB_MAX} pairs of two different joint indices in [0, {self.J})")
        # (written so that a NaN fails, as in the library)
        if not (self.min_frames >= 1 and self.window >= self.min_frames and self.relearn >= 0 and self.gate_sigma >= 0
                and self.gate_mm >= 0 and 0 <= self.stiffness <= 1 and 1 <= self.iters <= 32):
            raise capi.FvpError(f"LimbModel needs min_frames >= 1, window >= min_frames, relearn >= 0, gate_sigma and gate_mm "
                                f">= 0, stiffness in [0, 1] and iters in [1, 32] (min_frames = {self.min_frames}, window = "
                                f"{self.window}, relearn = {self.relearn}, gate_sigma = {self.gate_sigma}, gate_mm = "
                                f"{self.gate_mm}, stiffness = {self.stiffness}, iters = {self.iters})")
        self._limbs = (C.c_int32 * (2 * self.L))(*[j for ab in self.limbs for j in ab])
        dev, shape = self.device, (self.nseq, self.T, self.L)
        self.limb_len = torch.zeros(shape, device=dev)
        self.limb_var = torch.zeros(shape, device=dev)
        self.limb_cnt = torch.zeros(shape, dtype=torch.int32, device=dev)
        self.limb_out = torch.zeros(shape, dtype=torch.int32, device=dev)
        self.limb_id = torch.full((self.nseq, self.T), -1, dtype=torch.int32, device=dev)
        # the tracker's numbering when built from one; else sequence name -> state row in order of first appearance
        self._rows = SequenceRows(limit=self.nseq)
        self.seq_ids = self.tracker.seq_ids if self.tracker is not None else self._rows.ids

    # ---------------------------------------------------------------------------------------------
    def frame_sets(self, seqs):
        """[B] int32 device tensor of state rows for a list of sequence names: the tracker's numbering when built from one."""
        if self.tracker is not None:
            return self.tracker.frame_sets(seqs)
        return self._rows.rows(seqs, self.device)

    def _poses(self, name, poses):
        t = tensor_arg(name, poses, torch.float32, ("B", self.N, self.J, 5))
        if not device_matches(t.device, self.device):
            raise capi.FvpError(f"{name} lives on {t.device}, the limb model was built for {self.device}")
        return t

    def update(self, fused_poses, ids, slots, joint_conf=None, meta=None, sequences=None):
        """One batch ``fused_poses [B,N,J,5]`` with the ``ids [B,N]`` and ``slots [B,N]`` ``PoseTracker.update`` returned
        for it, frames in time order -> ``(target [B,N,L], limb_obs [B,N,L,2], limb_state [B,N,L] int32)``: ``target`` is
        the learned length (mm) of every limb of the person in that slot after this frame, 0 while it has fewer than
        ``min_frames`` samples; ``limb_obs`` = (measured length, its difference to the length before this frame), (-1, 0)
        for a limb that was not measured; ``limb_state`` one of ``capi.FVP_LIMB_*``.  One launch on the current stream, no
        host synchronisation.

        ``joint_conf [B,N,J]`` (``last_evidence[1]``): a limb with an end below ``conf_min`` is not measured; None: every
        finite joint is supported.  ``sequences`` / ``meta`` as for ``PoseTracker.update``."""
        t = self._poses("fused_poses", fused_poses)
        B = t.shape[0]
        for name, x in (("ids", ids), ("slots", slots)):
            tensor_arg(name, x, torch.int32, (B, self.N), t.device, hint="what PoseTracker.update returned for this batch")
        tensor_arg("joint_conf", joint_conf, torch.float32, (B, self.N, self.J), t.device, optional=True)
        fs = frame_rows(self.frame_sets, sequences, meta, B, t.device)
        target = torch.empty((B, self.N, self.L), device=self.device)
        limb_obs = torch.empty((B, self.N, self.L, 2), device=self.device)
        limb_state = torch.empty((B, self.N, self.L), dtype=torch.int32, device=self.device)
        if B == 0:
            return target, limb_obs, limb_state
        rc = self.lib.fvp_limb_learn(_ptr(t), _ptr(fs), _ptr(ids), _ptr(slots), _ptr(joint_conf), self._limbs, self.L,
                                     _ptr(self.limb_len), _ptr(self.limb_var), _ptr(self.limb_cnt), _ptr(self.limb_out),
                                     _ptr(self.limb_id), _ptr(target), _ptr(limb_obs), _ptr(limb_state), B, self.N, self.J,
                                     self.nseq, self.T, self.conf_min, self.min_frames, self.window, self.gate_sigma,
                                     self.gate_mm, self.relearn, stream_ptr(self.device))
        capi.check(self.lib, rc, "fvp_limb_learn")
        return target, limb_obs, limb_state

    def fit(self, poses, target, ids=None, joint_conf=None):
        """``poses [B,N,J,5]`` - any poses of the layout: the forward's ``fused_poses``, the smoother's ``smooth`` - moved
        onto ``target [B,N,L]`` -> ``(fitted [B,N,J,5], resid [B,N,L])``: ``fitted`` is ``poses`` with the xyz of every
        valid slot (flag >= 0, and ``ids >= 0`` when given) constrained, columns 3:5 and invalid slots copied; ``resid`` the
        length error (mm) every constrained limb is left with, else 0.  A limb whose target is 0 constrains nothing.  Stateless;
        one launch on the current stream, no host synchronisation."""
        t = self._poses("poses", poses)
        B = t.shape[0]
        tensor_arg("target", target, torch.float32, (B, self.N, self.L), t.device)
        tensor_arg("ids", ids, torch.int32, (B, self.N), t.device, optional=True)
        tensor_arg("joint_conf", joint_conf, torch.float32, (B, self.N, self.J), t.device, optional=True)
        fitted = torch.empty_like(t)
        resid = torch.empty((B, self.N, self.L), device=self.device)
        if B == 0:
            return fitted, resid
        rc = self.lib.fvp_limb_fit(_ptr(t), _ptr(ids), _ptr(joint_conf), _ptr(target), self._limbs, self.L, _ptr(fitted),
                                   _ptr(resid), B, self.N, self.J, self.conf_min, self.stiffness, self.iters,
                                   stream_ptr(self.device))
        capi.check(self.lib, rc, "fvp_limb_fit")
        return fitted, resid

    def __call__(self, fused_poses, ids, slots, joint_conf=None, meta=None, sequences=None):
        """``update`` followed by ``fit`` on the same poses -> ``(fitted, target, limb_state, resid)``."""
        target, _, limb_state = self.update(fused_poses, ids, slots, joint_conf, meta, sequences)
        fitted, resid = self.fit(fused_poses, target, ids, joint_conf)
        return fitted, target, limb_state, resid

    def reset(self, seq=None):
        """Back to the initial state (nothing learned): every sequence, or one (a state row or a name)."""
        if seq is None:
            rows = slice(None)
        else:
            rows = self.seq_ids[seq] if not isinstance(seq, int) else seq
            if not 0 <= rows < self.nseq:
                raise capi.FvpError(f"sequence row {rows} outside [0, {self.nseq})")
        self.limb_len[rows] = 0.0
        self.limb_var[rows] = 0.0
        self.limb_cnt[rows] = 0
        self.limb_out[rows] = 0
        self.limb_id[rows] = -1

    def state(self):
        """Clones of the five state tensors (checkpointing, tests)."""
        return {k: getattr(self, k).clone() for k in self._STATE}

    def load_state(self, state):
        """The inverse of ``state()``."""
        for k in self._STATE:
            getattr(self, k).copy_(state[k])
