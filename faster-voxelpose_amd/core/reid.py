"""Old identities back after a gap: ``PersonReId`` owns the device-side state of ``fvp_track_reid`` and issues
``fvp_person_signature`` + ``fvp_track_reid`` (include/fvp.h, ABI 20), one launch each, on the caller's current HIP stream.

``PoseTracker`` forgets a track after ``max_age`` frames: a person who leaves the capture volume, stays hidden for longer or
re-appears further than ``gate_mm`` from where they vanished comes back under a new track id.  ``signature`` reads a colour
signature per person and body part from the camera frames under the person's limbs (the pixels of ``joint_evidence``, the
occluder table of ``JointVisibility``); ``update`` keeps the signatures of retired tracks in a gallery per sequence and gives
every track a PERSON id - the track id of the first track that person ever had - that a returning person gets back
``min_frames`` frames after they re-appear.  All of it is defined bit for bit in include/fvp.h.

The object is used BEHIND the forward on the same stream; it is not a stage of the forward (INTEGRATION.md has the recipe for
the plain forward, a captured graph and the pipeline's consumer stream).  Not built: NV12 surfaces, learned embeddings,
re-identification across sequences, feeding the person ids back into the tracker's association.

No arithmetic happens here and nothing synchronises with the host: PyTorch is used for device memory and streams only.
"""
import ctypes as C

import torch

from .. import _capi as capi
from .._args import (SequenceRows, device_matches, frame_rows, load_lib, require_gpu, stream_ptr, tensor_arg)
from .._args import ptr as _ptr
from ..dataset.images import Nv12Frames

MAX_PEOPLE, MAX_LIMBS, MAX_SAMPLES = 32, 64, 32          # the limits of fvp_person_signature
# joints of the legs (hips, knees, ankles) in the two joint sets with a default part table: a limb between two of them is
# part 1, every other limb is part 0
_LEG_JOINTS = {15: (2, 6, 7, 8, 12, 13, 14), 17: (11, 12, 13, 14, 15, 16)}


class PersonReId:
    """``PersonReId(cfg_or_N_J, nseq=1, max_tracks=None, gallery=32, limbs=None, limb_part=None, parts=2, samples=8,
    max_age=15, min_samples=32, min_frames=5, window=64, sim_min=0.7, margin=0.1, gallery_max_age=0, conf_min=0.0,
    device=None)``

    ``cfg_or_N_J``       a config (``CAPTURE_SPEC.MAX_PEOPLE``, ``DATASET.NUM_JOINTS``, ``DEVICE``) or the pair ``(N, J)``;
    ``nseq``             camera sequences side by side, numbered as ``PoseTracker`` numbers them;
    ``max_tracks``       track slots per sequence, the tracker's T (default 2 N);
    ``gallery``          retired tracks remembered per sequence, 1 .. ``FVP_REID_MAX_GALLERY``; a full gallery loses its oldest;
    ``limbs``            joint index pairs [L,2] the samples lie on; default: the table of ``utils.vis`` for J in {14, 15, 17};
    ``limb_part``        the body part in [0, parts) of every limb; default for J in {15, 17}: legs 1, the rest 0;
    ``parts``            body parts of a signature, 1 .. ``FVP_SIG_MAX_PARTS``;
    ``samples``          pixels sampled per limb and view, 1 .. 32;
    ``max_age``          the tracker's own: a track unseen for more than max_age frames is retired into the gallery;
    ``min_samples``      a frame adds to a track's signature when it holds at least that many samples of the person;
    ``min_frames``       frames a track accumulates before its identity is decided (and before it is worth remembering);
    ``window``           frames after which the accumulated signature is halved, ``min_frames`` .. ``FVP_REID_MAX_WINDOW``;
    ``sim_min``          a gallery entry is adopted when its histogram intersection with the track is at least this ...
    ``margin``           ... and ahead of the second-best entry by at least this;
    ``gallery_max_age``  a gallery entry older than that many frames is forgotten; 0 = never;
    ``conf_min``         with ``joint_conf`` given, a joint below it is not sampled.
    The defaults are guesses, not tuned values: nothing was measured on real footage.

    State (device tensors, one row per sequence): ``slot_sig [nseq,T,P,64]``, ``slot_tid``, ``slot_pid``, ``slot_frames``,
    ``slot_age`` ``[nseq,T]`` int32, ``slot_sim [nseq,T]`` fp32, ``gal_sig [nseq,G,P,64]``, ``gal_pid``, ``gal_age``
    ``[nseq,G]`` int32."""

    _STATE = ("slot_sig", "slot_tid", "slot_pid", "slot_frames", "slot_age", "slot_sim", "gal_sig", "gal_pid", "gal_age")
    _INIT = dict(slot_tid=-1, slot_pid=-1, slot_sim=-1.0, gal_pid=-1)

    def __init__(self, cfg_or_N_J, nseq=1, max_tracks=None, gallery=32, limbs=None, limb_part=None, parts=2, samples=8,
                 max_age=15, min_samples=32, min_frames=5, window=64, sim_min=0.7, margin=0.1, gallery_max_age=0,
                 conf_min=0.0, device=None, _lib=None):
        self.lib, self._injected = load_lib(_lib)
        if isinstance(cfg_or_N_J, (tuple, list)):
            N, J = cfg_or_N_J
        else:
            N, J = cfg_or_N_J.CAPTURE_SPEC.MAX_PEOPLE, cfg_or_N_J.DATASET.NUM_JOINTS
            device = cfg_or_N_J.DEVICE if device is None else device
        self.N, self.J, self.nseq = int(N), int(J), int(nseq)
        self.T = 2 * self.N if max_tracks is None else int(max_tracks)
        self.G, self.P, self.K = int(gallery), int(parts), int(samples)
        self.max_age, self.min_samples, self.min_frames = int(max_age), int(min_samples), int(min_frames)
        self.window, self.gallery_max_age = int(window), int(gallery_max_age)
        self.sim_min, self.margin, self.conf_min = float(sim_min), float(margin), float(conf_min)
        self.device = torch.device("cuda" if device is None else device)
        require_gpu("the re-identification", self.device, self._injected)
        if self.N < 1 or self.J < 1 or self.nseq < 1 or self.T < self.N or self.max_age < 0 or self.G < 1 or self.P < 1:
            raise capi.FvpError(f"PersonReId needs N, J, nseq, gallery, parts >= 1, max_tracks >= N and max_age >= 0 (N = "
                                f"{self.N}, J = {self.J}, nseq = {self.nseq}, gallery = {self.G}, parts = {self.P}, "
                                f"max_tracks = {self.T}, max_age = {self.max_age})")
        if self.N > capi.FVP_TRACK_MAX_DETS or self.T > capi.FVP_TRACK_MAX_TRACKS or self.J > capi.FVP_MAX_JOINTS \
                or self.G > capi.FVP_REID_MAX_GALLERY or self.P > capi.FVP_SIG_MAX_PARTS:
            raise capi.FvpError(f"PersonReId limits: N <= {capi.FVP_TRACK_MAX_DETS}, max_tracks <= "
                                f"{capi.FVP_TRACK_MAX_TRACKS}, J <= {capi.FVP_MAX_JOINTS}, gallery <= "
                                f"{capi.FVP_REID_MAX_GALLERY}, parts <= {capi.FVP_SIG_MAX_PARTS} (N = {self.N}, max_tracks = "
                                f"{self.T}, J = {self.J}, gallery = {self.G}, parts = {self.P})")
        # (written so that a NaN fails, as in the library)
        if not (1 <= self.K <= MAX_SAMPLES and self.min_samples >= 0 and self.min_frames >= 1
                and self.min_frames <= self.window <= capi.FVP_REID_MAX_WINDOW and self.gallery_max_age >= 0
                and self.sim_min == self.sim_min and self.margin == self.margin and self.conf_min == self.conf_min):
            raise capi.FvpError(f"PersonReId needs 1 <= samples <= {MAX_SAMPLES}, min_samples >= 0, 1 <= min_frames <= window <= "
                                f"{capi.FVP_REID_MAX_WINDOW}, gallery_max_age >= 0 and sim_min, margin, conf_min that are not "
                                f"NaN (samples = {samples}, min_samples = {min_samples}, min_frames = {min_frames}, window = "
                                f"{window}, gallery_max_age = {gallery_max_age}, sim_min = {sim_min}, margin = {margin}, "
                                f"conf_min = {conf_min})")
        if limbs is None:
            from ..utils.vis import _LIMBS               # (imports matplotlib: only for the default table)
            if self.J not in _LIMBS:
                raise capi.FvpError(f"no default skeleton for {self.J} joints (known: {sorted(_LIMBS)}): pass limbs")
            limbs = _LIMBS[self.J]
        self.limbs = [(int(a), int(b)) for a, b in limbs]
        if not 1 <= len(self.limbs) <= MAX_LIMBS or any(not (0 <= j < self.J) for ab in self.limbs for j in ab):
            raise capi.FvpError(f"limbs: 1 to {MAX_LIMBS} pairs of joint indices in [0, {self.J})")
        if limb_part is None:
            if self.P == 1:
                limb_part = [0] * len(self.limbs)
            elif self.J in _LEG_JOINTS:
                legs = _LEG_JOINTS[self.J]
                limb_part = [1 if a in legs and b in legs else 0 for a, b in self.limbs]
            else:
                raise capi.FvpError(f"no default body parts for {self.J} joints (known: {sorted(_LEG_JOINTS)}): pass limb_part")
        self.limb_part = [int(p) for p in limb_part]
        if len(self.limb_part) != len(self.limbs) or any(not (0 <= p < self.P) for p in self.limb_part):
            raise capi.FvpError(f"limb_part: one part in [0, {self.P}) per limb ({len(self.limbs)} limbs), got {limb_part}")
        L = len(self.limbs)
        self._limbs = (C.c_int32 * (2 * L))(*[j for ab in self.limbs for j in ab])
        self._parts = (C.c_int32 * L)(*self.limb_part)
        dev, bins = self.device, capi.FVP_SIG_BINS
        i32 = dict(dtype=torch.int32, device=dev)
        self.slot_sig = torch.zeros((self.nseq, self.T, self.P, bins), **i32)
        self.slot_tid = torch.full((self.nseq, self.T), -1, **i32)
        self.slot_pid = torch.full((self.nseq, self.T), -1, **i32)
        self.slot_frames = torch.zeros((self.nseq, self.T), **i32)
        self.slot_age = torch.zeros((self.nseq, self.T), **i32)
        self.slot_sim = torch.full((self.nseq, self.T), -1.0, device=dev)
        self.gal_sig = torch.zeros((self.nseq, self.G, self.P, bins), **i32)
        self.gal_pid = torch.full((self.nseq, self.G), -1, **i32)
        self.gal_age = torch.zeros((self.nseq, self.G), **i32)
        self._rows = SequenceRows(limit=self.nseq)
        self.seq_ids = self._rows.ids                  # sequence name -> row of the state, in order of first appearance

    # ---------------------------------------------------------------------------------------------
    def frame_sets(self, seqs):
        """[B] int32 device tensor of state rows for a list of sequence names (uploaded once per distinct list)."""
        return self._rows.rows(seqs, self.device)

    def signature(self, frames, views, ids=None, joint_conf=None, occluder=None):
        """``frames`` uint8 ``[B,V,Hs,Ws,3]`` (the camera frames the forward was fed, before any overlay paints them) and
        ``views [B,V,N,J,4]`` (``last_evidence[0]``) -> ``(sig [B,N,P,64] int32, sig_count [B,N,P] int32)``: per person and
        body part, the 2-bit-per-channel colour histogram of the pixels under the person's limbs over all views, and its
        sum.  ``ids [B,N]`` int32 (``last_tracks[0]``): slots with a negative id get zeros; ``joint_conf [B,N,J]``: joints
        below ``conf_min`` are not sampled; ``occluder [B,V,N,J]`` int32 (``last_visibility[0]``): a joint is sampled only in
        the views that see it.  One launch on the current stream."""
        if isinstance(frames, Nv12Frames):
            raise capi.FvpError("PersonReId.signature: NV12 is not built; pass uint8 RGB frames [B,V,Hs,Ws,3]")
        f = tensor_arg("frames", frames, torch.uint8, ("B", "V", "Hs", "Ws", 3), hint="HWC camera frames")
        if not device_matches(f.device, self.device):
            raise capi.FvpError(f"frames live on {f.device}, the re-identification was built for {self.device}")
        B, V, Hs, Ws = f.shape[:4]
        v = tensor_arg("views", views, torch.float32, (B, V, self.N, self.J, 4), f.device, hint="what joint_evidence returns")
        if V > capi.FVP_MAX_VIEWS or self.N > MAX_PEOPLE or min(Hs, Ws) < 1:
            raise capi.FvpError(f"PersonReId.signature limits: N <= {MAX_PEOPLE}, V <= {capi.FVP_MAX_VIEWS}, Hs, Ws >= 1 (N = "
                                f"{self.N}, V = {V}, Hs = {Hs}, Ws = {Ws})")
        tensor_arg("ids", ids, torch.int32, (B, self.N), f.device, hint="what PoseTracker.update returns", optional=True)
        c = tensor_arg("joint_conf", joint_conf, torch.float32, (B, self.N, self.J), f.device, optional=True)
        o = tensor_arg("occluder", occluder, torch.int32, (B, V, self.N, self.J), f.device,
                       hint="what JointVisibility returns first", optional=True)
        alloc = torch.zeros if B * V == 0 else torch.empty       # no view: no launch, no sample
        sig = alloc((B, self.N, self.P, capi.FVP_SIG_BINS), dtype=torch.int32, device=f.device)
        count = alloc((B, self.N, self.P), dtype=torch.int32, device=f.device)
        if B * V == 0:
            return sig, count
        rc = self.lib.fvp_person_signature(_ptr(f), B, V, Hs, Ws, _ptr(v), _ptr(ids), _ptr(c), _ptr(o), self.N, self.J,
                                           self._limbs, self._parts, len(self.limbs), self.P, self.K, self.conf_min,
                                           _ptr(sig), _ptr(count), stream_ptr(f.device))
        capi.check(self.lib, rc, "fvp_person_signature")
        return sig, count

    def update(self, ids, slots, sig, sig_count, meta=None, sequences=None):
        """``ids [B,N]`` and ``slots [B,N]`` as ``PoseTracker.update`` returned them for this batch, ``sig`` and ``sig_count``
        as ``signature`` returned them, frames in time order -> ``(pids [B,N] int32, reid_state [B,N] int32, reid_sim [B,N]
        float32)``: the person id of every valid slot (the track id while the track is pending), 0 pending / 1 a new
        person / 2 re-identified, and the similarity to the best gallery entry at the track's decision (-1 before it and
        when the gallery was empty); -1, -1, -1 for an invalid slot.  One launch on the current stream, no host
        synchronisation.  ``sequences`` / ``meta`` as for ``PoseTracker.update``."""
        t = tensor_arg("ids", ids, torch.int32, ("B", self.N), hint="what PoseTracker.update returned for this batch")
        if not device_matches(t.device, self.device):
            raise capi.FvpError(f"ids live on {t.device}, the re-identification was built for {self.device}")
        B = t.shape[0]
        tensor_arg("slots", slots, torch.int32, (B, self.N), t.device, hint="what PoseTracker.update returned for this batch")
        tensor_arg("sig", sig, torch.int32, (B, self.N, self.P, capi.FVP_SIG_BINS), t.device, hint="what signature() returns")
        tensor_arg("sig_count", sig_count, torch.int32, (B, self.N, self.P), t.device, hint="what signature() returns")
        fs = frame_rows(self.frame_sets, sequences, meta, B, t.device)
        pids = torch.empty((B, self.N), dtype=torch.int32, device=self.device)
        state = torch.empty((B, self.N), dtype=torch.int32, device=self.device)
        sim = torch.empty((B, self.N), device=self.device)
        if B == 0:
            return pids, state, sim
        rc = self.lib.fvp_track_reid(_ptr(t), _ptr(slots), _ptr(sig), _ptr(sig_count), _ptr(fs), _ptr(self.slot_sig),
                                     _ptr(self.slot_tid), _ptr(self.slot_pid), _ptr(self.slot_frames), _ptr(self.slot_age),
                                     _ptr(self.slot_sim), _ptr(self.gal_sig), _ptr(self.gal_pid), _ptr(self.gal_age),
                                     _ptr(pids), _ptr(state), _ptr(sim), B, self.N, self.nseq, self.T, self.G, self.P,
                                     self.max_age, self.min_samples, self.min_frames, self.window, self.sim_min, self.margin,
                                     self.gallery_max_age, stream_ptr(self.device))
        capi.check(self.lib, rc, "fvp_track_reid")
        return pids, state, sim

    def __call__(self, frames, views, ids, slots, joint_conf=None, occluder=None, meta=None, sequences=None):
        """``signature`` then ``update``: returns ``(pids, reid_state, reid_sim)``."""
        sig, count = self.signature(frames, views, ids=ids, joint_conf=joint_conf, occluder=occluder)
        return self.update(ids, slots, sig, count, meta=meta, sequences=sequences)

    def reset(self, seq=None):
        """Back to the initial state (no tracks, an empty gallery): every sequence, or one (a state row or a name)."""
        if seq is None:
            rows = slice(None)
        else:
            rows = self.seq_ids[seq] if not isinstance(seq, int) else seq
            if not 0 <= rows < self.nseq:
                raise capi.FvpError(f"sequence row {rows} outside [0, {self.nseq})")
        for k in self._STATE:
            getattr(self, k)[rows] = self._INIT.get(k, 0)

    def state(self):
        """Clones of the nine state tensors (checkpointing, tests)."""
        return {k: getattr(self, k).clone() for k in self._STATE}

    def load_state(self, state):
        """The inverse of ``state()``."""
        for k in self._STATE:
            getattr(self, k).copy_(state[k])
