"""What every stream-side wrapper (tracker, smoother, limb model, overlay, crops, visibility, triangulation, re-fit, ingest) does
before it launches: the library seam, the "GPU only" refusal, the tensor checks, pointers and the stream handle for the C ABI, and
the upload-once tables that turn sequence names and camera dicts into device tensors.  No arithmetic on tensors happens here
and nothing synchronises with the host."""
import ctypes as C

import numpy as np
import torch

from . import _capi as capi


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def stream_ptr(device):
    """The caller's current HIP stream on ``device`` (None on the CPU: the emulated library takes no stream)."""
    if device.type == "cuda":
        return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
    return None


def f3(v):
    v = [float(x) for x in v]
    assert len(v) == 3
    return (C.c_float * 3)(*v)


def load_lib(_lib):
    """``(lib, injected)``: ``_lib`` is a test seam (tests/hipemu); the product always loads libfvp_hip.so."""
    return (capi.load(), False) if _lib is None else (_lib, True)


def require_gpu(what, device, injected):
    if not injected and device.type != "cuda":
        raise capi.FvpError(f"{what} runs on a ROCm GPU device (spelled 'cuda:N' in PyTorch-ROCm), not on {device}; there "
                            "is no CPU fallback")


def device_matches(t_device, built_device):
    """``cuda`` without an index stands for any ``cuda:N``."""
    return t_device == built_device or (built_device.index is None and t_device.type == built_device.type)


def tensor_arg(name, t, dtype, shape, device=None, hint=None, optional=False):
    """``t`` if it is a contiguous ``dtype`` tensor of ``shape`` (on ``device``, when given), else an ``FvpError`` that says
    what was expected and what arrived.  In ``shape`` an int is a fixed extent; None or a name ("B") matches any."""
    if t is None and optional:
        return None
    if not torch.is_tensor(t) or t.dtype != dtype or t.dim() != len(shape) or not t.is_contiguous() \
            or (device is not None and t.device != device) \
            or any(isinstance(n, int) and n != m for n, m in zip(shape, t.shape)):
        want = ",".join("*" if n is None else str(n) for n in shape)
        got = f"{t.dtype} {tuple(t.shape)} on {t.device}" if torch.is_tensor(t) else type(t).__name__
        raise capi.FvpError(f"{name} must be a contiguous {dtype} tensor [{want}]" + (f" on {device}" if device is not None else "")
                            + (f" ({hint})" if hint else "") + f", got {got}")
    return t


# ---- sequence rows and camera tables -----------------------------------------------------------------------------------
class SequenceRows:
    """Sequence name -> row, numbered in order of first appearance (the rule of ``HotPath.frame_sets``, so an object fed
    the ``meta['seq']`` lists the engine is fed numbers the sequences as the engine does), and the int32 device tensor of
    rows of every distinct list of names, uploaded once."""

    def __init__(self, limit=None):
        self.ids, self.limit, self._cache = {}, limit, {}

    def rows(self, seqs, device):
        seqs = tuple(seqs)
        for s in seqs:
            if s not in self.ids:
                if self.limit is not None and len(self.ids) >= self.limit:
                    raise capi.FvpError(f"sequence {s!r} is one more than the nseq = {self.limit} this state was built for "
                                        f"(known: {list(self.ids)})")
                self.ids[s] = len(self.ids)
        if seqs not in self._cache:
            if len(self._cache) >= 256:                 # bounded, as in the engine: a long run over many sequence mixes
                self._cache.pop(next(iter(self._cache)))
            self._cache[seqs] = torch.tensor([self.ids[s] for s in seqs], dtype=torch.int32, device=device)
        return self._cache[seqs]


class CameraTables(SequenceRows):
    """``SequenceRows`` with the camera records of every sequence, ``cams [nsets,V,24]``, uploaded when it is first seen."""

    def __init__(self):
        super().__init__()
        self.cams = None

    def tables(self, cameras, seqs, V, device):
        """Camera dicts and sequence names -> ``(cams [nsets,V,24], frame_set [B])``."""
        from .engine import HotPath
        for s in dict.fromkeys(seqs):
            if s not in self.ids:
                if s not in cameras or len(cameras[s]) != V:
                    raise capi.FvpError(f"cameras holds no {V} cameras for sequence {s!r}")
                rows = np.stack([HotPath._cam_row(cameras[s][c]) for c in range(V)])
                t = torch.from_numpy(rows).to(device)[None]
                self.cams = t if self.cams is None else torch.cat([self.cams, t], dim=0)
                self.ids[s] = self.cams.shape[0] - 1
                self._cache.clear()                     # (kept from the first version: a new sequence drops the cached row tensors)
        return self.cams, self.rows(seqs, device)


def resolve_cameras(tables, cameras_or_cams, frame_set_or_meta, B, V, device):
    """The camera arguments of visibility and triangulation -> ``(cams, frame_set, V)``: a float32 tensor ``[nsets,V,24]``
    with an int32 tensor ``[B]`` of set rows, or the forward's ``cameras`` dict with its ``meta`` (or a list of B sequence
    names), resolved through ``tables``.  ``V``: the view count the caller already knows, or None."""
    if torch.is_tensor(cameras_or_cams):
        cams = tensor_arg("cams", cameras_or_cams, torch.float32, ("nsets", V or "V", capi.FVP_CAM_FLOATS), device)
        if cams.shape[0] < 1:
            raise capi.FvpError("cams holds no camera set")
        fs = tensor_arg("frame_set", frame_set_or_meta, torch.int32, (B,), device,
                        hint="with a cams tensor, the camera set row of every frame")
        return cams, fs, cams.shape[1]
    seqs = frame_set_or_meta["seq"] if isinstance(frame_set_or_meta, dict) else frame_set_or_meta
    if len(seqs) != B:
        raise capi.FvpError(f"{len(seqs)} sequence names for {B} frames")
    if V is None:
        V = len(cameras_or_cams[seqs[0]]) if B else 1
    cams, fs = tables.tables(cameras_or_cams, seqs, V, device)
    return cams, fs, V


def frame_rows(frame_sets, sequences, meta, B, device):
    """The ``sequences`` / ``meta`` arguments of tracker and smoother -> an int32 tensor ``[B]`` of state rows (a tensor as
    given, names through ``frame_sets``), or None: row 0 for every frame."""
    if sequences is None and meta is not None:
        sequences = meta["seq"]
    if sequences is None:
        return None
    if torch.is_tensor(sequences):
        return tensor_arg("sequences", sequences, torch.int32, (B,), device)
    if len(sequences) != B:
        raise capi.FvpError(f"{len(sequences)} sequence names for {B} frames")
    return frame_sets(sequences)
