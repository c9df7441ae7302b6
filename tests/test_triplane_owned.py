"""The owned form of the fused tri-plane projection (k_project_triplane_own): x strips that keep their x-y maxima in
registers and their x-z cells in LDS, only y-z merged through global atomics.

Reference of every case: the materialised path, fvp_project_individual followed by fvp_triplane_max; the planes must be
bit-equal (torch.equal on the int32 view).  Both halves call the C ABI directly with hand-written person boxes
([tl, s, e] per person, the layout fvp_person_boxes writes), so that every window the new control flow can get wrong
occurs on miniature cubes:

  frame 0 (camera set A)                                   frame 1 (camera set B: shifted cameras)
  0  x extent C - 2 (no multiple of the strip), y extent    6, 7  two overlapping full windows
     C - 3 (no multiple of 4), z clipped low: C - 3 cells   8     interior window, 9 .. 12 y cells (3 y blocks)
  1  one x column (narrower than a strip)                   9     invalid person with a sane box
  2  clipped by the space on the low side (s > tl)          10    empty x window (s >= e)
  3  clipped on the high side (e = fine)                    11    18 y cells at C = 32 (5 y blocks), 15 at C = 16 (4 blocks)
  4  empty y window (s >= e), valid
  5  invalid person with a sane box

One more fixture repeats the twelve windows over eight frames (different heatmaps, alternating camera sets): a frame count
that is a multiple of 8 takes the kernels' XCD-major workgroup numbering.

The z ranges C - 3 (person 0), C - 5 (person 3) and 11 (person 8) are no multiples of the 16-cell z block.  The segment
count of a strip is forced through the diagnostics switch FVP_TRI_NY: 1 (plain stores of x-z), 2, 3 and 4 give uneven
segments (3 y blocks in 2 segments: 2 + 1; 5 blocks in 4: 2 + 2 + 1 + 0, an empty last segment; 4 blocks in 3: 2 + 2 + 0),
and the shape rule's own choice runs too.  FVP_TRI_OWNED=0 selects the block form the new one replaces.

The zero fill of `planes` is part of the contract (engine.jln fills it): cells outside a person's window [s, e) are written
by neither form, and the y-z plane is merged with atomicMax onto the zeros.  Every pass here starts from a zero-filled
tensor, as the engine does; a NaN pre-fill pass would not apply to this design."""
import ctypes as C
import copy

import numpy as np
import pytest
import torch

import fvp_synthetic as S
from faster_voxelpose_amd.engine import _ptr
from faster_voxelpose_amd.models import faster_voxelpose as FV

SHAPES = [(16, 15, 3), (16, 17, 5), (32, 17, 3), (32, 15, 5)]        # (C, J, V)
N = 6                                                                  # person slots per frame


def _boxes(Cn, fine):
    F0, F1, F2 = fine
    b = lambda tl, s, e: list(tl) + list(s) + list(e)
    full = lambda tl: b(tl, [max(v, 0) for v in tl], [min(v + Cn, f) for v, f in zip(tl, fine)])
    rows = [
        b((10, 20, -3), (11, 21, 0), (10 + Cn - 1, 20 + Cn - 2, Cn - 3)),
        b((14, 9, 0), (14 + Cn // 2, 10, 0), (14 + Cn // 2 + 1, 9 + Cn - 1, min(Cn, F2))),
        full((-5, -7, -3)),
        full((F0 - Cn + 6, F1 - Cn + 3, F2 - Cn + 5)),
        b((30, 12, 0), (31, 12 + Cn // 2 + 1, 0), (30 + Cn - 1, 12 + Cn // 2 - 1, min(Cn, F2))),
        full((22, 31, 0)),
        full((30, 30, 0)),
        full((33, 28, 0)),
        b((40, 40, 0), (41, 42, 2), (40 + Cn - 2, 42 + 10, 13)),
        full((50, 50, 0)),
        b((44, 18, 0), (44 + Cn // 2 + 2, 18, 0), (44 + Cn // 2 - 2, 18 + Cn, min(Cn, F2))),
        b((52, 3, 0), (53, 4, 0), (52 + Cn - 3, 3 + min(19, Cn), min(Cn, F2))),
    ]
    valid = [1, 1, 1, 1, 1, 0, 1, 1, 1, 0, 1, 1]
    return torch.tensor(rows, dtype=torch.int32), torch.tensor(valid, dtype=torch.uint8)


class Fixture:
    """One (C, J, V) shape on one library / device: inputs, the reference planes (computed once), the fused call."""

    def __init__(self, lib, dev, shape, frames=2):
        Cn, J, V = shape
        cfg = S.make_cfg("tiny", device=dev, cube=[Cn, Cn, Cn], max_people=N)
        cfg.DATASET.NUM_JOINTS, cfg.DATASET.CAMERA_NUM = J, V
        cams0, seq = S.load_cameras("tiny")
        base = cams0[seq]

        def cam_set(shift):                                  # cameras beyond the three of the fixture: shifted copies
            out = []
            for i in range(V):
                c = copy.deepcopy(base[i % len(base)])
                c["T"] = (np.asarray(c["T"], np.float64).reshape(3, 1)
                          + np.array([[37.0 * i + shift], [-21.0 * i - shift], [5.0 * i]])).tolist()
                out.append(c)
            return out
        cams = {"a": cam_set(0.0), "b": cam_set(240.0)}
        model = FV.FasterVoxelPoseNet(cfg, _lib=lib)
        if dev != "cpu":
            model = model.to(dev)
        e = self.e = model.engine
        self.Cn, self.J, self.V, self.dev = Cn, J, V, dev
        self.rt = S.resize_transform(cfg).to(dev)
        heat = S.heatmaps_uniform(cfg, frames, seed=11).to(dev)
        self.g = e.geom(self.rt)
        self.g.V = V
        self.fs = e.frame_sets({"seq": ["a", "b"] * (frames // 2)}, cams, V)
        self.hcl = e.heat_cl(heat, self.g).clone()
        self.pf = e.person_frame(frames, N)
        boxes, valid = _boxes(Cn, e.fine)
        assert bool((boxes[:, 3:6] >= boxes[:, 0:3]).all()) and bool((boxes[:, 6:9] <= boxes[:, 0:3] + Cn).all())
        assert bool((boxes[:, 6:9] <= torch.tensor(e.fine)).all()) and bool((boxes[:, 3:6] >= 0).all())
        boxes, valid = boxes.repeat(frames // 2, 1), valid.repeat(frames // 2)       # frames 2 k, 2 k + 1: the same twelve windows
        self.boxes, self.valid = boxes.to(dev), valid.to(dev)
        self.nP = boxes.shape[0]
        self.dead = [p for p in range(self.nP) if p % 12 in (4, 5, 9, 10)]
        self.fgrid = None
        # ---- the reference: materialised cubes, then the three maxima
        s = e.stream()
        fa = e.fine_axes
        cubes = torch.zeros((self.nP, J, Cn, Cn, Cn), device=dev)
        want = torch.zeros((self.nP, 3, J, Cn, Cn), device=dev)
        e._call("fvp_project_individual", _ptr(self.hcl), _ptr(e.geo.cams), _ptr(self.fs), _ptr(self.pf), _ptr(self.valid),
                _ptr(self.boxes), _ptr(fa[0]), _ptr(fa[1]), _ptr(fa[2]), _ptr(e.fine_dev), Cn, self.nP, C.byref(self.g),
                _ptr(cubes), s)
        e._call("fvp_triplane_max", _ptr(cubes), _ptr(want), self.nP, J, Cn, s)
        self.want = want.cpu()
        live = [p for p in range(self.nP) if p not in self.dead]
        assert all(float(self.want[p, k].max()) > 0 for p in live for k in range(3)), "fixture: a live window without signal"
        for p in self.dead:
            assert float(self.want[p].abs().max()) == 0.0

    def fused(self, cached):
        e = self.e
        if cached and self.fgrid is None:
            self.fgrid = e.fine_grid_cache(self.rt, self.V)
            assert self.fgrid is not None
        planes = torch.zeros((self.nP, 3, self.J, self.Cn, self.Cn), device=self.dev)    # the engine's zero fill
        fa = e.fine_axes
        e._call("fvp_project_individual_triplane", _ptr(self.hcl), _ptr(e.geo.cams), _ptr(self.fs), _ptr(self.pf),
                _ptr(self.valid), _ptr(self.boxes), _ptr(fa[0]), _ptr(fa[1]), _ptr(fa[2]), e.fine_host, self.Cn, self.nP,
                C.byref(self.g), _ptr(planes), N, _ptr(self.fgrid if cached else None), e.stream())
        return planes.cpu()

    def check(self, got, what):
        for p in self.dead:                                  # empty windows and invalid persons: untouched zeros
            assert float(got[p].abs().max()) == 0.0, (what, p)
        for p in range(self.nP):
            for k, name in enumerate(("xy", "xz", "yz")):
                assert torch.equal(got[p, k].view(torch.int32), self.want[p, k].view(torch.int32)), (what, p, name)


_FIX = {}


def _fixture(lib, dev, shape):
    key = (dev, shape)
    if key not in _FIX:
        _FIX[key] = Fixture(lib, dev, shape)
    return _FIX[key]


def _switches(fx, cached, monkeypatch, ny_list):
    """Every form on one fixture: the shape rule's own segment count, forced counts, the block form, the two-group form."""
    fx.check(fx.fused(cached), "owned, ny by the shape rule")
    for ny in ny_list:
        monkeypatch.setenv("FVP_TRI_NY", str(ny))
        fx.check(fx.fused(cached), "owned, ny = %d" % ny)
    monkeypatch.delenv("FVP_TRI_NY")
    if fx.J == 17:                                           # JP = 20: the two-group form instead of the five-quad form
        monkeypatch.setenv("FVP_TRI_NO_Q5", "1")
        monkeypatch.setenv("FVP_TRI_NY", "2")
        fx.check(fx.fused(cached), "owned, two quad groups, ny = 2")
        monkeypatch.delenv("FVP_TRI_NO_Q5")
        monkeypatch.delenv("FVP_TRI_NY")
    monkeypatch.setenv("FVP_TRI_OWNED", "0")
    fx.check(fx.fused(cached), "block form")
    monkeypatch.delenv("FVP_TRI_OWNED")


@pytest.mark.parametrize("cached", [False, True], ids=["recomputed", "cached"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "C%d_J%d_V%d" % s)
def test_emulated_owned_form_is_bit_equal_to_the_materialised_path(emu_lib, monkeypatch, shape, cached):
    fx = _fixture(emu_lib, "cpu", shape)
    _switches(fx, cached, monkeypatch, [1, 2, 3, 4] if shape[0] == 16 else [1, 4])


def _eight_frames(lib, dev, monkeypatch):
    """Eight frames of six persons: with a frame count that is a multiple of 8 the kernels number their workgroups
    frame-major per XCD (id & 7 = frame mod 8) - the other index decode.  Different heatmaps per frame, the two camera
    sets alternating; the shape rule's segment count, a forced uneven one, and the block form."""
    fx = Fixture(lib, dev, SHAPES[0], frames=8)
    assert fx.nP == 48 and fx.nP // N == 8
    for cached in (False, True):
        fx.check(fx.fused(cached), "8 frames, ny by the shape rule")
        monkeypatch.setenv("FVP_TRI_NY", "3")
        fx.check(fx.fused(cached), "8 frames, ny = 3")
        monkeypatch.delenv("FVP_TRI_NY")
    monkeypatch.setenv("FVP_TRI_OWNED", "0")
    fx.check(fx.fused(True), "8 frames, block form")


def test_emulated_eight_frames_take_the_xcd_major_index_decode(emu_lib, monkeypatch):
    _eight_frames(emu_lib, "cpu", monkeypatch)


@pytest.mark.gpu
def test_gpu_eight_frames_take_the_xcd_major_index_decode(diag_lib, monkeypatch):
    _eight_frames(diag_lib, "cuda:0", monkeypatch)


def test_emulated_launches_the_owned_kernel(emu_lib, monkeypatch):
    """The emulator's launch log names the kernel: the owned form by default, the block form under FVP_TRI_OWNED=0."""
    fx = _fixture(emu_lib, "cpu", SHAPES[0])
    emu_lib.hipemu_launch_log.restype = C.c_char_p

    def log_of(cached):
        emu_lib.hipemu_launch_log_reset()
        fx.fused(cached)
        return emu_lib.hipemu_launch_log().decode()
    for cached in (False, True):
        log = log_of(cached)
        assert "k_project_triplane_own" in log and "k_project_triplane_blk" not in log, log
    monkeypatch.setenv("FVP_TRI_OWNED", "0")
    log = log_of(False)
    assert "k_project_triplane_blk" in log and "k_project_triplane_own" not in log, log


@pytest.mark.gpu
@pytest.mark.parametrize("cached", [False, True], ids=["recomputed", "cached"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "C%d_J%d_V%d" % s)
def test_gpu_owned_form_is_bit_equal_to_the_materialised_path(diag_lib, monkeypatch, shape, cached):
    fx = _fixture(diag_lib, "cuda:0", shape)
    _switches(fx, cached, monkeypatch, [1, 2, 3, 4])


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "C%d_J%d_V%d" % s)
def test_gpu_shipped_library_is_bit_equal_to_the_materialised_path(shape):
    """The shipped library reads no switch: its own choice of form and segment count, cached and recomputed coordinates."""
    from faster_voxelpose_amd import _capi as capi
    fx = Fixture(capi.load(), "cuda:0", shape)
    fx.check(fx.fused(False), "shipped, recomputed")
    fx.check(fx.fused(True), "shipped, cached")
