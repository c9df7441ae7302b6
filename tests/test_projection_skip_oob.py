"""The fused projection skips samples that cannot contribute: a (voxel, view) whose voxel lies outside the person's
window, or whose four bilinear taps all lie outside the image, issues no loads and no FMAs in k_project_triplane_own /
_blk (fvp_project_lds.h: a negative tap base, tap_contributes).  Skipping must not move a bit; this file builds inputs in
which the skip decides a large share of the samples, proves that on the CPU with the oracle BEFORE a kernel runs, and then
compares bit for bit.

Which samples can be skipped at all.  The sampling coordinate is clamped to +-1.1 (project_whole.py:59), i.e. to pixel
-0.05 (W - 1) .. 1.05 (W - 1): a heat map of fewer than 22 columns (rows) keeps one tap column (row) inside for EVERY
sample, so below 22 x 22 pixels no sample is ever wholly outside the image and only the window test can skip.  The 12 x 16
map of this file is that case (asserted: nothing wholly outside; it is exempt from the 10-60 % share, exercises the window
skip alone, and every in-window sample keeps its four loads with zero weights where taps are out), 22 x 30 and 24 x 32
are the sizes where the skip acts.  The resize transform has an offset (a crop): with the identity the pixel clamp at -1
(project_whole.py:51) would keep the left and top edges partly inside as well.

Rig: three cameras around a 4 x 4 x 2 m space.  Camera 0 stands close at mid height and looks at the centre: the near part
of the space leaves its image through all four edges, and the small window in the high corner is wholly outside it.
Camera 1 looks across from the side, camera 2 from high up: both see the centre whole and lose a corner.  V = 2 takes
cameras 0 and 1.  Persons per frame: 0 at the centre (wholly inside every image: nothing skipped), 1 in the high corner
with a margin (window clipped by the space and by the margin: voxels outside the window; wholly outside camera 0), 2 and
3 towards two other corners (clipped by the space, cut by image borders in two views each).  Frame 1 holds the same four
in reverse order with other heat maps.

Required content, asserted per case on the oracle's own sampling grid (_content): 10-60 % of the in-window (voxel, view)
samples have no tap inside; the out-of-image region is entered through each of the four image edges in some view; some
group of 16 voxels that share a sampling pass of a wave (one x, 4 y of a block, 4 consecutive z, counted from the window
start as the kernels do) is wholly out in some view and some group is mixed; a window is clipped by the space; one person
is wholly inside every image; one view skips every sample of one person.

Assertions (numpy.array_equal on the int32 view):
  fused planes (recomputed and cached coordinates) == fvp_project_individual -> fvp_triplane_max;
  those materialised planes against the oracle's project_individual -> triplane_max under the rule of the existing
  projection tests (tests/edge_cases.py: |difference| <= 2.5e-7, the oracle's restated bilinear sum is within 2 ulp of 1.0
  of the kernels' fma chain); both exactly zero in every plane cell outside the window;
  whole-space z-max and proposal columns == the materialised cubes;
  owned form == block form (FVP_TRI_OWNED=0, diagnostics build: the emulated library is one).
Heat maps: uniform in [-1, 1.5] with a fifth of the pixels exactly zero, so products of either sign and -0 occur."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import fvp_oracle as O
import projection_cases as P
from faster_voxelpose_amd import _capi as capi
from faster_voxelpose_amd.engine import _ptr

F32 = np.float32
SPACE_CENTER = [0.0, 0.0, 1000.0]
SPACE_SIZE = [4000.0, 4000.0, 2000.0]
IND_SIZE = [2000.0, 2000.0, 2000.0]
ORI_SIZE = [640, 480]
IMAGE_SIZE = [512, 384]
RT = np.array([[0.9, 0.0, -40.0], [0.0, 0.9, -30.0]], F32)             # original pixel -> network input: a crop

CAMS = [P._cam((3900.0, -300.0, 1050.0), (0.0, 100.0, 1000.0), 0.05, (540.0, 535.0), (330.0, 236.0)),
        P._cam((-600.0, 4300.0, 1900.0), (-800.0, 0.0, 1000.0), 0.3, (400.0, 395.0), (315.0, 238.0)),
        P._cam((-2500.0, -3600.0, 2600.0), (0.0, 100.0, 800.0), -0.08, (600.0, 605.0), (322.0, 244.0),
               k=(-0.05, 0.01, 0.0), p=(0.001, -0.0005))]

#         C   J   V  (H, W)
CASES = [(8, 15, 2, (24, 32)),
         (8, 17, 3, (22, 30)),
         (16, 15, 3, (24, 32)),
         (16, 17, 2, (24, 32)),
         (16, 15, 2, (12, 16)),       # below 22 x 22: no sample is wholly outside the image (see above)
         (64, 15, 2, (24, 32))]       # GPU only: the owned form at the segment count of the shipped shape rule (C / 4)
EMU_CASES = [c for c in CASES if c[0] <= 16]
IDS = lambda c: "C%d_J%d_V%d_%dx%d" % (c[0], c[1], c[2], c[3][0], c[3][1])

# person centres of a frame [x, y, z, -, -, bbox w, bbox h] (bbox 1.0: no margin; 0.7: a margin in x and y)
CENTERS = np.array([[0.0, 100.0, 1000.0, 0, 1, 1.0, 1.0],
                    [1750.0, 1800.0, 1350.0, 0, 1, 0.3, 0.3],
                    [1100.0, 1500.0, 700.0, 0, 1, 1.0, 0.7],
                    [1700.0, -1700.0, 1000.0, 0, 1, 0.7, 1.0]], F32)


def _cfg(Cn, J, V, hw):
    H, W = hw
    return types.SimpleNamespace(
        DATASET=types.SimpleNamespace(HEATMAP_SIZE=[W, H], ORI_IMAGE_SIZE=ORI_SIZE, IMAGE_SIZE=IMAGE_SIZE),
        CAPTURE_SPEC=types.SimpleNamespace(SPACE_CENTER=SPACE_CENTER, SPACE_SIZE=SPACE_SIZE),
        INDIVIDUAL_SPEC=types.SimpleNamespace(SPACE_SIZE=IND_SIZE, VOXELS_PER_AXIS=[Cn, Cn, Cn]))


def _geom(J, V, hw):
    H, W = hw
    g = capi.FvpGeom()
    g.clamp_max = float(max(ORI_SIZE))
    for i, v in enumerate(RT.reshape(-1)):
        g.rt[i] = float(v)
    g.hm_w, g.hm_h = float(W), float(H)
    g.img_w, g.img_h = float(IMAGE_SIZE[0]), float(IMAGE_SIZE[1])
    g.W, g.H, g.V, g.J, g.JP = W, H, V, J, (J + 3) // 4 * 4
    return g


def _cam_rows(V):
    rows = np.zeros((V, capi.FVP_CAM_FLOATS), F32)
    for v, cam in enumerate(CAMS[:V]):
        rows[v, 0:9] = np.asarray(cam["R"]).reshape(9)
        rows[v, 9:12] = np.asarray(cam["T"]).reshape(3)
        rows[v, 12:16] = [cam["fx"], cam["fy"], cam["cx"], cam["cy"]]
        rows[v, 16:19] = cam["k"]
        rows[v, 19:21] = cam["p"]
    return rows


def _heat(B, V, J, hw, seed):
    rs = np.random.RandomState(seed)
    h = rs.uniform(-1.0, 1.5, (B, V, J) + tuple(hw))
    h[rs.uniform(size=h.shape) < 0.2] = 0.0
    return h.astype(F32)


def _no_tap_inside(grid, W, H):
    """grid [..., 2] fp32 (torch) -> (out, left, right, top, bottom) bool: the four taps of a sample all lie outside the image
    (floor(ix) + 1 < 0, floor(ix) > W - 1, or the same in y), and through which edge.  Pixel coordinates as
    oracle.bilinear_mean forms them."""
    ix = (grid[..., 0] + 1) * ((W - 1) / 2)
    iy = (grid[..., 1] + 1) * ((H - 1) / 2)
    x0, y0 = torch.floor(ix), torch.floor(iy)
    left, right, top, bottom = x0 + 1 < 0, x0 > W - 1, y0 + 1 < 0, y0 > H - 1
    return left | right | top | bottom, left, right, top, bottom


# ---------------------------------------------------------------------------------------------------------------------
# the oracle's side of a case, computed once: boxes, sampling grids of the windows, content, reference planes

_REF = {}


def _reference(case):
    if case in _REF:
        return _REF[case]
    Cn, J, V, hw = case
    H, W = hw
    cfg, spec = _cfg(*case), None
    spec = O.IndividualSpec(cfg)
    cams = CAMS[:V]
    ppf = 4
    frames = 2
    heat = _heat(frames, V, J, hw, seed=1000 * Cn + 10 * J + V)
    cen = [torch.as_tensor(CENTERS[:ppf]), torch.as_tensor(CENTERS[:ppf][::-1].copy())]      # frame 1: the persons in reverse
    boxes, planes, stats = [], [], []
    for b in range(frames):
        cubes, _, (tl, s, e) = O.project_individual(spec, cfg, torch.as_tensor(heat[b]), cen[b], cams, RT)
        planes.append(O.triplane_max(cubes).view(3, ppf, J, Cn, Cn).permute(1, 0, 2, 3, 4))
        boxes.append(torch.cat([tl, s, e], dim=1))
        if b == 0:
            for i in range(ppf):
                grid = O.build_sample_grids(spec.fine_points(s[i], e[i]), cams, cfg, RT)
                d = (e[i] - s[i]).tolist()
                stats.append([c.view(V, d[0], d[1], d[2]) for c in _no_tap_inside(grid, W, H)])
    r = types.SimpleNamespace(case=case, cfg=cfg, spec=spec, ppf=ppf, frames=frames, heat=heat,
                              boxes=torch.cat(boxes).to(torch.int32).numpy(), planes=torch.cat(planes), stats=stats)
    _content(r)
    _REF[case] = r
    return r


def _content(r):
    """The inputs exercise the skip (frame 0; frame 1 holds the same windows): see the module docstring."""
    Cn, J, V, (H, W) = r.case
    out = [s[0] for s in r.stats]
    n_out, n_all = sum(int(o.sum()) for o in out), sum(o.numel() for o in out)
    share = n_out / n_all
    bx = r.boxes[:r.ppf]
    clipped = [i for i in range(r.ppf) if (bx[i, 3:6] > bx[i, 0:3]).any() or (bx[i, 6:9] < bx[i, 0:3] + Cn).any()]
    fine = np.asarray([int(v) for v in r.spec.fine])
    by_space = [i for i in range(r.ppf) if (bx[i, 0:3] < 0).any() or (bx[i, 0:3] + Cn > fine).any()]
    print(r.case, "no tap inside: %.3f of %d samples; per person and view:" % (share, n_all),
          [[round(float(o[v].float().mean()), 3) for v in range(V)] for o in out], "clipped by the space:", by_space)
    assert by_space and set(by_space) <= set(clipped), "fixture: no window clipped by the space bounds"
    if W < 22 and H < 22:
        assert n_out == 0, "a sample wholly outside a map below 22 x 22"
        return
    assert 0.10 <= share <= 0.60, share
    for k, name in enumerate(("left", "right", "top", "bottom")):
        assert any(bool(s[1 + k].any()) for s in r.stats), "fixture: no sample leaves through the %s edge" % name
    assert any(not bool(o.any()) for o in out), "fixture: no person wholly inside every image"
    assert any(bool(o[v].all()) for o in out for v in range(V)), "fixture: no view skips every sample of a person"
    whole, mixed = 0, 0
    for o in out:                                  # o [V][dx][dy][dz]: groups of 4 y x 4 z from the window start, one x
        _, dx, dy, dz = o.shape
        pad = torch.zeros(V, dx, (dy + 3) // 4 * 4, (dz + 3) // 4 * 4, dtype=torch.bool)
        live = pad.clone()
        pad[:, :, :dy, :dz], live[:, :, :dy, :dz] = o, True
        grp = lambda t: t.view(V, dx, pad.shape[2] // 4, 4, pad.shape[3] // 4, 4).permute(0, 1, 2, 4, 3, 5).reshape(V, dx, -1, 16)
        n_o, n_l = grp(pad).sum(-1), grp(live).sum(-1)
        whole += int(((n_o == n_l) & (n_l == 16)).sum())
        mixed += int(((n_o > 0) & (n_o < n_l)).sum())
    assert whole > 0 and mixed > 0, (whole, mixed)


# ---------------------------------------------------------------------------------------------------------------------
# the library's side


def _run_person(cx, case, monkeypatch, forms):
    """forms: (name, environment) pairs run after the shape rule's own form; every one on recomputed and cached coordinates."""
    r = _reference(case)
    Cn, J, V, hw = case
    g = _geom(J, V, hw)
    nP = r.boxes.shape[0]
    ax = [cx.up(a.numpy(), torch.float32) for a in r.spec.fine_axes]
    fine = [int(v) for v in r.spec.fine]
    hcl = P.stage(cx, r.heat, g)
    cams = cx.up(_cam_rows(V)[None])
    fs = cx.up(np.zeros(r.frames, np.int32))
    pf = cx.up((np.arange(nP) // r.ppf).astype(np.int32))
    valid = cx.up(np.ones(nP, np.uint8))
    boxes = cx.up(r.boxes)
    cubes = cx.full((nP, J, Cn, Cn, Cn), -5.0)
    cx.call("fvp_project_individual", _ptr(hcl), _ptr(cams), _ptr(fs), _ptr(pf), _ptr(valid), _ptr(boxes), _ptr(ax[0]),
            _ptr(ax[1]), _ptr(ax[2]), cx.p(np.asarray(fine, np.int32)), Cn, nP, C.byref(g), _ptr(cubes), cx.stream())
    want = cx.full((nP, 3, J, Cn, Cn), -5.0)
    cx.call("fvp_triplane_max", _ptr(cubes), _ptr(want), nP, J, Cn, cx.stream())
    want = want.cpu().numpy()
    del cubes
    # the materialised planes against the oracle's (frame-major, as the boxes)
    ref = r.planes.numpy()
    diff = np.abs(want - ref)
    print(case, "materialised planes vs oracle: max |difference| %.3g" % float(diff.max()))
    assert float(diff.max()) <= 2.5e-7, float(diff.max())
    assert float(want.max()) > 0.0
    inside = np.zeros((nP, 3, 1, Cn, Cn), bool)                                   # plane cells some window voxel projects to
    for p in range(nP):
        lo, hi = r.boxes[p, 3:6] - r.boxes[p, 0:3], r.boxes[p, 6:9] - r.boxes[p, 0:3]
        for k, (a, b) in enumerate(((0, 1), (0, 2), (1, 2))):                     # x-y, x-z, y-z
            inside[p, k, 0, lo[a]:hi[a], lo[b]:hi[b]] = True
    outside = np.broadcast_to(~inside, want.shape)
    assert outside.any() and (want[outside] == 0.0).all() and (ref[outside] == 0.0).all(), "a plane cell outside a window is not zero"
    fgrid = cx.up(torch.as_tensor(P.grid_of(cx, [a.numpy() for a in r.spec.fine_axes], _cam_rows(V), g))[None])
    fine_host = (C.c_int32 * 3)(*fine)

    def fused(cached):
        planes = torch.zeros((nP, 3, J, Cn, Cn), device=cx.dev)                  # the caller's zero fill
        cx.call("fvp_project_individual_triplane", _ptr(hcl), _ptr(cams), _ptr(fs), _ptr(pf), _ptr(valid), _ptr(boxes),
                _ptr(ax[0]), _ptr(ax[1]), _ptr(ax[2]), fine_host, Cn, nP, C.byref(g), _ptr(planes), r.ppf,
                _ptr(fgrid if cached else None), cx.stream())
        return planes.cpu().numpy()

    got = {}
    for name, env in [("shape rule", {})] + list(forms):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        for cached in (False, True):
            got[name, cached] = fused(cached)
            assert np.array_equal(got[name, cached].view(np.int32), want.view(np.int32)), \
                "%s, %s coordinates: %d plane cells differ from the materialised path" % (
                    name, "cached" if cached else "recomputed", int((got[name, cached] != want).sum()))
        for k in env:
            monkeypatch.delenv(k)
    for (name, cached), planes in got.items():                                      # owned form == block form (and the others)
        assert np.array_equal(planes.view(np.int32), got["shape rule", cached].view(np.int32)), name


SWITCHED = [("block form", {"FVP_TRI_OWNED": "0"}), ("two segments", {"FVP_TRI_NY": "2"})]
WHOLE = [((16, 16, 8), 15, 3, (24, 32)), ((13, 9, 8), 17, 2, (22, 30))]     # grid, J, V, (H, W): 256-voxel workgroups, full and ragged


def _run_whole(cx, grid, J, V, hw):
    """The whole-space kernels (k_project_whole_q, k_project_columns_q) skip a view with no tap inside too (they always did):
    cubes against the oracle, fused z-max and proposal columns against the cubes, on a grid the image borders cut."""
    H, W = hw
    cfg, g = _cfg(8, J, V, hw), _geom(J, V, hw)
    ax3 = [O.axis_coords(SPACE_SIZE[a], SPACE_CENTER[a], grid[a]) for a in range(3)]
    pts = O.compute_grid(SPACE_SIZE, SPACE_CENTER, grid)
    sgrid = O.build_sample_grids(pts, CAMS[:V], cfg, RT)
    out = _no_tap_inside(sgrid, W, H)[0]                                        # [V][n], z fastest
    share = float(out.float().mean())
    grp = out[:, :out.shape[1] // 16 * 16].view(V, -1, 16).sum(-1)              # 16 consecutive voxels: a wave of the kernel
    print(grid, hw, "no tap inside: %.3f" % share, "waves wholly out / mixed:", int((grp == 16).sum()), int(((grp > 0) & (grp < 16)).sum()))
    assert 0.10 <= share <= 0.60 and bool((grp == 16).any()) and bool(((grp > 0) & (grp < 16)).any()), share
    B = 2
    heat = _heat(B, V, J, hw, seed=77 + J)
    want = O.project_whole(torch.as_tensor(heat), [sgrid] * B, grid)
    hcl = P.stage(cx, heat, g)
    cams, fs = _cam_rows(V)[None], np.zeros(B, np.int32)
    ax3 = [a.numpy() for a in ax3]
    rc, cubes, zmax = P.project_whole(cx, g, ax3, hcl, cams, fs, B)
    assert rc == 0, rc
    assert float((cubes - want).abs().max()) <= 2.5e-7, float((cubes - want).abs().max())
    assert np.array_equal(zmax.numpy().view(np.int32), cubes.max(dim=4)[0].numpy().view(np.int32)), "z-max differs from the cubes"
    X, Y, Z = grid
    dead = torch.nonzero(out.view(V, X * Y, Z).all(dim=2).all(dim=0)).reshape(-1).tolist()   # columns no view sees, if any
    flat = np.array([[0, X * Y - 1, 5, X * Y // 2] + dead[:2] for b in range(B)], np.int64)
    N = flat.shape[1]
    feat = cx.full((B * N, J, Z), -5.0)
    dax = [cx.up(a, torch.float32) for a in ax3]
    cx.call("fvp_project_columns", _ptr(hcl), cx.p(cams), cx.p(fs), _ptr(dax[0]), _ptr(dax[1]), _ptr(dax[2]), X, Y, Z, B,
            C.byref(g), cx.p(flat), N, _ptr(feat), cx.stream())
    cols = cubes.view(B, J, X * Y, Z)[:, :, torch.as_tensor(flat[0])].permute(0, 2, 1, 3).contiguous()
    assert np.array_equal(feat.cpu().view(B, N, J, Z).numpy().view(np.int32), cols.numpy().view(np.int32)), "columns differ from the cubes"


# ---------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_inputs_exercise_the_skip(case):
    """The content assertions alone (CPU, oracle only), for every case including the GPU-only one."""
    _reference(case)


@pytest.mark.parametrize("case", EMU_CASES, ids=IDS)
def test_emulated_fused_planes_keep_their_bits(emu_lib, monkeypatch, case):
    _run_person(P.Ctx(emu_lib, "cpu"), case, monkeypatch, SWITCHED + ([("two quad groups", {"FVP_TRI_NO_Q5": "1"})] if case[1] == 17 else []))


@pytest.mark.parametrize("grid,J,V,hw", WHOLE, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_emulated_whole_space_and_columns(emu_lib, grid, J, V, hw):
    _run_whole(P.Ctx(emu_lib, "cpu"), grid, J, V, hw)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_gpu_fused_planes_keep_their_bits(case, monkeypatch):
    """The shipped library: the form and segment count of its own shape rule (C = 64: the owned form at ny = 16)."""
    _run_person(P.Ctx(capi.load(), "cuda:0"), case, monkeypatch, [])


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_gpu_owned_form_equals_the_block_form(diag_lib, monkeypatch, case):
    _run_person(P.Ctx(diag_lib, "cuda:0"), case, monkeypatch, SWITCHED + ([("two quad groups", {"FVP_TRI_NO_Q5": "1"})] if case[1] == 17 else []))


@pytest.mark.gpu
@pytest.mark.parametrize("grid,J,V,hw", WHOLE, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_gpu_whole_space_and_columns(grid, J, V, hw):
    _run_whole(P.Ctx(capi.load(), "cuda:0"), grid, J, V, hw)
