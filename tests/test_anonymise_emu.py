"""fvp_anonymise_rois and fvp_anonymise_rois_nv12 on the CPU emulation of the kernels (tests/hipemu): every case of
tests/anonymise_cases.py against the independent numpy restatement of include/fvp.h, whole allocations byte for byte; the
read fence (exactly the touched cells are loaded; FILL and an all-inactive list load nothing; padding, gaps, guards and other
frames are never touched); ROI order; the privacy property; the case set against seven mutated yardsticks; every argument
error; FaceAnonymiser; and one forward -> anonymise -> overlay run."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import anonymise_cases as AC
import fvp_synthetic as FS
from faster_voxelpose_amd import _capi as capi
from faster_voxelpose_amd.models import faster_voxelpose as FV
from faster_voxelpose_amd.utils.anonymise import _HEAD_JOINTS, FaceAnonymiser
from faster_voxelpose_amd.utils.overlay import PoseOverlay

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY_LIMBS = [(0, 1), (1, 2), (2, 3), (3, 4)]            # the tiny configuration has 5 joints: no default skeleton


def test_header_and_binding_hold_the_two_exports(emu_lib):
    assert capi.ABI_VERSION >= 23 and emu_lib.fvp_version() == capi.ABI_VERSION
    header = open(os.path.join(ROOT, "include", "fvp.h")).read()
    assert f"#define FVP_ABI_VERSION {capi.ABI_VERSION}" in header
    for name in ("fvp_anonymise_rois", "fvp_anonymise_rois_nv12"):
        assert name in capi.SIGNATURES and hasattr(emu_lib, name) and f"int {name}(" in header
    for name, value in (("RECT", AC.RECT), ("ELLIPSE", AC.ELLIPSE), ("MOSAIC", AC.MOSAIC), ("FILL", AC.FILL)):
        assert f"#define FVP_ANON_{name} {value}" in header and getattr(capi, "ANON_" + name) == value
    for std, row in AC.RGB2YUV.items():                                          # the yardstick's table is the header's
        name = ("BT601_LIMITED", "BT709_LIMITED", "BT601_FULL", "BT709_FULL")[std]
        assert f"#define FVP_RGB2YUV_{name}_COEFFS {{ " + ", ".join(str(v) for v in row) + " }" in header


@pytest.mark.parametrize("name", AC.CASES)
def test_frames_equal_the_yardstick(emu_lib, name):
    AC.check(emu_lib, "cpu", name)


def test_cases_hold_what_their_names_say():
    hs, ws = 38, 70
    assert hs % AC.TILE_H and ws % AC.TILE_W and hs > AC.TILE_H and ws > AC.TILE_W           # two tiles each way, ragged
    assert all(hs % c and ws % c for c in AC.CELLS[1:]) and ws // 2 % 2                      # ragged last cells (cell 2: chroma)
    cov = {n: AC.roi_coverage(b, hs, ws, AC.RECT) for n, b in AC.BOXES.items()}
    ell = {n: AC.roi_coverage(b, hs, ws, AC.ELLIPSE) for n, b in AC.BOXES.items()}
    for n in AC.BOXES:
        assert AC.active(AC.BOXES[n]) == (n not in AC.INACTIVE), n
        assert cov[n].any() == (n not in AC.NOTHING) and ell[n].any() == (n not in AC.NOTHING + ("at_bound",)), n
        # the ellipse lies in its box, but for the two boxes whose x1 / y1 sit on pixel centres: <= keeps what < drops
        assert not (ell[n] & ~cov[n]).any() or n in ("ellipse_exact", "on_centres")
    ys, xs = np.nonzero(cov["inside_cell"])
    assert set(xs) == {16, 17} and set(ys) == {8, 9}
    for cell in AC.CELLS:
        assert len({(y // cell, x // cell) for y, x in zip(ys, xs)}) == 1
    ys, xs = np.nonzero(cov["across_tile"])
    assert xs.min() < AC.TILE_W <= xs.max() and ys.min() < AC.TILE_H <= ys.max()
    assert cov["over_left"][:, 0].any() and cov["over_top"][0].any() and cov["over_right"][:, -1].any() and cov["over_bottom"][-1].any()
    assert AC.BOXES["at_bound"][0] == -65536.0 and -AC.BEYOND == np.nextafter(np.float32(-65536), np.float32(-np.inf))
    assert cov["at_bound"][:, 0].any() and not cov["beyond_bound"].any()
    ys, xs = np.nonzero(cov["on_centres"])                                                  # x0 = 40.5 is in, x1 = 43.5 is out
    assert set(xs) == {40, 41, 42} and set(ys) == {20, 21}
    # the ellipse through pixel centres: equality holds at (40, 13), (30, 13), (35, 10), (35, 16) and they are covered -
    # (40, 13) and (35, 16) beyond the RECT reading of the same box (xc < x1, yc < y1)
    for x, y in ((40, 13), (30, 13), (35, 10), (35, 16)):
        lhs, rhs = AC.ellipse_sides(AC.BOXES["ellipse_exact"], x, y)
        assert lhs == rhs == np.float32(225.0) and ell["ellipse_exact"][y, x]
    assert not ell["ellipse_exact"][13, 41] and not cov["ellipse_exact"][13, 40] and ell["ellipse_exact"][13, 40]
    assert (cov["overlap_a"] & cov["overlap_b"]).any() and (ell["overlap_a"] & ell["overlap_b"]).any()
    assert AC.roi_coverage(AC.TINY_BOX, hs, ws, AC.ELLIPSE).all() and not AC.roi_coverage(AC.TINY_BOX, hs, ws, AC.RECT).any()
    kinds = {(c["kind"], c["cell"]) for c in (AC.case(n)[0] for n in AC.CASES) if c["mode"] == AC.MOSAIC}
    assert kinds >= {(k, c) for k in ("rgb", "nv12") for c in AC.CELLS}
    for kind in ("rgb", "nv12"):
        cs = [AC.case(n)[0] for n in AC.CASES if AC.case(n)[0]["kind"] == kind]
        assert {c["rpf"] for c in cs} == {1, 3, 64}
        assert {(c["shape"], c["mode"]) for c in cs} == {(s, m) for s in (AC.RECT, AC.ELLIPSE) for m in (AC.MOSAIC, AC.FILL)}
    assert {AC.case(n)[0]["standard"] for n in AC.CASES if n.startswith("nv12_fill")} == {0, 1, 2, 3}
    assert AC.yuv_of((0, 0, 255), 2)[1] == 255 and AC.yuv_of((255, 0, 0), 3)[2] == 255       # 256 without the clip
    for n in AC.CASES:
        c, (want, loads, may_read) = AC.case(n)
        assert len(c["rois"]) == c["F"] * c["rpf"] and c["F"] == 4
        changed = any((w != b).any() for w, b in zip(want, c["bufs"]))
        assert changed == (n.split("_", 1)[1] not in ("nothing", "inactive")), n
        assert (loads > 0) == (changed and c["mode"] == AC.MOSAIC), n
        used = AC.used_bytes(c)
        for w, b, u, m in zip(want, c["bufs"], used, may_read):
            assert not (w != b)[~u].any() and not m[~u].any()                              # the yardstick itself keeps to the pixels
        if c["kind"] == "nv12" and "small" not in n:
            assert c["y_fs"] > (c["hs"] - 1) * c["y_pitch"] + c["ws"]
    c = AC.case("nv12_c4_rect_r3_planes")[0]
    assert c["y_pitch"] % 2 == 1 and c["y_fs"] % 2 == 1 and len(c["bufs"]) == 2
    c = AC.case("nv12_c2_ellipse_r3")[0]
    assert c["y_pitch"] % 2 == 1 and len(c["bufs"]) == 1 and c["y_fs"] - ((c["uv"][1] - c["y"][1]) + 19 * c["uv_pitch"]) > 0
    for n in ("rgb_small_c32", "nv12_small_c32"):
        c = AC.case(n)[0]
        assert (c["hs"], c["ws"], c["cell"]) == (6, 10, 32)
    # the whole-frame ellipse changes frame 1 completely and leaves frame 2 alone
    c, (want, _, _) = AC.case("rgb_underflow")
    got, src = AC.rgb_view(c, want), AC.rgb_view(c, c["bufs"])
    assert np.array_equal(got[2], src[2]) and all(len(np.unique(got[1][j:j + 8, i:i + 8, 0])) == 1 for j in (0, 32) for i in (0, 64))


@pytest.mark.parametrize("name", AC.CASES)
def test_loads_exactly_the_touched_cells(emu_lib, name):
    """The emulator's read fence over whole allocations counts every frame-byte load: one per in-frame pixel of a touched
    cell (NV12: one per luma byte and one per (U, V) pair) - none for FILL, none for a list without an active ROI."""
    c, (want, loads, _) = AC.case(name)
    rc, got, reads = AC.call(emu_lib, "cpu", c, fences=[[(0, len(b))] for b in c["bufs"]])
    assert rc == 0 and AC.same(got, want)
    assert reads == loads
    if c["mode"] == AC.FILL or "inactive" in name or "nothing" in name:
        assert reads == 0


@pytest.mark.parametrize("name", [n for n in AC.CASES if AC.BUILDERS[n]()["mode"] == AC.MOSAIC])
def test_nothing_else_is_loaded(emu_lib, name):
    """Fences over everything that must not be loaded - untouched cells, pitch padding, frame gaps, guards, the frames no
    active ROI belongs to - stay silent while the touched cells are read."""
    c, (want, loads, may_read) = AC.case(name)
    fences = AC.forbidden_fences(may_read)
    assert all(ranges and ranges[0][0] == 3 and ranges[-1][1] == len(b) for ranges, b in zip(fences, c["bufs"]))
    rc, got, reads = AC.call(emu_lib, "cpu", c, fences=fences)
    assert rc == 0 and reads == 0 and AC.same(got, want)


def test_other_frames_are_not_touched(emu_lib):
    """rois_per_frame = 3 with active ROIs in frame 1 only: frames 0, 2 and 3 are fenced whole and stay unread."""
    for name in ("rgb_c8_ellipse_r3", "nv12_c8_rect_r3"):
        c = dict(AC.case(name)[0])
        rois = np.zeros_like(c["rois"])
        rois[3:6] = c["rois"][[0, 1, 5]]
        c["rois"] = rois
        want, loads, may_read = AC.reference(c)
        only = AC.used_bytes(c)
        if c["kind"] == "rgb":
            AC.rgb_view(c, only)[1] = False
        else:
            y, uv = AC.nv12_views(c, only)
            y[1], uv[1] = False, False
        assert loads > 0 and not any((m & o).any() for m, o in zip(may_read, only))
        rc, got, reads = AC.call(emu_lib, "cpu", c, fences=[[(a + 3, e) for a, e in AC.runs(o) if e - a > 3] for o in only])
        assert rc == 0 and reads == 0 and AC.same(got, want)


@pytest.mark.parametrize("name", ["rgb_c8_rect_r64", "rgb_c32_ellipse_r64", "nv12_c8_ellipse_r64_planes", "rgb_c4_ellipse_r3",
                                  "nv12_fill_601f"])
def test_roi_order_does_not_matter(emu_lib, name):
    AC.check_reversed(emu_lib, "cpu", name)


def test_privacy_property(emu_lib):
    """What a covered pixel shows is a function of its cell's pixels as a SET: shuffling the source pixels inside every cell
    leaves every covered output pixel unchanged (and moves uncovered ones)."""
    c, (want, _, _) = AC.case("rgb_c8_ellipse_r3")
    p = AC.permuted_within_cells(c)
    assert not np.array_equal(p["bufs"][0], c["bufs"][0])
    rc, got = AC.call(emu_lib, "cpu", p)
    cov = AC.coverage(c)
    assert rc == 0 and cov.any() and np.array_equal(AC.rgb_view(c, got)[cov], AC.rgb_view(c, want)[cov])
    assert np.array_equal(AC.rgb_view(c, got)[~cov], AC.rgb_view(p, p["bufs"])[~cov])
    assert AC.same(AC.reference(p)[0], got)


def test_case_set_tells_the_mutants_apart(emu_lib):
    """Each wrong reading of the definition changes the expected bytes of at least one case - and the kernel's bytes there
    are the definition's, not the mutant's."""
    first = {"no_half": ("rgb_c8_rect_r64", "nv12_c8_rect_r3"), "box_anchored": ("rgb_c8_ellipse_r3",),
             "covered_mean": ("rgb_c8_ellipse_r3", "nv12_c8_rect_r3"), "trunc_mean": ("rgb_c4_ellipse_r3", "nv12_c2_ellipse_r3"),
             "x1_inclusive": ("rgb_c8_rect_r64", "rgb_c16_ellipse_r1"), "wrong_frame": ("rgb_c8_rect_r64", "nv12_c4_rect_r3_planes"),
             "chroma_topleft": ("nv12_c8_rect_r3", "nv12_fill_601l")}
    assert set(first) == set(AC.MUTANTS)
    for mut, names in first.items():
        for name in names:
            c, (want, _, _) = AC.case(name)
            assert not AC.same(AC.reference(c, mut)[0], want), f"{name} does not tell {mut!r} apart"
            rc, got = AC.call(emu_lib, "cpu", c)
            assert rc == 0 and AC.same(got, want), (mut, name)


def test_argument_errors(emu_lib):
    AC.argument_errors(emu_lib, "cpu")


# ---- host side ------------------------------------------------------------------------------------------------------------
def test_head_presets_agree_with_the_joint_tables():
    """Panoptic-15: LIMBS15 starts with the neck-nose limb and the nose is a leaf; COCO-17: nose, eyes and ears are the five
    joints LIMBS17 connects among themselves, and they hang on the shoulders 5 and 6 by the ears alone."""
    from faster_voxelpose_amd.utils.vis import LIMBS15, LIMBS17
    assert _HEAD_JOINTS == {15: (0, 1), 17: (0, 1, 2, 3, 4)}
    assert LIMBS15[0] == [0, 1] and sum(1 in ab for ab in LIMBS15) == 1 and sum(0 in ab for ab in LIMBS15) == 4
    head = set(_HEAD_JOINTS[17])
    assert [ab for ab in LIMBS17 if set(ab) <= head] == [[0, 1], [0, 2], [1, 2], [1, 3], [2, 4]]
    assert [ab for ab in LIMBS17 if len(set(ab) & head) == 1] == [[3, 5], [4, 6]]
    assert FaceAnonymiser(15, _lib=object()).joint_mask == 0b11 and FaceAnonymiser(17, _lib=object()).joint_mask == 0b11111
    assert FaceAnonymiser(FS.make_cfg("panoptic", device="cpu"), _lib=object()).joints == [0, 1]
    assert FaceAnonymiser(14, joints=[12, 13], _lib=object()).joint_mask == 0b11 << 12
    with pytest.raises(capi.FvpError, match="pass joints"):
        FaceAnonymiser(14, _lib=object())


@pytest.mark.parametrize("kind,J", [("rgb", 17), ("nv12", 15)])
def test_face_anonymiser_class(emu_lib, kind, J):
    """rois(), apply() and __call__ equal the yardsticks of the two launches on RGB frames and on an NV12 surface; caller-made
    boxes; the constructor's and the methods' refusals."""
    B, V, N = 2, 2, 3
    kw = dict(scale=2.0, pad_px=1.5, min_joints=2, aspect=0.8, conf_min=0.3, cell=4, shape="ellipse", mode="mosaic", _lib=emu_lib)
    fa = FaceAnonymiser(J, **kw)
    views, ids, conf = AC.head_scene(J, list(fa.joints), 38, 70, 5)
    want_rois, want_count, want_score = AC.head_rois(views, ids, conf, fa.joints, 2.0, 1.5, 2, 0.8, 0.3)
    tv, ti, tc = (torch.from_numpy(a) for a in (views, ids, conf))
    rois, count, score = fa.rois(tv, ids=ti, joint_conf=tc)
    assert np.array_equal(rois.numpy().view(np.uint32), want_rois.view(np.uint32)) and np.array_equal(count.numpy(), want_count)
    assert np.array_equal(score.numpy().view(np.uint32), want_score.view(np.uint32))
    assert want_count.any() and not want_count[0, :, 1].any() and not want_count[0, 1, 2]
    per_frame = [[tuple(b) for b in want_rois[b, v]] for b in range(B) for v in range(V)]
    c = AC._case(kind, 4, AC.ELLIPSE, AC.MOSAIC, N, per_frame, 41, standard=3, y_pitch=75, uv_pitch=72, split=True, gap=6)
    want, loads, _ = AC.reference(c)
    assert loads > 0
    for run in ("apply", "call"):
        bufs = [torch.from_numpy(b.copy()) for b in c["bufs"]]
        frames = AC.torch_frames(c, bufs, (B, V))
        out = fa.apply(frames, rois) if run == "apply" else fa(frames, tv, ids=ti, joint_conf=tc)
        assert out is frames and AC.same([t.numpy() for t in bufs], want)
    # caller-made boxes, rect + fill
    c2, (want2, _, _) = AC.case("rgb_fill_rect_r3" if kind == "rgb" else "nv12_fill_709l_planes")
    bufs2 = [torch.from_numpy(b.copy()) for b in c2["bufs"]]
    fill = FaceAnonymiser(J, cell=8, shape="rect", mode="fill", colour=c2["colour"], _lib=emu_lib)
    fill.apply(AC.torch_frames(c2, bufs2, (2, 2)), torch.from_numpy(c2["rois"]).view(2, 2, 3, 4))
    assert AC.same([t.numpy() for t in bufs2], want2)
    with pytest.raises(capi.FvpError):
        fa.apply(frames, rois[:, :1].contiguous())                               # V differs
    with pytest.raises(capi.FvpError):
        fa.apply(frames, rois.double())
    with pytest.raises(capi.FvpError):
        fa.apply(frames, rois.to("meta"))                                        # frames and rois on different devices
    with pytest.raises(capi.FvpError):
        fa.apply(frames, torch.zeros(B, V, 65, 4))                               # more than 64 boxes per frame
    with pytest.raises(capi.FvpError):
        fa.apply(frames, torch.zeros(B, V, 0, 4))
    with pytest.raises(capi.FvpError):
        fa.apply(bufs[0], rois)                                                  # not [B,V,Hs,Ws,3]
    with pytest.raises(capi.FvpError):
        FaceAnonymiser(J).apply(frames, rois)                                    # the product: host memory is refused
    with pytest.raises(capi.FvpError):
        FaceAnonymiser(J).rois(tv)
    with pytest.raises(capi.FvpError):
        fa.rois(tv[..., :3].contiguous())
    with pytest.raises(capi.FvpError):
        fa.rois(tv, ids=ti.long())
    with pytest.raises(capi.FvpError):
        fa.rois(tv, joint_conf=tc[:, :, :5].contiguous())
    for bad in (dict(scale=0.0), dict(scale=float("nan")), dict(pad_px=-1.0), dict(pad_px=float("inf")), dict(min_joints=0),
                dict(aspect=0.0), dict(aspect=float("inf")), dict(conf_min=float("nan")), dict(joints=[0, J]), dict(joints=[]),
                dict(cell=3), dict(cell=64), dict(cell=8.5), dict(shape="circle"), dict(mode="blur"), dict(colour=(0, 0)),
                dict(colour=(0, 0, 256)), dict(colour=(-1, 0, 0)), dict(colour=5)):
        with pytest.raises(capi.FvpError):
            FaceAnonymiser(J, **{**kw, **bad})
    with pytest.raises(capi.FvpError):
        FaceAnonymiser(capi.FVP_MAX_JOINTS + 1, joints=[0], _lib=emu_lib)


def _launches(lib, fn):
    lib.hipemu_launch_log.restype = C.c_char_p
    lib.hipemu_launch_log_reset()
    out = fn()
    return out, lib.hipemu_launch_log().decode().split()


@pytest.mark.parametrize("kind", ["rgb", "nv12"])
def test_forward_then_anonymise_then_overlay(emu_lib, kind):
    """Tiny configuration through a torch backbone with model.evidence: FaceAnonymiser on last_evidence, then overlay.draw,
    equals the two C-level routes on a pristine copy of the frames (the anonymiser's yardstick on the boxes, then the overlay),
    in that order and not in the other; constructing and calling the anonymiser adds nothing to the forward's launches."""
    cfg = FS.make_cfg("tiny", device="cpu", min_score=-1.0)
    cams, seq = FS.load_cameras("tiny")
    rt = FS.resize_transform(cfg)
    model = FV.FasterVoxelPoseNet(cfg, _lib=emu_lib)
    model.load_state_dict(FS.fill_state_dict(model.state_dict(), seed=7))
    ws, hs = cfg.DATASET.ORI_IMAGE_SIZE
    J, nv = cfg.DATASET.NUM_JOINTS, cfg.DATASET.CAMERA_NUM
    N = model.max_people
    c = AC._case(kind, 8, AC.ELLIPSE, AC.MOSAIC, N, [[] for _ in range(2 * nv)], 51, hs=hs, ws=ws, standard=1, y_pitch=ws + 7,
                 uv_pitch=ws + 8, split=True, gap=4)
    bufs = [torch.from_numpy(b.copy()) for b in c["bufs"]]
    frames = AC.torch_frames(c, bufs, (2, nv))
    meta = {"seq": [seq, seq]}

    class Stub(torch.nn.Module):
        def forward(self, x):
            pooled = torch.nn.functional.avg_pool2d(x, 4).mean(dim=1, keepdim=True)
            return pooled.expand(-1, J, -1, -1).contiguous()

    kw = dict(backbone=Stub(), meta=meta, cameras=cams, resize_transform=rt)
    with torch.no_grad():
        model.evidence = True
        model(views=frames, **kw)                                                    # packs the weights, fills the caches
        _, parent = _launches(emu_lib, lambda: model(views=frames, **kw))
        fa = FaceAnonymiser(cfg, joints=[0, 1], scale=2.0, pad_px=6.0, cell=8, _lib=emu_lib)
        overlay = PoseOverlay(cfg, limbs=TINY_LIMBS, alpha=0.5, nv12=True, _lib=emu_lib)
        out, launches = _launches(emu_lib, lambda: model(views=frames, **kw))
        assert launches == parent and not any("anonymise" in k for k in launches)    # not a stage: the forward is the parent's
        assert AC.same([t.numpy() for t in bufs], c["bufs"])
        px, conf = model.last_evidence
        _, two = _launches(emu_lib, lambda: fa(frames, px, joint_conf=conf))
        assert len(two) == 2 and "k_person_rois" in two[0] and "k_anonymise_rois" in two[1]
        assert ("k_anonymise_rois_nv12" in two[1]) == (kind == "nv12")
        overlay.draw(frames, px, joint_conf=conf)
        # the direct route on a pristine copy: the yardstick on the boxes, then the overlay's own call
        rois = fa.rois(px, joint_conf=conf)[0]
        d = dict(c)
        d["rois"] = rois.numpy().reshape(-1, 4)
        hidden, loads, _ = AC.reference(d)
        assert loads > 0 and not AC.same(hidden, c["bufs"])                          # some head is in some view
        direct = [torch.from_numpy(b.copy()) for b in hidden]
        overlay.draw(AC.torch_frames(c, direct, (2, nv)), px, joint_conf=conf)
        assert AC.same([t.numpy() for t in bufs], [t.numpy() for t in direct])
        assert not AC.same([t.numpy() for t in direct], hidden)                      # the skeletons are on top, unsmeared
        other = [torch.from_numpy(b.copy()) for b in c["bufs"]]                      # the wrong order smears them
        fa.apply(overlay.draw(AC.torch_frames(c, other, (2, nv)), px, joint_conf=conf), rois)
        assert not AC.same([t.numpy() for t in other], [t.numpy() for t in direct])
