"""fvp_person_rois, fvp_crop_rois and fvp_crop_rois_nv12 on the CPU emulation of the kernels (tests/hipemu): every case of
tests/crop_cases.py against the independent numpy restatement, bit for bit; the tie of every crop to the ingest call with
the derived matrix; the identity; the read fence (what is not needed is not loaded, padding is never touched); the case set
against six mutated yardsticks; every argument error; PersonCrops and model.crops; the pipelines' refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

import crop_cases as CC
import fvp_synthetic as FS
from faster_voxelpose_amd import _capi as capi
from faster_voxelpose_amd.core.smoothing import PoseSmoother
from faster_voxelpose_amd.core.tracking import PoseTracker
from faster_voxelpose_amd.models import faster_voxelpose as FV
from faster_voxelpose_amd.utils.crops import PersonCrops
from faster_voxelpose_amd.utils.overlay import PoseOverlay

TINY_LIMBS = [(0, 1), (1, 2), (2, 3), (3, 4)]            # the tiny configuration has 5 joints: no default skeleton


def test_header_and_binding_hold_the_three_exports(emu_lib):
    assert capi.ABI_VERSION >= 16 and emu_lib.fvp_version() == capi.ABI_VERSION
    for name in ("fvp_person_rois", "fvp_crop_rois", "fvp_crop_rois_nv12"):
        assert name in capi.SIGNATURES and hasattr(emu_lib, name)


# ---- fvp_person_rois ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,J", CC.ROI_CASES)
def test_rois_equal_the_yardstick(emu_lib, name, J):
    CC.roi_check(emu_lib, "cpu", name, J)


def test_roi_cases_hold_what_their_names_say():
    for J in (5, 17):
        _, (rois, count, _, branches) = CC.roi_case("tall_and_wide", J)
        assert branches == {True, False}                                       # both aspect branches are taken
        assert (count == J).all()
        _, (rois, count, score, _) = CC.roi_case("mask_none", J)
        assert not count.any() and not rois.any() and not score.any()
        _, (rois, count, _, _) = CC.roi_case("mask_two", J)
        assert (count == 2).all()
        _, (rois, count, _, _) = CC.roi_case("k_at_min", J)
        assert count[0, 0, 0] == 3 and rois[0, 0, 0].any() and count[0, 0, 1] == 0 and not rois[0, 0, 1].any()
        _, (rois, count, _, _) = CC.roi_case("single_joint", J)
        assert (count[:, :, 0] == 1).all() and (rois[:, :, 0, 0] == rois[:, :, 0, 2]).all()      # degenerate: x1 == x0
        assert not any(CC.croppable(r) for r in rois[:, :, 0].reshape(-1, 4))
        _, (rois, count, _, _) = CC.roi_case("ids_minus1", J)
        assert not count[0, :, 1].any() and not count[1, :, 0].any() and count[0, :, 0].all()
        on, off = CC.roi_case("conf_on", J)[1], CC.roi_case("conf_off", J)[1]
        assert (on[1] < off[1]).any() and (off[1] == J).all()
        _, (_, count, _, _) = CC.roi_case("behind_camera", J)
        assert count[0, 0, 0] == J - 1 and count[1, 1, 2] == J - 1
        _, (_, count, _, _) = CC.roi_case("nan_pixel", J)
        assert count[0, 1, 1] == J - 1 and count[0, 1, 2] == J - 1 and count[1, 0, 0] == J - 1 and count[1, 0, 1] == J


def test_roi_outputs_may_be_null(emu_lib):
    CC.roi_check_null_outputs(emu_lib, "cpu")


def test_roi_argument_errors(emu_lib):
    CC.roi_argument_errors(emu_lib, "cpu")


# ---- fvp_crop_rois / fvp_crop_rois_nv12 ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CC.CROP_CASES)
def test_crops_equal_the_yardstick(emu_lib, name):
    CC.crop_check(emu_lib, "cpu", name)


@pytest.mark.parametrize("name", [n for n in CC.CROP_CASES if "nothing" not in n])
def test_crop_equals_the_ingest_with_the_derived_matrix(emu_lib, name):
    assert CC.crop_check_tie(emu_lib, "cpu", name) >= 2


@pytest.mark.parametrize("name", ["rgb_identity", "nv12_709f_identity_planes"])
def test_whole_frame_at_its_own_size_is_the_identity_ingest(emu_lib, name):
    CC.crop_check_identity(emu_lib, "cpu", name)


def test_crop_cases_hold_what_their_names_say():
    boxes = dict(CC.roi_list(24, 40))
    assert sum(CC.croppable(b) for b in boxes.values()) == 10 and len(boxes) == 18
    for n in ("x1_eq_x0", "x1_lt_x0", "y1_eq_y0", "nan", "nan_y1", "inf", "minus_inf", "zeros"):
        assert not CC.croppable(boxes[n]), n
    assert CC.crop_matrix(boxes["inside_up"], 8, 8)[0] < 1 < CC.crop_matrix(boxes["inside_down"], 8, 8)[0]      # up and down
    for name in CC.CROP_CASES:
        c, (want, taps) = CC.crop_case(name)
        assert len(c["rois"]) == c["F"] * c["rpf"] and (c["h"] * (c["w"] // 2)) % 256 != 0
        assert (taps == 0) == ("nothing" in name)
        if c["kind"] == "nv12":
            assert c["hs"] == 26 and c["ws"] == 40
    assert {CC.crop_case(n)[0]["standard"] for n in CC.CROP_CASES if n.startswith("nv12") and "nothing" not in n} == {0, 1, 2, 3}
    c = CC.crop_case("nv12_709l_8x8_per3_planes")[0]
    assert c["y_pitch"] % 2 == 1 and c["y_fs"] % 2 == 1 and len(c["bufs"]) == 2 and c["rpf"] == 3
    assert CC.crop_case("rgb_identity")[0]["h"] * 20 > 256                                # more than one block per ROI


@pytest.mark.parametrize("name", CC.CROP_CASES)
def test_loads_exactly_the_taps_inside_the_frame(emu_lib, name):
    """The emulator's read fence over whole allocations: one load per in-frame tap of a croppable ROI (NV12: a luma byte and
    a chroma pair) - nothing for a non-croppable ROI, nothing for a tap outside the frame."""
    c, (want, taps) = CC.crop_case(name)
    rc, _, o32, reads = CC.crop_call(emu_lib, "cpu", c, fences=[[(0, len(b))] for b in c["bufs"]])
    assert rc == 0 and np.array_equal(CC.bits(o32), CC.bits(want))
    assert reads == taps * (2 if c["kind"] == "nv12" else 1)


@pytest.mark.parametrize("name", ["nv12_601l_6x4", "nv12_709l_8x8_per3_planes", "nv12_709f_identity_planes"])
def test_padding_is_never_touched(emu_lib, name):
    """Pitch padding, frame gaps and the bytes behind the planes.  A fence counts a read when the four bytes from its
    address on meet the range: the padding fences begin three bytes in."""
    c, (want, taps) = CC.crop_case(name)
    pads = [[(a + 3, e) for a, e in ranges if e - a > 3] for ranges in CC.nv12_padding(c)]
    assert sum(len(p) for p in pads) >= c["F"] * c["hs"] and taps > 0              # every luma row has its padding fenced
    rc, _, o32, reads = CC.crop_call(emu_lib, "cpu", c, fences=pads)
    assert rc == 0 and reads == 0 and np.array_equal(CC.bits(o32), CC.bits(want))


def test_other_frames_are_not_touched(emu_lib):
    """rois_per_frame = 3 with only the ROIs of frame 1 croppable: frames 0 and 2.. are fenced and stay unread."""
    c = dict(CC.crop_case("rgb_8x8_per3_swap")[0])
    rois = np.zeros_like(c["rois"])
    rois[3:6] = c["rois"][[0, 2, 6]]
    c["rois"] = rois
    want, taps = CC.crop_reference(c)
    fb = c["hs"] * c["ws"] * 3
    fences = [[(3, fb), (2 * fb + 3, c["F"] * fb)]]
    rc, _, o32, reads = CC.crop_call(emu_lib, "cpu", c, fences=fences)
    assert rc == 0 and reads == 0 and taps > 0 and np.array_equal(CC.bits(o32), CC.bits(want))


def test_crop_argument_errors(emu_lib):
    CC.crop_argument_errors(emu_lib, "cpu")


def test_case_set_tells_the_mutants_apart(emu_lib):
    """Each wrong reading of a definition changes the expected bits of at least one case - and the kernel's bits there are
    the definition's, not the mutant's."""
    first = {"no_half": "rgb_6x4", "wh_swapped": "rgb_6x4", "clip": "rgb_6x4", "frame_index": "rgb_8x8_per3_swap"}
    assert set(first) == set(CC.CROP_MUTANTS)
    for mut, name in first.items():
        c, (want, _) = CC.crop_case(name)
        assert not np.array_equal(CC.bits(CC.crop_reference(c, mut)[0]), CC.bits(want)), f"no case tells {mut!r} apart"
        assert np.array_equal(CC.bits(CC.crop_call(emu_lib, "cpu", c)[2]), CC.bits(want)), mut
    for mut in ("no_half", "wh_swapped", "clip", "frame_index"):                  # the NV12 kernel's cases tell them too
        name = "nv12_709l_8x8_per3_planes" if mut != "wh_swapped" else "nv12_601l_6x4"
        c, (want, _) = CC.crop_case(name)
        assert not np.array_equal(CC.bits(CC.crop_reference(c, mut)[0]), CC.bits(want)), (mut, name)
        assert np.array_equal(CC.bits(CC.crop_call(emu_lib, "cpu", c)[2]), CC.bits(want)), mut
    # clipping to the frame changes exactly the overhanging boxes
    c, (want, _) = CC.crop_case("rgb_6x4")
    clipped = CC.crop_reference(c, "clip")[0]
    names = [n for n, _ in CC.roi_list(24, 40)]
    differ = {names[r] for r in range(len(names)) if not np.array_equal(CC.bits(clipped[r]), CC.bits(want[r]))}
    assert {"over_left", "over_right", "over_top", "over_bottom", "over_all"} <= differ and "inside_up" not in differ
    roi_first = {"minmax_all": "behind_camera", "aspect_reversed": "tall_and_wide"}
    assert set(roi_first) == set(CC.ROI_MUTANTS)
    for mut, name in roi_first.items():
        for J in (5, 17):
            case, (rois, count, score, _) = CC.roi_case(name, J)
            assert not np.array_equal(CC.bits(CC.roi_reference(case, mut)[0]), CC.bits(rois)), (mut, J)
            rc, (r, _, _) = CC.roi_call(emu_lib, "cpu", case)
            assert rc == 0 and np.array_equal(CC.bits(r), CC.bits(rois)), mut
    case, (rois, _, _, _) = CC.roi_case("nan_pixel", 17)
    assert not np.array_equal(CC.bits(CC.roi_reference(case, "minmax_all")[0]), CC.bits(rois))


# ---- host side ------------------------------------------------------------------------------------------------------------
def _u16(t):
    return t.view(torch.int16).numpy().view(np.uint16)


def test_person_crops_class(emu_lib):
    """rois(), crop() and __call__ equal the C calls (the yardstick's bits) on RGB frames and on an NV12 surface, fp32 and
    bf16; the constructor's and the methods' refusals."""
    J, size = 17, (8, 6)
    views, ids, conf = CC.person_scene(J, 26, 40, 3)
    kw = dict(size=size, scale=1.5, pad_px=2.0, min_joints=3, conf_min=0.3, _lib=emu_lib)
    pc = PersonCrops(J, joints=[0, 1, 2, 5, 9, 16], **kw)
    assert (pc.h, pc.w, pc.joint_mask, pc.bf16) == (8, 6, 0b10000001000100111, False)
    case = dict(views=views, ids=ids, conf=conf, mask=pc.joint_mask, min_joints=3, scale=1.5, pad_px=2.0, aspect=6 / 8,
                conf_min=0.3)
    want_rois, want_count, want_score, _ = CC.roi_reference(case)
    tv, ti, tc = (torch.from_numpy(a) for a in (views, ids, conf))
    rois, count, score = pc.rois(tv, ids=ti, joint_conf=tc)
    assert np.array_equal(CC.bits(rois.numpy()), CC.bits(want_rois)) and np.array_equal(count.numpy(), want_count)
    assert np.array_equal(CC.bits(score.numpy()), CC.bits(want_score))
    assert want_count.any() and not want_count[0, :, 1].any() and not want_count[0, 1, 2]
    for kind in ("rgb", "nv12"):
        c = CC._crop(kind, 26, 40, size, CC.N, 31, swap=kind == "rgb", standard=3, y_pitch=47, uv_pitch=48, split=True, gap=4,
                     rois=want_rois.reshape(-1, 4))
        want, _ = CC.crop_reference(c)
        bufs = [torch.from_numpy(b.copy()) for b in c["bufs"]]
        frames = bufs[0].view(CC.B, CC.V, 26, 40, 3) if kind == "rgb" else CC.nv12_frames(c, bufs, (CC.B, CC.V))
        pk = PersonCrops(J, joints=[0, 1, 2, 5, 9, 16], swap_rb=kind == "rgb", **kw)
        patches = pk.crop(frames, rois)
        assert patches.shape == (CC.B, CC.V, CC.N, 3, 8, 6) and patches.dtype == torch.float32
        assert np.array_equal(CC.bits(patches.numpy().reshape(-1, 3, 8, 6)), CC.bits(want))
        both = pk(frames, tv, ids=ti, joint_conf=tc)
        assert torch.equal(both[0].view(torch.int32), patches.view(torch.int32)) and torch.equal(both[2], count)
        assert torch.equal(both[1].view(torch.int32), rois.view(torch.int32))
        assert torch.equal(both[3].view(torch.int32), score.view(torch.int32))
        p16 = PersonCrops(J, bf16=True, swap_rb=kind == "rgb", **kw).crop(frames, rois)
        assert p16.shape == (CC.B, CC.V, CC.N, 8, 3, 8) and p16.dtype == torch.bfloat16
        assert np.array_equal(_u16(p16).reshape(-1, 8, 3, 8), CC.pack_nhwc8(want))
        with pytest.raises(capi.FvpError):
            pk.crop(frames, rois[:, :1].contiguous())                            # V differs
        with pytest.raises(capi.FvpError):
            pk.crop(frames, rois.double())
        with pytest.raises(capi.FvpError):
            pk.crop(frames, rois.to("meta"))                                     # frames and rois on different devices
        with pytest.raises(capi.FvpError):
            PersonCrops(J, size=size).crop(frames, rois)                         # the product: host memory is refused
    with pytest.raises(capi.FvpError):
        PersonCrops(J, swap_rb=True, **kw).crop(frames, rois)                    # swap_rb on an NV12 surface
    with pytest.raises(capi.FvpError):
        pc.crop(bufs[0], rois)                                                   # not [B,V,Hs,Ws,3]
    for bad in (dict(size=(8, 7)), dict(size=(0, 6)), dict(size=8), dict(scale=0.0), dict(scale=float("nan")), dict(pad_px=-1.0),
                dict(min_joints=0), dict(conf_min=float("nan")), dict(joints=[0, J]), dict(std=(1.0, 0.0, 1.0)),
                dict(mean=(0.0, 1.0))):
        with pytest.raises(capi.FvpError):
            PersonCrops(J, **{**kw, **bad})
    with pytest.raises(capi.FvpError):
        PersonCrops(capi.FVP_MAX_JOINTS + 1, _lib=emu_lib)
    with pytest.raises(capi.FvpError):
        pc.rois(tv[..., :3].contiguous())
    with pytest.raises(capi.FvpError):
        pc.rois(tv, ids=ti.long())
    with pytest.raises(capi.FvpError):
        pc.rois(tv, joint_conf=tc[:, :, :5].contiguous())
    with pytest.raises(capi.FvpError):
        PersonCrops(J, size=size).rois(tv)                                       # the product: host memory is refused


def _launches(lib, fn):
    lib.hipemu_launch_log.restype = C.c_char_p
    lib.hipemu_launch_log_reset()
    out = fn()
    return out, lib.hipemu_launch_log().decode().split()


@pytest.mark.parametrize("kind", ["rgb", "nv12"])
def test_model_crops_attribute(emu_lib, kind):
    """model.crops on the tiny configuration through a torch backbone.  Unset, the forward issues exactly the launches it
    issued before; set, two launches more behind the rest (with a smoother: its own, ONE evidence launch shared with the
    overlay, then the two), the outputs keep their bits, and the patches equal a direct call on a pristine copy of the
    frames - also when an overlay paints the frames in the same forward."""
    cfg = FS.make_cfg("tiny", device="cpu", min_score=-1.0)
    cams, seq = FS.load_cameras("tiny")
    rt = FS.resize_transform(cfg)
    model = FV.FasterVoxelPoseNet(cfg, _lib=emu_lib)
    model.load_state_dict(FS.fill_state_dict(model.state_dict(), seed=7))
    ws, hs = cfg.DATASET.ORI_IMAGE_SIZE
    J, nv = cfg.DATASET.NUM_JOINTS, cfg.DATASET.CAMERA_NUM
    c = CC._crop(kind, hs, ws, (8, 6), 1, 41, standard=1, y_pitch=ws + 7, uv_pitch=ws + 8, split=True, gap=4,
                 rois=[(0.0, 0.0, 1.0, 1.0)] * (2 * nv))
    bufs = [torch.from_numpy(b.copy()) for b in c["bufs"]]
    before = [t.clone() for t in bufs]

    def as_frames(bb):
        return bb[0].view(2, nv, hs, ws, 3) if kind == "rgb" else CC.nv12_frames(c, bb, (2, nv))

    frames = as_frames(bufs)
    meta = {"seq": [seq, seq]}

    class Stub(torch.nn.Module):
        def forward(self, x):
            pooled = torch.nn.functional.avg_pool2d(x, 4).mean(dim=1, keepdim=True)
            return pooled.expand(-1, J, -1, -1).contiguous()

    def same(a, b):
        return all(torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)
                   for x, y in zip(a, b))

    def direct(px, ids):
        return model.crops(as_frames([b.clone() for b in before]), px, ids=ids, joint_conf=model.last_evidence[1])

    kw = dict(backbone=Stub(), meta=meta, cameras=cams, resize_transform=rt)
    with torch.no_grad():
        model.crops = PersonCrops(cfg, size=(8, 6), _lib=emu_lib)
        with pytest.raises(capi.FvpError, match="model.evidence"):
            model(views=frames, **kw)
        model.evidence = True
        with pytest.raises(capi.FvpError, match="camera frames"):
            model(views=torch.zeros(2, nv, 3, cfg.DATASET.IMAGE_SIZE[1], cfg.DATASET.IMAGE_SIZE[0]), **kw)
        model.crops = None
        model(views=frames, **kw)                                                    # packs the weights, fills the caches
        plain, unset = _launches(emu_lib, lambda: model(views=frames, **kw))
        assert not any("k_person_rois" in k or "k_crop_rois" in k for k in unset) and model.last_crops is None
        model.crops = PersonCrops(cfg, size=(8, 6), min_joints=1, _lib=emu_lib)
        out, with_crops = _launches(emu_lib, lambda: model(views=frames, **kw))
        assert with_crops[:-2] == unset and "k_person_rois" in with_crops[-2]        # two launches more, behind the rest
        assert ("k_crop_rois_nv12" in with_crops[-1]) == (kind == "nv12") and "k_crop_rois" in with_crops[-1]
        assert same(out[:3], plain[:3]) and same(bufs, before)
        patches, rois, count, score = model.last_crops
        assert patches.shape == (2, nv, model.max_people, 3, 8, 6) and count.any()
        assert same(model.last_crops, direct(model.last_evidence[0], None))
        # tracker: its ids select the persons
        model.tracker = PoseTracker(cfg, _lib=emu_lib)
        _, launches = _launches(emu_lib, lambda: model(views=frames, **kw))
        assert len(launches) == len(unset) + 3
        assert same(model.last_crops, direct(model.last_evidence[0], model.last_tracks[0]))
        # tracker, smoother and overlay: the steady poses' pixels, one evidence launch for both, crops before the paint
        model.smoother = PoseSmoother(model.tracker)
        model.overlay = PoseOverlay(cfg, limbs=TINY_LIMBS, alpha=0.5, nv12=True, _lib=emu_lib)
        out, launches = _launches(emu_lib, lambda: model(views=frames, **kw))
        assert len(launches) == len(unset) + 1 + 1 + 1 + 2 + 1                     # tracker, smoother, evidence, crops, draw
        assert "k_person_rois" in launches[-3] and "k_crop_rois" in launches[-2] and "k_draw_poses" in launches[-1]
        assert sum("k_joint_evidence" in k for k in launches) == sum("k_joint_evidence" in k for k in unset) + 1
        ev = model.engine.joint_evidence(model.last_smooth[0], out[3], meta, cams, rt)[0]
        assert torch.equal(model.last_overlay_views, ev) and not same(bufs, before)  # the frames are painted ...
        assert same(model.last_crops, direct(ev, model.last_tracks[0]))              # ... the patches hold clean pixels
        # the pipelines refuse a model with crops
        model.tracker = model.smoother = model.overlay = None
        with pytest.raises(capi.FvpError, match="consumer stream"):
            FV.PipelinedForward(model, depth=1, streams=[None])
        with pytest.raises(capi.FvpError, match="consumer stream"):
            FV.GraphedPipeline(model, 1, meta, out[3], cams, rt, streams=[None])
