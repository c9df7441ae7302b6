"""fvp_draw_poses on the CPU emulation of the kernels (tests/hipemu): every case of tests/overlay_cases.py against the
independent integer restatement of the definition, the whole frame byte for byte; the read fence on frames nothing is drawn
on; every argument error; the case-set check against six mutated yardsticks; PoseOverlay and model.overlay."""
import ctypes as C

import numpy as np
import pytest
import torch

import fvp_synthetic as FS
import overlay_cases as OC
from faster_voxelpose_amd import _capi as capi
from faster_voxelpose_amd.core.smoothing import PoseSmoother
from faster_voxelpose_amd.core.tracking import PoseTracker
from faster_voxelpose_amd.models import faster_voxelpose as FV
from faster_voxelpose_amd.utils.overlay import PALETTE, PoseOverlay

TINY_LIMBS = [(0, 1), (1, 2), (2, 3), (3, 4)]            # the tiny configuration has 5 joints: no default skeleton


@pytest.mark.parametrize("name", list(OC.CASES))
def test_equals_the_yardstick(emu_lib, name):
    OC.check_case(emu_lib, "cpu", name)


@pytest.mark.parametrize("name", ["nothing_drawable", "limb_wholly_outside"])
def test_frames_nothing_covers_are_not_read(emu_lib, name):
    """The emulator's read fence over the whole frame buffer: zero reads where nothing is drawable; the same fence counts
    the covered pixels of a case that draws (the fence is live)."""
    case, want = OC.expected(name)
    got, reads = OC.run(emu_lib, "cpu", case, fence=True)
    assert np.array_equal(got, case["frames"]) and reads == 0
    case, want = OC.expected("capsules")
    got, reads = OC.run(emu_lib, "cpu", case, fence=True)
    assert np.array_equal(got, want)
    assert reads == int((want != case["frames"]).any(axis=-1).sum()) > 0     # alpha = 256 on a random frame: covered = changed


def test_argument_errors(emu_lib):
    OC.case_argument_errors(emu_lib, "cpu")


def test_case_set_tells_the_mutants_apart():
    """Each wrong reading of the definition changes the expected frame of at least one case: the byte-for-byte comparison
    of test_equals_the_yardstick would catch a kernel that implements it."""
    first = {"disc_lt": "disc_edges", "perp_lt": "capsules", "trunc": "disc_edges", "descending": "blend_256",
             "per_primitive": "blend_128", "no_half": "blend_128"}
    assert set(first) == set(OC.MUTANTS)
    for mut in OC.MUTANTS:
        case, want = OC.expected(first[mut])
        assert not np.array_equal(OC.reference(case, mut), want), f"no case tells the mutant {mut!r} from the definition"
    # the named pixels of the edge cases: covered at exactly R / W, not covered one unit further
    case, want = OC.expected("disc_edges")
    changed = (want != case["frames"]).any(axis=-1)[0, 0]
    assert changed[10, 25] and changed[14, 23] and not changed[10, 26]           # |p-q| == R; R + 16
    assert not changed[18, 105] and changed[18, 104]                             # R^2 + 1 on the squared test
    assert changed[31, 65] and not changed[31, 54]                               # 959.5 -> 960: [55, 65]
    case, want = OC.expected("capsules")
    changed = (want != case["frames"]).any(axis=-1)[0, 0]
    assert changed[20, 24] and not changed[20, 25]                               # |cross| == W * 80 on d = (48, 64)


def test_pose_overlay_class(emu_lib):
    """The host class: defaults, Q4 / alpha conversion, draw() == the C call == the yardstick, and the refusals."""
    ov = PoseOverlay(15, _lib=emu_lib)
    assert (ov.joint_radius_q4, ov.limb_half_q4, ov.alpha, ov.conf_min) == (128, 32, 256, 0.0)
    assert ov.limbs == [tuple(ab) for ab in OC.LIMBS15] and ov.palette == [tuple(c) for c in PALETTE] and len(PALETTE) == 16
    assert PoseOverlay(17, _lib=emu_lib).limbs == [tuple(ab) for ab in OC.LIMBS17]
    assert len(PoseOverlay(14, _lib=emu_lib).limbs) == 14
    cfg = FS.make_cfg("tiny", device="cpu")
    assert PoseOverlay(cfg, limbs=TINY_LIMBS, _lib=emu_lib).J == cfg.DATASET.NUM_JOINTS == 5
    ov = PoseOverlay(17, joint_radius=2.5, limb_width=2.5, alpha=0.625, conf_min=0.2, palette=OC.PAL3, _lib=emu_lib)
    assert (ov.joint_radius_q4, ov.limb_half_q4, ov.alpha) == (40, 20, 160)
    case, _ = OC.expected("crowd")
    case = dict(case, palette=OC.PAL3)
    frames = torch.from_numpy(case["frames"].copy())
    out = ov.draw(frames, torch.from_numpy(case["views"]), ids=torch.from_numpy(case["ids"]),
                  joint_conf=torch.from_numpy(case["conf"]))
    assert out is frames and np.array_equal(frames.numpy(), OC.reference(case))
    views = torch.from_numpy(case["views"])
    good = torch.from_numpy(case["frames"].copy())
    bad = [(good.float(), views, None, None), (good[..., :2].contiguous(), views, None, None),
           (good.permute(0, 1, 4, 2, 3), views, None, None), (good[0], views, None, None), (good, views.double(), None, None),
           (good, views[:, :1].contiguous(), None, None), (good, views[..., :16, :].contiguous(), None, None),
           (good, views, torch.zeros((2, 3), dtype=torch.int64), None), (good, views, torch.zeros((2, 2), dtype=torch.int32), None),
           (good, views, None, torch.zeros((2, 3, 16))), (good, views, None, torch.zeros((2, 3, 17), dtype=torch.float64)),
           (good.numpy(), views, None, None)]
    for f, v, i, c in bad:
        with pytest.raises(capi.FvpError):
            ov.draw(f, v, ids=i, joint_conf=c)
    assert np.array_equal(good.numpy(), case["frames"])
    with pytest.raises(capi.FvpError):
        PoseOverlay(15).draw(good, views)                                # the product: frames on the CPU are refused
    for kw in (dict(alpha=0.0), dict(alpha=1.5), dict(alpha=float("nan")), dict(joint_radius=-1.0), dict(joint_radius=65.0),
               dict(limb_width=129.0), dict(conf_min=float("nan")), dict(limbs=[[0, 15]]), dict(limbs=[[0, 1]] * 65),
               dict(palette=[]), dict(palette=[[0, 0, 256]]), dict(palette=[[1, 2, 3]] * 65)):
        with pytest.raises(capi.FvpError):
            PoseOverlay(15, _lib=emu_lib, **kw)
    for J in (0, 33, 16):                                                # 16: no default skeleton
        with pytest.raises(capi.FvpError):
            PoseOverlay(J, _lib=emu_lib)
    assert PoseOverlay(16, limbs=[[0, 15]], _lib=emu_lib).limbs == [(0, 15)]


def _launches(lib, fn):
    lib.hipemu_launch_log.restype = C.c_char_p
    lib.hipemu_launch_log_reset()
    out = fn()
    return out, lib.hipemu_launch_log().decode().split()


def test_model_overlay_attribute(emu_lib):
    """model.overlay on the tiny configuration with uint8 frames through a torch backbone: the frames after the forward
    equal draw() applied to a copy taken before, with the model's own last_* tensors - tracker only, then tracker and
    smoother; unset, the frames keep their bits and the forward issues the launches it issued; the refusals."""
    cfg = FS.make_cfg("tiny", device="cpu", min_score=-1.0)
    cams, seq = FS.load_cameras("tiny")
    rt = FS.resize_transform(cfg)
    model = FV.FasterVoxelPoseNet(cfg, _lib=emu_lib)
    model.load_state_dict(FS.fill_state_dict(model.state_dict(), seed=7))
    ws, hs = cfg.DATASET.ORI_IMAGE_SIZE
    J, V = cfg.DATASET.NUM_JOINTS, cfg.DATASET.CAMERA_NUM
    g = torch.Generator().manual_seed(5)
    frames = torch.randint(0, 256, (2, V, hs, ws, 3), dtype=torch.uint8, generator=g)
    meta = {"seq": [seq, seq]}

    class Stub(torch.nn.Module):
        def forward(self, x):
            pooled = torch.nn.functional.avg_pool2d(x, 4).mean(dim=1, keepdim=True)
            return pooled.expand(-1, J, -1, -1).contiguous()

    kw = dict(backbone=Stub(), meta=meta, cameras=cams, resize_transform=rt)
    before = frames.clone()
    with torch.no_grad():
        assert model.overlay is None and model.last_overlay_views is None
        plain, parent = _launches(emu_lib, lambda: model(views=frames, **kw))
        assert torch.equal(frames, before) and not any("k_draw_poses" in k for k in parent)
        model.evidence = True
        model.tracker = PoseTracker(cfg, _lib=emu_lib)
        _, unset = _launches(emu_lib, lambda: model(views=frames, **kw))
        assert torch.equal(frames, before)
        model.tracker.reset()
        model.overlay = PoseOverlay(cfg, limbs=TINY_LIMBS, alpha=0.5, conf_min=0.0, _lib=emu_lib)
        out, with_overlay = _launches(emu_lib, lambda: model(views=frames, **kw))
        assert with_overlay[:-1] == unset and "k_draw_poses" in with_overlay[-1]      # one launch more, behind the rest
        for a, b in zip(out[:3], plain[:3]):
            assert torch.equal(a, b)
        assert model.last_overlay_views is None
        want = model.overlay.draw(before.clone(), model.last_evidence[0], ids=model.last_tracks[0],
                                  joint_conf=model.last_evidence[1])
        assert torch.equal(frames, want) and not torch.equal(frames, before)
        # tracker and smoother: the picture shows the steady poses
        model.smoother = PoseSmoother(model.tracker)
        frames.copy_(before)
        out, launches = _launches(emu_lib, lambda: model(views=frames, **kw))
        assert len(launches) == len(unset) + 3 and "k_draw_poses" in launches[-1]      # smoother, evidence again, draw
        ev = model.engine.joint_evidence(model.last_smooth[0], out[3], meta, cams, rt)[0]
        assert torch.equal(model.last_overlay_views, ev)
        want = model.overlay.draw(before.clone(), model.last_overlay_views, ids=model.last_tracks[0],
                                  joint_conf=model.last_evidence[1])
        assert torch.equal(frames, want) and not torch.equal(frames, before)
        # the refusals
        frames.copy_(before)
        model.evidence = False
        with pytest.raises(capi.FvpError):
            model(views=frames, **kw)                                              # no evidence
        model.evidence = True
        from faster_voxelpose_amd.dataset.images import ingest_frames
        with pytest.raises(capi.FvpError):
            model(views=ingest_frames(frames, rt, cfg.DATASET.IMAGE_SIZE, _lib=emu_lib), **kw)      # float views
        with pytest.raises(capi.FvpError):
            model(input_heatmaps=out[3], meta=meta, cameras=cams, resize_transform=rt)             # no frames at all
        assert torch.equal(frames, before)
        model.tracker = model.smoother = None
        with pytest.raises(capi.FvpError):
            FV.PipelinedForward(model, depth=1, streams=[None])
