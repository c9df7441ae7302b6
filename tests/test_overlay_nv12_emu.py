"""fvp_draw_poses_nv12 on the CPU emulation of the kernels (tests/hipemu): every case of tests/overlay_nv12_cases.py against
the independent integer restatement of the definition, whole allocations byte for byte; the tie to fvp_draw_poses; the
colours of all four standards and the header's constants; the round trip through fvp_ingest_nv12; the read fence; the case
set against seven mutated yardsticks; every argument error; PoseOverlay on Nv12Frames and model.overlay."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import fvp_synthetic as FS
import overlay_cases as OC
import overlay_nv12_cases as NC
from faster_voxelpose_amd import _capi as capi
from faster_voxelpose_amd.core.smoothing import PoseSmoother
from faster_voxelpose_amd.core.tracking import PoseTracker
from faster_voxelpose_amd.models import faster_voxelpose as FV
from faster_voxelpose_amd.utils.overlay import PALETTE, PoseOverlay

TINY_LIMBS = [(0, 1), (1, 2), (2, 3), (3, 4)]            # the tiny configuration has 5 joints: no default skeleton
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", list(NC.CASES))
def test_equals_the_yardstick(emu_lib, name):
    NC.check_case(emu_lib, "cpu", name)


@pytest.mark.parametrize("name", NC.TIE_CASES)
def test_luma_equals_the_rgb_kernel(emu_lib, name):
    NC.check_tie_to_rgb(emu_lib, "cpu", name)


@pytest.mark.parametrize("standard", sorted(NC.STANDARDS))
def test_colours_of_the_standard(emu_lib, standard):
    NC.check_colours(emu_lib, "cpu", standard)


def test_header_constants_and_the_clip():
    """The twelve #defines per standard equal round(k * 2^16) of the float64 values; over all 2^24 colours the limited
    ranges stay inside 16..235 / 16..240 without the clip, full range reaches 256 on U (pure blue) and V (pure red)."""
    assert tuple(PALETTE) == tuple(NC.PALETTE16)
    text = open(os.path.join(ROOT, "include", "fvp.h")).read()
    seen = {m.group(1): [int(v) for v in m.group(2).split(",")]
            for m in re.finditer(r"#define FVP_RGB2YUV_(\w+)_COEFFS \{([^}]*)\}", text)}
    assert sorted(seen) == sorted(NC.STANDARD_NAMES.values())
    r, g, b = np.meshgrid(*[np.arange(256, dtype=np.int64)] * 3, indexing="ij")
    for std, name in NC.STANDARD_NAMES.items():
        k = NC.colour_constants(std)
        assert seen[name] == k and len(k) == 12, name
        lo_hi = [(int(v.min()), int(v.max())) for v in
                 (k[4 * c] + ((k[4 * c + 1] * r + k[4 * c + 2] * g + k[4 * c + 3] * b + 32768) >> 16) for c in range(3))]
        assert lo_hi == ([(0, 255), (1, 256), (1, 256)] if std >= 2 else [(16, 235), (16, 240), (16, 240)]), (name, lo_hi)
    for std in (2, 3):
        assert NC.yuv_of((0, 0, 255), std, clip=False)[1] == 256 and NC.yuv_of((0, 0, 255), std)[1] == 255
        assert NC.yuv_of((255, 0, 0), std, clip=False)[2] == 256 and NC.yuv_of((255, 0, 0), std)[2] == 255


@pytest.mark.parametrize("standard", sorted(NC.STANDARDS))
def test_round_trip_through_the_ingest(emu_lib, standard):
    NC.check_round_trip(emu_lib, "cpu", standard)


@pytest.mark.parametrize("name", ["carried_nothing_drawable", "carried_limb_wholly_outside"])
def test_nothing_drawable_reads_nothing(emu_lib, name):
    """The emulator's read fence over both allocations, padding and gaps included: zero reads."""
    case, want, _ = NC.expected(name)
    got, reads = NC.run(emu_lib, "cpu", case, fences=[[(0, len(b))] for b in case["surface"].bufs])
    assert reads == 0 and all(np.array_equal(g, b) for g, b in zip(got, case["surface"].bufs))


@pytest.mark.parametrize("name", ["chroma_disc_edge", "layout_planes", "layout_contiguous", "carried_capsules"])
def test_reads_exactly_the_covered_bytes(emu_lib, name):
    """A case that draws reads the covered luma bytes, one by one, and one pair per quad with any coverage - nothing else of
    the allocations; and nothing inside pitch padding, frame gaps or the bytes before and behind the planes.  A fence
    counts a read when the four bytes from its address on meet the range: the padding fences begin three bytes in."""
    case, want, counts = NC.expected(name)
    s = case["surface"]
    got, reads = NC.run(emu_lib, "cpu", case, fences=[[(0, len(b))] for b in s.bufs])
    assert all(np.array_equal(g, w) for g, w in zip(got, want))
    assert reads == counts["luma"] + counts["quads"] and counts["quads"] > 0
    pads = [[(a + 3, e) for a, e in ranges if e - a > 3] for ranges in s.padding()]
    assert sum(len(p) for p in pads) >= s.B * s.V * s.Hs                  # every luma row has its padding fenced
    got, reads = NC.run(emu_lib, "cpu", case, fences=pads)
    assert reads == 0 and all(np.array_equal(g, w) for g, w in zip(got, want))


def test_layouts_hold_the_same_planes(emu_lib):
    """A contiguous from_buffer surface and separately allocated, padded planes with the same contents: the same planes
    afterwards."""
    NC.check_layouts_agree(emu_lib, "cpu")
    ca = NC.expected("layout_planes")[0]
    assert ca["surface"].y_pitch % 2 == 1 and ca["surface"].uv_pitch % 2 == 0 and ca["surface"].y[1] % 2 == 1


def test_argument_errors(emu_lib):
    NC.case_argument_errors(emu_lib, "cpu")


def test_case_set_tells_the_mutants_apart(emu_lib):
    """Each wrong reading of the definition changes the expected bytes of at least one case - and the kernel's bytes there
    are the definition's, not the mutant's; and the named quads of chroma_quads hold what their comments say."""
    first = {"chroma_all_or_nothing": "chroma_quads_256", "chroma_per_pixel": "chroma_quads_128",
             "chroma_top_left": "chroma_quads_256", "uv_swapped": "chroma_quads_256", "descending": "chroma_two_persons",
             "no_half": "chroma_quads_128", "shift8": "chroma_quads_128"}
    assert set(first) == set(NC.MUTANTS)
    for mut in NC.MUTANTS:
        case, want, _ = NC.expected(first[mut])
        got = NC.reference(case, mut)
        assert any(not np.array_equal(g, w) for g, w in zip(got, want)), f"no case tells the mutant {mut!r} from the definition"
        assert all(np.array_equal(g, w) for g, w in zip(NC.run(emu_lib, "cpu", case), want)), mut
    for mut in ("chroma_all_or_nothing", "chroma_top_left", "descending"):      # the disc edge tells them too
        case, want, _ = NC.expected("chroma_disc_edge" if mut != "descending" else "carried_blend_128")
        assert any(not np.array_equal(g, w) for g, w in zip(NC.reference(case, mut), want)), mut
    for alpha in (256, 128):
        case, want, _ = NC.expected(f"chroma_quads_{alpha}")
        s = case["surface"]
        Y0, U0 = s.planes(s.bufs)
        Y1, U1 = s.planes(want)
        uc, vc = NC.yuv_of(case["palette"][0], s.standard)[1:]
        for k, (cy, cx) in NC.QUADS.items():
            assert int((Y1[0, 0, 2 * cy:2 * cy + 2, 2 * cx:2 * cx + 2] != Y0[0, 0, 2 * cy:2 * cy + 2, 2 * cx:2 * cx + 2]).sum()) <= k
            a = alpha * k
            assert tuple(U1[0, 0, cy, cx]) == tuple((c * a + int(o) * (1024 - a) + 512) >> 10 for c, o in zip((uc, vc), U0[0, 0, cy, cx]))
        if alpha == 256:
            assert tuple(U1[0, 0, 5, 25]) == (uc, vc)                            # k = 4, opaque: the colour itself
        cov = NC.coverage(case, 0, 0, 0)
        assert (11, 11) in cov and (10, 10) not in cov                           # k = 1: not the quad's top-left pixel
        assert not np.array_equal(U1[0, 0, 10, 35], U0[0, 0, 10, 35])             # person 1's quad, its top-right pixel
    case, want, _ = NC.expected("chroma_two_persons")
    k0, k1 = ([len([p for p in NC.coverage(case, 0, 0, n) if (p[0] >> 1, p[1] >> 1) == q]) for q in ((5, 15), (10, 30))]
              for n in (0, 1))
    assert (k0, k1) == ([1, 3], [3, 1])


def test_pose_overlay_class_on_nv12(emu_lib):
    """draw() on an Nv12Frames equals the C call (the yardstick's bytes) and returns the object, for padded planes and for
    a from_buffer surface; the refusals."""
    for name in ("layout_planes", "layout_contiguous"):
        case, want, _ = NC.expected(name)
        s = case["surface"]
        ov = PoseOverlay(17, joint_radius=2.5, limb_width=2.5, alpha=0.625, conf_min=0.2, palette=case["palette"], _lib=emu_lib)
        assert (ov.joint_radius_q4, ov.limb_half_q4, ov.alpha, ov.nv12) == (case["R"], case["W"], case["alpha"], False)
        bufs = [torch.from_numpy(b.copy()) for b in s.bufs]
        fr = NC.nv12_frames(s, bufs)
        assert (fr.y_pitch, fr.uv_pitch, fr.y_frame_stride, fr.uv_frame_stride, fr.standard) == \
            (s.y_pitch, s.uv_pitch, s.y_fs, s.uv_fs, s.standard)
        views, ids, conf = (torch.from_numpy(case[k]) for k in ("views", "ids", "conf"))
        out = ov.draw(fr, views, ids=ids, joint_conf=conf)
        assert out is fr and all(np.array_equal(t.numpy(), w) for t, w in zip(bufs, want))
    assert PoseOverlay(17, nv12=True, _lib=emu_lib).nv12 is True
    before = [t.clone() for t in bufs]
    from faster_voxelpose_amd.dataset.images import Nv12Frames
    flat = Nv12Frames(fr.y[0], fr.uv[0], "bt709", True)                          # leading dimensions [V] only
    with pytest.raises(capi.FvpError):
        ov.draw(flat, views, ids=ids, joint_conf=conf)
    with pytest.raises(capi.FvpError):
        ov.draw(fr, views[:, :1].contiguous(), ids=ids, joint_conf=conf)         # V differs
    with pytest.raises(capi.FvpError):
        ov.draw(fr, views.to("meta"), ids=ids, joint_conf=conf)                  # planes and views on different devices
    with pytest.raises(capi.FvpError):
        PoseOverlay(17, palette=case["palette"]).draw(fr, views)                 # the product: a CPU surface is refused
    assert all(torch.equal(a, b) for a, b in zip(bufs, before))


def _launches(lib, fn):
    lib.hipemu_launch_log.restype = C.c_char_p
    lib.hipemu_launch_log_reset()
    out = fn()
    return out, lib.hipemu_launch_log().decode().split()


def test_model_overlay_attribute_on_nv12(emu_lib):
    """model.overlay on the tiny configuration with Nv12Frames views through a torch backbone: a default overlay still
    refuses them; built with nv12=True, the outputs equal the plain forward's, the forward issues one launch more (three
    with a smoother) and the surface equals draw() applied to a clone taken before; unset, the surface keeps its bits."""
    cfg = FS.make_cfg("tiny", device="cpu", min_score=-1.0)
    cams, seq = FS.load_cameras("tiny")
    rt = FS.resize_transform(cfg)
    model = FV.FasterVoxelPoseNet(cfg, _lib=emu_lib)
    model.load_state_dict(FS.fill_state_dict(model.state_dict(), seed=7))
    ws, hs = cfg.DATASET.ORI_IMAGE_SIZE
    J, V = cfg.DATASET.NUM_JOINTS, cfg.DATASET.CAMERA_NUM
    s = NC.Surface(2, V, hs, ws, standard=1, seed=70)
    bufs = [torch.from_numpy(b.copy()) for b in s.bufs]
    before = [t.clone() for t in bufs]
    frames = NC.nv12_frames(s, bufs)
    meta = {"seq": [seq, seq]}

    class Stub(torch.nn.Module):
        def forward(self, x):
            pooled = torch.nn.functional.avg_pool2d(x, 4).mean(dim=1, keepdim=True)
            return pooled.expand(-1, J, -1, -1).contiguous()

    def same(a, b):
        return all(torch.equal(x, y) for x, y in zip(a, b))

    def restore():
        for t, b in zip(bufs, before):
            t.copy_(b)

    def drawn_on_a_clone(ov, px):
        clone = [b.clone() for b in before]
        ov.draw(NC.nv12_frames(s, clone), px, ids=model.last_tracks[0], joint_conf=model.last_evidence[1])
        return clone

    kw = dict(backbone=Stub(), meta=meta, cameras=cams, resize_transform=rt)
    with torch.no_grad():
        plain, parent = _launches(emu_lib, lambda: model(views=frames, **kw))
        assert same(bufs, before) and not any("k_draw_poses" in k for k in parent)
        model.evidence = True
        model.tracker = PoseTracker(cfg, _lib=emu_lib)
        _, unset = _launches(emu_lib, lambda: model(views=frames, **kw))
        assert same(bufs, before)                                              # overlay unset: the surface keeps its bits
        model.tracker.reset()
        model.overlay = PoseOverlay(cfg, limbs=TINY_LIMBS, alpha=0.5, _lib=emu_lib)
        with pytest.raises(capi.FvpError):
            model(views=frames, **kw)                                          # the default overlay refuses NV12 views
        assert same(bufs, before)
        model.tracker.reset()
        model.overlay = PoseOverlay(cfg, limbs=TINY_LIMBS, alpha=0.5, nv12=True, _lib=emu_lib)
        out, with_overlay = _launches(emu_lib, lambda: model(views=frames, **kw))
        assert with_overlay[:-1] == unset and "k_draw_poses_nv12" in with_overlay[-1]      # one launch more, behind the rest
        for a, b in zip(out[:3], plain[:3]):
            assert torch.equal(a, b)
        assert model.last_overlay_views is None
        assert same(bufs, drawn_on_a_clone(model.overlay, model.last_evidence[0])) and not same(bufs, before)
        # tracker and smoother: the picture shows the steady poses
        model.smoother = PoseSmoother(model.tracker)
        restore()
        out, launches = _launches(emu_lib, lambda: model(views=frames, **kw))
        assert len(launches) == len(unset) + 3 and "k_draw_poses_nv12" in launches[-1]     # smoother, evidence again, draw
        ev = model.engine.joint_evidence(model.last_smooth[0], out[3], meta, cams, rt)[0]
        assert torch.equal(model.last_overlay_views, ev)
        assert same(bufs, drawn_on_a_clone(model.overlay, model.last_overlay_views)) and not same(bufs, before)
        # uint8 RGB frames still go to fvp_draw_poses with an nv12=True overlay; the pipelines keep refusing an overlay
        rgb = torch.randint(0, 256, (2, V, hs, ws, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(5))
        _, launches = _launches(emu_lib, lambda: model(views=rgb, **kw))
        assert "k_draw_poses" in launches[-1] and "k_draw_poses_nv12" not in launches[-1]
        model.tracker = model.smoother = None
        with pytest.raises(capi.FvpError):
            FV.PipelinedForward(model, depth=1, streams=[None])
