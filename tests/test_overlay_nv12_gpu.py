"""fvp_draw_poses_nv12 of the shipped library on the MI355X: every case of tests/overlay_nv12_cases.py against the
independent integer restatement of the definition, whole allocations byte for byte, one launch per case; the tie to
fvp_draw_poses; the colours of the four standards; the round trip through fvp_ingest_nv12; every argument error;
PoseOverlay.draw on Nv12Frames (eager and under hipGraph capture) and model.overlay with NV12 views."""
import ctypes as C

import numpy as np
import pytest
import torch

import fvp_synthetic as FS
import overlay_nv12_cases as NC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TINY_LIMBS = [(0, 1), (1, 2), (2, 3), (3, 4)]            # the tiny configuration has 5 joints: no default skeleton


@pytest.fixture(scope="module")
def lib():
    from faster_voxelpose_amd import _capi as capi
    return capi.load()


@pytest.mark.parametrize("name", list(NC.CASES))
def test_equals_the_yardstick(lib, name):
    NC.check_case(lib, DEV, name)


@pytest.mark.parametrize("name", NC.TIE_CASES)
def test_luma_equals_the_rgb_kernel(lib, name):
    NC.check_tie_to_rgb(lib, DEV, name)


def test_layouts_hold_the_same_planes(lib):
    NC.check_layouts_agree(lib, DEV)


@pytest.mark.parametrize("standard", sorted(NC.STANDARDS))
def test_colours_of_the_standard(lib, standard):
    NC.check_colours(lib, DEV, standard)


@pytest.mark.parametrize("standard", sorted(NC.STANDARDS))
def test_round_trip_through_the_ingest(lib, standard):
    NC.check_round_trip(lib, DEV, standard)


def test_argument_errors(lib):
    NC.case_argument_errors(lib, DEV)


def _on_device(surface):
    bufs = [torch.from_numpy(b.copy()).to(DEV) for b in surface.bufs]
    return bufs, NC.nv12_frames(surface, bufs)


def test_pose_overlay_class_on_nv12():
    """draw() on an Nv12Frames equals the C call (the yardstick's bytes) and returns the object - padded planes and a
    from_buffer surface; captured once into a hipGraph and replayed onto the restored surface, the same bytes; the
    refusals leave the surface alone."""
    from faster_voxelpose_amd import _capi as capi
    from faster_voxelpose_amd.dataset.images import Nv12Frames
    from faster_voxelpose_amd.utils.overlay import PoseOverlay
    for name in ("layout_planes", "layout_contiguous"):
        case, want, _ = NC.expected(name)
        s = case["surface"]
        ov = PoseOverlay(17, joint_radius=2.5, limb_width=2.5, alpha=0.625, conf_min=0.2, palette=case["palette"])
        bufs, fr = _on_device(s)
        views, ids, conf = (torch.from_numpy(case[k]).to(DEV) for k in ("views", "ids", "conf"))
        out = ov.draw(fr, views, ids=ids, joint_conf=conf)
        torch.cuda.synchronize()
        assert out is fr and all(np.array_equal(t.cpu().numpy(), w) for t, w in zip(bufs, want))
    clean = [torch.from_numpy(b.copy()).to(DEV) for b in s.bufs]
    graph = torch.cuda.CUDAGraph()
    for t, c in zip(bufs, clean):
        t.copy_(c)
    with torch.cuda.graph(graph):
        ov.draw(fr, views, ids=ids, joint_conf=conf)
    for t, c in zip(bufs, clean):
        t.copy_(c)
    graph.replay()
    torch.cuda.synchronize()
    assert all(np.array_equal(t.cpu().numpy(), w) for t, w in zip(bufs, want))
    before = [t.clone() for t in bufs]
    with pytest.raises(capi.FvpError):
        ov.draw(Nv12Frames(fr.y[0], fr.uv[0], "bt709", True), views, ids=ids, joint_conf=conf)      # leading dimensions [V]
    with pytest.raises(capi.FvpError):
        ov.draw(fr, views.cpu(), ids=ids, joint_conf=conf)                       # planes and views on different devices
    host = [t.cpu() for t in bufs]
    with pytest.raises(capi.FvpError):
        ov.draw(NC.nv12_frames(s, host), views.cpu())                            # a surface in host memory
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(bufs, before))


def _total_launches(lib, run):
    """Launches of every kernel class made by ``run()`` (the per-launch profiler, fvp_prof_enable(2))."""
    from faster_voxelpose_amd import _capi as capi
    lib.fvp_prof_reset()
    lib.fvp_prof_enable(2)
    try:
        out = run()
        torch.cuda.synchronize()
        total = 0
        for cls in range(capi.K_COUNT):
            ms, n, fl = C.c_double(), C.c_int64(), C.c_double()
            lib.fvp_prof_read(cls, C.byref(ms), C.byref(n), C.byref(fl))
            total += int(n.value)
    finally:
        lib.fvp_prof_enable(0)
        lib.fvp_prof_reset()
    return out, total


def test_model_overlay_attribute_on_nv12(lib):
    """Tiny configuration, Nv12Frames views through a torch backbone: a default overlay still refuses them; built with
    nv12=True the outputs equal the plain forward's, the forward issues one launch more (three with a smoother) and the
    surface equals draw() applied to a clone taken before; unset, the surface keeps its bits."""
    from faster_voxelpose_amd import _capi as capi
    from faster_voxelpose_amd.core.smoothing import PoseSmoother
    from faster_voxelpose_amd.core.tracking import PoseTracker
    from faster_voxelpose_amd.models import faster_voxelpose as FV
    from faster_voxelpose_amd.utils.overlay import PoseOverlay
    cfg = FS.make_cfg("tiny", device=DEV, min_score=-1.0)
    cams, seq = FS.load_cameras("tiny")
    rt = FS.resize_transform(cfg).to(DEV)
    model = FV.get(cfg).to(DEV)
    model.load_state_dict(FS.fill_state_dict(model.state_dict(), seed=7))
    ws, hs = cfg.DATASET.ORI_IMAGE_SIZE
    J, V = cfg.DATASET.NUM_JOINTS, cfg.DATASET.CAMERA_NUM
    s = NC.Surface(2, V, hs, ws, standard=1, seed=70)
    bufs, frames = _on_device(s)
    before = [t.clone() for t in bufs]

    class Stub(torch.nn.Module):
        def forward(self, x):
            pooled = torch.nn.functional.avg_pool2d(x, 4).mean(dim=1, keepdim=True)
            return pooled.expand(-1, J, -1, -1).contiguous()

    def same(a, b):
        torch.cuda.synchronize()
        return all(torch.equal(x, y) for x, y in zip(a, b))

    def drawn_on_a_clone(ov, px):
        clone = [b.clone() for b in before]
        ov.draw(NC.nv12_frames(s, clone), px, ids=model.last_tracks[0], joint_conf=model.last_evidence[1])
        return clone

    kw = dict(backbone=Stub(), meta={"seq": [seq, seq]}, cameras=cams, resize_transform=rt)
    with torch.no_grad():
        plain = [t.clone() for t in model(views=frames, **kw)[:3]]
        model.evidence = True
        model.tracker = PoseTracker(cfg)
        _, unset = _total_launches(lib, lambda: model(views=frames, **kw))
        assert same(bufs, before)                                              # overlay unset: the surface keeps its bits
        model.tracker.reset()
        model.overlay = PoseOverlay(cfg, limbs=TINY_LIMBS, alpha=0.5)
        with pytest.raises(capi.FvpError):
            model(views=frames, **kw)                                          # the default overlay refuses NV12 views
        assert same(bufs, before)
        model.tracker.reset()
        model.overlay = PoseOverlay(cfg, limbs=TINY_LIMBS, alpha=0.5, nv12=True)
        out, n = _total_launches(lib, lambda: model(views=frames, **kw))
        assert n == unset + 1
        for a, b in zip(out[:3], plain):
            assert torch.equal(a, b)
        assert model.last_overlay_views is None
        assert same(bufs, drawn_on_a_clone(model.overlay, model.last_evidence[0])) and not same(bufs, before)
        model.smoother = PoseSmoother(model.tracker)
        for t, b in zip(bufs, before):
            t.copy_(b)
        out, n = _total_launches(lib, lambda: model(views=frames, **kw))
        assert n == unset + 3                                                 # smoother, evidence of the steady poses, draw
        ev = model.joint_evidence(model.last_smooth[0], out[3], kw["meta"], cams, rt)[0]
        assert torch.equal(model.last_overlay_views, ev)
        assert same(bufs, drawn_on_a_clone(model.overlay, model.last_overlay_views)) and not same(bufs, before)
        model.tracker = model.smoother = None
        with pytest.raises(capi.FvpError):
            FV.PipelinedForward(model, depth=2)                                # the pipelines keep refusing an overlay
