"""fvp_draw_poses of the shipped library on the MI355X: every case of tests/overlay_cases.py against the independent integer
restatement of the definition, the whole frame byte for byte; then PoseOverlay.draw under hipGraph capture, model.overlay
with tracker and with tracker + smoother, the forward with the attribute unset, and the refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

import fvp_synthetic as FS
import overlay_cases as OC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TINY_LIMBS = [(0, 1), (1, 2), (2, 3), (3, 4)]            # the tiny configuration has 5 joints: no default skeleton


@pytest.fixture(scope="module")
def lib():
    from faster_voxelpose_amd import _capi as capi
    return capi.load()


@pytest.mark.parametrize("name", list(OC.CASES))
def test_equals_the_yardstick(lib, name):
    OC.check_case(lib, DEV, name)


def test_argument_errors(lib):
    OC.case_argument_errors(lib, DEV)


def test_draw_under_graph_capture():
    """PoseOverlay.draw captured once (limbs and palette are baked into the launch by value), replayed onto a restored
    frame: equals the eager call and the yardstick."""
    from faster_voxelpose_amd.utils.overlay import PoseOverlay
    case, _ = OC.expected("crowd")
    case = dict(case, palette=OC.PAL3)
    ov = PoseOverlay(17, joint_radius=2.5, limb_width=2.5, alpha=0.625, conf_min=0.2, palette=OC.PAL3)
    clean = torch.from_numpy(case["frames"].copy()).to(DEV)
    views, ids, conf = (torch.from_numpy(case[k]).to(DEV) for k in ("views", "ids", "conf"))
    eager = ov.draw(clean.clone(), views, ids=ids, joint_conf=conf)
    torch.cuda.synchronize()
    assert np.array_equal(eager.cpu().numpy(), OC.reference(case))
    static = clean.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ov.draw(static, views, ids=ids, joint_conf=conf)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    static.copy_(clean)
    with torch.cuda.graph(graph):
        ov.draw(static, views, ids=ids, joint_conf=conf)
    for _ in range(2):
        static.copy_(clean)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(static, eager)


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


def _tiny():
    from faster_voxelpose_amd.models import faster_voxelpose as FV
    cfg = FS.make_cfg("tiny", device=DEV, min_score=-1.0)
    cams, seq = FS.load_cameras("tiny")
    rt = FS.resize_transform(cfg).to(DEV)
    model = FV.get(cfg).to(DEV)
    model.load_state_dict(FS.fill_state_dict(model.state_dict(), seed=7))
    ws, hs = cfg.DATASET.ORI_IMAGE_SIZE
    J = cfg.DATASET.NUM_JOINTS
    g = torch.Generator().manual_seed(5)
    frames = torch.randint(0, 256, (2, cfg.DATASET.CAMERA_NUM, hs, ws, 3), dtype=torch.uint8, generator=g).to(DEV)

    class Stub(torch.nn.Module):
        def forward(self, x):
            pooled = torch.nn.functional.avg_pool2d(x, 4).mean(dim=1, keepdim=True)
            return pooled.expand(-1, J, -1, -1).contiguous()

    return cfg, model, frames, dict(backbone=Stub(), meta={"seq": [seq, seq]}, cameras=cams, resize_transform=rt)


def test_model_overlay_attribute(lib):
    """Tiny configuration, uint8 frames: unset, the frames keep their bits and the forward issues the launches it issued;
    set, the frames after the forward equal draw() applied to a copy taken before with the model's own last_* tensors -
    with a tracker only (one launch more), then with tracker and smoother."""
    from faster_voxelpose_amd.core.smoothing import PoseSmoother
    from faster_voxelpose_amd.core.tracking import PoseTracker
    from faster_voxelpose_amd.utils.overlay import PoseOverlay
    cfg, model, frames, kw = _tiny()
    before = frames.clone()
    with torch.no_grad():
        plain = model(views=frames, **kw)
        assert model.overlay is None and model.last_overlay_views is None
        model.evidence = True
        model.tracker = PoseTracker(cfg)
        _, unset = _total_launches(lib, lambda: model(views=frames, **kw))
        assert torch.equal(frames, before)
        model.tracker.reset()
        model.overlay = PoseOverlay(cfg, limbs=TINY_LIMBS, alpha=0.5)
        out, n = _total_launches(lib, lambda: model(views=frames, **kw))
        assert n == unset + 1
        for a, b in zip(out[:3], plain[:3]):
            assert torch.equal(a, b)
        want = model.overlay.draw(before.clone(), model.last_evidence[0], ids=model.last_tracks[0],
                                  joint_conf=model.last_evidence[1])
        torch.cuda.synchronize()
        assert torch.equal(frames, want) and not torch.equal(frames, before) and model.last_overlay_views is None
        model.smoother = PoseSmoother(model.tracker)
        frames.copy_(before)
        out, n = _total_launches(lib, lambda: model(views=frames, **kw))
        assert n == unset + 3                                                 # smoother, evidence of the steady poses, draw
        ev = model.joint_evidence(model.last_smooth[0], out[3], kw["meta"], kw["cameras"], kw["resize_transform"])[0]
        want = model.overlay.draw(before.clone(), model.last_overlay_views, ids=model.last_tracks[0],
                                  joint_conf=model.last_evidence[1])
        torch.cuda.synchronize()
        assert torch.equal(model.last_overlay_views, ev)
        assert torch.equal(frames, want) and not torch.equal(frames, before)


def test_refusals():
    from faster_voxelpose_amd import _capi as capi
    from faster_voxelpose_amd.dataset.images import Nv12Frames, ingest_frames
    from faster_voxelpose_amd.models.faster_voxelpose import PipelinedForward
    from faster_voxelpose_amd.utils.overlay import PoseOverlay
    cfg, model, frames, kw = _tiny()
    before = frames.clone()
    model.overlay = PoseOverlay(cfg, limbs=TINY_LIMBS)
    B, V, hs, ws = frames.shape[:4]
    nv12 = Nv12Frames(torch.zeros((B, V, hs, ws), dtype=torch.uint8, device=DEV),
                      torch.zeros((B, V, hs // 2, ws // 2, 2), dtype=torch.uint8, device=DEV))
    with torch.no_grad():
        with pytest.raises(capi.FvpError):
            model(views=frames, **kw)                                             # no evidence
        model.evidence = True
        with pytest.raises(capi.FvpError):
            model(views=ingest_frames(frames, kw["resize_transform"], cfg.DATASET.IMAGE_SIZE), **kw)      # float views
        with pytest.raises(capi.FvpError):
            model(views=nv12, **kw)                                               # NV12 surfaces
        with pytest.raises(capi.FvpError):
            PipelinedForward(model, depth=2)                                      # pipelines
        with pytest.raises(capi.FvpError):
            model.overlay.draw(frames.cpu(), torch.zeros((B, V, 1, cfg.DATASET.NUM_JOINTS, 4)))          # host tensors
    torch.cuda.synchronize()
    assert torch.equal(frames, before)
