"""fvp_person_rois, fvp_crop_rois and fvp_crop_rois_nv12 of the shipped library on the MI355X: every case of
tests/crop_cases.py against the independent numpy restatement, bit for bit; the tie of every crop to the ingest call with
the derived matrix; the identity; every argument error; PersonCrops eager and under hipGraph capture; model.crops with RGB
and NV12 views, with and without tracker, smoother and overlay; the pipelines' refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

import crop_cases as CC
import fvp_synthetic as FS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TINY_LIMBS = [(0, 1), (1, 2), (2, 3), (3, 4)]            # the tiny configuration has 5 joints: no default skeleton


@pytest.fixture(scope="module")
def lib():
    from faster_voxelpose_amd import _capi as capi
    return capi.load()


def test_library_holds_the_three_exports(lib):
    from faster_voxelpose_amd import _capi as capi
    assert capi.ABI_VERSION >= 16 and lib.fvp_version() == capi.ABI_VERSION
    for name in ("fvp_person_rois", "fvp_crop_rois", "fvp_crop_rois_nv12"):
        assert name in capi.SIGNATURES and hasattr(lib, name)


@pytest.mark.parametrize("name,J", CC.ROI_CASES)
def test_rois_equal_the_yardstick(lib, name, J):
    CC.roi_check(lib, DEV, name, J)


def test_roi_outputs_may_be_null(lib):
    CC.roi_check_null_outputs(lib, DEV)


def test_roi_argument_errors(lib):
    CC.roi_argument_errors(lib, DEV)


@pytest.mark.parametrize("name", CC.CROP_CASES)
def test_crops_equal_the_yardstick(lib, name):
    CC.crop_check(lib, DEV, name)


@pytest.mark.parametrize("name", [n for n in CC.CROP_CASES if "nothing" not in n])
def test_crop_equals_the_ingest_with_the_derived_matrix(lib, name):
    assert CC.crop_check_tie(lib, DEV, name) >= 2


@pytest.mark.parametrize("name", ["rgb_identity", "nv12_709f_identity_planes"])
def test_whole_frame_at_its_own_size_is_the_identity_ingest(lib, name):
    CC.crop_check_identity(lib, DEV, name)


def test_crop_argument_errors(lib):
    CC.crop_argument_errors(lib, DEV)


def _u16(t):
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


def _same(a, b):
    torch.cuda.synchronize()
    return all(torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)
               for x, y in zip(a, b))


@pytest.mark.parametrize("kind", ["rgb", "nv12"])
def test_person_crops_class(kind):
    """__call__ equals the yardstick's bits, fp32 and bf16; captured once into a hipGraph and replayed on other frames and
    other poses in the same memory, the replay's bits are the yardstick's for those; the refusals."""
    from faster_voxelpose_amd import _capi as capi
    from faster_voxelpose_amd.utils.crops import PersonCrops
    J, size = 17, (8, 6)
    kw = dict(size=size, scale=1.5, pad_px=2.0, min_joints=3, conf_min=0.3, swap_rb=kind == "rgb")
    pc, pc16 = PersonCrops(J, **kw), PersonCrops(J, bf16=True, **kw)

    def scene(seed):
        views, ids, conf = CC.person_scene(J, 26, 40, seed)
        case = dict(views=views, ids=ids, conf=conf, mask=(1 << J) - 1, min_joints=3, scale=1.5, pad_px=2.0, aspect=6 / 8,
                    conf_min=0.3)
        rois, count, score, _ = CC.roi_reference(case)
        c = CC._crop(kind, 26, 40, size, CC.N, 31 + seed, swap=kind == "rgb", standard=3, y_pitch=47, uv_pitch=48, split=True,
                     gap=4, rois=rois.reshape(-1, 4))
        return (views, ids, conf), c, (CC.crop_reference(c)[0], rois, count, score)

    def check(got, want, got16):
        torch.cuda.synchronize()
        assert np.array_equal(CC.bits(got[0].cpu().numpy().reshape(-1, 3, 8, 6)), CC.bits(want[0]))
        assert np.array_equal(CC.bits(got[1].cpu().numpy()), CC.bits(want[1]))
        assert np.array_equal(got[2].cpu().numpy(), want[2]) and want[2].any()
        assert np.array_equal(CC.bits(got[3].cpu().numpy()), CC.bits(want[3]))
        assert got16.dtype == torch.bfloat16 and np.array_equal(_u16(got16).reshape(-1, 8, 3, 8), CC.pack_nhwc8(want[0]))

    (views, ids, conf), c, want = scene(3)
    bufs = [torch.from_numpy(b.copy()).to(DEV) for b in c["bufs"]]
    frames = bufs[0].view(CC.B, CC.V, 26, 40, 3) if kind == "rgb" else CC.nv12_frames(c, bufs, (CC.B, CC.V))
    tv, ti, tc = (torch.from_numpy(a).to(DEV) for a in (views, ids, conf))
    check(pc(frames, tv, ids=ti, joint_conf=tc), want, pc16(frames, tv, ids=ti, joint_conf=tc)[0])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = pc(frames, tv, ids=ti, joint_conf=tc)
        got16 = pc16(frames, tv, ids=ti, joint_conf=tc)[0]
    (views2, ids2, conf2), c2, want2 = scene(4)
    for t, b in zip(bufs, c2["bufs"]):
        t.copy_(torch.from_numpy(b))
    tv.copy_(torch.from_numpy(views2))
    ti.copy_(torch.from_numpy(ids2))
    tc.copy_(torch.from_numpy(conf2))
    graph.replay()
    check(got, want2, got16)
    assert not np.array_equal(CC.bits(want2[0]), CC.bits(want[0]))
    with pytest.raises(capi.FvpError):
        pc.rois(tv.cpu())                                                        # host memory
    with pytest.raises(capi.FvpError):
        pc.crop(frames, got[1].cpu())                                            # frames and rois on different devices
    with pytest.raises(capi.FvpError):
        pc.crop(frames, got[1][:, :1].contiguous())                              # V differs


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


@pytest.mark.parametrize("kind", ["rgb", "nv12"])
def test_model_crops_attribute(lib, kind):
    """Tiny configuration through a torch backbone: set, the forward issues two launches more (with a smoother its own, one
    evidence launch shared with the overlay, then the two), the outputs keep their bits and the patches equal a direct call
    on a pristine copy of the frames - also when an overlay paints the frames in the same forward; the refusals."""
    from faster_voxelpose_amd import _capi as capi
    from faster_voxelpose_amd.core.smoothing import PoseSmoother
    from faster_voxelpose_amd.core.tracking import PoseTracker
    from faster_voxelpose_amd.models import faster_voxelpose as FV
    from faster_voxelpose_amd.utils.crops import PersonCrops
    from faster_voxelpose_amd.utils.overlay import PoseOverlay
    cfg = FS.make_cfg("tiny", device=DEV, min_score=-1.0)
    cams, seq = FS.load_cameras("tiny")
    rt = FS.resize_transform(cfg).to(DEV)
    model = FV.get(cfg).to(DEV)
    model.load_state_dict(FS.fill_state_dict(model.state_dict(), seed=7))
    ws, hs = cfg.DATASET.ORI_IMAGE_SIZE
    J, nv = cfg.DATASET.NUM_JOINTS, cfg.DATASET.CAMERA_NUM
    c = CC._crop(kind, hs, ws, (8, 6), 1, 41, standard=1, y_pitch=ws + 7, uv_pitch=ws + 8, split=True, gap=4,
                 rois=[(0.0, 0.0, 1.0, 1.0)] * (2 * nv))
    bufs = [torch.from_numpy(b.copy()).to(DEV) for b in c["bufs"]]
    before = [t.clone() for t in bufs]

    def as_frames(bb):
        return bb[0].view(2, nv, hs, ws, 3) if kind == "rgb" else CC.nv12_frames(c, bb, (2, nv))

    frames = as_frames(bufs)
    meta = {"seq": [seq, seq]}

    class Stub(torch.nn.Module):
        def forward(self, x):
            pooled = torch.nn.functional.avg_pool2d(x, 4).mean(dim=1, keepdim=True)
            return pooled.expand(-1, J, -1, -1).contiguous()

    def direct(px, ids):
        return model.crops(as_frames([b.clone() for b in before]), px, ids=ids, joint_conf=model.last_evidence[1])

    kw = dict(backbone=Stub(), meta=meta, cameras=cams, resize_transform=rt)
    with torch.no_grad():
        model.crops = PersonCrops(cfg, size=(8, 6))
        with pytest.raises(capi.FvpError, match="model.evidence"):
            model(views=frames, **kw)
        model.evidence = True
        with pytest.raises(capi.FvpError, match="camera frames"):
            model(views=torch.zeros(2, nv, 3, cfg.DATASET.IMAGE_SIZE[1], cfg.DATASET.IMAGE_SIZE[0], device=DEV), **kw)
        model.crops = None
        plain = [t.clone() for t in model(views=frames, **kw)[:3]]               # packs the weights, fills the caches
        _, unset = _total_launches(lib, lambda: model(views=frames, **kw))
        assert model.last_crops is None
        model.crops = PersonCrops(cfg, size=(8, 6), min_joints=1)
        out, n = _total_launches(lib, lambda: model(views=frames, **kw))
        assert n == unset + 2
        assert _same(out[:3], plain) and _same(bufs, before)
        assert model.last_crops[0].shape == (2, nv, model.max_people, 3, 8, 6) and bool(model.last_crops[2].any())
        assert _same(model.last_crops, direct(model.last_evidence[0], None))
        model.tracker = PoseTracker(cfg)
        _, n = _total_launches(lib, lambda: model(views=frames, **kw))
        assert n == unset + 3
        assert _same(model.last_crops, direct(model.last_evidence[0], model.last_tracks[0]))
        model.smoother = PoseSmoother(model.tracker)
        model.overlay = PoseOverlay(cfg, limbs=TINY_LIMBS, alpha=0.5, nv12=True)
        out, n = _total_launches(lib, lambda: model(views=frames, **kw))
        assert n == unset + 1 + 1 + 1 + 2 + 1                                    # tracker, smoother, evidence, crops, draw
        ev = model.joint_evidence(model.last_smooth[0], out[3], meta, cams, rt)[0]
        assert torch.equal(model.last_overlay_views, ev) and not _same(bufs, before)      # the frames are painted ...
        assert _same(model.last_crops, direct(ev, model.last_tracks[0]))                  # ... the patches hold clean pixels
        model.tracker = model.smoother = model.overlay = None
        with pytest.raises(capi.FvpError, match="consumer stream"):
            FV.PipelinedForward(model, depth=2)
        with pytest.raises(capi.FvpError, match="consumer stream"):
            FV.GraphedPipeline(model, 2, meta, out[3], cams, rt)
