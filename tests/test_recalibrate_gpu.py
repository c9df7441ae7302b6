"""fvp_camera_refit_accumulate / fvp_camera_refit_solve of the shipped library on the MI355X: every scene of
tests/recalibrate_cases.py against the independent numpy restatement of the header's definition - accumulators, corrected
cameras, statistics and states bit for bit, guard elements around every buffer; decay across two calls; every argument error
with nothing written; NULL outputs; three rounds against the truth; CameraRefiner eager and under hipGraph capture;
model.recalibrator set and unset; GraphedForward; the pipelines' refusal."""
import ctypes as C

import numpy as np
import pytest
import torch

import recalibrate_cases as RC
from cases import make_inputs, make_weights

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def lib():
    from faster_voxelpose_amd import _capi as capi
    return capi.load()


def test_library_holds_the_exports(lib):
    from faster_voxelpose_amd import _capi as capi
    assert capi.ABI_VERSION >= 19 and lib.fvp_version() == capi.ABI_VERSION
    for name in ("fvp_camera_refit_accumulate", "fvp_camera_refit_solve"):
        assert name in capi.SIGNATURES and hasattr(lib, name)


@pytest.mark.parametrize("name", RC.CASES)
def test_outputs_equal_the_yardstick(lib, name):
    RC.check(lib, DEV, name)


def test_decay_across_two_calls(lib):
    RC.check_decay(lib, DEV)


def test_read_fence(lib):
    RC.check_fence(lib, DEV)


def test_outputs_may_be_null(lib):
    RC.check_null_outputs(lib, DEV)


def test_argument_errors_write_nothing(lib):
    RC.argument_errors(lib, DEV)


def test_three_rounds_against_the_truth(lib):
    """As on the emulator: the card's cameras within 2 x the figures of tests/golden/refit_floor.json of the truth."""
    RC.check_floor(lib, DEV)


def _same(a, b):
    torch.cuda.synchronize()
    return all(torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)
               for x, y in zip(a, b))


def test_camera_refiner_class():
    """accumulate + solve equal the yardstick's bits; refine equals the yardstick's rounds; one reset-accumulate-solve round
    captured into a hipGraph and replayed on another scene in the same memory gives the yardstick's bits for that scene; host
    memory is refused."""
    from faster_voxelpose_amd import _capi as capi
    case, want = RC.get("random_v5_j7")
    other = RC.random_scene(5, 7, 53, B=5)
    ref = RC.refiner_for(case, decay=1.0)
    t = RC.tensors(case, DEV)
    args = [t[k] for k in RC.TENSORS]
    acc = ref.accumulate(*args)
    out = ref.solve(t["cams"])
    torch.cuda.synchronize()
    RC.assert_equal(dict(RC.as_dict(out), acc=acc.cpu().numpy()), want, "eager")
    got = RC.as_dict(ref.refine(*args, iters=3))
    RC.assert_equal(got, RC.ref_refine(case, 3), "refine", keys=RC.SOLVE_OUTPUTS)
    ref.reset()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ref.reset()
        ref.accumulate(*args)
        out = ref.solve(t["cams"])
    for k in RC.TENSORS:
        t[k].copy_(torch.from_numpy(other[k]))
    graph.replay()
    torch.cuda.synchronize()
    want2 = RC.reference(other)
    RC.assert_equal(dict(RC.as_dict(out), acc=ref.acc.cpu().numpy()), want2, "replay", keys=("acc",) + RC.SOLVE_OUTPUTS)
    assert RC.differs(want2, want)
    with pytest.raises(capi.FvpError):
        ref.accumulate(*[RC.tensors(case, "cpu")[k] for k in RC.TENSORS])        # host memory
    with pytest.raises(capi.FvpError):
        ref.accumulate(t["points"], t["obs"], t["view_state"], t["cams"].cpu(), t["frame_set"])   # tables on another device


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


def _model():
    from faster_voxelpose_amd.models import faster_voxelpose as FV
    from faster_voxelpose_amd.utils.triangulate import JointTriangulator
    name = "tiny_g_b2_all"
    cfg, cams, seq, rt, heat, meta, _ = make_inputs(name, device=DEV)
    model = FV.get(cfg).to(DEV)
    model.load_state_dict(make_weights(name, model.state_dict()))
    rt, heat = rt.to(DEV), heat.to(DEV)
    model.triangulator = JointTriangulator(cfg, radius=8, min_peak=0.0)          # 30 used joint-views on this input
    return FV, model, cfg, cams, rt, heat, meta


def _forward_case(model, out, points, meta, cams, heat, huber_px):
    tri = model.last_triangulation
    fs = model.engine.frame_sets(meta, cams, heat.shape[1])
    torch.cuda.synchronize()
    return dict(points=(out[0] if points == "fused" else tri[0]).cpu().numpy(), obs=tri[3].cpu().numpy(),
                view_state=tri[4].cpu().numpy(), cams=model.engine.geo.cams.cpu().numpy(), frame_set=fs.cpu().numpy(),
                params=dict(huber_px=huber_px))


def test_model_recalibrator_attribute(lib):
    """Tiny configuration: unset, the forward issues the launches it issued; set, exactly one more; the returned tuple keeps
    its bits; the accumulators equal the yardstick on the forward's own tensors (fused and triangulated joints); the
    refusals."""
    from faster_voxelpose_amd import _capi as capi
    from faster_voxelpose_amd.utils.recalibrate import CameraRefiner
    FV, model, cfg, cams, rt, heat, meta = _model()
    kw = dict(meta=meta, input_heatmaps=heat, cameras=cams, resize_transform=rt)
    with torch.no_grad():
        model.evidence = True
        plain = [t.clone() for t in model(**kw)[:3]]                                 # packs the weights, fills the caches
        _, unset = _total_launches(lib, lambda: model(**kw))
        for points in ("fused", "tri"):
            model.recalibrator = CameraRefiner(cfg, huber_px=4.0)
            model.recalibrator_points = points
            out, n = _total_launches(lib, lambda: model(**kw))
            assert n == unset + 1 and _same(out[:3], plain)
            case = _forward_case(model, out, points, meta, cams, heat, 4.0)
            want = RC.ref_accumulate(case)
            RC.assert_equal(dict(acc=model.recalibrator.acc.cpu().numpy()), dict(acc=want), points)
            assert (want[..., 29] > 0).any()
        model.recalibrator = None
        _, n = _total_launches(lib, lambda: model(**kw))
        assert n == unset
        model.recalibrator = CameraRefiner(cfg)
        with pytest.raises(capi.FvpError, match="consumer stream"):
            FV.PipelinedForward(model, depth=2)
        with pytest.raises(capi.FvpError, match="consumer stream"):
            FV.GraphedPipeline(model, 2, meta, heat, cams, rt)
        model.triangulator = None
        with pytest.raises(capi.FvpError, match="model.triangulator"):
            model(**kw)


def test_graphed_forward_with_recalibrator():
    """One capture; after reset() two replays with different inputs leave the accumulators the yardstick gives for the two
    eager forwards' tensors, one on top of the other."""
    import fvp_synthetic as S
    from faster_voxelpose_amd.utils.recalibrate import CameraRefiner
    FV, model, cfg, cams, rt, heat, meta = _model()
    inputs = [S.heatmaps_blobs(cfg, cams, meta["seq"][0], heat.shape[0], people=2, seed=s).to(DEV) for s in (21, 22)]
    model.recalibrator = CameraRefiner(cfg, huber_px=4.0)
    gf = FV.GraphedForward(model, meta, heat, cams, rt)
    model.recalibrator.reset()
    for x in inputs:
        gf(x)
    torch.cuda.synchronize()
    got = model.recalibrator.acc.cpu().numpy().copy()
    model.recalibrator = None
    want = None
    with torch.no_grad():
        for x in inputs:
            out = model(meta=meta, input_heatmaps=x, cameras=cams, resize_transform=rt)
            want = RC.ref_accumulate(_forward_case(model, out, "fused", meta, cams, heat, 4.0), acc=want)
    RC.assert_equal(dict(acc=got), dict(acc=want), "two replays")
    assert (want[..., 29] > 0).any()
