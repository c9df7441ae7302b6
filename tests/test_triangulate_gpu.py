"""fvp_triangulate_joints of the shipped library on the MI355X: every scene of tests/triangulate_cases.py against the
independent numpy restatement of the header's definition, all seven outputs bit for bit; the read fence; every argument error
with nothing written; every combination of NULL outputs; the definition against the truth; JointTriangulator eager and under
hipGraph capture; model.triangulator set and unset; the pipelines' refusal."""
import ctypes as C

import numpy as np
import pytest
import torch

import triangulate_cases as TC
from cases import make_inputs, make_weights

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def lib():
    from faster_voxelpose_amd import _capi as capi
    return capi.load()


def test_library_holds_the_export(lib):
    from faster_voxelpose_amd import _capi as capi
    assert capi.ABI_VERSION >= 18 and lib.fvp_version() == capi.ABI_VERSION
    assert "fvp_triangulate_joints" in capi.SIGNATURES and hasattr(lib, "fvp_triangulate_joints")


@pytest.mark.parametrize("name", TC.CASES)
def test_outputs_equal_the_yardstick(lib, name):
    TC.check(lib, DEV, name)


def test_read_fence(lib):
    TC.check_fence(lib, DEV)


def test_outputs_may_be_null(lib):
    TC.check_null_outputs(lib, DEV)


def test_argument_errors_write_nothing(lib):
    TC.argument_errors(lib, DEV)


def test_definition_against_the_truth(lib):
    """As on the emulator: the card's X within 2 x ((a) + (b)) of tests/golden/triangulate_floor.json of the truth."""
    TC.check_floor(lib, DEV)


def _same(a, b):
    torch.cuda.synchronize()
    return all(torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)
               for x, y in zip(a, b))


def test_joint_triangulator_class():
    """__call__ equals the yardstick's bits; captured once into a hipGraph and replayed on another scene in the same memory,
    the replay's bits are the yardstick's for that scene; host memory is refused."""
    from faster_voxelpose_amd import _capi as capi
    case, want = TC.get("random_v5_j5")
    other = TC.random_scene(5, 5, 23, B=3)
    tri = TC.triangulator_for(case)
    t = TC.tensors(case, DEV)
    got = TC.run_class(tri, t)
    torch.cuda.synchronize()
    TC.assert_equal(TC.as_dict(got), want, "eager")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = TC.run_class(tri, t)
    for k in TC.KEYS:
        t[k].copy_(torch.from_numpy(other[k]))
    graph.replay()
    torch.cuda.synchronize()
    want2 = TC.reference(other)
    TC.assert_equal(TC.as_dict(got), want2, "replay")
    assert TC.differs(want2, want)
    with pytest.raises(capi.FvpError):
        TC.run_class(tri, TC.tensors(case, "cpu"))                               # host memory
    with pytest.raises(capi.FvpError):
        tri(t["poses"], t["cams"].cpu(), t["frame_set"], t["heat"])              # tables on another device


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


def test_model_triangulator_attribute(lib):
    """Tiny configuration: unset, the forward issues the launches it issued; set, two more (one without per_camera); the
    returned tuple keeps its bits; last_triangulation equals the yardstick, with the occluder table when model.visibility is
    set; the refusals."""
    from faster_voxelpose_amd import _capi as capi
    from faster_voxelpose_amd.models import faster_voxelpose as FV
    from faster_voxelpose_amd.utils.triangulate import JointTriangulator
    from faster_voxelpose_amd.utils.visibility import JointVisibility
    name = "tiny_g_b2_all"
    cfg, cams, seq, rt, heat, meta, _ = make_inputs(name, device=DEV)
    model = FV.get(cfg).to(DEV)
    model.load_state_dict(make_weights(name, model.state_dict()))
    rt, heat = rt.to(DEV), heat.to(DEV)
    kw = dict(meta=meta, input_heatmaps=heat, cameras=cams, resize_transform=rt)
    with torch.no_grad():
        model.evidence = True
        plain = [t.clone() for t in model(**kw)[:3]]                                 # packs the weights, fills the caches
        _, unset = _total_launches(lib, lambda: model(**kw))
        assert model.last_triangulation is None
        model.triangulator = JointTriangulator(cfg, radius=4, reject_px=6.0, per_camera=False)
        out, n = _total_launches(lib, lambda: model(**kw))
        assert n == unset + 1 and _same(out[:3], plain) and model.last_triangulation[5] is None
        model.triangulator = JointTriangulator(cfg, radius=4, reject_px=6.0)
        out, n = _total_launches(lib, lambda: model(**kw))
        assert n == unset + 2 and _same(out[:3], plain)
        got = TC.as_dict(model.last_triangulation)
        TC.assert_equal(got, TC.reference(TC.model_case(model, cfg, rt, heat, meta, cams, out)), "model.last_triangulation")
        assert (got["tri_count"] != -2).any() and (got["view_state"] != TC.NOT_EVALUATED).any()
        model.visibility = JointVisibility(cfg, prims=[(0, 1), (1, 2), (2, 3), (3, 4)], radius=80.0)
        out, n = _total_launches(lib, lambda: model(**kw))
        assert n == unset + 3 and _same(out[:3], plain)
        want = TC.reference(TC.model_case(model, cfg, rt, heat, meta, cams, out, occluder=model.last_visibility[0]))
        TC.assert_equal(TC.as_dict(model.last_triangulation), want, "with the occluder table")
        model.visibility = None
        with pytest.raises(capi.FvpError, match="consumer stream"):
            FV.PipelinedForward(model, depth=2)
        with pytest.raises(capi.FvpError, match="consumer stream"):
            FV.GraphedPipeline(model, 2, meta, heat, cams, rt)


def test_graphed_forward_with_triangulator():
    """One capture, two replays with different inputs: last_triangulation holds static tensors whose bits equal the eager
    forwards'."""
    import fvp_synthetic as S
    from faster_voxelpose_amd.models import faster_voxelpose as FV
    from faster_voxelpose_amd.utils.triangulate import JointTriangulator
    name = "tiny_g_b2_all"
    cfg, cams, seq, rt, heat, meta, _ = make_inputs(name, device=DEV)
    model = FV.get(cfg).to(DEV)
    model.load_state_dict(make_weights(name, model.state_dict()))
    rt, heat = rt.to(DEV), heat.to(DEV)
    inputs = [S.heatmaps_blobs(cfg, cams, meta["seq"][0], heat.shape[0], people=2, seed=s).to(DEV) for s in (21, 22)]
    model.triangulator = JointTriangulator(cfg, radius=4)
    gf = FV.GraphedForward(model, meta, heat, cams, rt)
    static = model.last_triangulation                    # the graph's static tensors, rewritten by every replay
    got = []
    for x in inputs:
        out = gf(x)
        torch.cuda.synchronize()
        got.append([t.clone() for t in (out[0],) + tuple(static)])
    with torch.no_grad():
        for x, g in zip(inputs, got):
            out = model(meta=meta, input_heatmaps=x, cameras=cams, resize_transform=rt)
            assert _same((out[0],) + tuple(model.last_triangulation), g)
    assert bool((got[0][2] != -2).any())
