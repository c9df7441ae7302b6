"""fvp_joint_visibility of the shipped library on the MI355X: every scene of tests/visibility_cases.py against the independent
fp32 numpy restatement of the definition, occluder, vis_conf and vis_count bit for bit; every argument error with nothing
written; JointVisibility eager and under hipGraph capture; model.visibility set and unset, eager and in the model's captured
graph; the pipelines' refusal."""
import ctypes as C

import numpy as np
import pytest
import torch

import visibility_cases as VC
from cases import make_inputs, make_weights

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TINY_PRIMS = [(0, 1), (1, 2), (2, 3), (3, 4)]            # the tiny configuration has 5 joints: no default skeleton


@pytest.fixture(scope="module")
def lib():
    from faster_voxelpose_amd import _capi as capi
    return capi.load()


def test_library_holds_the_export(lib):
    from faster_voxelpose_amd import _capi as capi
    assert capi.ABI_VERSION >= 17 and lib.fvp_version() == capi.ABI_VERSION
    assert "fvp_joint_visibility" in capi.SIGNATURES and hasattr(lib, "fvp_joint_visibility")


@pytest.mark.parametrize("name", VC.CASES)
def test_outputs_equal_the_yardstick(lib, name):
    VC.check(lib, DEV, name)


def test_outputs_may_be_null(lib):
    VC.check_null_outputs(lib, DEV)


def test_argument_errors_write_nothing(lib):
    VC.argument_errors(lib, DEV)


def test_float64_restatement_agrees(lib):
    """As on the emulator: the card's occluder against the definition in float64, 4 500 joint-views."""
    case = VC.fp64_scene()
    rc, got = VC.call(lib, DEV, case)
    assert rc == 0
    n, left_out, occluded, wrong, slots, slot_wrong = VC.fp64_compare(got[0], case)
    assert n == 4500 and left_out <= 0.05 and wrong == 0 and slots > 1000 and slot_wrong == 0


def _same(a, b):
    torch.cuda.synchronize()
    return all(torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)
               for x, y in zip(a, b))


def test_joint_visibility_class():
    """__call__ equals the yardstick's bits; captured once into a hipGraph and replayed on another scene in the same memory,
    the replay's bits are the yardstick's for that scene; host memory is refused."""
    from faster_voxelpose_amd import _capi as capi
    from faster_voxelpose_amd.utils.visibility import JointVisibility
    prims, radius = VC.body15()
    jv = JointVisibility(15, prims=prims, radius=radius, guard=50.0)
    case, want = VC.get("random_b2_v3_n4_j15")
    other = VC.random_scene(2, 3, 4, 15, prims, radius, seed=17, nsets=2)
    keys = ("poses", "cams", "frame_set", "ids", "views")
    t = {k: torch.from_numpy(case[k]).to(DEV) for k in keys}

    def run():
        return jv(t["poses"], t["cams"], t["frame_set"], views=t["views"], ids=t["ids"], frame_size=(VC.HS, VC.WS))

    got = run()
    torch.cuda.synchronize()
    VC.assert_equal([g.cpu().numpy() for g in got], want, "eager")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = run()
    for k in keys:
        t[k].copy_(torch.from_numpy(other[k]))
    graph.replay()
    torch.cuda.synchronize()
    want2 = VC.reference(other)
    VC.assert_equal([g.cpu().numpy() for g in got], want2, "replay")
    assert not np.array_equal(want2[0], want[0])
    with pytest.raises(capi.FvpError):
        jv(t["poses"].cpu(), t["cams"].cpu(), t["frame_set"].cpu())              # host memory
    with pytest.raises(capi.FvpError):
        jv(t["poses"], t["cams"].cpu(), t["frame_set"])                          # tables on another device


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


def _model(case):
    from faster_voxelpose_amd.models import faster_voxelpose as FV
    cfg, cams, seq, rt, heat, meta, _ = make_inputs(case, device=DEV)
    model = FV.get(cfg).to(DEV)
    model.load_state_dict(make_weights(case, model.state_dict()))
    return model, cams, rt.to(DEV), heat.to(DEV), meta


def test_model_visibility_attribute(lib):
    """Tiny configuration: unset, the forward issues the launches it issued; set, one more; the outputs keep their bits;
    last_visibility equals a direct call and the yardstick; with feeds_conf the smoother gets vis_conf; the refusals."""
    from faster_voxelpose_amd import _capi as capi
    from faster_voxelpose_amd.core.smoothing import PoseSmoother
    from faster_voxelpose_amd.core.tracking import PoseTracker
    from faster_voxelpose_amd.models import faster_voxelpose as FV
    from faster_voxelpose_amd.utils.visibility import JointVisibility
    model, cams, rt, heat, meta = _model("tiny_g_b2_all")
    cfg = model.cfg
    kw = dict(meta=meta, input_heatmaps=heat, cameras=cams, resize_transform=rt)
    ws, hs = cfg.DATASET.ORI_IMAGE_SIZE
    mk = dict(prims=TINY_PRIMS, radius=80.0, spheres={0: 120.0}, guard=60.0)
    with torch.no_grad():
        model.visibility = JointVisibility(cfg, **mk)
        with pytest.raises(capi.FvpError, match="model.evidence"):
            model(**kw)
        model.visibility = None
        model.evidence = True
        plain = [t.clone() for t in model(**kw)[:3]]                                 # packs the weights, fills the caches
        _, unset = _total_launches(lib, lambda: model(**kw))
        assert model.last_visibility is None
        model.visibility = JointVisibility(cfg, **mk)
        out, n = _total_launches(lib, lambda: model(**kw))
        assert n == unset + 1 and _same(out[:3], plain)
        direct = model.visibility(out[0], cams, meta, views=model.last_evidence[0])
        assert _same(model.last_visibility, direct)
        fs = model.engine.frame_sets(meta, cams, heat.shape[1])
        scene = dict(poses=out[0].cpu().numpy(), cams=model.engine.geo.cams.cpu().numpy(), frame_set=fs.cpu().numpy(), ids=None,
                     views=model.last_evidence[0].cpu().numpy(), prims=model.visibility.prims, radius=model.visibility.radius,
                     guard=60.0, Hs=hs, Ws=ws)
        VC.assert_equal([t.cpu().numpy() for t in model.last_visibility], VC.reference(scene), "model.last_visibility")
        assert bool((model.last_visibility[0] != -2).any())
        for feeds in (True, False):
            model.visibility = JointVisibility(cfg, feeds_conf=feeds, **mk)
            model.tracker = PoseTracker(cfg)
            model.smoother = PoseSmoother(model.tracker, conf_min=0.3)
            alone_t = PoseTracker(cfg)
            alone = PoseSmoother(alone_t, conf_min=0.3)
            out, n = _total_launches(lib, lambda: model(**kw))
            assert n == unset + 3
            ids, slots, _ = alone_t.update(out[0], meta)
            jc = model.last_visibility[1] if feeds else model.last_evidence[1]
            assert _same(model.last_smooth, alone.update(out[0], ids, slots, joint_conf=jc, meta=meta))
        model.tracker = model.smoother = None
        with pytest.raises(capi.FvpError, match="consumer stream"):
            FV.PipelinedForward(model, depth=2)
        with pytest.raises(capi.FvpError, match="consumer stream"):
            FV.GraphedPipeline(model, 2, meta, heat, cams, rt)


def test_graphed_forward_with_visibility():
    """One capture, two replays with different inputs: last_visibility holds static tensors whose bits equal the eager
    forwards'."""
    import fvp_synthetic as S
    from faster_voxelpose_amd.models.faster_voxelpose import GraphedForward
    from faster_voxelpose_amd.utils.visibility import JointVisibility
    model, cams, rt, heat, meta = _model("tiny_g_b2_all")
    inputs = [S.heatmaps_blobs(model.cfg, cams, meta["seq"][0], heat.shape[0], people=2, seed=s).to(DEV) for s in (21, 22)]
    model.evidence = True
    model.visibility = JointVisibility(model.cfg, prims=TINY_PRIMS, radius=80.0, spheres={0: 120.0})
    gf = GraphedForward(model, meta, heat, cams, rt)
    static = model.last_visibility                       # the graph's static tensors, rewritten by every replay
    got = []
    for x in inputs:
        out = gf(x)
        torch.cuda.synchronize()
        got.append([t.clone() for t in (out[0],) + tuple(static)])
    with torch.no_grad():
        for x, g in zip(inputs, got):
            out = model(meta=meta, input_heatmaps=x, cameras=cams, resize_transform=rt)
            assert _same((out[0],) + tuple(model.last_visibility), g)
    assert bool((got[0][1] != -2).any())
