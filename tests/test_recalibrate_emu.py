"""fvp_camera_refit_accumulate / fvp_camera_refit_solve on the CPU emulation of the kernels (tests/hipemu): every scene of
tests/recalibrate_cases.py against the independent numpy restatement of the header's definition - the accumulators (fp64),
the corrected cameras, the statistics and the states bit for bit, with guard elements around every buffer; what every
constructed scene is about; the scene set against nine wrong readings of the definition; decay across two calls; every
argument error with nothing written; NULL outputs; three rounds against the truth (tests/golden/refit_floor.json);
CameraRefiner, model.recalibrator and the pipelines' refusal."""
import ctypes as C

import numpy as np
import pytest
import torch

import recalibrate_cases as RC
from cases import make_inputs, make_weights
from faster_voxelpose_amd import _capi as capi


def test_header_and_binding_hold_the_exports(emu_lib):
    assert capi.ABI_VERSION >= 19 and emu_lib.fvp_version() == capi.ABI_VERSION
    header = open(RC.__file__.replace("tests/recalibrate_cases.py", "include/fvp.h")).read()
    for name in ("fvp_camera_refit_accumulate", "fvp_camera_refit_solve"):
        assert name in capi.SIGNATURES and hasattr(emu_lib, name) and f"int {name}(" in header
    assert f"#define FVP_ABI_VERSION {capi.ABI_VERSION}" in header and f"#define FVP_CAL_ACC {RC.ACC}" in header
    assert (capi.FVP_CAL_OK, capi.FVP_CAL_CLAMPED, capi.FVP_CAL_FEW, capi.FVP_CAL_DEGENERATE) == (RC.OK, RC.CLAMPED, RC.FEW, RC.DEGENERATE)
    for name, val in (("OK", "1"), ("CLAMPED", "2"), ("FEW", "0"), ("DEGENERATE", "(-1)")):
        assert f"#define FVP_CAL_{name} {val}" in header


@pytest.mark.parametrize("name", RC.CASES)
def test_outputs_equal_the_yardstick(emu_lib, name):
    RC.check(emu_lib, "cpu", name)


@pytest.mark.parametrize("name", [n for n in RC.CASES if not n.startswith("random")])
def test_scenes_hold_what_their_names_say(name):
    RC.check_expectations(name)


def test_scene_set_tells_the_mutants_apart(emu_lib):
    """Each wrong reading of the definition changes the expected values of the scene named against it - and the kernels'
    values there are the definition's, not the mutant's."""
    assert set(RC.TELLS) == set(RC.MUTANTS)
    for mut, name in RC.TELLS.items():
        case, want = RC.get(name)
        assert RC.differs(RC.reference(case, mutant=mut), want), f"no scene tells {mut!r} apart"
        RC.assert_equal(RC.run(emu_lib, "cpu", case), want, mut)


def test_random_scenes_are_not_trivial():
    states = set()
    for name in ("random_v3_j5", "random_v5_j7"):
        case, want = RC.get(name)
        states |= set(np.unique(want["cal_state"]).tolist())
        assert (want["acc"][..., 30] > 0).any() and (want["acc"][..., 29] < np.prod(case["points"].shape[:3])).all()
        assert ((case["frame_set"] < 0) | (case["frame_set"] >= case["cams"].shape[0])).any()
    assert {RC.OK, RC.FEW} <= states


def test_decay_across_two_calls(emu_lib):
    RC.check_decay(emu_lib, "cpu")


def test_read_fence(emu_lib):
    RC.check_fence(emu_lib, "cpu")


def test_outputs_may_be_null(emu_lib):
    RC.check_null_outputs(emu_lib, "cpu")


def test_argument_errors_write_nothing(emu_lib):
    RC.argument_errors(emu_lib, "cpu")


def test_three_rounds_against_the_truth(emu_lib):
    """Figures of tests/golden/refit_floor.json (the numpy yardstick alone, the largest over seeds 201-203): a camera bumped
    by 1.5 degrees and 30 mm goes 24.5 px -> 0.16 px -> 1.0e-4 px rms and ends 3.5e-4 mm and 8.7e-7 degrees from the float64
    truth after three rounds - the resolution of a float32 record at 4 m; the untouched cameras stay within 2.3e-4 mm and
    2.0e-6 degrees.  The kernels, on seed 204, must land within 2 x each figure (they give 1.5e-4 mm, 4.1e-7 degrees, 1.0e-4 px)."""
    RC.check_floor(emu_lib, "cpu")


# ---- host side ------------------------------------------------------------------------------------------------------------
def test_camera_refiner_class(emu_lib):
    """accumulate + solve equal the yardstick's bits; refine equals the hand-rolled loop and the yardstick's rounds; the
    outputs ping-pong between two preallocated sets; reset; the refusals."""
    from faster_voxelpose_amd.utils.recalibrate import CameraRefiner
    case, want = RC.get("random_v5_j7")
    ref = RC.refiner_for(case, emu_lib, decay=1.0)
    t = RC.tensors(case, "cpu")
    acc = ref.accumulate(*[t[k] for k in RC.TENSORS])
    assert acc.dtype == torch.float64 and tuple(acc.shape) == want["acc"].shape
    RC.assert_equal(dict(acc=acc.numpy()), want, "accumulate")
    out = ref.solve(t["cams"])
    RC.assert_equal(RC.as_dict(out), want, "solve")
    assert out[2].dtype == torch.int32 and out[0].shape == t["cams"].shape
    again = ref.solve(t["cams"])
    third = ref.solve(t["cams"])
    assert again[0].data_ptr() != out[0].data_ptr() and third[0].data_ptr() == out[0].data_ptr()     # two sets, in turn
    ref.reset(sets=[1])
    assert (ref.acc[1] == 0).all() and (ref.acc[0] != 0).any()
    ref.reset()
    assert (ref.acc == 0).all()
    # refine = the hand-rolled loop = the yardstick's rounds
    got = RC.as_dict(ref.refine(*[t[k] for k in RC.TENSORS], iters=3))
    RC.assert_equal(got, RC.ref_refine(case, 3), "refine", keys=RC.SOLVE_OUTPUTS)
    hand = RC.refiner_for(case, emu_lib, decay=1.0)
    cams = t["cams"]
    for _ in range(3):
        hand.reset()
        hand.accumulate(t["points"], t["obs"], t["view_state"], cams, t["frame_set"])
        res = hand.solve(cams)
        cams = res[0]
    RC.assert_equal(RC.as_dict(res), got, "hand-rolled", keys=RC.SOLVE_OUTPUTS)
    assert RC.differs(got, want, RC.SOLVE_OUTPUTS)
    empty = ref.accumulate(t["points"][:0], t["obs"][:0], t["view_state"][:0], t["cams"], t["frame_set"][:0])
    assert tuple(empty.shape) == want["acc"].shape
    cfg = RC.Cfg(7)
    for bad in (dict(nseq=0), dict(undistort_iters=17), dict(undistort_iters=-1), dict(min_obs=5), dict(huber_px=float("nan")),
                dict(decay=1.5), dict(decay=-0.1), dict(lam=-1.0), dict(lam=float("inf")), dict(min_pivot=0.0),
                dict(max_angle_deg=0.0), dict(max_shift_mm=float("nan"))):
        with pytest.raises(capi.FvpError):
            CameraRefiner(cfg, **{**dict(_lib=emu_lib), **bad})
    with pytest.raises(capi.FvpError):
        CameraRefiner(RC.Cfg(capi.FVP_MAX_JOINTS + 1), _lib=emu_lib)
    args = [t[k] for k in RC.TENSORS]
    for i, wrong in ((0, t["points"].double()), (1, t["obs"][..., :3].contiguous()), (2, t["view_state"].long()),
                     (3, t["cams"][..., :20].contiguous()), (4, t["frame_set"].long()), (4, t["frame_set"][:1])):
        with pytest.raises(capi.FvpError):
            ref.accumulate(*[wrong if k == i else a for k, a in enumerate(args)])
    with pytest.raises(capi.FvpError):
        ref.solve(t["cams"].double())
    with pytest.raises(capi.FvpError):
        ref.refine(*args, iters=0)
    with pytest.raises(capi.FvpError):
        RC.refiner_for(case).accumulate(*args)                                  # the product: host memory is refused


def test_camera_dicts_round_trip():
    """camera_dicts -> the engine's own table builder -> the same 24 floats."""
    from faster_voxelpose_amd.utils.recalibrate import CameraRefiner
    case, want = RC.get("two_sets")
    names = ["hall_a", "hall_b"]
    dicts = CameraRefiner.camera_dicts(torch.from_numpy(want["cams_out"]), names)
    assert list(dicts) == names and len(dicts["hall_a"]) == 3 and set(dicts["hall_a"][0]) == {"R", "T", "fx", "fy", "cx", "cy", "k", "p"}
    assert np.array_equal(RC.bits(RC.camera_records(dicts, names)), RC.bits(want["cams_out"]))
    with pytest.raises(capi.FvpError):
        CameraRefiner.camera_dicts(torch.from_numpy(want["cams_out"]), names[:1])


def _launches(lib, fn):
    lib.hipemu_launch_log.restype = C.c_char_p
    lib.hipemu_launch_log_reset()
    out = fn()
    return out, lib.hipemu_launch_log().decode().split()


def _same(a, b):
    return all(torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)
               for x, y in zip(a, b))


def test_model_recalibrator_attribute(emu_lib):
    """model.recalibrator on the tiny configuration.  Unset, the forward issues exactly the launches it issued before; set,
    one launch more, right behind the triangulation's; the returned tuple keeps its bits; the accumulators equal the
    yardstick on the forward's own tensors, with the fused and with the triangulated joints; without a triangulator it is
    an error; the pipelines refuse it."""
    from faster_voxelpose_amd.models import faster_voxelpose as FV
    from faster_voxelpose_amd.utils.recalibrate import CameraRefiner
    from faster_voxelpose_amd.utils.triangulate import JointTriangulator
    name = "tiny_g_b2_all"
    cfg, cams, seq, rt, heat, meta, _ = make_inputs(name)
    model = FV.FasterVoxelPoseNet(cfg, _lib=emu_lib)
    model.load_state_dict(make_weights(name, model.state_dict()))
    assert model.recalibrator is None and model.recalibrator_points == "fused"
    kw = dict(meta=meta, input_heatmaps=heat, cameras=cams, resize_transform=rt)
    with torch.no_grad():
        model.evidence = True
        model.triangulator = JointTriangulator(cfg, radius=8, min_peak=0.0, _lib=emu_lib)     # 30 used joint-views
        model(**kw)                                                                  # packs the weights, fills the caches
        plain, unset = _launches(emu_lib, lambda: model(**kw))
        plain = [t.clone() for t in plain[:3]]
        assert not any("k_camera_refit" in k for k in unset)
        for points in ("fused", "tri"):
            model.recalibrator = CameraRefiner(cfg, huber_px=4.0, _lib=emu_lib)
            model.recalibrator_points = points
            out, with_cal = _launches(emu_lib, lambda: model(**kw))
            at = [i for i, k in enumerate(with_cal) if "k_camera_refit_accumulate" in k]
            assert len(at) == 1 and "k_view_residual" in with_cal[at[0] - 1] and "k_triangulate_joints" in with_cal[at[0] - 2]
            assert with_cal[:at[0]] + with_cal[at[0] + 1:] == unset                   # and nothing else changes
            assert _same(out[:3], plain)
            tri = model.last_triangulation
            fs = model.engine.frame_sets(meta, cams, heat.shape[1])
            case = dict(points=(out[0] if points == "fused" else tri[0]).numpy(), obs=tri[3].numpy(), view_state=tri[4].numpy(),
                        cams=model.engine.geo.cams.numpy(), frame_set=fs.numpy(), params=dict(huber_px=4.0))
            want = RC.ref_accumulate(case)
            RC.assert_equal(dict(acc=model.recalibrator.acc.numpy()), dict(acc=want), points)
            assert (want[..., 29] > 0).any()
            model(**kw)                                                              # a second forward accumulates on top
            RC.assert_equal(dict(acc=model.recalibrator.acc.numpy()), dict(acc=RC.ref_accumulate(case, acc=want)), points + " twice")
        res = model.recalibrator.solve(model.engine.geo.cams)
        RC.assert_equal(RC.as_dict(res), RC.ref_solve(model.recalibrator.acc.numpy(), model.engine.geo.cams.numpy(),
                                                      dict(huber_px=4.0)), "solve on the engine's tables")
        model.recalibrator_points = "smoothed"
        with pytest.raises(capi.FvpError, match="recalibrator_points"):
            model(**kw)
        model.recalibrator_points = "fused"
        with pytest.raises(capi.FvpError, match="consumer stream"):
            FV.PipelinedForward(model, depth=1, streams=[None])
        with pytest.raises(capi.FvpError, match="consumer stream"):
            FV.GraphedPipeline(model, 1, meta, heat, cams, rt, streams=[None])
        tri, model.triangulator = model.triangulator, None
        with pytest.raises(capi.FvpError, match="model.triangulator"):
            model(**kw)
        with pytest.raises(capi.FvpError, match="recalibrator"):
            FV.PipelinedForward(model, depth=1, streams=[None])
