"""fvp_triangulate_joints on the CPU emulation of the kernels (tests/hipemu): every scene of tests/triangulate_cases.py against
the independent numpy restatement of the header's definition, all seven outputs bit for bit; what every constructed scene is
about; the scene set against ten wrong readings of the definition; the read fence; every argument error with nothing written;
every combination of NULL outputs; the definition against the truth (tests/golden/triangulate_floor.json); JointTriangulator,
model.triangulator and the pipelines' refusal."""
import ctypes as C

import numpy as np
import pytest
import torch

import triangulate_cases as TC
from cases import make_inputs, make_weights
from faster_voxelpose_amd import _capi as capi


def test_header_and_binding_hold_the_export(emu_lib):
    assert capi.ABI_VERSION >= 18 and emu_lib.fvp_version() == capi.ABI_VERSION
    assert "fvp_triangulate_joints" in capi.SIGNATURES and hasattr(emu_lib, "fvp_triangulate_joints")
    assert capi.FVP_TRI_MAX_RADIUS == TC.MAX_RADIUS
    header = open(TC.__file__.replace("tests/triangulate_cases.py", "include/fvp.h")).read()
    assert "int fvp_triangulate_joints(" in header and f"#define FVP_ABI_VERSION {capi.ABI_VERSION}" in header
    assert f"#define FVP_TRI_MAX_RADIUS {TC.MAX_RADIUS}" in header


@pytest.mark.parametrize("name", TC.CASES)
def test_outputs_equal_the_yardstick(emu_lib, name):
    TC.check(emu_lib, "cpu", name)


@pytest.mark.parametrize("name", [n for n in TC.CASES if not n.startswith("random") and n != "fence"])
def test_scenes_hold_what_their_names_say(name):
    TC.check_expectations(name)


def test_scene_set_tells_the_mutants_apart(emu_lib):
    """Each wrong reading of the definition changes the expected values of the scene built against it - and the kernel's
    values there are the definition's, not the mutant's."""
    assert set(TC.TELLS) == set(TC.MUTANTS)
    for mut, name in TC.TELLS.items():
        case, want = TC.get(name)
        assert TC.differs(TC.reference(case, mutant=mut), want), f"no scene tells {mut!r} apart"
        rc, got = TC.call(emu_lib, "cpu", case)
        assert rc == 0
        TC.assert_equal(got, want, mut)


def test_random_scenes_are_not_trivial():
    states = set()
    for name in ("random_v3_j3", "random_v5_j5"):
        case, want = TC.get(name)
        states |= set(np.unique(want["view_state"]).tolist())
        assert (want["tri_count"] >= 2).any() and (want["tri_count"] == -2).any()
        assert (want["cam_count"] > 0).any() and (want["tri_stats"] > 0).any()
    assert states == {TC.USED, TC.NOT_EVALUATED, TC.OUTSIDE, TC.PEAK_LOW, TC.NOT_ENCLOSED, TC.OCCLUDED, TC.REJECTED, TC.UNSOLVED}
    assert TC.get("random_v3_j3")[0]["heat"].shape[-1] == 4 and TC.get("random_v5_j5")[0]["heat"].shape[-1] == 8


def test_read_fence(emu_lib):
    TC.check_fence(emu_lib, "cpu")


def test_outputs_may_be_null(emu_lib):
    TC.check_null_outputs(emu_lib, "cpu")


def test_argument_errors_write_nothing(emu_lib):
    TC.argument_errors(emu_lib, "cpu")


def test_definition_against_the_truth(emu_lib):
    """Figures of tests/golden/triangulate_floor.json (the numpy yardstick alone, seeds 101-103): paraboloid peaks - float64
    to the truth 1.8e-4 mm, float32 to float64 1.9e-3 mm, no state differs, every joint triangulated, 0.7 % of the views not
    enclosed; Gaussian peaks of sigma 3 - 0.25 mm (the parabola's bias) and 1.5e-3 mm.  The kernel, on seed 104, lies 1.3e-3 mm
    and 0.18 mm from the truth."""
    fl = TC.floor()
    for kind in ("paraboloid", "gaussian"):
        assert fl[kind]["state_mismatch_share"] <= 0.05 and fl[kind]["triangulated_share"] >= 0.90
    TC.check_floor(emu_lib, "cpu")


# ---- host side ------------------------------------------------------------------------------------------------------------
def test_joint_triangulator_class(emu_lib):
    """__call__ equals the yardstick's bits with camera tables and with a cameras dict + meta; the outputs are preallocated
    per shape; per_camera=False leaves the per-camera outputs out; the refusals."""
    from faster_voxelpose_amd.utils.triangulate import JointTriangulator
    case, want = TC.get("random_v5_j5")
    tri = TC.triangulator_for(case, emu_lib)
    t = TC.tensors(case, "cpu")
    out = TC.run_class(tri, t)
    TC.assert_equal(TC.as_dict(out), want, "tensor tables")
    assert out[1].dtype == torch.int32 and out[4].dtype == torch.int32 and out[3].shape == (3, 5, 2, 5, 4)
    again = TC.run_class(tri, t)
    assert all(a.data_ptr() == b.data_ptr() for a, b in zip(out, again))            # preallocated: the same memory
    lean = TC.triangulator_for(case, emu_lib, per_camera=False)
    out = TC.run_class(lean, t)
    assert out[5] is None and out[6] is None
    TC.assert_equal(TC.as_dict(out), want, "per_camera=False")
    # a cameras dict and meta: sequences numbered in order of first appearance
    names = ["seq_b", "seq_a"]
    cameras = {names[s]: [dict(R=case["cams"][s, v, :9].reshape(3, 3), T=case["cams"][s, v, 9:12], fx=case["cams"][s, v, 12],
                               fy=case["cams"][s, v, 13], cx=case["cams"][s, v, 14], cy=case["cams"][s, v, 15],
                               k=case["cams"][s, v, 16:19], p=case["cams"][s, v, 19:21]) for v in range(5)] for s in range(2)}
    order = list(dict.fromkeys(int(s) for s in case["frame_set"]))
    remap = {s: i for i, s in enumerate(order)}
    meta = {"seq": [names[remap[int(s)]] for s in case["frame_set"]]}
    cameras = {names[remap[s]]: cameras[names[s]] for s in order}
    got = tri(t["poses"], cameras, meta, t["heat"], occluder=t["occluder"], ids=t["ids"])
    TC.assert_equal(TC.as_dict(got), want, "cameras dict")
    empty = tri(t["poses"][:0], t["cams"], t["frame_set"][:0], t["heat"][:0])
    assert empty[0].shape == (0, 2, 5, 5) and empty[3].shape == (0, 5, 2, 5, 4)
    cfg = TC.Cfg(5)
    for bad in (dict(radius=0), dict(radius=9), dict(undistort_iters=17), dict(undistort_iters=-1), dict(min_views=1),
                dict(min_peak=float("nan")), dict(min_det=float("inf")), dict(reject_px=float("nan"))):
        with pytest.raises(capi.FvpError):
            JointTriangulator(cfg, **{**dict(_lib=emu_lib), **bad})
    with pytest.raises(capi.FvpError):
        JointTriangulator(TC.Cfg(capi.FVP_MAX_JOINTS + 1), _lib=emu_lib)
    with pytest.raises(capi.FvpError):
        tri(t["poses"].double(), t["cams"], t["frame_set"], t["heat"])
    with pytest.raises(capi.FvpError):
        tri(t["poses"], t["cams"], t["frame_set"], t["heat"][:, :, :, :, :4].contiguous())       # JP differs
    with pytest.raises(capi.FvpError):
        tri(t["poses"], t["cams"][:, :3].contiguous(), t["frame_set"], t["heat"])                 # V differs
    with pytest.raises(capi.FvpError):
        tri(t["poses"], t["cams"], t["frame_set"].long(), t["heat"])
    with pytest.raises(capi.FvpError):
        tri(t["poses"], t["cams"], t["frame_set"], t["heat"], occluder=t["occluder"].long())
    with pytest.raises(capi.FvpError):
        tri(t["poses"], t["cams"], t["frame_set"], t["heat"], ids=t["ids"][:, :1].contiguous())
    with pytest.raises(capi.FvpError):
        TC.run_class(TC.triangulator_for(case), t)                              # the product: host memory is refused


def _launches(lib, fn):
    lib.hipemu_launch_log.restype = C.c_char_p
    lib.hipemu_launch_log_reset()
    out = fn()
    return out, lib.hipemu_launch_log().decode().split()


def _same(a, b):
    return all(torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)
               for x, y in zip(a, b))


def test_model_triangulator_attribute(emu_lib):
    """model.triangulator on the tiny configuration.  Unset, the forward issues exactly the launches it issued before; set,
    two launches more (the triangulation and the per-camera reduction) behind the evidence launch - behind the visibility
    launch when model.visibility is set, whose occluder table is then passed; the returned tuple keeps its bits;
    last_triangulation equals the yardstick; the pipelines refuse it."""
    from faster_voxelpose_amd.models import faster_voxelpose as FV
    from faster_voxelpose_amd.utils.triangulate import JointTriangulator
    from faster_voxelpose_amd.utils.visibility import JointVisibility
    name = "tiny_g_b2_all"
    cfg, cams, seq, rt, heat, meta, _ = make_inputs(name)
    model = FV.FasterVoxelPoseNet(cfg, _lib=emu_lib)
    model.load_state_dict(make_weights(name, model.state_dict()))
    assert model.triangulator is None and model.last_triangulation is None
    kw = dict(meta=meta, input_heatmaps=heat, cameras=cams, resize_transform=rt)
    with torch.no_grad():
        model.evidence = True
        model(**kw)                                                                  # packs the weights, fills the caches
        plain, unset = _launches(emu_lib, lambda: model(**kw))
        plain = [t.clone() for t in plain[:3]]
        assert not any("k_triangulate_joints" in k for k in unset) and model.last_triangulation is None
        model.triangulator = JointTriangulator(cfg, radius=4, reject_px=6.0, _lib=emu_lib)
        out, with_tri = _launches(emu_lib, lambda: model(**kw))
        at = [i for i, k in enumerate(with_tri) if "k_triangulate_joints" in k]
        assert len(at) == 1 and "k_joint_evidence" in with_tri[at[0] - 1] and "k_view_residual" in with_tri[at[0] + 1]
        assert with_tri[:at[0]] + with_tri[at[0] + 2:] == unset                      # and nothing else changes
        assert _same(out[:3], plain)
        got = TC.as_dict(model.last_triangulation)
        TC.assert_equal(got, TC.reference(TC.model_case(model, cfg, rt, heat, meta, cams, out)), "model.last_triangulation")
        assert (got["tri_count"] != -2).any() and (got["view_state"] != TC.NOT_EVALUATED).any()
        # with model.visibility the occluder table goes in, and the launch sits behind the visibility's
        model.visibility = JointVisibility(cfg, prims=[(0, 1), (1, 2), (2, 3), (3, 4)], radius=80.0, _lib=emu_lib)
        seen = {}
        tri = model.triangulator

        def spy(*a, **k):
            seen.update(k)
            return tri(*a, **k)

        model.triangulator = spy
        out, with_vis = _launches(emu_lib, lambda: model(**kw))
        at = [i for i, k in enumerate(with_vis) if "k_triangulate_joints" in k]
        assert len(at) == 1 and "k_joint_visibility" in with_vis[at[0] - 1]
        assert seen["occluder"] is model.last_visibility[0] and _same(out[:3], plain)
        model.triangulator = tri
        want = TC.reference(TC.model_case(model, cfg, rt, heat, meta, cams, out, occluder=model.last_visibility[0]))
        TC.assert_equal(TC.as_dict(model.last_triangulation), want, "with the occluder table")
        model.visibility = None
        with pytest.raises(capi.FvpError, match="consumer stream"):
            FV.PipelinedForward(model, depth=1, streams=[None])
        with pytest.raises(capi.FvpError, match="consumer stream"):
            FV.GraphedPipeline(model, 1, meta, heat, cams, rt, streams=[None])
