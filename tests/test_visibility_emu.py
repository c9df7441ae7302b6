"""fvp_joint_visibility on the CPU emulation of the kernels (tests/hipemu): every scene of tests/visibility_cases.py against
the independent fp32 numpy restatement of the definition, occluder, vis_conf and vis_count bit for bit; what every constructed
scene is about; the scene set against seventeen wrong readings of the definition; the float64 restatement as a second judge;
every argument error with nothing written; JointVisibility, model.visibility and the pipelines' refusal."""
import ctypes as C

import numpy as np
import pytest
import torch

import visibility_cases as VC
from cases import make_inputs, make_weights
from faster_voxelpose_amd import _capi as capi
from faster_voxelpose_amd.core.smoothing import PoseSmoother
from faster_voxelpose_amd.core.tracking import PoseTracker
from faster_voxelpose_amd.models import faster_voxelpose as FV
from faster_voxelpose_amd.utils.visibility import JointVisibility

TINY_PRIMS = [(0, 1), (1, 2), (2, 3), (3, 4)]            # the tiny configuration has 5 joints: no default skeleton


def test_header_and_binding_hold_the_export(emu_lib):
    assert capi.ABI_VERSION >= 17 and emu_lib.fvp_version() == capi.ABI_VERSION
    assert "fvp_joint_visibility" in capi.SIGNATURES and hasattr(emu_lib, "fvp_joint_visibility")
    header = open(VC.__file__.replace("tests/visibility_cases.py", "include/fvp.h")).read()
    assert "int fvp_joint_visibility(" in header and f"#define FVP_ABI_VERSION {capi.ABI_VERSION}" in header


@pytest.mark.parametrize("name", VC.CASES)
def test_outputs_equal_the_yardstick(emu_lib, name):
    VC.check(emu_lib, "cpu", name)


@pytest.mark.parametrize("name", [n for n in VC.CASES if not n.startswith("random")])
def test_scenes_hold_what_their_names_say(name):
    VC.check_expectations(name)


def test_scene_set_tells_the_mutants_apart(emu_lib):
    """Each wrong reading of the definition changes the expected values of the scene built against it - and the kernel's
    values there are the definition's, not the mutant's."""
    assert set(VC.TELLS) == set(VC.MUTANTS)
    for mut, name in VC.TELLS.items():
        case, want = VC.get(name)
        wrong = VC.reference(case, mutant=mut)
        assert any(a is not None and not np.array_equal(VC.bits(a) if a.dtype == VC.f32 else a, VC.bits(b) if b.dtype == VC.f32 else b)
                   for a, b in zip(wrong, want)), f"no scene tells {mut!r} apart"
        rc, got = VC.call(emu_lib, "cpu", case)
        assert rc == 0
        VC.assert_equal(got, want, mut)


def test_random_scenes_are_not_trivial():
    for name in ("random_b2_v3_n4_j15", "random_b1_v8_n32_j32_l64"):
        case, (occ, conf, count) = VC.get(name)
        assert (occ == -2).any() and (occ == -1).any() and (occ >= 0).any()
        own = occ == np.arange(occ.shape[2])[None, None, :, None]
        assert own.any() and ((occ >= 0) & ~own).any()                          # self-occlusion and other people
        assert (count == 0).any() and (count > 1).any() and (conf > 0).any()
    assert len(VC.get("random_b1_v8_n32_j32_l64")[0]["prims"]) == VC.MAX_PRIMS


def test_outputs_may_be_null(emu_lib):
    VC.check_null_outputs(emu_lib, "cpu")


def test_argument_errors_write_nothing(emu_lib):
    VC.argument_errors(emu_lib, "cpu")


def test_float64_restatement_agrees(emu_lib):
    """The fp32 kernel against the same definition in float64 on 4 500 joint-views: occluded / not occluded agree wherever no
    candidate primitive passes within 0.25 mm of its own surface; the occluder's slot agrees wherever the runner-up hit of
    another person is at least 1e-3 away in s; at most 5 % of the joint-views are left out.  The margin is not a tolerance
    on the kernel: both bounds are set by fp32's resolution at these distances (an ulp of 1e4 mm is 1e-3 mm; the squared
    distances compared are ~1e4 mm^2 with products of ~1e7 inside, a relative 6e-8 each), far below 0.25 mm."""
    case = VC.fp64_scene()
    rc, got = VC.call(emu_lib, "cpu", case)
    assert rc == 0
    n, left_out, occluded, wrong, slots, slot_wrong = VC.fp64_compare(got[0], case)
    print(f"fp64: {n} joint-views, {100 * left_out:.2f} % left out, {100 * occluded:.1f} % occluded, {wrong} disagree; "
          f"{slots} slots compared, {slot_wrong} disagree")
    assert n == 4500 and left_out <= 0.05 and 0.3 < occluded < 0.9
    assert wrong == 0 and slots > 1000 and slot_wrong == 0


# ---- host side ------------------------------------------------------------------------------------------------------------
def _same(a, b):
    return all(torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)
               for x, y in zip(a, b))


def test_joint_visibility_class(emu_lib):
    """__call__ equals the yardstick's bits with the engine's tables and with a cameras dict + meta; the default body model per
    J; radius and spheres; the refusals."""
    case, want = VC.get("random_b2_v3_n4_j15")
    prims, radius = VC.body15()
    jv = JointVisibility(15, radius=60.0, spheres={1: 110.0}, guard=50.0, _lib=emu_lib)
    assert jv.prims == VC.LIMBS15 + [(1, 1)] and jv.radius == [60.0] * 14 + [110.0] and jv.feeds_conf
    jv = JointVisibility(15, prims=prims[:14] + [prims[15]], radius=radius[:14] + [radius[15]], spheres={1: 110.0}, guard=50.0,
                         _lib=emu_lib)
    assert sorted(zip(jv.prims, jv.radius)) == sorted(zip(prims, radius))
    jv = JointVisibility(15, prims=prims, radius=radius, guard=50.0, feeds_conf=False, _lib=emu_lib)
    t = {k: torch.from_numpy(case[k]) for k in ("poses", "cams", "frame_set", "ids", "views")}
    got = jv(t["poses"], t["cams"], t["frame_set"], views=t["views"], ids=t["ids"], frame_size=(VC.HS, VC.WS))
    VC.assert_equal([g.numpy() for g in got], want, "tensor tables")
    assert got[0].dtype == torch.int32 and got[2].dtype == torch.int32 and got[0].shape == (2, 3, 4, 15)
    occ, conf, count = jv(t["poses"], t["cams"], t["frame_set"], ids=t["ids"])
    assert conf is None and count is None and np.array_equal(occ.numpy(), want[0])
    # a cameras dict and meta: sequences numbered in order of first appearance, as the engine does
    names = ["seq_b", "seq_a"]
    cameras = {names[s]: [dict(R=np.eye(3), T=case["cams"][s, v, 9:12], fx=1.0, fy=1.0, cx=0.0, cy=0.0, k=np.zeros(3), p=np.zeros(2))
                          for v in range(3)] for s in range(2)}
    order = list(dict.fromkeys(int(s) for s in case["frame_set"]))
    meta = {"seq": [names[int(s)] for s in case["frame_set"]]}
    got = jv(t["poses"], cameras, meta, views=t["views"], ids=t["ids"], frame_size=(VC.HS, VC.WS))
    VC.assert_equal([g.numpy() for g in got], want, "cameras dict")
    assert [names[s] for s in order] == list(jv._seq_ids)
    empty = jv(t["poses"][:0], t["cams"], t["frame_set"][:0], views=t["views"][:0], frame_size=(VC.HS, VC.WS))
    assert empty[0].shape == (0, 3, 4, 15) and empty[1].shape == (0, 4, 15)
    for bad in (dict(radius=0.0), dict(radius=float("nan")), dict(radius=[50.0] * 3), dict(spheres={15: 50.0}),
                dict(spheres={0: -1.0}), dict(guard=-1.0), dict(guard=float("inf")), dict(prims=[(0, 15)]),
                dict(prims=[(0, 1)] * 65), dict(prims=[(0, 1)] * 64, spheres={0: 50.0})):
        with pytest.raises(capi.FvpError):
            JointVisibility(15, **{**dict(_lib=emu_lib), **bad})
    with pytest.raises(capi.FvpError):
        JointVisibility(5, _lib=emu_lib)                                         # no default skeleton for 5 joints
    with pytest.raises(capi.FvpError):
        JointVisibility(capi.FVP_MAX_JOINTS + 1, prims=[], _lib=emu_lib)
    assert len(JointVisibility(17, _lib=emu_lib).prims) == 19 and len(JointVisibility(14, _lib=emu_lib).prims) == 14
    with pytest.raises(capi.FvpError):
        jv(t["poses"].double(), t["cams"], t["frame_set"])
    with pytest.raises(capi.FvpError):
        jv(t["poses"][:, :, :5].contiguous(), t["cams"], t["frame_set"])
    with pytest.raises(capi.FvpError):
        jv(t["poses"], t["cams"], t["frame_set"].long())
    with pytest.raises(capi.FvpError):
        jv(t["poses"], t["cams"][:, :2].contiguous(), t["frame_set"], views=t["views"], frame_size=(VC.HS, VC.WS))   # V differs
    with pytest.raises(capi.FvpError):
        jv(t["poses"], t["cams"], t["frame_set"], views=t["views"])              # views without a frame size
    with pytest.raises(capi.FvpError):
        jv(t["poses"], t["cams"], t["frame_set"], ids=t["ids"].long())
    with pytest.raises(capi.FvpError):
        jv(t["poses"].repeat(1, 9, 1, 1), t["cams"], t["frame_set"])             # N = 36
    with pytest.raises(capi.FvpError):
        jv(t["poses"], t["cams"].repeat(1, 3, 1), t["frame_set"])                # V = 9
    with pytest.raises(capi.FvpError):
        JointVisibility(15).__call__(t["poses"], t["cams"], t["frame_set"])      # the product: host memory is refused


def _launches(lib, fn):
    lib.hipemu_launch_log.restype = C.c_char_p
    lib.hipemu_launch_log_reset()
    out = fn()
    return out, lib.hipemu_launch_log().decode().split()


def test_model_visibility_attribute(emu_lib):
    """model.visibility on the tiny configuration.  Unset, the forward issues exactly the launches it issued before; set, one
    launch more, right behind the evidence launch; the outputs keep their bits; last_visibility equals a direct call and the
    yardstick; with feeds_conf, vis_conf is the joint_conf the smoother gets; the pipelines refuse it."""
    case = "tiny_g_b2_all"
    cfg, cams, seq, rt, heat, meta, _ = make_inputs(case)
    model = FV.FasterVoxelPoseNet(cfg, _lib=emu_lib)
    model.load_state_dict(make_weights(case, model.state_dict()))
    assert model.visibility is None and model.last_visibility is None
    kw = dict(meta=meta, input_heatmaps=heat, cameras=cams, resize_transform=rt)
    ws, hs = cfg.DATASET.ORI_IMAGE_SIZE
    mk = dict(prims=TINY_PRIMS, radius=80.0, spheres={0: 120.0}, guard=60.0, _lib=emu_lib)
    with torch.no_grad():
        model.visibility = JointVisibility(cfg, **mk)
        with pytest.raises(capi.FvpError, match="model.evidence"):
            model(**kw)
        model.visibility = None
        model.evidence = True
        model(**kw)                                                                  # packs the weights, fills the caches
        plain, unset = _launches(emu_lib, lambda: model(**kw))
        assert not any("k_joint_visibility" in k for k in unset) and model.last_visibility is None
        plain_conf = model.last_evidence[1].clone()
        model.visibility = JointVisibility(cfg, **mk)
        assert model.visibility.frame_size == (hs, ws)
        out, with_vis = _launches(emu_lib, lambda: model(**kw))
        at = [i for i, k in enumerate(with_vis) if "k_joint_visibility" in k]
        assert len(at) == 1 and "k_joint_evidence" in with_vis[at[0] - 1]            # right behind the evidence launch
        assert with_vis[:at[0]] + with_vis[at[0] + 1:] == unset                      # and nothing else changes
        assert _same(out[:3], plain[:3]) and _same([model.last_evidence[1]], [plain_conf])
        occ, conf, count = model.last_visibility
        V, N, J = heat.shape[1], model.max_people, cfg.DATASET.NUM_JOINTS
        assert occ.shape == (heat.shape[0], V, N, J) and conf.shape == (heat.shape[0], N, J) == count.shape
        direct = model.visibility(out[0], cams, meta, views=model.last_evidence[0])
        assert _same(model.last_visibility, direct)
        fs = model.engine.frame_sets(meta, cams, V)
        scene = dict(poses=out[0].numpy(), cams=model.engine.geo.cams.numpy(), frame_set=fs.numpy(), ids=None,
                     views=model.last_evidence[0].numpy(), prims=model.visibility.prims, radius=model.visibility.radius,
                     guard=60.0, Hs=hs, Ws=ws)
        VC.assert_equal([t.numpy() for t in model.last_visibility], VC.reference(scene), "model.last_visibility")
        valid = out[0][:, :, 0, 3] >= 0
        assert bool(valid.any()) and bool(((occ != -2).all(dim=3).all(dim=1) == valid).all())
        # feeds_conf: the smoother's joint_conf is vis_conf; unset, it stays last_evidence[1]
        for feeds in (True, False):
            model.visibility = JointVisibility(cfg, feeds_conf=feeds, **mk)
            model.tracker = PoseTracker(cfg, _lib=emu_lib)
            model.smoother = PoseSmoother(model.tracker, conf_min=0.3)
            alone_t = PoseTracker(cfg, _lib=emu_lib)
            alone = PoseSmoother(alone_t, conf_min=0.3)
            out, launches = _launches(emu_lib, lambda: model(**kw))
            assert len(launches) == len(unset) + 3
            ids, slots, _ = alone_t.update(out[0], meta)
            jc = model.last_visibility[1] if feeds else model.last_evidence[1]
            assert _same(model.last_smooth, alone.update(out[0], ids, slots, joint_conf=jc, meta=meta))
        assert not _same([model.last_visibility[1]], [model.last_evidence[1]])
        model.tracker = model.smoother = None
        with pytest.raises(capi.FvpError, match="consumer stream"):
            FV.PipelinedForward(model, depth=1, streams=[None])
        with pytest.raises(capi.FvpError, match="consumer stream"):
            FV.GraphedPipeline(model, 1, meta, heat, cams, rt, streams=[None])
