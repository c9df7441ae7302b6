"""fvp_limb_learn / fvp_limb_fit on the CPU emulation of the kernels (tests/hipemu), through PoseTracker / LimbModel(_lib=emu):
every case of tests/limb_cases.py against the independent fp32 numpy restatement of the definition, bit for bit - target,
limb_obs, limb_state, fitted, resid and the five state arrays after every call."""
import os

import pytest
import torch

import fvp_synthetic as FS
import limb_cases as S
from cases import make_inputs, make_weights
from faster_voxelpose_amd import _capi as capi
from faster_voxelpose_amd.core.skeleton import LimbModel
from faster_voxelpose_amd.core.tracking import PoseTracker


@pytest.fixture
def mk(emu_lib):
    def make(N, J, nseq, T, max_age, limbs, **kw):
        tr = PoseTracker((N, J), nseq=nseq, max_tracks=T, max_age=max_age, device="cpu", _lib=emu_lib)
        return tr, LimbModel(tr, limbs, **kw)
    return make


@pytest.fixture
def mk_shape(emu_lib):
    return lambda N, J, T, nseq, limbs, **kw: LimbModel((N, J, T, nseq), limbs, device="cpu", _lib=emu_lib, **kw)


def test_abi(emu_lib):
    assert capi.ABI_VERSION >= 22 and emu_lib.fvp_version() == capi.ABI_VERSION
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fvp.h")).read()
    assert "int fvp_limb_learn(" in header and "int fvp_limb_fit(" in header
    for name, v in (("LEARNED", S.LEARNED), ("LEARNING", S.LEARNING), ("NOT_MEASURED", S.NOT_MEASURED), ("OUTLIER", S.OUTLIER),
                    ("RELEARNED", S.RELEARNED), ("INVALID", S.INVALID)):
        assert getattr(capi, "FVP_LIMB_" + name) == v
        assert f"#define FVP_LIMB_{name} {v if v >= 0 else '(%d)' % v}" in header
    assert f"#define FVP_LIMB_MAX {capi.FVP_LIMB_MAX}" in header and capi.FVP_LIMB_MAX == 64
    from faster_voxelpose_amd.utils import vis
    assert {J: [tuple(ab) for ab in t] for J, t in vis._LIMBS.items()} == S.LIMBS        # the yardstick's own copy of the tables


@pytest.mark.parametrize("J,T_,B,limbs", S.WALKERS, ids=[f"J{w[0]}-T{w[1]}-B{w[2]}-L{len(w[3])}" for w in S.WALKERS])
def test_noisy_walkers(mk, J, T_, B, limbs):
    S.case_walkers(mk, J, T_, B, limbs)


@pytest.mark.parametrize("J,B", [(15, 1), (17, 3), (14, 8)])
def test_constant_pose(mk, J, B):
    S.case_constant(mk, J, B)


def test_first_sample_min_frames_and_window_edges(mk_shape):
    S.case_first_sample_and_edges(mk_shape)


def test_gate_edges(mk_shape):
    S.case_gate_edges(mk_shape)


def test_outlier_burst_and_relearn(mk_shape):
    S.case_outliers_and_relearn(mk_shape)


@pytest.mark.parametrize("J", [15, 17])
def test_conf_min_edge(mk_shape, J):
    S.case_conf_edge(mk_shape, J)


@pytest.mark.parametrize("J", [15, 17])
def test_nonfinite_joints_and_coincident_ends(mk_shape, J):
    S.case_nonfinite(mk_shape, J)


@pytest.mark.parametrize("J", [15, 17])
def test_id_change_resets_every_limb_in_that_frame(mk, J):
    S.case_id_changes(mk, J)


@pytest.mark.parametrize("J,B", [(15, 1), (17, 3), (15, 8)])
def test_gaps_keep_the_lengths_reuse_resets_them(mk, J, B):
    S.case_gaps(mk, J, B)


def test_fit_weights(mk_shape):
    S.case_fit_weights(mk_shape)


@pytest.mark.parametrize("J", [15, 17])
def test_fit_parameters_and_65_people(mk_shape, J):
    S.case_fit_parameters(mk_shape, J)


@pytest.mark.parametrize("J", [14, 17])
def test_fit_invalid_slots(mk_shape, J):
    S.case_fit_invalid_slots(mk_shape, J)


@pytest.mark.parametrize("J", [15, 17])
def test_chunk_invariance(mk, J):
    S.case_chunk_invariance(mk, J)


def test_two_sequences_interleaved_and_a_frame_of_none(mk):
    S.case_two_sequences(mk, 15)


def test_null_arguments(emu_lib):
    S.case_null_arguments(emu_lib, "cpu")


def test_argument_limits_and_parameter_errors(emu_lib):
    S.case_argument_limits(emu_lib, "cpu")


@pytest.mark.parametrize("J,seed", S.PROPERTY)
def test_property_walkers(mk_shape, J, seed):
    S.case_property_walkers(mk_shape, J, seed)


@pytest.mark.parametrize("J", [15, 17])
def test_property_occluded_end(mk_shape, J):
    S.case_property_occluded_end(mk_shape, J)


def test_host_class_checks_and_reset(mk, mk_shape):
    tr, lm = mk(4, 15, 2, 8, 7, None)
    assert (lm.N, lm.J, lm.T, lm.nseq, lm.L, lm.device) == (4, 15, 8, 2, 14, tr.device) and lm.seq_ids is tr.seq_ids
    assert lm.limbs == S.LIMBS[15] and mk_shape(4, 17, 8, 1, None).limbs == S.LIMBS[17] and mk_shape(4, 14, 8, 1, None).L == 14
    assert (lm.min_frames, lm.window, lm.relearn, lm.iters) == (10, 64, 15, 4)
    assert (lm.conf_min, lm.gate_sigma, lm.gate_mm, lm.stiffness) == (0.0, 3.0, 20.0, 1.0)
    poses = torch.from_numpy(S._mixed(15)[1][:2].copy())
    meta = {"seq": ["b", "a"]}
    ids, slots, _ = tr.update(poses, meta)
    target, obs, state = lm.update(poses, ids, slots, meta=meta)             # names -> rows: the tracker's numbering
    assert tr.seq_ids == {"b": 0, "a": 1} and target.dtype == obs.dtype == torch.float32 and state.dtype == torch.int32
    assert (tuple(target.shape), tuple(obs.shape), tuple(state.shape)) == ((2, 4, 14), (2, 4, 14, 2), (2, 4, 14))
    assert S.same(lm.state()["limb_id"], tr.state()["trk_id"]) and (lm.state()["limb_cnt"] == 1).any(dim=2).any(dim=1).all()
    fitted, resid = lm.fit(poses, target)
    assert (tuple(fitted.shape), tuple(resid.shape)) == ((2, 4, 15, 5), (2, 4, 14)) and S.same(fitted, poses)   # nothing learned yet
    with pytest.raises(capi.FvpError):
        lm.update(poses, ids, slots, meta={"seq": ["a", "c"]})               # a third sequence
    own = mk_shape(4, 15, 8, 2, None)                                        # without a tracker: its own numbering
    own.update(poses, ids, slots, meta=meta)
    assert own.seq_ids == {"b": 0, "a": 1} and S.same(own.state()["limb_len"], lm.state()["limb_len"])
    # __call__ = update + fit on the same poses
    a, b = mk_shape(4, 15, 8, 1, None, min_frames=1), mk_shape(4, 15, 8, 1, None, min_frames=1)
    fitted, target, state, resid = a(poses, ids, slots)
    t2, _, s2 = b.update(poses, ids, slots)
    f2, r2 = b.fit(poses, t2, ids)
    assert S.same(fitted, f2) and S.same(target, t2) and S.same(state, s2) and S.same(resid, r2) and (target > 0).any()
    saved = lm.state()
    lm.reset("a")
    st = lm.state()
    assert (st["limb_id"][1] == -1).all() and (st["limb_len"][1] == 0).all() and (st["limb_id"][0] >= 0).any()
    lm.reset()
    fresh = mk_shape(4, 15, 8, 2, None).state()
    assert all(S.same(v, fresh[k]) for k, v in lm.state().items())
    lm.load_state(saved)
    assert all(S.same(v, saved[k]) for k, v in lm.state().items())
    empty = lm.update(poses[:0], ids[:0], slots[:0]) + lm.fit(poses[:0], target[:0])
    assert [tuple(t.shape) for t in empty] == [(0, 4, 14), (0, 4, 14, 2), (0, 4, 14), (0, 4, 15, 5), (0, 4, 14)]
    conf = torch.ones((2, 4, 15))
    bad = [(poses.double(), ids, slots, None), (poses[:, :, :14].contiguous(), ids, slots, None),
           (poses[..., :4].contiguous(), ids, slots, None), (poses, ids.long(), slots, None), (poses, ids, slots[:1], None),
           (poses, ids, None, None), (poses, ids, slots, conf.double()), (poses, ids, slots, conf[:, :, :14].contiguous())]
    for p, i, s, c in bad:
        with pytest.raises(capi.FvpError):
            lm.update(p, i, s, joint_conf=c)
    for p, t, i in ((poses, t2[:, :, :13].contiguous(), None), (poses, t2.double(), None), (poses, None, None), (poses, t2, ids.long())):
        with pytest.raises(capi.FvpError):
            lm.fit(p, t, i)
    nan = float("nan")
    for kw in (dict(min_frames=0), dict(min_frames=65), dict(window=0), dict(relearn=-1), dict(gate_sigma=-1.0),
               dict(gate_sigma=nan), dict(gate_mm=-1.0), dict(gate_mm=nan), dict(stiffness=1.5), dict(stiffness=-0.5),
               dict(stiffness=nan), dict(iters=0), dict(iters=33)):
        with pytest.raises(capi.FvpError):
            mk_shape(4, 15, 8, 1, None, **kw)
    for limbs in ([], [(0, 15)], [(-1, 2)], [(3, 3)], S.random_limbs(1, 15, 65)):
        with pytest.raises(capi.FvpError):
            mk_shape(4, 15, 8, 1, limbs)
    for shape in ((4, 15, 3, 1), (4, 15, 65, 1), (33, 15, 64, 1), (4, 33, 8, 1), (4, 15, 8, 0), (4, 16, 8, 1)):
        with pytest.raises(capi.FvpError):
            mk_shape(*shape, None)


@pytest.mark.parametrize("smoother", [False, True], ids=["fused_poses", "smoothed"])
def test_limb_model_behind_an_emulated_forward(emu_lib, smoother):
    """LimbModel is no model attribute: it runs behind the forward, on what the forward left in last_tracks, last_evidence and
    last_smooth."""
    from faster_voxelpose_amd.core.smoothing import PoseSmoother
    from faster_voxelpose_amd.models import faster_voxelpose as FV
    case = "tiny_g_b2_all"
    cfg, cams, seq, rt, heat, meta, _ = make_inputs(case)
    model = FV.FasterVoxelPoseNet(cfg, _lib=emu_lib)
    model.load_state_dict(make_weights(case, model.state_dict()))
    assert not hasattr(model, "limbs") and not hasattr(model, "limb_model")
    model.tracker = PoseTracker(cfg, _lib=emu_lib)
    model.evidence = True
    if smoother:
        model.smoother = PoseSmoother(model.tracker, conf_min=0.3)
    limbs = [(0, 1), (1, 2), (2, 3), (3, 4), (0, 4)]      # the tiny configuration has 5 joints: no default skeleton; a cycle
    kw = dict(conf_min=0.3, min_frames=2, gate_mm=200.0)
    lm = LimbModel(model.tracker, limbs, **kw)
    heats = [FS.heatmaps_blobs(cfg, cams, seq, heat.shape[0], people=2, seed=s) for s in (51, 51)]
    S.case_behind_forward(model, lm, S.Spec(lm.N, lm.J, lm.T, limbs, lm.nseq, **kw), heats, meta, cams, rt, smoother)


def test_bench_tool_host_route_equals_the_definition(mk):
    """tools/bench_limbs.py times the kernels against a host route; that route (vectorised numpy) is the definition, bit for
    bit: fitted poses and every state array against the yardstick and the emulated kernels over a stream of noisy walkers."""
    import sys

    import numpy as np
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import bench_limbs
    J, F, limbs = 15, 24, S.LIMBS[15]
    _, poses, _, conf = S._scene(J, F, seed=5)
    poses[7, :, 3, 0] = np.nan                                               # an unsupported joint by value
    kw = dict(conf_min=0.2, min_frames=3, gate_mm=8.0, relearn=2, window=6)
    tr, lm = mk(S.N, J, 1, 8, 15, limbs, **kw)
    host = bench_limbs.HostLimbs(lm)
    spec = S.Spec(S.N, J, 8, limbs, 1, **kw)
    seen = set()
    for f in range(0, F, 4):
        x, c = poses[f:f + 4], conf[f:f + 4]
        ids, slots, _ = tr.update(torch.from_numpy(x.copy()))
        fitted, target, state, _ = lm(torch.from_numpy(x.copy()), ids, slots, joint_conf=torch.from_numpy(c.copy()))
        got = host(x, S._np(ids), S._np(slots), c)
        want_t, _, _ = spec.update(x, S._np(ids), S._np(slots), c)
        want = spec.fit(x, want_t, S._np(ids), c)[0]
        assert S.same(got, want) and S.same(got, fitted)
        for a, b in zip((host.len, host.var, host.cnt, host.out, host.id), spec.state().values()):
            assert S.same(a, b[0])
        seen |= set(S._np(state).ravel().tolist())
    assert seen == {S.LEARNED, S.LEARNING, S.NOT_MEASURED, S.OUTLIER, S.RELEARNED, S.INVALID}, seen
