"""fvp_track_smooth on the CPU emulation of the kernels (tests/hipemu), through PoseTracker / PoseSmoother(_lib=emu): every
case of tests/smooth_cases.py against the independent fp32 numpy restatement of the definition, bit for bit - smooth,
track_poses, track_state and the four state arrays after every call."""
import numpy as np
import pytest
import torch

import smooth_cases as S
from cases import make_inputs, make_weights
from faster_voxelpose_amd import _capi as capi
from faster_voxelpose_amd.core.smoothing import PoseSmoother
from faster_voxelpose_amd.core.tracking import PoseTracker
from faster_voxelpose_amd.models import faster_voxelpose as FV


@pytest.fixture
def mk(emu_lib):
    def make(N, J, nseq, T, max_age, **kw):
        tr = PoseTracker((N, J), nseq=nseq, max_tracks=T, max_age=max_age, device="cpu", _lib=emu_lib)
        return tr, PoseSmoother(tr, **kw)
    return make


@pytest.fixture
def mk_shape(emu_lib):
    return lambda N, J, T, nseq, **kw: PoseSmoother((N, J, T, nseq), device="cpu", _lib=emu_lib, **kw)


@pytest.mark.parametrize("J,T_,B", S.WALKERS)
def test_noisy_walkers(mk, J, T_, B):
    S.case_walkers(mk, J, T_, B)


@pytest.mark.parametrize("J,B", [(15, 1), (17, 3), (15, 8)])
def test_constant_pose_keeps_its_bits(mk, J, B):
    S.case_constant(mk, J, B)


@pytest.mark.parametrize("J", [15, 17])
def test_conf_min_edge(mk_shape, J):
    S.case_conf_edge(mk_shape, J)


@pytest.mark.parametrize("J", [15, 17])
def test_nan_and_inf_joints_are_predicted(mk_shape, J):
    S.case_nonfinite_joint(mk_shape, J)


def test_nan_born_track_poisons_no_neighbour(mk):
    S.case_nan_born(mk, 17)


@pytest.mark.parametrize("J,B", [(15, 1), (17, 3), (15, 8)])
def test_gaps(mk, J, B):
    S.case_gaps(mk, J, B)


@pytest.mark.parametrize("J", [15, 17])
def test_coasting_damps_the_velocity_then_frees_the_slot(mk, J):
    S.case_coasting_velocity(mk, J)


@pytest.mark.parametrize("J", [15, 17])
def test_full_table_eviction_reinitialises(mk, J):
    S.case_full_table(mk, J)


@pytest.mark.parametrize("J", [15, 17])
def test_chunk_invariance(mk, J):
    S.case_chunk_invariance(mk, J)


def test_two_sequences_interleaved_and_a_frame_of_none(mk):
    S.case_two_sequences(mk, 15)


def test_null_output_combinations(emu_lib):
    S.case_null_outputs(emu_lib, "cpu")


def test_argument_limits_and_parameter_errors(emu_lib):
    S.case_argument_limits(emu_lib, "cpu")


def test_property_jitter(mk_shape):
    S.case_property_jitter(mk_shape)


def test_property_lag(mk_shape):
    S.case_property_lag(mk_shape)


def test_property_step(mk_shape):
    S.case_property_step(mk_shape)


def test_host_class_checks_and_reset(mk, mk_shape, emu_lib):
    tr, sm = mk(4, 15, 2, 8, 7)
    assert (sm.N, sm.J, sm.T, sm.nseq, sm.max_age, sm.device) == (4, 15, 8, 2, 7, tr.device) and sm.seq_ids is tr.seq_ids
    assert PoseSmoother(tr, max_age=3).max_age == 3 and mk_shape(4, 15, 8, 1).max_age == 15
    poses = torch.from_numpy(S._mixed(15)[1][:2].copy())
    meta = {"seq": ["b", "a"]}
    ids, slots, _ = tr.update(poses, meta)
    smooth, tp, ts = sm.update(poses, ids, slots, meta=meta)                 # names -> rows: the tracker's numbering
    assert tr.seq_ids == {"b": 0, "a": 1} and smooth.dtype == tp.dtype == torch.float32 and ts.dtype == torch.int32
    assert (tuple(smooth.shape), tuple(tp.shape), tuple(ts.shape)) == ((2, 4, 15, 5), (2, 8, 15, 4), (2, 8, 2))
    assert S.same(sm.state()["flt_id"], tr.state()["trk_id"]) and (sm.state()["flt_id"] >= 0).any(dim=1).all()
    with pytest.raises(capi.FvpError):
        sm.update(poses, ids, slots, meta={"seq": ["a", "c"]})               # a third sequence
    own = mk_shape(4, 15, 8, 2)                                              # without a tracker: its own numbering
    own.update(poses, ids, slots, meta=meta)
    assert own.seq_ids == {"b": 0, "a": 1} and S.same(own.state()["flt_id"], sm.state()["flt_id"])
    saved = sm.state()
    sm.reset("a")
    st = sm.state()
    assert (st["flt_id"][1] == -1).all() and (st["flt_pose"][1] == 0).all() and (st["flt_id"][0] >= 0).any()
    sm.reset()
    fresh = mk_shape(4, 15, 8, 2).state()
    assert all(S.same(v, fresh[k]) for k, v in sm.state().items())
    sm.load_state(saved)
    assert all(S.same(v, saved[k]) for k, v in sm.state().items())
    empty = sm.update(poses[:0], ids[:0], slots[:0])
    assert [tuple(t.shape) for t in empty] == [(0, 4, 15, 5), (0, 8, 15, 4), (0, 8, 2)]
    conf = torch.ones((2, 4, 15))
    bad = [(poses.double(), ids, slots, None), (poses[:, :, :14].contiguous(), ids, slots, None),
           (poses[..., :4].contiguous(), ids, slots, None), (poses, ids.long(), slots, None), (poses, ids, slots[:1], None),
           (poses, ids, None, None), (poses, ids, slots, conf.double()), (poses, ids, slots, conf[:, :, :14].contiguous()),
           (poses.transpose(0, 1).contiguous().transpose(0, 1), ids, slots, None)]
    for p, i, s, c in bad:
        with pytest.raises(capi.FvpError):
            sm.update(p, i, s, joint_conf=c)
    nan = float("nan")
    for kw in (dict(rate_hz=0.0), dict(rate_hz=nan), dict(min_cutoff=0.0), dict(d_cutoff=-1.0), dict(beta=-1.0), dict(beta=nan),
               dict(damp=1.5), dict(damp=-0.5), dict(damp=nan), dict(max_age=-1)):
        with pytest.raises(capi.FvpError):
            mk_shape(4, 15, 8, 1, **kw)
    for shape in ((4, 15, 3, 1), (4, 15, 65, 1), (33, 15, 64, 1), (4, 33, 8, 1), (4, 15, 8, 0)):
        with pytest.raises(capi.FvpError):
            mk_shape(*shape)


def test_model_smoother_attribute(emu_lib):
    """model.smoother: the returned tuple is what a forward without it returns; last_smooth equals a standalone update from
    the same prior state, with and without model.evidence; a smoother without a tracker is refused."""
    case = "tiny_g_b2_all"
    cfg, cams, seq, rt, heat, meta, _ = make_inputs(case)
    model = FV.FasterVoxelPoseNet(cfg, _lib=emu_lib)
    model.load_state_dict(make_weights(case, model.state_dict()))
    assert model.smoother is None and model.last_smooth is None
    kw = dict(meta=meta, input_heatmaps=heat, cameras=cams, resize_transform=rt)
    with torch.no_grad():
        plain = model(**kw)
        assert model.last_smooth is None
        model.smoother = PoseSmoother((cfg.CAPTURE_SPEC.MAX_PEOPLE, cfg.DATASET.NUM_JOINTS, 8, 1), device="cpu", _lib=emu_lib)
        with pytest.raises(capi.FvpError):
            model(**kw)
        for evidence in (False, True):
            model.evidence = evidence
            model.tracker = PoseTracker(cfg, _lib=emu_lib)
            model.smoother = PoseSmoother(model.tracker, conf_min=0.3)
            alone_t = PoseTracker(cfg, _lib=emu_lib)
            alone = PoseSmoother(alone_t, conf_min=0.3)
            for _ in range(2):                           # the second forward starts from the state the first left
                out = model(**kw)
                ids, slots, _ = alone_t.update(out[0], meta)
                want = alone.update(out[0], ids, slots, joint_conf=model.last_evidence[1] if evidence else None, meta=meta)
                for a, b in zip(out[:3], plain[:3]):
                    assert S.same(a, b)
                for a, b in zip(model.last_smooth, want):
                    assert S.same(a, b)
            for k, v in alone.state().items():
                assert S.same(model.smoother.state()[k], v)
            seen = (model.last_smooth[2][..., 0] >= 0) & (model.last_smooth[2][..., 1] == 0)
            flags = model.last_smooth[1][..., 3][seen]
            assert flags.numel() and (evidence or (flags == 1).all())          # without joint_conf every seen joint is measured
    assert np.isfinite(S._np(model.last_smooth[0])).all()
