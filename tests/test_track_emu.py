"""fvp_track_update on the CPU emulation of the kernels (tests/hipemu), through PoseTracker(_lib=emu): every case of
tests/track_cases.py against the independent fp32 numpy restatement of the definition, bit for bit - ids, slots, costs and
the four state arrays after every call."""
import pytest
import torch

import track_cases as T
from cases import make_inputs, make_weights
from faster_voxelpose_amd import _capi as capi
from faster_voxelpose_amd.core.tracking import PoseTracker
from faster_voxelpose_amd.models import faster_voxelpose as FV


@pytest.fixture
def mk(emu_lib):
    return lambda N, J, **kw: PoseTracker((N, J), device="cpu", _lib=emu_lib, **kw)


@pytest.mark.parametrize("J,N,T_,B", T.CONTINUITY)
def test_continuity(mk, J, N, T_, B):
    T.case_continuity(mk, J, N, T_, B)


@pytest.mark.parametrize("J", [15, 17])
def test_exact_ties(mk, J):
    T.case_ties(mk, J)


@pytest.mark.parametrize("J", [15, 17])
def test_gate_edge(mk, J):
    T.case_gate_edge(mk, J)


@pytest.mark.parametrize("J,B", [(15, 1), (17, 3), (15, 8)])
def test_gaps(mk, J, B):
    T.case_gaps(mk, J, B)


@pytest.mark.parametrize("J", [15, 17])
def test_full_table_evicts_the_oldest(mk, J):
    T.case_full_table(mk, J)


@pytest.mark.parametrize("J,B", [(15, 1), (17, 3), (15, 8)])
def test_empty_frames_and_first_frame(mk, J, B):
    T.case_empty_and_first(mk, J, B)


@pytest.mark.parametrize("J", [15, 17])
def test_chunk_invariance(mk, J):
    T.case_chunk_invariance(mk, J)


def test_two_sequences_interleaved(mk):
    T.case_two_sequences(mk, 15)


def test_nan_detection_is_born_not_matched(mk):
    T.case_nan(mk, 17)


def test_argument_limits(emu_lib):
    T.case_argument_limits(emu_lib, "cpu")


def test_host_class_checks_and_reset(mk):
    tr = mk(10, 15, nseq=2)
    assert (tr.N, tr.J, tr.T, tr.nseq) == (10, 15, 20, 2)
    poses = torch.from_numpy(T._mixed(15)[:2].copy())
    ids, slots, costs = tr.update(poses, meta={"seq": ["b", "a"]})         # names -> rows in order of first appearance
    assert tr.seq_ids == {"b": 0, "a": 1} and ids.dtype == slots.dtype == torch.int32 and costs.dtype == torch.float32
    assert tr.state()["next_id"].tolist() == [int((ids[0] >= 0).sum()), int((ids[1] >= 0).sum())]
    with pytest.raises(capi.FvpError):
        tr.update(poses, meta={"seq": ["a", "c"]})                         # a third sequence
    tr.reset("a")
    st = tr.state()
    assert st["next_id"][1] == 0 and (st["trk_id"][1] == -1).all() and (st["trk_id"][0] >= 0).any()
    tr.reset()
    fresh = mk(10, 15, nseq=2).state()
    assert all(T.same(v, fresh[k]) for k, v in tr.state().items())
    empty = tr.update(poses[:0])
    assert [tuple(t.shape) for t in empty] == [(0, 10)] * 3
    bad = {"float64": poses.double(), "joint count": poses[:, :, :14].contiguous(), "slot count": poses[:, :9].contiguous(),
           "four columns": poses[..., :4].contiguous(), "not contiguous": poses.transpose(0, 1).contiguous().transpose(0, 1)}
    for what, t in bad.items():
        with pytest.raises(capi.FvpError):
            tr.update(t)
    for kw in (dict(max_tracks=9), dict(max_tracks=65), dict(max_age=-1), dict(nseq=0)):
        with pytest.raises(capi.FvpError):
            mk(10, 15, **kw)
    with pytest.raises(capi.FvpError):
        mk(33, 15, max_tracks=64)


def test_model_tracker_attribute(emu_lib):
    """model.tracker: the returned tuple is what a forward without it returns; last_tracks equals a standalone update from
    the same prior state on the returned poses."""
    case = "tiny_g_b2_all"
    cfg, cams, seq, rt, heat, meta, _ = make_inputs(case)
    model = FV.FasterVoxelPoseNet(cfg, _lib=emu_lib)
    model.load_state_dict(make_weights(case, model.state_dict()))
    assert model.tracker is None and model.last_tracks is None
    kw = dict(meta=meta, input_heatmaps=heat, cameras=cams, resize_transform=rt)
    with torch.no_grad():
        plain = model(**kw)
        assert model.last_tracks is None
        model.tracker = PoseTracker(cfg, _lib=emu_lib)
        alone = PoseTracker(cfg, _lib=emu_lib)
        out = model(**kw)
        want = alone.update(out[0], meta)
        for a, b in zip(out[:3], plain[:3]):
            assert T.same(a, b)
        for a, b in zip(model.last_tracks, want):
            assert T.same(a, b)
    for k, v in alone.state().items():
        assert T.same(model.tracker.state()[k], v)
    assert (model.last_tracks[0] >= 0).any()
