"""fvp_track_update of the shipped library on the MI355X: every case of tests/track_cases.py against the independent fp32
numpy restatement of the definition, bit for bit, then the model attribute, a captured graph and the pipelined forward."""
import pytest
import torch

import fvp_synthetic as S
import track_cases as T
from cases import make_inputs, make_weights

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture
def mk():
    from faster_voxelpose_amd.core.tracking import PoseTracker
    return lambda N, J, **kw: PoseTracker((N, J), device=DEV, **kw)


def _model(case):
    from faster_voxelpose_amd.models import faster_voxelpose as FV
    cfg, cams, seq, rt, heat, meta, _ = make_inputs(case, device=DEV)
    model = FV.get(cfg).to(DEV)
    model.load_state_dict(make_weights(case, model.state_dict()))
    return model, cams, rt.to(DEV), heat.to(DEV), meta


def _inputs(model, cams, meta, heat, seeds):
    return [S.heatmaps_blobs(model.cfg, cams, meta["seq"][0], heat.shape[0], people=2, seed=s).to(DEV) for s in seeds]


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


def test_argument_limits():
    from faster_voxelpose_amd import _capi as capi
    T.case_argument_limits(capi.load(), DEV)
    torch.cuda.synchronize()


@pytest.mark.parametrize("case", ["tiny_g_b2_all", "panoptic_g_b2_thr"])
def test_model_tracker_attribute(case):
    from faster_voxelpose_amd.core.tracking import PoseTracker
    model, cams, rt, heat, meta = _model(case)
    kw = dict(meta=meta, input_heatmaps=heat, cameras=cams, resize_transform=rt)
    with torch.no_grad():
        plain = model(**kw)
        assert model.tracker is None and model.last_tracks is None
        model.tracker = PoseTracker(model.cfg)
        alone = PoseTracker(model.cfg)
        for _ in range(2):                               # the second forward starts from the state the first left
            out = model(**kw)
            want = alone.update(out[0], meta)
            torch.cuda.synchronize()
            for a, b in zip(out[:3], plain[:3]):
                assert T.same(a, b)
            for a, b in zip(model.last_tracks, want):
                assert T.same(a, b)
    for k, v in alone.state().items():
        assert T.same(model.tracker.state()[k], v)
    valid = out[0][:, :, 0, 3] >= 0
    assert valid.any() and ((model.last_tracks[0] >= 0) == valid).all()


def test_graphed_forward_with_tracker():
    """One capture, reset() after it, three replays with different inputs: ids and state equal three eager forwards from a
    fresh tracker."""
    from faster_voxelpose_amd.core.tracking import PoseTracker
    from faster_voxelpose_amd.models.faster_voxelpose import GraphedForward
    model, cams, rt, heat, meta = _model("tiny_g_b2_all")
    inputs = _inputs(model, cams, meta, heat, (21, 22, 23))
    model.tracker = PoseTracker(model.cfg)
    gf = GraphedForward(model, meta, heat, cams, rt)
    assert int(model.tracker.state()["next_id"][0]) > 0, "warm-up and capture runs advance the state"
    model.tracker.reset()
    static = model.last_tracks                           # the graph's static tensors, rewritten by every replay
    got = []
    for x in inputs:
        out = gf(x)
        torch.cuda.synchronize()
        got.append([t.clone() for t in (out[0],) + tuple(static)] + [model.tracker.state()])
    model.tracker = PoseTracker(model.cfg)
    with torch.no_grad():
        for x, g in zip(inputs, got):
            out = model(meta=meta, input_heatmaps=x, cameras=cams, resize_transform=rt)
            torch.cuda.synchronize()
            assert T.same(out[0], g[0])
            for a, b in zip(model.last_tracks, g[1:4]):
                assert T.same(a, b)
            for k, v in model.tracker.state().items():
                assert T.same(v, g[4][k])
    assert int(model.tracker.state()["next_id"][0]) > 0


def test_pipelined_forward_tracker_on_the_consumer_stream():
    """PipelinedForward(depth=2), four batches, tracker.update on the current stream in submit order after each event:
    equals the serial forwards."""
    from faster_voxelpose_amd import _capi as capi
    from faster_voxelpose_amd.core.tracking import PoseTracker
    from faster_voxelpose_amd.models.faster_voxelpose import PipelinedForward
    model, cams, rt, heat, meta = _model("tiny_g_b2_all")
    inputs = _inputs(model, cams, meta, heat, (31, 32, 33, 34))
    serial, want = PoseTracker(model.cfg), []
    with torch.no_grad():
        for x in inputs:
            out = model(meta=meta, input_heatmaps=x, cameras=cams, resize_transform=rt)
            want.append([t.clone() for t in serial.update(out[0], meta)])
    torch.cuda.synchronize()
    model.tracker = serial
    with pytest.raises(capi.FvpError):
        PipelinedForward(model, depth=2)
    model.tracker = None
    pipe = PipelinedForward(model, depth=2)
    tracker, got = PoseTracker(model.cfg), []
    for x in inputs:
        out, ev = pipe.submit(meta=meta, input_heatmaps=x, cameras=cams, resize_transform=rt)
        ev.wait()
        pipe.consume(out)
        got.append(tracker.update(out[0], meta))
    pipe.synchronize()
    torch.cuda.synchronize()
    for g, w in zip(got, want):
        for a, b in zip(g, w):
            assert T.same(a, b)
    for k, v in serial.state().items():
        assert T.same(tracker.state()[k], v)
    assert int(tracker.state()["next_id"][0]) > 0
