"""fvp_track_smooth of the shipped library on the MI355X: every case of tests/smooth_cases.py against the independent fp32
numpy restatement of the definition, bit for bit, then the model attribute, a captured graph, the pipelined forward with
tracker and smoother on the consumer stream, and the refusals."""
import pytest
import torch

import fvp_synthetic as FS
import smooth_cases as S
from cases import make_inputs, make_weights

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture
def mk():
    from faster_voxelpose_amd.core.smoothing import PoseSmoother
    from faster_voxelpose_amd.core.tracking import PoseTracker

    def make(N, J, nseq, T, max_age, **kw):
        tr = PoseTracker((N, J), nseq=nseq, max_tracks=T, max_age=max_age, device=DEV)
        return tr, PoseSmoother(tr, **kw)
    return make


@pytest.fixture
def mk_shape():
    from faster_voxelpose_amd.core.smoothing import PoseSmoother
    return lambda N, J, T, nseq, **kw: PoseSmoother((N, J, T, nseq), device=DEV, **kw)


def _model(case):
    from faster_voxelpose_amd.models import faster_voxelpose as FV
    cfg, cams, seq, rt, heat, meta, _ = make_inputs(case, device=DEV)
    model = FV.get(cfg).to(DEV)
    model.load_state_dict(make_weights(case, model.state_dict()))
    return model, cams, rt.to(DEV), heat.to(DEV), meta


def _inputs(model, cams, meta, heat, seeds):
    return [FS.heatmaps_blobs(model.cfg, cams, meta["seq"][0], heat.shape[0], people=2, seed=s).to(DEV) for s in seeds]


def _pair(cfg, **kw):
    from faster_voxelpose_amd.core.smoothing import PoseSmoother
    from faster_voxelpose_amd.core.tracking import PoseTracker
    tr = PoseTracker(cfg)
    return tr, PoseSmoother(tr, **kw)


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


def test_null_output_combinations():
    from faster_voxelpose_amd import _capi as capi
    S.case_null_outputs(capi.load(), DEV)
    torch.cuda.synchronize()


def test_argument_limits_and_parameter_errors():
    from faster_voxelpose_amd import _capi as capi
    S.case_argument_limits(capi.load(), DEV)
    torch.cuda.synchronize()


def test_property_jitter(mk_shape):
    S.case_property_jitter(mk_shape)


def test_property_lag(mk_shape):
    S.case_property_lag(mk_shape)


def test_property_step(mk_shape):
    S.case_property_step(mk_shape)


@pytest.mark.parametrize("case,evidence", [("tiny_g_b2_all", False), ("tiny_g_b2_all", True), ("panoptic_g_b2_thr", True)])
def test_model_smoother_attribute(case, evidence):
    """The tuple equals a plain forward's; last_smooth equals a standalone update from the same prior state, with
    last_evidence[1] as joint_conf when model.evidence is on."""
    model, cams, rt, heat, meta = _model(case)
    kw = dict(meta=meta, input_heatmaps=heat, cameras=cams, resize_transform=rt)
    with torch.no_grad():
        plain = model(**kw)
        assert model.smoother is None and model.last_smooth is None
        model.evidence = evidence
        model.tracker, model.smoother = _pair(model.cfg, conf_min=0.3)
        alone_t, alone = _pair(model.cfg, conf_min=0.3)
        for _ in range(2):                               # the second forward starts from the state the first left
            out = model(**kw)
            ids, slots, _ = alone_t.update(out[0], meta)
            want = alone.update(out[0], ids, slots, joint_conf=model.last_evidence[1] if evidence else None, meta=meta)
            torch.cuda.synchronize()
            for a, b in zip(out[:3], plain[:3]):
                assert S.same(a, b)
            for a, b in zip(model.last_smooth, want):
                assert S.same(a, b)
    for k, v in alone.state().items():
        assert S.same(model.smoother.state()[k], v)
    smooth, tp, ts = model.last_smooth
    valid = out[0][:, :, 0, 3] >= 0
    assert valid.any() and S.same(smooth[~valid], out[0][~valid]) and S.same(smooth[..., 3:], out[0][..., 3:])
    seen = (ts[..., 0] >= 0) & (ts[..., 1] == 0)
    assert seen.sum() == valid.sum() and (evidence or (tp[..., 3][seen] == 1).all())


def test_graphed_forward_with_smoother():
    """One capture, reset() of both after it, three replays with different inputs: last_smooth and the filter state equal
    three eager forwards from a fresh pair."""
    from faster_voxelpose_amd.models.faster_voxelpose import GraphedForward
    model, cams, rt, heat, meta = _model("tiny_g_b2_all")
    inputs = _inputs(model, cams, meta, heat, (21, 22, 23))
    model.tracker, model.smoother = _pair(model.cfg)
    gf = GraphedForward(model, meta, heat, cams, rt)
    assert (model.smoother.state()["flt_id"] >= 0).any(), "warm-up and capture runs advance the state"
    model.tracker.reset()
    model.smoother.reset()
    static = model.last_smooth                           # the graph's static tensors, rewritten by every replay
    got = []
    for x in inputs:
        out = gf(x)
        torch.cuda.synchronize()
        got.append([t.clone() for t in (out[0],) + tuple(static)] + [model.smoother.state()])
    model.tracker, model.smoother = _pair(model.cfg)
    with torch.no_grad():
        for x, g in zip(inputs, got):
            out = model(meta=meta, input_heatmaps=x, cameras=cams, resize_transform=rt)
            torch.cuda.synchronize()
            assert S.same(out[0], g[0])
            for a, b in zip(model.last_smooth, g[1:4]):
                assert S.same(a, b)
            for k, v in model.smoother.state().items():
                assert S.same(v, g[4][k])
    assert (model.smoother.state()["flt_id"] >= 0).any()


def test_pipelined_forward_smoother_on_the_consumer_stream_and_the_refusals():
    """PipelinedForward(depth=2), four batches, tracker.update + smoother.update on the current stream in submit order after
    each event: equals the serial forwards.  A model that carries a smoother is refused by the pipeline; a smoother without
    a tracker is refused by the forward."""
    from faster_voxelpose_amd import _capi as capi
    from faster_voxelpose_amd.models.faster_voxelpose import PipelinedForward
    model, cams, rt, heat, meta = _model("tiny_g_b2_all")
    inputs = _inputs(model, cams, meta, heat, (31, 32, 33, 34))
    model.tracker, model.smoother = _pair(model.cfg)
    want = []
    with torch.no_grad():
        for x in inputs:
            model(meta=meta, input_heatmaps=x, cameras=cams, resize_transform=rt)
            want.append([t.clone() for t in model.last_smooth])
    torch.cuda.synchronize()
    serial = model.smoother
    with pytest.raises(capi.FvpError):
        PipelinedForward(model, depth=2)                 # tracker and smoother
    model.tracker = None
    with pytest.raises(capi.FvpError):
        PipelinedForward(model, depth=2)                 # the smoother alone
    with pytest.raises(capi.FvpError), torch.no_grad():
        model(meta=meta, input_heatmaps=inputs[0], cameras=cams, resize_transform=rt)      # a smoother without a tracker
    model.smoother = None
    pipe = PipelinedForward(model, depth=2)
    tracker, smoother = _pair(model.cfg)
    got = []
    for x in inputs:
        out, ev = pipe.submit(meta=meta, input_heatmaps=x, cameras=cams, resize_transform=rt)
        ev.wait()
        pipe.consume(out)
        ids, slots, _ = tracker.update(out[0], meta)
        got.append(smoother.update(out[0], ids, slots, meta=meta))
    pipe.synchronize()
    torch.cuda.synchronize()
    for g, w in zip(got, want):
        for a, b in zip(g, w):
            assert S.same(a, b)
    for k, v in serial.state().items():
        assert S.same(smoother.state()[k], v)
    assert (smoother.state()["flt_id"] >= 0).any()
