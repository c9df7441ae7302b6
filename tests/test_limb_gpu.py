"""fvp_limb_learn / fvp_limb_fit of the shipped library on the MI355X: every case of tests/limb_cases.py against the independent
fp32 numpy restatement of the definition, bit for bit, then LimbModel behind a real forward (with the evidence kernel's
joint_conf, and on the smoother's poses), forward + learn + fit captured in one hipGraph, and the pipelined forward with
tracker -> limb model on the consumer stream."""
import pytest
import torch

import fvp_synthetic as FS
import limb_cases as S
from cases import make_inputs, make_weights

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TINY_LIMBS = [(0, 1), (1, 2), (2, 3), (3, 4), (0, 4)]    # the tiny configuration has 5 joints: no default skeleton; a cycle
KW = dict(conf_min=0.3, min_frames=2, gate_mm=200.0)


@pytest.fixture
def mk():
    from faster_voxelpose_amd.core.skeleton import LimbModel
    from faster_voxelpose_amd.core.tracking import PoseTracker

    def make(N, J, nseq, T, max_age, limbs, **kw):
        tr = PoseTracker((N, J), nseq=nseq, max_tracks=T, max_age=max_age, device=DEV)
        return tr, LimbModel(tr, limbs, **kw)
    return make


@pytest.fixture
def mk_shape():
    from faster_voxelpose_amd.core.skeleton import LimbModel
    return lambda N, J, T, nseq, limbs, **kw: LimbModel((N, J, T, nseq), limbs, device=DEV, **kw)


@pytest.fixture(scope="module")
def lib():
    from faster_voxelpose_amd import _capi as capi
    return capi.load()


def test_library_holds_the_two_exports(lib):
    from faster_voxelpose_amd import _capi as capi
    assert capi.ABI_VERSION >= 22 and lib.fvp_version() == capi.ABI_VERSION
    for name in ("fvp_limb_learn", "fvp_limb_fit"):
        assert name in capi.SIGNATURES and hasattr(lib, name)


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


def test_null_arguments(lib):
    S.case_null_arguments(lib, DEV)
    torch.cuda.synchronize()


def test_argument_limits_and_parameter_errors(lib):
    S.case_argument_limits(lib, DEV)
    torch.cuda.synchronize()


@pytest.mark.parametrize("J,seed", S.PROPERTY)
def test_property_walkers(mk_shape, J, seed):
    S.case_property_walkers(mk_shape, J, seed)


@pytest.mark.parametrize("J", [15, 17])
def test_property_occluded_end(mk_shape, J):
    S.case_property_occluded_end(mk_shape, J)


# ---- behind the forward ---------------------------------------------------------------------------------------------------
def _model(case="tiny_g_b2_all"):
    from faster_voxelpose_amd.models import faster_voxelpose as FV
    cfg, cams, seq, rt, heat, meta, _ = make_inputs(case, device=DEV)
    model = FV.get(cfg).to(DEV)
    model.load_state_dict(make_weights(case, model.state_dict()))
    return model, cams, rt.to(DEV), heat.to(DEV), meta


def _inputs(model, cams, meta, heat, seeds):
    return [FS.heatmaps_blobs(model.cfg, cams, meta["seq"][0], heat.shape[0], people=2, seed=s).to(DEV) for s in seeds]


def _limb(tracker, **kw):
    from faster_voxelpose_amd.core.skeleton import LimbModel
    return LimbModel(tracker, TINY_LIMBS, **dict(KW, **kw))


def _spec(lm):
    return S.Spec(lm.N, lm.J, lm.T, TINY_LIMBS, lm.nseq, **KW)


@pytest.mark.parametrize("smoother", [False, True], ids=["fused_poses", "smoothed"])
def test_limb_model_behind_a_real_forward(smoother):
    """model.tracker and model.evidence set, joint_conf = last_evidence[1]: update on fused_poses, fit on fused_poses or on
    last_smooth[0], every output and the state against the yardstick after every forward.  All sequences of the batch are
    one sequence here, so the yardstick's row is the tracker's."""
    from faster_voxelpose_amd.core.smoothing import PoseSmoother
    from faster_voxelpose_amd.core.tracking import PoseTracker
    model, cams, rt, heat, meta = _model()
    model.tracker = PoseTracker(model.cfg)
    model.evidence = True
    if smoother:
        model.smoother = PoseSmoother(model.tracker, conf_min=0.3)
    lm = _limb(model.tracker)
    S.case_behind_forward(model, lm, _spec(lm), _inputs(model, cams, meta, heat, (51, 51, 52, 51)), meta, cams, rt, smoother)


def test_forward_learn_and_fit_captured_in_one_graph():
    """The forward with model.tracker and model.evidence, then the two limb launches, captured into one hipGraph; reset()
    of both after the capture; three replays with different heatmaps: the outputs and the state after each equal three
    eager runs from a reset pair, bit for bit."""
    from faster_voxelpose_amd.core.tracking import PoseTracker
    model, cams, rt, heat, meta = _model()
    heats = _inputs(model, cams, meta, heat, (41, 41, 42))
    model.tracker = PoseTracker(model.cfg)
    model.evidence = True
    lm = _limb(model.tracker)
    static_heat = heats[0].clone()
    kw = dict(meta=meta, cameras=cams, resize_transform=rt)

    def step(h):
        out = model(input_heatmaps=h, **kw)
        ids, slots, _ = model.last_tracks
        return (out[0], ids, slots) + tuple(lm(out[0], ids, slots, joint_conf=model.last_evidence[1], meta=meta))

    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        for _ in range(2):                                                            # packs weights, fills caches
            step(static_heat)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    geo = model.engine.geo
    geo.pending = [ev for ev in geo.pending if not ev.query()]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        static_out = step(static_heat)
    assert int((lm.state()["limb_id"] >= 0).sum()) > 0, "warm-up and capture runs advance the state"
    model.tracker.reset()
    lm.reset()
    got = []
    for h in heats:
        static_heat.copy_(h)
        graph.replay()
        torch.cuda.synchronize()
        got.append(([t.clone() for t in static_out], lm.state()))
    model.tracker.reset()
    lm.reset()
    with torch.no_grad():
        for h, (outs, st) in zip(heats, got):
            now = step(h)
            torch.cuda.synchronize()
            for a, b in zip(now, outs):
                assert S.same(a, b)
            for k, v in lm.state().items():
                assert S.same(v, st[k]), k
    assert (got[-1][0][1] >= 0).any() and (got[-1][0][4] > 0).any()                  # people were seen, limbs were learned


def test_pipelined_forward_limb_model_on_the_consumer_stream():
    """PipelinedForward(depth=2), four batches, tracker.update + the limb model on the current stream in submit order after
    each event: equals the serial forwards followed by the same calls."""
    from faster_voxelpose_amd.core.tracking import PoseTracker
    from faster_voxelpose_amd.models.faster_voxelpose import PipelinedForward
    model, cams, rt, heat, meta = _model()
    inputs = _inputs(model, cams, meta, heat, (31, 31, 32, 33))
    tracker = PoseTracker(model.cfg)
    serial = _limb(tracker)
    want = []
    with torch.no_grad():
        for x in inputs:
            out = model(meta=meta, input_heatmaps=x, cameras=cams, resize_transform=rt)
            ids, slots, _ = tracker.update(out[0], meta)
            want.append([t.clone() for t in serial(out[0], ids, slots, meta=meta)])
    torch.cuda.synchronize()
    pipe = PipelinedForward(model, depth=2)
    tracker = PoseTracker(model.cfg)
    lm = _limb(tracker)
    got = []
    for x in inputs:
        out, ev = pipe.submit(meta=meta, input_heatmaps=x, cameras=cams, resize_transform=rt)
        ev.wait()
        pipe.consume(out)
        ids, slots, _ = tracker.update(out[0], meta)
        got.append(lm(out[0], ids, slots, meta=meta))
    pipe.synchronize()
    torch.cuda.synchronize()
    for g, w in zip(got, want):
        for a, b in zip(g, w):
            assert S.same(a, b)
    for k, v in serial.state().items():
        assert S.same(lm.state()[k], v)
    assert (lm.state()["limb_cnt"] >= 2).any() and (want[-1][1] > 0).any()
