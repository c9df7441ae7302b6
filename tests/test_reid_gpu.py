"""fvp_person_signature and fvp_track_reid of the shipped library on the MI355X: every case of tests/reid_cases.py against the
independent numpy restatement, bit for bit - outputs and every state array after every call; every edge of the state machine;
chunk invariance; every argument error; the closed loop with painted people, the evidence kernel's pixels and a real
PoseTracker; the two launches captured behind the forward in one hipGraph."""
import numpy as np
import pytest
import torch

import fvp_synthetic as S
import reid_cases as RC
from cases import make_inputs, make_weights

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TINY_LIMBS = [(0, 1), (1, 2), (2, 3), (3, 4)]            # the tiny configuration has 5 joints: no default skeleton


@pytest.fixture(scope="module")
def lib():
    from faster_voxelpose_amd import _capi as capi
    return capi.load()


def test_library_holds_the_two_exports(lib):
    from faster_voxelpose_amd import _capi as capi
    assert capi.ABI_VERSION >= 20 and lib.fvp_version() == capi.ABI_VERSION
    for name in ("fvp_person_signature", "fvp_track_reid"):
        assert name in capi.SIGNATURES and hasattr(lib, name)


@pytest.mark.parametrize("name", RC.SIG_CASES)
def test_signatures_equal_the_yardstick(lib, name):
    RC.sig_check(lib, DEV, name)


def test_signature_outputs_may_be_null(lib):
    RC.sig_check_null_outputs(lib, DEV)


def test_signature_argument_errors(lib):
    RC.sig_argument_errors(lib, DEV)


@pytest.mark.parametrize("name", list(RC.SCENARIOS))
def test_state_machine_edge(lib, name):
    RC.SCENARIOS[name](lib, DEV)


@pytest.mark.parametrize("seed,n,t,g,p,nseq", RC.RANDOM_STREAMS)
def test_random_streams_and_chunk_invariance(lib, seed, n, t, g, p, nseq):
    RC.random_stream_check(lib, DEV, seed, n, t, g, p, nseq)


def test_reid_argument_errors(lib):
    RC.reid_argument_errors(lib, DEV)


@pytest.mark.parametrize("variant", ["return", "twins"])
def test_closed_loop(variant):
    RC.closed_loop_check(None, DEV, variant)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                                                                     b.view(torch.int32) if b.dtype == torch.float32 else b)


def test_reid_captured_behind_the_forward_in_one_graph():
    """The forward with model.tracker and model.evidence, then the two re-ID launches on static frames, captured into one
    hipGraph; reset() after the capture; three replays with different heatmaps and frames: the outputs and the state after
    each equal three eager runs from a reset object."""
    from faster_voxelpose_amd.core.reid import PersonReId
    from faster_voxelpose_amd.core.tracking import PoseTracker
    from faster_voxelpose_amd.models import faster_voxelpose as FV
    case = "tiny_g_b2_all"
    cfg, cams, seq, rt, heat, meta, _ = make_inputs(case, device=DEV)
    model = FV.get(cfg).to(DEV)
    model.load_state_dict(make_weights(case, model.state_dict()))
    rt, heat = rt.to(DEV), heat.to(DEV)
    B, V = heat.shape[:2]
    ws, hs = cfg.DATASET.ORI_IMAGE_SIZE
    gen = torch.Generator().manual_seed(9)
    heats = [S.heatmaps_blobs(cfg, cams, seq, B, people=2, seed=s).to(DEV) for s in (41, 42, 43)]
    frames = [torch.randint(0, 256, (B, V, hs, ws, 3), generator=gen, dtype=torch.uint8).to(DEV) for _ in range(3)]
    model.tracker = PoseTracker(cfg)
    model.evidence = True
    reid = PersonReId(cfg, limbs=TINY_LIMBS, limb_part=[0, 0, 1, 1], min_samples=1, min_frames=2, window=4, max_age=1)
    static_heat, static_frames = heats[0].clone(), frames[0].clone()
    kw = dict(meta=meta, cameras=cams, resize_transform=rt)

    def step(h, f):
        out = model(input_heatmaps=h, **kw)
        ids, slots, _ = model.last_tracks
        views, conf = model.last_evidence
        return out[0], ids, slots, reid(f, views, ids, slots, joint_conf=conf, meta=meta)

    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        for _ in range(2):                                                            # packs weights, fills caches
            step(static_heat, static_frames)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    geo = model.engine.geo
    geo.pending = [ev for ev in geo.pending if not ev.query()]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        static_out = step(static_heat, static_frames)
    assert int((reid.state()["slot_tid"] >= 0).sum()) > 0, "warm-up and capture runs advance the state"
    model.tracker.reset()
    reid.reset()
    got = []
    for h, f in zip(heats, frames):
        static_heat.copy_(h)
        static_frames.copy_(f)
        graph.replay()
        torch.cuda.synchronize()
        fused, ids, slots, (pids, rstate, rsim) = static_out
        got.append(([t.clone() for t in (fused, ids, slots, pids, rstate, rsim)], reid.state()))
    model.tracker.reset()
    reid.reset()
    with torch.no_grad():
        for h, f, (outs, st) in zip(heats, frames, got):
            fused, ids, slots, (pids, rstate, rsim) = step(h, f)
            torch.cuda.synchronize()
            for a, b in zip((fused, ids, slots, pids, rstate, rsim), outs):
                assert _same(a, b)
            for k, v in reid.state().items():
                assert _same(v, st[k]), k
    assert (got[-1][0][3] >= 0).any() and (got[-1][0][4] >= 1).any()                  # people were seen and decided
    assert np.isin(got[-1][0][4].cpu().numpy(), (-1, 0, 1, 2)).all()
