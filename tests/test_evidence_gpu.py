"""fvp_joint_evidence of the shipped library on the MI355X: the reference's own values (tests/golden/evidence.npz), the
cross-check against fvp_project_whole at voxel centres, the model-level attribute and a captured graph.  Bit for bit."""
import pytest
import torch

import evidence_cases as E
import fvp_synthetic as S
from cases import make_inputs, make_weights

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _engine(shape):
    from faster_voxelpose_amd.engine import HotPath
    cfg = S.make_cfg(shape, device=DEV, min_score=-1.0)
    cams, seq = S.load_cameras(shape)
    return HotPath(cfg), cfg, cams, seq, S.resize_transform(cfg)


def _model(case):
    from faster_voxelpose_amd.models import faster_voxelpose as FV
    cfg, cams, seq, rt, heat, meta, _ = make_inputs(case, device=DEV)
    model = FV.get(cfg).to(DEV)
    model.load_state_dict(make_weights(case, model.state_dict()))
    return model, cams, rt.to(DEV), heat.to(DEV), meta


@pytest.mark.parametrize("shape", E.SHAPES)
def test_golden_from_the_reference(shape):
    E.check_golden(_engine(shape)[0], shape)


@pytest.mark.parametrize("shape,B,N,invalid", [("panoptic", 2, 10, [(0, 3), (1, 9)]), ("shelf", 1, 10, [])])
def test_voxel_centres_equal_the_whole_space_cubes(shape, B, N, invalid):
    engine, cfg, cams, seq, rt = _engine(shape)
    assert engine.JP == {"panoptic": 16, "shelf": 20}[shape]
    E.check_against_cubes(engine, cfg, cams, seq, rt, B, N, invalid=invalid)
    torch.cuda.synchronize()


@pytest.mark.parametrize("case", ["tiny_g_b2_all", "panoptic_g_b2_thr"])
def test_model_evidence_attribute(case):
    model, cams, rt, heat, meta = _model(case)
    kw = dict(meta=meta, input_heatmaps=heat, cameras=cams, resize_transform=rt)
    with torch.no_grad():
        plain = model(**kw)
        assert model.last_evidence is None
        model.evidence = True
        out = model(**kw)
        views, conf = model.last_evidence
        v2, c2 = model.joint_evidence(out[0], heat, meta, cams, rt)
    torch.cuda.synchronize()
    for a, b in zip(out[:3], plain[:3]):
        assert E.same_bits(a, b)
    assert E.same_bits(views, v2) and E.same_bits(conf, c2)
    valid = out[0][:, :, 0, 3] >= 0
    assert valid.any() and torch.isfinite(views).all()
    assert (conf[~valid] == 0).all() and (conf[valid] > 0).any()


def test_graphed_forward_with_evidence():
    """One capture on a single stream, two replays with different inputs: each equals the eager forward."""
    from faster_voxelpose_amd.models.faster_voxelpose import GraphedForward
    model, cams, rt, heat, meta = _model("tiny_g_b2_all")
    model.evidence = True
    cfg = model.cfg
    inputs = [S.heatmaps_blobs(cfg, cams, meta["seq"][0], heat.shape[0], people=2, seed=s).to(DEV) for s in (21, 22)]
    gf = GraphedForward(model, meta, heat, cams, rt)
    static = model.last_evidence                       # the graph's static tensors, rewritten by every replay
    got = []
    for x in inputs:
        out = gf(x)
        torch.cuda.synchronize()
        got.append([t.clone() for t in (out[0],) + tuple(static)])
    assert not E.same_bits(got[0][1], got[1][1]), "the two inputs must give different evidence"
    with torch.no_grad():
        for x, g in zip(inputs, got):
            out = model(meta=meta, input_heatmaps=x, cameras=cams, resize_transform=rt)
            torch.cuda.synchronize()
            assert E.same_bits(out[0], g[0])
            assert E.same_bits(model.last_evidence[0], g[1]) and E.same_bits(model.last_evidence[1], g[2])
