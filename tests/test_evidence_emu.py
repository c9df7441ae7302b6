"""fvp_joint_evidence on the CPU emulation of the kernels (tests/hipemu), through HotPath(_lib=emu): the reference's own
values (tests/golden/evidence.npz), the cross-check against fvp_project_whole at voxel centres, invalid slots, NULL outputs
and argument checks.  Every comparison is bit for bit: the call adds no arithmetic the projection kernels do not have."""
import numpy as np
import pytest
import torch

import evidence_cases as E
import fvp_synthetic as S
from cases import make_inputs, make_weights
from faster_voxelpose_amd import _capi as capi
from faster_voxelpose_amd.engine import HotPath
from faster_voxelpose_amd.models import faster_voxelpose as FV


def tiny_engine(emu_lib):
    cfg = S.make_cfg("tiny", device="cpu", min_score=-1.0)
    cams, seq = S.load_cameras("tiny")
    return HotPath(cfg, _lib=emu_lib), cfg, cams, seq, S.resize_transform(cfg)


@pytest.mark.parametrize("shape", E.SHAPES)
def test_golden_from_the_reference(shape, emu_lib):
    cfg = S.make_cfg(shape, device="cpu", min_score=-1.0)
    E.check_golden(HotPath(cfg, _lib=emu_lib), shape)


def test_voxel_centres_equal_the_whole_space_cubes(emu_lib):
    engine, cfg, cams, seq, rt = tiny_engine(emu_lib)
    assert (engine.J, engine.JP) == (5, 8)
    E.check_against_cubes(engine, cfg, cams, seq, rt, B=2, N=3)


def test_invalid_slots_null_outputs_and_every_element_written(emu_lib):
    engine, cfg, cams, seq, rt = tiny_engine(emu_lib)
    B, N, J, V = 2, 3, engine.J, 3
    invalid = [(0, 1), (1, 0), (1, 2)]
    fused, heat, meta, views, conf = E.check_against_cubes(engine, cfg, cams, seq, rt, B, N, invalid=invalid)
    for b, n in invalid:
        assert (views[b, :, n] == 0).all() and (conf[b, n] == 0).all()
    assert (conf[0, 0] > 0).all() and (views[0, :, 0, :, 2] != 0).all()
    # the flag is read from joint 0 alone, whatever the other joints carry
    f2 = fused.clone()
    f2[:, :, 1:, 3] = -1.0
    v2, c2 = engine.joint_evidence(f2, heat, meta, cams, rt)
    assert E.same_bits(v2, views) and E.same_bits(c2, conf)
    # outputs pre-filled with NaN: every element is written, by either form of the call
    nan_v = torch.full((B, V, N, J, 4), float("nan"))
    nan_c = torch.full((B, N, J), float("nan"))
    assert E.raw_call(engine, fused, heat, meta, cams, rt, nan_v, nan_c) == 0
    assert E.same_bits(nan_v, views) and E.same_bits(nan_c, conf)
    only_v = torch.full((B, V, N, J, 4), float("nan"))
    assert E.raw_call(engine, fused, heat, meta, cams, rt, only_v, None) == 0
    assert E.same_bits(only_v, views)
    only_c = torch.full((B, N, J), float("nan"))
    assert E.raw_call(engine, fused, heat, meta, cams, rt, None, only_c) == 0
    assert E.same_bits(only_c, conf)
    assert E.raw_call(engine, fused, heat, meta, cams, rt, None, None) == 10001          # FVP_EINVAL: nothing to write
    # no people / no frames: nothing is launched, nothing fails
    v0, c0 = engine.joint_evidence(fused[:, :0].contiguous(), heat, meta, cams, rt)
    assert v0.shape == (B, V, 0, J, 4) and c0.shape == (B, 0, J)


def test_wrong_dtype_device_or_shape_raises(emu_lib):
    engine, cfg, cams, seq, rt = tiny_engine(emu_lib)
    heat = S.heatmaps_uniform(cfg, 2, 3)
    meta = {"seq": [seq] * 2}
    fused, _ = E.centre_poses(engine, 2, 3)
    engine.joint_evidence(fused, heat, meta, cams, rt)
    bad = {
        "float64": fused.double(),
        "other device": torch.empty(fused.shape, device="meta"),
        "four columns": fused[..., :4].contiguous(),
        "joint count": fused[:, :, :4].contiguous(),
        "three dimensions": fused.view(6, engine.J, 5),
        "batch of the heatmaps": fused[:1].contiguous(),
        "not contiguous": fused.transpose(0, 1).contiguous().transpose(0, 1)[:, :, :, :],
    }
    assert not bad["not contiguous"].is_contiguous()
    for what, t in bad.items():
        try:
            engine.joint_evidence(t, heat, meta, cams, rt)
        except capi.FvpError:
            continue
        pytest.fail(f"fused_poses with the wrong {what} was accepted")


def test_model_evidence_attribute(emu_lib):
    """model.evidence = True: forward leaves last_evidence, bit-equal to the standalone call on the poses it returned; the
    returned tuple is what a forward without evidence returns."""
    case = "tiny_g_b2_all"
    cfg, cams, seq, rt, heat, meta, _ = make_inputs(case)
    model = FV.FasterVoxelPoseNet(cfg, _lib=emu_lib)
    model.load_state_dict(make_weights(case, model.state_dict()))
    assert model.evidence is False and model.last_evidence is None
    with torch.no_grad():
        plain = model(meta=meta, input_heatmaps=heat, cameras=cams, resize_transform=rt)
        assert model.last_evidence is None
        model.evidence = True
        out = model(meta=meta, input_heatmaps=heat, cameras=cams, resize_transform=rt)
        views, conf = model.last_evidence
        v2, c2 = model.joint_evidence(out[0], heat, meta, cams, rt)
    assert len(out) == len(plain) == 5
    for a, b in zip(out[:3], plain[:3]):
        assert E.same_bits(a, b)
    assert E.same_bits(views, v2) and E.same_bits(conf, c2)
    valid = out[0][:, :, 0, 3] >= 0
    assert valid.any() and np.isfinite(views.numpy()).all()
    assert (conf[~valid] == 0).all() and (conf[valid] > 0).any()
