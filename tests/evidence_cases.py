"""Shared by tests/test_evidence_emu.py (CPU emulator) and tests/test_evidence_gpu.py (the shipped library on the card):
the golden inputs of tests/golden/evidence.npz (make_golden_evidence.py), the voxel-centre cross-check against
fvp_project_whole, and a runner that calls the entry point on caller-owned outputs.  Every comparison is bit for bit."""
import ctypes as C
import os

import numpy as np
import torch

import fvp_synthetic as S
from common import GOLDEN_DIR

SHAPES = ("panoptic", "shelf", "campus")
_golden = {}


def golden():
    if "g" not in _golden:
        _golden["g"] = np.load(os.path.join(GOLDEN_DIR, "evidence.npz"))
    return _golden["g"]


def poses_from_points(points, flag=0.0, conf=0.5):
    """[B,N,J,3] -> fused_poses [B,N,J,5]: xyz, the slot's valid flag, the person confidence."""
    p = torch.as_tensor(points, dtype=torch.float32)
    out = torch.empty(p.shape[:-1] + (5,))
    out[..., :3] = p
    out[..., 3] = flag
    out[..., 4] = conf
    return out.contiguous()


def golden_case(shape, device):
    """cfg, cameras, resize transform, heatmaps, meta, fused_poses [1,4,J,5] and the reference's views [1,V,4,J,4] /
    joint_conf [1,4,J] of one shape set."""
    g = golden()
    cfg = S.make_cfg(shape, device=device, min_score=-1.0)
    cams, seq = S.load_cameras(shape)
    rt = S.resize_transform(cfg)
    heat = S.heatmaps_uniform(cfg, 1, int(g["heat_seed"]))
    pts = g[shape + "_points"]                                   # [P, J, 3]
    P, J = pts.shape[:2]
    V = cfg.DATASET.CAMERA_NUM
    views = np.concatenate([g[shape + "_px"], g[shape + "_depth"][..., None], g[shape + "_sample"][..., None]], axis=2)
    views = views.reshape(1, V, P, J, 4)
    conf = g[shape + "_conf"].reshape(1, P, J)
    return cfg, cams, rt, heat, {"seq": [seq]}, poses_from_points(pts[None]), views, conf


def same_bits(a, b):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    b = b.detach().cpu().numpy() if torch.is_tensor(b) else np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.int32), b.view(np.int32))


def check_golden(engine, shape):
    cfg, cams, rt, heat, meta, fused, want_views, want_conf = golden_case(shape, str(engine.device))
    dev = engine.device
    views, conf = engine.joint_evidence(fused.to(dev), heat.to(dev), meta, cams, rt.to(dev))
    views, conf = views.cpu().numpy(), conf.cpu().numpy()
    for k, name in enumerate(("px", "py", "depth", "sample")):
        bad = np.argwhere(views[..., k].view(np.int32) != want_views[..., k].view(np.int32))
        assert bad.size == 0, f"{shape}: {name} differs from the reference at {len(bad)} (b,v,n,j), first {bad[0]}: " \
                              f"{views[..., k][tuple(bad[0])]!r} vs {want_views[..., k][tuple(bad[0])]!r}"
    assert same_bits(conf, want_conf), f"{shape}: joint_conf differs from the reference"


def centre_poses(engine, B, N, invalid=(), seed=0):
    """Every joint on a randomly drawn voxel centre of the whole-space grid (engine.whole_axes values verbatim);
    slots listed in ``invalid`` [(b, n), ...] carry the flag -1.  Returns fused_poses [B,N,J,5] (CPU) and the indices."""
    gen = torch.Generator().manual_seed(seed)
    J = engine.J
    idx = [torch.randint(0, d, (B, N, J), generator=gen) for d in (engine.X, engine.Y, engine.Z)]
    ax = [a.cpu() for a in engine.whole_axes]
    fused = poses_from_points(torch.stack([ax[k][idx[k]] for k in range(3)], dim=-1))
    for b, n in invalid:
        fused[b, n, :, 3] = -1.0
    return fused, idx


def check_against_cubes(engine, cfg, cams, seq, rt, B, N, invalid=(), seed=5):
    """joint_conf at voxel centres == the cubes fvp_project_whole writes there; the view samples reproduce joint_conf."""
    dev = engine.device
    heat = S.heatmaps_uniform(cfg, B, seed).to(dev)
    meta = {"seq": [seq] * B}
    fused, (ix, iy, iz) = centre_poses(engine, B, N, invalid, seed)
    views, conf = engine.joint_evidence(fused.to(dev), heat, meta, cams, rt.to(dev))
    cubes, _ = engine.project_whole(heat, meta, cams, rt.to(dev), True, False)
    cubes = cubes.cpu()
    J, V = engine.J, heat.shape[1]
    bb = torch.arange(B).view(B, 1, 1).expand(B, N, J)
    jj = torch.arange(J).view(1, 1, J).expand(B, N, J)
    want = cubes[bb, jj, ix, iy, iz].clone()
    valid = fused[:, :, 0, 3] >= 0
    want[~valid] = 0.0
    assert valid.sum() > 0 and float(want.max()) > 0
    assert same_bits(conf, want), "joint_conf != the whole-space cube at the same voxel centre"
    # clamp((s_0 + s_1 + ... ) / V, 0, 1) in view order, every operation rounded to float32 on its own
    s = views[..., 3].cpu().numpy()                              # [B, V, N, J]
    acc = s[:, 0].copy()
    for v in range(1, V):
        acc = (acc + s[:, v]).astype(np.float32)
    mean = np.clip((acc / np.float32(V)).astype(np.float32), np.float32(0), np.float32(1))
    assert same_bits(mean, conf), "the view samples do not sum to joint_conf"
    vz = views.cpu()[~valid[:, None].expand(B, V, N)]
    assert vz.numel() == len(invalid) * V * J * 4 and (vz == 0).all(), "an invalid slot is not all zero"
    return fused, heat, meta, views, conf


def raw_call(engine, fused, heat, meta, cams, rt, views, conf):
    """fvp_joint_evidence on caller-owned outputs (either may be None), through the engine's own geometry and staging."""
    from faster_voxelpose_amd.engine import _ptr
    B, N = fused.shape[:2]
    V = heat.shape[1]
    g = engine.geom(rt)
    g.V = V
    fs = engine.frame_sets(meta, cams, V)
    hcl = engine.heat_cl(heat, g)
    return engine.lib.fvp_joint_evidence(_ptr(hcl), _ptr(engine.geo.cams), _ptr(fs), _ptr(fused), B, N, C.byref(g),
                                         _ptr(views), _ptr(conf), engine.stream())
