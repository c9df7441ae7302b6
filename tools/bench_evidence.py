#!/usr/bin/env python
"""Joint evidence (fvp_joint_evidence): the launch alone, HIP-event timed, next to the only route the tree
offered before for the same numbers - torch ops on the same device (camera model, clamp, resize transform, grid_sample at
the joints, view mean), alternating window by window in the same job.  Inputs (staged heatmaps and poses) rotate so that
no window re-reads what the previous launch left in the caches.

--headline [bench.py arguments]: run bench.py's own measurement with ``model.evidence = True`` on every model it builds
(bench.py itself is not changed: FV.get is wrapped for this process)."""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import fvp_synthetic as S  # noqa: E402
from faster_voxelpose_amd.engine import HotPath, _ptr  # noqa: E402
from faster_voxelpose_amd.models import faster_voxelpose as FV  # noqa: E402


def torch_route(cam, g, heat, fused):
    """views [B,V,N,J,4], joint_conf [B,N,J] with torch ops.  cam: [V,24] table; heat [B,V,J,H,W]; fused [B,N,J,5]."""
    B, V, J, H, W = heat.shape
    N = fused.shape[1]
    x = fused[..., :3].reshape(B, 1, N * J, 3)
    R, T = cam[:, 0:9].view(1, V, 3, 3), cam[:, 9:12].view(1, V, 1, 3)
    f, c, k, p = cam[:, 12:14], cam[:, 14:16], cam[:, 16:19], cam[:, 19:21]
    xc = torch.matmul(x - T, R.transpose(2, 3))                                   # [B,V,NJ,3]
    y = xc[..., :2] / (xc[..., 2:3] + 1e-5)
    r = (y * y).sum(-1)
    k0, k1, k2 = (k[:, i].view(1, V, 1) for i in range(3))
    p0, p1 = (p[:, i].view(1, V, 1) for i in range(2))
    d = 1 + k0 * r + k1 * r * r + k2 * r * r * r
    y0, y1 = y[..., 0], y[..., 1]
    u = y0 * d + 2 * p0 * y0 * y1 + p1 * (r + 2 * y0 * y0)
    v = y1 * d + 2 * p1 * y0 * y1 + p0 * (r + 2 * y1 * y1)
    px = torch.stack([f[:, 0].view(1, V, 1) * u + c[:, 0].view(1, V, 1), f[:, 1].view(1, V, 1) * v + c[:, 1].view(1, V, 1)], -1)
    q = px.clamp(-1.0, g.clamp_max)
    rt = torch.tensor(list(g.rt), device=heat.device).view(2, 3)
    a = q @ rt[:, :2].T + rt[:, 2]
    a = a * torch.tensor([g.hm_w, g.hm_h], device=heat.device) / torch.tensor([g.img_w, g.img_h], device=heat.device)
    grid = (a / torch.tensor([g.hm_w - 1, g.hm_h - 1], device=heat.device) * 2.0 - 1.0).clamp(-1.1, 1.1)
    s = F.grid_sample(heat.view(B * V, J, H, W), grid.view(B * V, 1, N * J, 2), align_corners=True)     # [BV,J,1,NJ]
    jj = (torch.arange(N * J, device=heat.device) % J).view(1, 1, N * J)
    s = s[:, :, 0, :].gather(1, jj.expand(B * V, 1, N * J))[:, 0].view(B, V, N, J)
    valid = (fused[:, :, 0, 3] >= 0).view(B, 1, N, 1)
    views = torch.cat([px.view(B, V, N, J, 2), xc[..., 2].view(B, V, N, J, 1), s.unsqueeze(-1)], -1) * valid.unsqueeze(-1)
    conf = (s * valid).mean(1).clamp(0.0, 1.0)
    return views, conf


def window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(iters):
        fn(i)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters * 1e3           # us per call


def kernel_bench(args):
    dev = "cuda:0"
    cfg = S.make_cfg(args.config, device=dev, min_score=-1.0)
    cams, seq = S.load_cameras(args.config)
    rt = S.resize_transform(cfg).to(dev)
    eng = HotPath(cfg)
    B, N, J, V = args.batch, args.people, eng.J, cfg.DATASET.CAMERA_NUM
    meta = {"seq": [seq] * B}
    g = eng.geom(rt)
    g.V = V
    fs = eng.frame_sets(meta, cams, V)
    gen = torch.Generator().manual_seed(1)
    size, centre = torch.tensor(cfg.CAPTURE_SPEC.SPACE_SIZE), torch.tensor(cfg.CAPTURE_SPEC.SPACE_CENTER)
    heats, hcls, poses = [], [], []
    for i in range(args.inputs):
        h = S.heatmaps_uniform(cfg, B, seed=30 + i).to(dev)
        heats.append(h)
        hcls.append(eng.heat_cl(h, g).clone())
        p = torch.zeros(B, N, J, 5)
        p[..., :3] = (torch.rand(B, N, J, 3, generator=gen) - 0.5) * size + centre
        p[:, N - 2:, :, 3] = -1.0                                                # two empty slots per frame, as in a live batch
        poses.append(p.to(dev))
    views = torch.empty((B, V, N, J, 4), device=dev)
    conf = torch.empty((B, N, J), device=dev)
    cam = eng.geo.cams
    st = eng.stream()

    def k(i):
        j = i % args.inputs
        eng._call("fvp_joint_evidence", _ptr(hcls[j]), _ptr(cam), _ptr(fs), _ptr(poses[j]), B, N, C.byref(g), _ptr(views),
                  _ptr(conf), st)

    def t(i):
        j = i % args.inputs
        return torch_route(cam[0], g, heats[j], poses[j])

    k(0)
    tv, tc = t(0)
    torch.cuda.synchronize()
    dv = (views[..., :3] - tv[..., :3]).abs().max().item(), (views[..., 3] - tv[..., 3]).abs().max().item()
    dc = (conf - tc).abs().max().item()
    for i in range(args.warmup):
        k(i)
        t(i)
    torch.cuda.synchronize()
    ks, ts = [], []
    for _ in range(args.repeats):                    # alternating windows: both routes see the same clocks
        ks.append(window(k, args.iters))
        ts.append(window(t, args.iters))
    print(torch.cuda.get_device_name(0))
    print(f"== {args.config}: B = {B} frames x N = {N} slots x J = {J} joints x V = {V} views = {B * N * J * V} items, "
          f"{args.inputs} inputs in rotation ({hcls[0].numel() * 4 / 1e6:.0f} MB of staged heatmaps each); {args.warmup} warm-up "
          f"calls, median / min / max over {args.repeats} windows of {args.iters} calls")
    print(f"fvp_joint_evidence (k_joint_evidence, one launch)   {statistics.median(ks):8.1f} us  (min {min(ks):.1f}, max {max(ks):.1f})")
    print(f"torch ops on the same device (camera model + grid_sample + mean)   {statistics.median(ts):8.1f} us  "
          f"(min {min(ts):.1f}, max {max(ts):.1f})")
    print(f"max |torch route - kernel|: pixel / depth {dv[0]:.3e}, sample {dv[1]:.3e}, joint_conf {dc:.3e}")


def headline(rest):
    import bench
    orig = FV.get

    def get(cfg):
        m = orig(cfg)
        m.evidence = True
        return m
    FV.get = get
    sys.argv = ["bench.py"] + rest
    bench.main()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--headline", action="store_true")
    ap.add_argument("--config", default="panoptic")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--people", type=int, default=10)
    ap.add_argument("--inputs", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=20)
    a, rest = ap.parse_known_args()
    headline(rest) if a.headline else kernel_bench(a)
