#!/usr/bin/env python
"""Joint visibility (fvp_joint_visibility): the call alone, HIP-event timed, next to the route a user had
before - ``fused_poses.cpu()`` and ``views.cpu()``, the same definition in numpy on the host (the yardstick of
tests/visibility_cases.py: vectorised over (view, person, joint), a Python loop over frames, persons and primitives), the three
results copied back to the device - alternating window by window in the same job.  The host route's results are checked
against the kernel's, bit for bit, before anything is timed.

Shape: B = 8 frames x V = 5 cameras on a 5 m ring x N = 10 people x J = 15 joints, L = 16 primitives (14 limbs of 60 mm, a
110 mm head sphere, a 140 mm torso capsule), guard 50 mm: the seeded random scene of the tests, every slot valid."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import visibility_cases as VC  # noqa: E402
from bench_track import window  # noqa: E402
from faster_voxelpose_amd.utils.visibility import JointVisibility  # noqa: E402


def main(args):
    dev = "cuda:0"
    B, V, N = args.batch, args.views, args.people
    prims, radius = VC.body15()
    case = VC.random_scene(B, V, N, 15, prims, radius, seed=13, guard=50.0, spoil=False)
    jv = JointVisibility(15, prims=prims, radius=radius, guard=50.0)
    t = {k: torch.from_numpy(case[k]).to(dev) for k in ("poses", "cams", "frame_set", "views")}

    def kernel(i):
        return jv(t["poses"], t["cams"], t["frame_set"], views=t["views"], frame_size=(VC.HS, VC.WS))

    def host(i):
        c = dict(case, poses=t["poses"].cpu().numpy(), views=t["views"].cpu().numpy())
        return [torch.from_numpy(a).to(dev) for a in VC.reference(c)]

    got, want = kernel(0), host(0)
    torch.cuda.synchronize()
    for g, w in zip(got, want):
        assert torch.equal(g.view(torch.int32), w.view(torch.int32)), "the host route and the kernel disagree"
    occ = got[0].cpu().numpy()
    for i in range(args.warmup):
        kernel(i)
    torch.cuda.synchronize()
    times = {"kernel": [], "host": []}
    for _ in range(args.repeats):                    # alternating windows: both legs see the same clocks
        times["kernel"].append(window(kernel, args.iters))
        times["host"].append(window(host, args.host_iters))
    print(torch.cuda.get_device_name(0))
    print(f"== B = {B} frames x V = {V} views x N = {N} people x J = 15 joints = {occ.size} joint-views, L = {len(prims)} primitives "
          f"per person ({occ.size * N * len(prims)} segment pairs at most), guard 50 mm; {100 * np.mean(occ >= 0):.1f} % occluded, "
          f"{100 * np.mean(occ == -1):.1f} % visible; {args.warmup} warm-up calls, median / min / max over {args.repeats} windows of "
          f"{args.iters} calls ({args.host_iters} for the host route)")
    names = {"kernel": "fvp_joint_visibility (k_joint_visibility, one launch, no host sync)       ",
             "host": "poses, views .cpu() + the definition in numpy + results to the device "}
    for k, ts in times.items():
        print(f"{names[k]} {statistics.median(ts):10.1f} us  (min {min(ts):.1f}, max {max(ts):.1f})")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--views", type=int, default=5)
    ap.add_argument("--people", type=int, default=10)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--host-iters", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=20)
    main(ap.parse_args())
