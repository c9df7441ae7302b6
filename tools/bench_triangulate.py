#!/usr/bin/env python
"""Triangulated joints (fvp_triangulate_joints): the call alone, HIP-event timed, with and without the
per-camera residual, next to the route a user had before - ``fused_poses.cpu()`` and ``heat_cl.cpu()``, the same definition in
numpy on the host (the yardstick of tests/triangulate_cases.py: vectorised over (frame, view, person, joint), a Python loop
over the window's cells and the views), the results copied back to the device - alternating window by window in the same
job.  The host route's results are checked against the kernel's, bit for bit, before anything is timed.

Shape: B = 8 frames x V = 5 Panoptic cameras x N = 10 people x J = 15 joints, heat maps of 240 x 128, radius 3: joints uniform in
the capture volume, a paraboloid peak wherever a view shows the joint, the fused input 20 mm off the truth."""
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

import triangulate_cases as TC  # noqa: E402
from bench_track import window  # noqa: E402


def main(args):
    dev = "cuda:0"
    case = TC.panoptic_scene(args.batch, args.people, seed=13, radius=args.radius)
    full = TC.triangulator_for(case)
    lean = TC.triangulator_for(case, per_camera=False)
    t = TC.tensors(case, dev)

    def kernel(i):
        return TC.run_class(full, t)

    def kernel_lean(i):
        return TC.run_class(lean, t)

    def host(i):
        c = dict(case, poses=t["poses"].cpu().numpy(), heat=t["heat"].cpu().numpy())
        ref = TC.reference(c)
        return [torch.from_numpy(np.ascontiguousarray(ref[k])).to(dev) for k in TC.OUTPUTS]

    got, want = TC.as_dict(kernel(0)), host(0)
    torch.cuda.synchronize()
    TC.assert_equal(got, {k: w.cpu().numpy() for k, w in zip(TC.OUTPUTS, want)}, "the host route and the kernel")
    for i in range(args.warmup):
        kernel(i)
        kernel_lean(i)
    torch.cuda.synchronize()
    times = {"kernel": [], "lean": [], "host": []}
    for _ in range(args.repeats):                    # alternating windows: all legs see the same clocks
        times["kernel"].append(window(kernel, args.iters))
        times["lean"].append(window(kernel_lean, args.iters))
        times["host"].append(window(host, args.host_iters))
    vs, cnt = got["view_state"], got["tri_count"]
    print(torch.cuda.get_device_name(0))
    print(f"== B = {args.batch} frames x V = {vs.shape[1]} views x N = {args.people} people x J = 15 joints = {vs.size} joint-views, "
          f"heat maps {case['geom']['W']} x {case['geom']['H']}, radius {args.radius} ({(2 * args.radius + 1) ** 2} cells per window); "
          f"{100 * np.mean(vs == TC.USED):.1f} % of the views used, {100 * np.mean(vs == TC.OUTSIDE):.1f} % outside, "
          f"{100 * np.mean(vs == TC.PEAK_LOW):.1f} % peak low, {100 * np.mean(vs == TC.NOT_ENCLOSED):.1f} % not enclosed; "
          f"{100 * np.mean(cnt >= 2):.1f} % of the joints triangulated, median shift {np.median(got['tri_stats'][..., 0][cnt >= 2]):.2f} mm; "
          f"{args.warmup} warm-up calls, median / min / max over {args.repeats} windows of {args.iters} calls "
          f"({args.host_iters} for the host route)")
    names = {"kernel": "fvp_triangulate_joints with cam_resid (k_triangulate_joints + k_view_residual, no host sync)",
             "lean": "fvp_triangulate_joints without cam_resid (k_triangulate_joints, one launch)            ",
             "host": "poses, heat_cl .cpu() + the definition in numpy + results to the device                 "}
    for k, ts in times.items():
        print(f"{names[k]} {statistics.median(ts):10.1f} us  (min {min(ts):.1f}, max {max(ts):.1f})")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--people", type=int, default=10)
    ap.add_argument("--radius", type=int, default=3)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--host-iters", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=20)
    main(ap.parse_args())
