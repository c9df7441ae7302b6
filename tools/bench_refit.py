#!/usr/bin/env python
"""Camera re-fit (fvp_camera_refit_accumulate / fvp_camera_refit_solve): each call alone, HIP-event timed,
next to the route a user would take without them - points, obs, view_state and the camera table ``.cpu()``, the same
definition in numpy on the host (the yardstick of tests/recalibrate_cases.py), the result copied back to the device -
alternating window by window in the same job.  The host route's results are checked against the kernels', bit for bit,
before anything is timed.

Shape: B = 8 frames x V = 5 cameras x N = 10 people x J = 15 joints, one camera bumped by 1.5 degrees and 30 mm, 0.5 px of
pixel noise, Huber at 3 px."""
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

import recalibrate_cases as RC  # noqa: E402
from bench_track import window  # noqa: E402


def main(args):
    dev = "cuda:0"
    case = RC.scene(args.batch, args.views, args.people, 15, 13, noise=0.5, params=dict(huber_px=3.0))
    ref = RC.refiner_for(case)
    t = RC.tensors(case, dev)
    inputs = [t[k] for k in RC.TENSORS]

    def accumulate(i):
        return ref.accumulate(*inputs)

    def solve(i):
        return ref.solve(t["cams"])

    def host_accumulate(i):
        c = dict(case, **{k: t[k].cpu().numpy() for k in RC.TENSORS})
        return torch.from_numpy(RC.ref_accumulate(c)).to(dev)

    def host_solve(i):
        res = RC.ref_solve(ref.acc.cpu().numpy(), t["cams"].cpu().numpy(), RC._prm(case))
        return [torch.from_numpy(res[k]).to(dev) for k in RC.SOLVE_OUTPUTS]

    ref.reset()
    acc = accumulate(0).cpu().numpy()
    RC.assert_equal(dict(acc=acc), dict(acc=host_accumulate(0).cpu().numpy()), "the host route and the accumulate kernel")
    got = RC.as_dict(solve(0))
    RC.assert_equal(got, {k: w.cpu().numpy() for k, w in zip(RC.SOLVE_OUTPUTS, host_solve(0))}, "the host route and the solve kernel")
    for i in range(args.warmup):
        accumulate(i)
        solve(i)
    torch.cuda.synchronize()
    ref.reset()
    accumulate(0)                                    # the solve legs see one batch's sums
    times = {"solve": [], "host_solve": [], "accumulate": [], "host_accumulate": []}
    for _ in range(args.repeats):                    # alternating windows: all legs see the same clocks
        times["solve"].append(window(solve, args.iters))
        times["host_solve"].append(window(host_solve, args.host_iters))
    for _ in range(args.repeats):
        times["accumulate"].append(window(accumulate, args.iters))
        times["host_accumulate"].append(window(host_accumulate, args.host_iters))
    print(torch.cuda.get_device_name(0))
    print(f"== B = {args.batch} frames x V = {args.views} views x N = {args.people} people x J = 15 joints = "
          f"{case['view_state'].size} joint-views, {int(acc[..., 29].sum())} counting, {int(acc[..., 30].sum())} beyond the Huber "
          f"threshold; states {got['cal_state'].reshape(-1).tolist()}, the bumped camera's step {got['cal_stats'][0, 0, 0]:.4f} rad "
          f"{got['cal_stats'][0, 0, 1]:.2f} mm, rms {got['cal_stats'][0, 0, 2]:.2f} -> {got['cal_stats'][0, 0, 3]:.2f} px; "
          f"{args.warmup} warm-up calls, median / min / max over {args.repeats} windows of {args.iters} calls "
          f"({args.host_iters} for the host routes)")
    names = {"accumulate": "fvp_camera_refit_accumulate (k_camera_refit_accumulate, one launch, no host sync)",
             "host_accumulate": "points, obs, view_state, cams .cpu() + the definition in numpy + acc to the device ",
             "solve": "fvp_camera_refit_solve (k_camera_refit_solve, one launch, no host sync)          ",
             "host_solve": "acc, cams .cpu() + the definition in numpy + results to the device               "}
    for k in names:
        ts = times[k]
        print(f"{names[k]} {statistics.median(ts):10.1f} us  (min {min(ts):.1f}, max {max(ts):.1f})")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--views", type=int, default=5)
    ap.add_argument("--people", type=int, default=10)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--host-iters", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=20)
    main(ap.parse_args())
