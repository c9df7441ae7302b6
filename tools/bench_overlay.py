#!/usr/bin/env python
"""Skeleton overlay (fvp_draw_poses): the launch alone, HIP-event timed, next to a kernel that merely
touches every byte of the same batch - ``frames.clone()`` - alternating window by window in the same job.

Shape: B = 8 frames x V = 5 views of 1080 x 1920, N = 10 people x J = 15 joints with the Panoptic limbs.  ``views`` come from
a seeded synthetic scene laid out in pixel space: every person is a 15-joint figure about ``--height`` pixels tall, placed at
random in every view, one person in ten outside the image, a tenth of the joints behind the camera.  Coverage is the
workload, so the frames are drawn on repeatedly.  Also reported: the share of 64 x 16 tiles the overlay touches (drawn once
onto black frames with opaque, non-black colours)."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_track import window  # noqa: E402
from faster_voxelpose_amd.utils.overlay import PoseOverlay  # noqa: E402

# a standing figure in units of its height, Panoptic joint order (neck, nose, hip centre, l shoulder / elbow / wrist,
# l hip / knee / ankle, r shoulder / elbow / wrist, r hip / knee / ankle): (x, y) with y down
FIGURE = np.array([[0, .16], [0, .06], [0, .5], [-.11, .17], [-.14, .33], [-.15, .47], [-.06, .52], [-.07, .75], [-.07, .98],
                   [.11, .17], [.14, .33], [.15, .47], [.06, .52], [.07, .75], [.07, .98]], np.float32)


def make_views(B, V, N, Hs, Ws, height, seed=0):
    rng = np.random.default_rng(seed)
    views = np.zeros((B, V, N, 15, 4), np.float32)
    scale = height * rng.uniform(0.6, 1.4, size=(B, V, N, 1, 1))
    origin = rng.uniform([0, -0.2 * height], [Ws, Hs - 0.8 * height], size=(B, V, N, 1, 2))
    origin[rng.random((B, V, N)) < 0.1] += (2 * Ws, 0)                     # outside this camera's image
    lean = rng.normal(0, 0.03, size=(B, V, N, 15, 2))
    views[..., :2] = origin + scale * (FIGURE + lean)
    views[..., 2] = np.where(rng.random((B, V, N, 15)) < 0.1, -1.0, 3000.0)
    views[..., 3] = rng.random((B, V, N, 15))
    return views


def main(args):
    dev = "cuda:0"
    B, V, N, Hs, Ws = args.batch, args.views, args.people, args.height_px, args.width_px
    views = torch.from_numpy(make_views(B, V, N, Hs, Ws, args.height)).to(dev)
    ids = torch.arange(B * N, dtype=torch.int32, device=dev).view(B, N) % 23
    frames = torch.randint(0, 256, (B, V, Hs, Ws, 3), dtype=torch.uint8, device=dev)
    ov = PoseOverlay(15, alpha=args.alpha)
    black = torch.zeros_like(frames)
    PoseOverlay(15, palette=[(255, 255, 255)]).draw(black, views, ids=ids)
    px = black.any(dim=-1)
    pad_h, pad_w = (-Hs) % 16, (-Ws) % 64
    tiles = torch.nn.functional.pad(px.to(torch.uint8), (0, pad_w, 0, pad_h)).view(B, V, (Hs + pad_h) // 16, 16, (Ws + pad_w) // 64, 64)
    touched = tiles.amax(dim=5).amax(dim=3) > 0
    del black

    def k(i):
        ov.draw(frames, views, ids=ids)

    def c(i):
        frames.clone()

    for i in range(args.warmup):
        k(i)
        c(i)
    torch.cuda.synchronize()
    ks, cs = [], []
    for _ in range(args.repeats):                    # alternating windows: both see the same clocks
        ks.append(window(k, args.iters))
        cs.append(window(c, args.iters))
    mb = frames.numel() / 1e6
    print(torch.cuda.get_device_name(0))
    print(f"== B = {B} x V = {V} frames of {Hs} x {Ws} x 3 ({mb:.0f} MB), N = {N} people x J = 15 joints + 14 limbs, figures of "
          f"about {args.height} px, radius 8 / width 4, alpha {args.alpha}; {args.warmup} warm-up calls, median / min / max "
          f"over {args.repeats} windows of {args.iters} calls")
    print(f"tiles touched: {int(touched.sum())} of {touched.numel()} ({100.0 * float(touched.float().mean()):.2f} %), pixels "
          f"covered: {100.0 * float(px.float().mean()):.3f} %")
    print(f"fvp_draw_poses (k_draw_poses, one launch, in place)   {statistics.median(ks):9.1f} us  "
          f"(min {min(ks):.1f}, max {max(ks):.1f})")
    print(f"frames.clone() (reads and writes every byte)          {statistics.median(cs):9.1f} us  "
          f"(min {min(cs):.1f}, max {max(cs):.1f})")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--views", type=int, default=5)
    ap.add_argument("--people", type=int, default=10)
    ap.add_argument("--height-px", type=int, default=1080)
    ap.add_argument("--width-px", type=int, default=1920)
    ap.add_argument("--height", type=float, default=300.0, help="height of a figure in pixels")
    ap.add_argument("--alpha", type=float, default=1.0)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=20)
    main(ap.parse_args())
