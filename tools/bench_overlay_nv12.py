#!/usr/bin/env python
"""Skeleton overlay on NV12 surfaces (fvp_draw_poses_nv12): the launch alone, HIP-event timed, next to
fvp_draw_poses on RGB frames of the same size and the same poses, alternating window by window in the same job.

Shape and scene are those of tools/bench_overlay.py: B = 8 frames x V = 5 views of 1080 x 1920, N = 10 people x J = 15 joints
with the Panoptic limbs, figures of about ``--height`` pixels.  The NV12 surface is one contiguous buffer per frame (Hs rows
of luma, Hs / 2 rows of chroma) at ``--pitch`` bytes per row.  Coverage is the workload, so both surfaces are drawn on
repeatedly.  Only these two calls are timed."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

from bench_overlay import make_views  # noqa: E402
from bench_track import window  # noqa: E402
from faster_voxelpose_amd.dataset.images import Nv12Frames  # noqa: E402
from faster_voxelpose_amd.utils.overlay import PoseOverlay  # noqa: E402


def main(args):
    dev = "cuda:0"
    B, V, N, Hs, Ws = args.batch, args.views, args.people, args.height_px, args.width_px
    views = torch.from_numpy(make_views(B, V, N, Hs, Ws, args.height)).to(dev)
    ids = torch.arange(B * N, dtype=torch.int32, device=dev).view(B, N) % 23
    rgb = torch.randint(0, 256, (B, V, Hs, Ws, 3), dtype=torch.uint8, device=dev)
    buf = torch.randint(0, 256, (B, V, Hs * 3 // 2, args.pitch), dtype=torch.uint8, device=dev)
    nv12 = Nv12Frames.from_buffer(buf, Hs, Ws, standard="bt709")
    ov = PoseOverlay(15, alpha=args.alpha)
    # covered luma pixels and touched quads, drawn once onto a zeroed surface with an opaque white
    zero = torch.zeros_like(buf)
    probe = Nv12Frames.from_buffer(zero, Hs, Ws, standard="bt709")
    PoseOverlay(15, palette=[(255, 255, 255)]).draw(probe, views, ids=ids)
    covered = float((probe.y != 0).float().mean())
    quads = float((probe.uv != 0).any(dim=-1).float().mean())
    del zero, probe

    def k(i):
        ov.draw(nv12, views, ids=ids)

    def c(i):
        ov.draw(rgb, views, ids=ids)

    for i in range(args.warmup):
        k(i)
        c(i)
    torch.cuda.synchronize()
    ks, cs = [], []
    for _ in range(args.repeats):                    # alternating windows: both see the same clocks
        ks.append(window(k, args.iters))
        cs.append(window(c, args.iters))
    print(torch.cuda.get_device_name(0))
    print(f"== B = {B} x V = {V} frames of {Hs} x {Ws}: NV12 at pitch {args.pitch} ({buf.numel() / 1e6:.0f} MB) and RGB "
          f"({rgb.numel() / 1e6:.0f} MB), N = {N} people x J = 15 joints + 14 limbs, figures of about {args.height} px, radius 8 "
          f"/ width 4, alpha {args.alpha}; {args.warmup} warm-up calls, median / min / max over {args.repeats} windows of "
          f"{args.iters} calls")
    print(f"luma pixels covered: {100.0 * covered:.3f} %, chroma pairs touched: {100.0 * quads:.3f} %")
    print(f"fvp_draw_poses_nv12 (k_draw_poses_nv12, NV12 surface)   {statistics.median(ks):9.1f} us  "
          f"(min {min(ks):.1f}, max {max(ks):.1f})")
    print(f"fvp_draw_poses      (k_draw_poses, RGB frames)          {statistics.median(cs):9.1f} us  "
          f"(min {min(cs):.1f}, max {max(cs):.1f})")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--views", type=int, default=5)
    ap.add_argument("--people", type=int, default=10)
    ap.add_argument("--height-px", type=int, default=1080)
    ap.add_argument("--width-px", type=int, default=1920)
    ap.add_argument("--pitch", type=int, default=2048, help="bytes per row of the NV12 buffer")
    ap.add_argument("--height", type=float, default=300.0, help="height of a figure in pixels")
    ap.add_argument("--alpha", type=float, default=1.0)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=20)
    main(ap.parse_args())
