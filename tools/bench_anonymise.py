#!/usr/bin/env python
"""Head anonymiser (fvp_person_rois + fvp_anonymise_rois / fvp_anonymise_rois_nv12): the calls alone, HIP-event
timed, next to the route a user had before - per frame ``avg_pool2d`` + nearest upsample + ``where`` under a mask on a float
copy of the frame, written back as uint8; for an NV12 surface the conversion of the whole surface to RGB first and back
afterwards - alternating window by window in the same job.

Shape: B = 8 frames x V = 5 views of 1080 x 1920, N = 10 people x J = 15 joints (the seeded scene of tools/bench_overlay.py,
figures of about ``--height`` pixels), one head box per (frame, view, person) from neck and nose.  The NV12 surface is one
contiguous buffer per frame at ``--pitch`` bytes per row.  The boxes are computed once by ``FaceAnonymiser.rois`` (timed on
its own); the torch route gets the covered-pixel masks ready-made (made by the FILL kernel, not timed), which favours it.
Coverage is the workload, so the frames are anonymised repeatedly.  Also reported: the share of 64 x 32 tiles that hold a
covered pixel, and the algorithmic bytes - the pixels of the touched cells read once, the covered pixels written once."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from bench_crops import nv12_to_rgb  # noqa: E402
from bench_overlay import make_views  # noqa: E402
from bench_track import window  # noqa: E402
from faster_voxelpose_amd.dataset.images import Nv12Frames  # noqa: E402
from faster_voxelpose_amd.utils.anonymise import FaceAnonymiser  # noqa: E402

# BT.709 limited range, float: R, G, B planes -> Y, U, V (the torch route's way back; its rounding is its own)
KR, KB = 0.2126, 0.0722


def rgb_to_nv12(planes, nv12):
    """planes [F,3,Hs,Ws] float -> the surface's two planes, in place."""
    r, g, b = planes.unbind(1)
    y = KR * r + (1 - KR - KB) * g + KB * b
    u, v = (b - y) / (2 * (1 - KB)), (r - y) / (2 * (1 - KR))
    nv12.y.flatten(0, 1).copy_((16 + y * (219 / 255)).round_().clamp_(0, 255))
    uv = torch.stack([F.avg_pool2d(u[:, None], 2)[:, 0], F.avg_pool2d(v[:, None], 2)[:, 0]], dim=-1)
    nv12.uv.flatten(0, 1).copy_((128 + uv * (224 / 255)).round_().clamp_(0, 255))


def torch_mosaic(planes, masks, cell):
    """planes [F,3,Hs,Ws] float, masks [F,1,Hs,Ws] bool -> mosaic under the mask, frame by frame (a float copy of all F frames
    of a batch at once would be the larger allocation; a user's loop is per camera frame)."""
    out = torch.empty_like(planes)
    hs, ws = planes.shape[-2:]
    for f in range(planes.shape[0]):
        p = planes[f:f + 1]
        m = F.avg_pool2d(p, cell, ceil_mode=True, count_include_pad=False)
        up = F.interpolate(m, scale_factor=cell, mode="nearest")[..., :hs, :ws]
        out[f] = torch.where(masks[f:f + 1], (up + 0.5).floor_(), p)[0]
    return out


def main(args):
    dev = "cuda:0"
    B, V, N, Hs, Ws = args.batch, args.views, args.people, args.height_px, args.width_px
    views = torch.from_numpy(make_views(B, V, N, Hs, Ws, args.height)).to(dev)
    rgb = torch.randint(0, 256, (B, V, Hs, Ws, 3), dtype=torch.uint8, device=dev)
    buf = torch.randint(0, 256, (B, V, Hs * 3 // 2, args.pitch), dtype=torch.uint8, device=dev)
    nv12 = Nv12Frames.from_buffer(buf, Hs, Ws, standard="bt709")
    fa = {(c, m): FaceAnonymiser(15, cell=c, mode=m, colour=(255, 255, 255)) for c in (8, 32) for m in ("mosaic", "fill")}
    rois, count, _ = fa[8, "mosaic"].rois(views)
    none = torch.zeros_like(rois)                                # the all-zero invalid box: an all-inactive list
    # coverage and the algorithmic bytes: FILL white onto black frames
    black = torch.zeros_like(rgb)
    fa[8, "fill"].apply(black, rois)
    px = (black != 0).any(dim=-1)                                # [B,V,Hs,Ws] bool
    del black
    masks = px.flatten(0, 1)[:, None]

    def share(th, tw):
        ph, pw = (-Hs) % th, (-Ws) % tw
        t = F.pad(px.to(torch.uint8), (0, pw, 0, ph)).view(B, V, (Hs + ph) // th, th, (Ws + pw) // tw, tw).amax(dim=5).amax(dim=3) > 0
        return int(t.sum()), t.numel()

    def cell_pixels(cell):                                       # in-frame pixels of the touched cells
        t = F.max_pool2d(px.flatten(0, 1)[:, None].float(), cell, ceil_mode=True)
        return int(F.interpolate(t, scale_factor=cell, mode="nearest")[..., :Hs, :Ws].sum())

    covered, tiles = int(px.sum()), share(32, 64)

    def route_rgb(cell):
        planes = rgb.flatten(0, 1).permute(0, 3, 1, 2).float()
        rgb.flatten(0, 1).copy_(torch_mosaic(planes, masks, cell).permute(0, 2, 3, 1))

    def route_nv12(cell):
        rgb_to_nv12(torch_mosaic(nv12_to_rgb(nv12), masks, cell), nv12)

    legs = {}
    for name, frames in (("fvp_anonymise_rois      RGB ", rgb), ("fvp_anonymise_rois_nv12 NV12", nv12)):
        for (c, m), obj in fa.items():
            legs[f"{name} cell {c:2d} {m:6s}"] = lambda i, obj=obj, frames=frames: obj.apply(frames, rois)
        legs[f"{name} all inactive  "] = lambda i, frames=frames: fa[8, "mosaic"].apply(frames, none)
    legs["fvp_person_rois (head mask)               "] = lambda i: fa[8, "mosaic"].rois(views)
    legs["torch pool+upsample+where RGB  cell  8    "] = lambda i: route_rgb(8)
    legs["torch pool+upsample+where RGB  cell 32    "] = lambda i: route_rgb(32)
    legs["torch convert+pool+..+convert NV12 cell  8"] = lambda i: route_nv12(8)
    iters = {k: (args.iters if k.startswith("fvp") else args.torch_iters) for k in legs}
    for k, fn in legs.items():
        for i in range(args.warmup if k.startswith("fvp") else 2):
            fn(i)
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(args.repeats):                    # alternating windows: every leg sees the same clocks
        for k, fn in legs.items():
            times[k].append(window(fn, iters[k]))
    print(torch.cuda.get_device_name(0))
    print(f"== B = {B} x V = {V} frames of {Hs} x {Ws}: RGB ({rgb.numel() / 1e6:.0f} MB) and NV12 at pitch {args.pitch} "
          f"({buf.numel() / 1e6:.0f} MB); N = {N} people x J = 15 joints, figures of about {args.height} px; {B * V * N} head boxes "
          f"({int((count > 0).sum())} valid), ellipse, scale {fa[8, 'mosaic'].scale}, pad {fa[8, 'mosaic'].pad_px} px; median / min / "
          f"max over {args.repeats} windows of {args.iters} calls (torch route: {args.torch_iters}), every window of every leg "
          f"alternating in one job")
    print(f"pixels covered: {covered} ({100.0 * covered / px.numel():.3f} %); 64 x 32 tiles with a covered pixel: {tiles[0]} of "
          f"{tiles[1]} ({100.0 * tiles[0] / tiles[1]:.2f} %)")
    for c in (8, 32):
        n = cell_pixels(c)
        print(f"cell {c:2d}: {n} pixels in touched cells; algorithmic bytes read + written: RGB {3 * n / 1e6:.2f} + "
              f"{3 * covered / 1e6:.2f} MB, NV12 {1.5 * n / 1e6:.2f} + about {1.5 * covered / 1e6:.2f} MB; FILL writes only")
    for k, ts in times.items():
        print(f"{k}   {statistics.median(ts):10.1f} us  (min {min(ts):.1f}, max {max(ts):.1f})")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--views", type=int, default=5)
    ap.add_argument("--people", type=int, default=10)
    ap.add_argument("--height-px", type=int, default=1080)
    ap.add_argument("--width-px", type=int, default=1920)
    ap.add_argument("--pitch", type=int, default=2048, help="bytes per row of the NV12 buffer")
    ap.add_argument("--height", type=float, default=300.0, help="height of a figure in pixels")
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--torch-iters", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=10)
    main(ap.parse_args())
