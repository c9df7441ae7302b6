#!/usr/bin/env python
"""Person crops (fvp_person_rois + fvp_crop_rois / fvp_crop_rois_nv12): the calls alone, HIP-event timed,
next to the route a user had before - per frame ``affine_grid`` + ``grid_sample`` over that frame's boxes on a float copy of
the frame, then the normalisation; for an NV12 surface the conversion of the whole surface to RGB first - alternating window
by window in the same job.

Shape: B = 8 frames x V = 5 views of 1080 x 1920, N = 10 people x J = 15 joints (the seeded scene of tools/bench_overlay.py,
figures of about ``--height`` pixels), one 256 x 192 patch per (frame, view, person): R = 400 crops.  The NV12 surface is one
contiguous buffer per frame at ``--pitch`` bytes per row.  The boxes are computed once by ``PersonCrops.rois`` (timed on its
own); the torch route gets the same boxes as ``theta``.  Its patches are compared with the kernel's before anything is timed
(same bilinear samples, another rounding order: a maximum difference is printed, nothing is asserted)."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from bench_overlay import make_views  # noqa: E402
from bench_track import window  # noqa: E402
from faster_voxelpose_amd.dataset.images import IMAGENET_MEAN, IMAGENET_STD, Nv12Frames  # noqa: E402
from faster_voxelpose_amd.utils.crops import PersonCrops  # noqa: E402

BT709_LIMITED = (16, 1220945, 1879825, -223607, -558796, 2215014)      # include/fvp.h


def thetas(rois, Hs, Ws):
    """rois [B,V,N,4] -> theta [B*V,N,2,3] for affine_grid(align_corners=False): patch pixel centres onto the box."""
    x0, y0, x1, y1 = rois.flatten(0, 1).unbind(-1)
    t = torch.zeros(x0.shape + (2, 3), device=rois.device)
    t[..., 0, 0], t[..., 0, 2] = (x1 - x0) / Ws, (x0 + x1) / Ws - 1
    t[..., 1, 1], t[..., 1, 2] = (y1 - y0) / Hs, (y0 + y1) / Hs - 1
    return t


def nv12_to_rgb(nv12):
    """The whole surface to float R, G, B planes [F,3,Hs,Ws] with the integer formula of include/fvp.h, in torch."""
    yoff, cy, crv, cgu, cgv, cbu = BT709_LIMITED
    y = nv12.y.flatten(0, 1).to(torch.int32)
    uv = nv12.uv.flatten(0, 1).to(torch.int32).repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
    c, d, e = (y - yoff).clamp_(min=0) * cy + (1 << 19), uv[..., 0] - 128, uv[..., 1] - 128
    rgb = torch.stack([(c + crv * e) >> 20, (c + cgu * d + cgv * e) >> 20, (c + cbu * d) >> 20], dim=1)
    return rgb.clamp_(0, 255).float()


def torch_route(planes, theta, size, mean, std, bf16):
    """planes [F,3,Hs,Ws] float -> patches [F,N,3,h,w]: per frame, grid_sample over its N boxes, then normalise."""
    out = []
    for f in range(planes.shape[0]):
        n = theta.shape[1]
        grid = F.affine_grid(theta[f], (n, 3) + size, align_corners=False)
        out.append(F.grid_sample(planes[f:f + 1].expand(n, -1, -1, -1), grid, mode="bilinear", padding_mode="zeros",
                                 align_corners=False))
    p = (torch.stack(out) / 255 - mean) / std
    return p.to(torch.bfloat16) if bf16 else p


def main(args):
    dev = "cuda:0"
    B, V, N, Hs, Ws = args.batch, args.views, args.people, args.height_px, args.width_px
    size = (args.crop_h, args.crop_w)
    views = torch.from_numpy(make_views(B, V, N, Hs, Ws, args.height)).to(dev)
    rgb = torch.randint(0, 256, (B, V, Hs, Ws, 3), dtype=torch.uint8, device=dev)
    buf = torch.randint(0, 256, (B, V, Hs * 3 // 2, args.pitch), dtype=torch.uint8, device=dev)
    nv12 = Nv12Frames.from_buffer(buf, Hs, Ws, standard="bt709")
    pc = {b: PersonCrops(15, size=size, bf16=b) for b in (False, True)}
    rois, count, _ = pc[False].rois(views)
    theta = thetas(rois, Hs, Ws)
    mean = torch.tensor(IMAGENET_MEAN, device=dev).view(1, 1, 3, 1, 1)
    std = torch.tensor(IMAGENET_STD, device=dev).view(1, 1, 3, 1, 1)
    # algorithmic bytes: the boxes' pixels inside the frame, read once, and the patches, written once
    x0, y0, x1, y1 = rois.unbind(-1)
    inside = ((x1.clamp(0, Ws) - x0.clamp(0, Ws)).clamp(min=0) * (y1.clamp(0, Hs) - y0.clamp(0, Hs)).clamp(min=0)).sum().item()
    R = B * V * N
    valid = int((count > 0).sum())

    def route_rgb(bf16):
        return torch_route(rgb.flatten(0, 1).permute(0, 3, 1, 2).float(), theta, size, mean, std, bf16)

    def route_nv12(bf16):
        return torch_route(nv12_to_rgb(nv12), theta, size, mean, std, bf16)

    diff_rgb = (pc[False].crop(rgb, rois) - route_rgb(False).view(B, V, N, 3, *size)).abs().max().item()
    diff_nv12 = (pc[False].crop(nv12, rois) - route_nv12(False).view(B, V, N, 3, *size)).abs().max().item()
    legs = {
        "fvp_crop_rois      RGB  -> fp32": lambda i: pc[False].crop(rgb, rois),
        "fvp_crop_rois      RGB  -> bf16": lambda i: pc[True].crop(rgb, rois),
        "fvp_crop_rois_nv12 NV12 -> fp32": lambda i: pc[False].crop(nv12, rois),
        "fvp_crop_rois_nv12 NV12 -> bf16": lambda i: pc[True].crop(nv12, rois),
        "fvp_person_rois                ": lambda i: pc[False].rois(views),
        "torch grid_sample  RGB  -> fp32": lambda i: route_rgb(False),
        "torch grid_sample  RGB  -> bf16": lambda i: route_rgb(True),
        "torch grid_sample  NV12 -> fp32": lambda i: route_nv12(False),
        "torch grid_sample  NV12 -> bf16": lambda i: route_nv12(True),
    }
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
          f"({buf.numel() / 1e6:.0f} MB); N = {N} people x J = 15 joints, figures of about {args.height} px; R = {R} patches of "
          f"{size[0]} x {size[1]} ({valid} valid boxes); median / min / max over {args.repeats} windows of {args.iters} calls "
          f"(torch route: {args.torch_iters}), every window of every leg alternating in one job")
    print(f"box pixels inside the frames: {inside / 1e6:.2f} M (source bytes read once: RGB {3 * inside / 1e6:.1f} MB, NV12 "
          f"{1.5 * inside / 1e6:.1f} MB); patch bytes: fp32 {R * size[0] * size[1] * 12 / 1e6:.1f} MB, bf16 "
          f"{R * size[0] * size[1] * 8 / 1e6:.1f} MB")
    print(f"max |kernel - torch route| over the fp32 patches: RGB {diff_rgb:.3e}, NV12 {diff_nv12:.3e}")
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
    ap.add_argument("--crop-h", type=int, default=256)
    ap.add_argument("--crop-w", type=int, default=192)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--torch-iters", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=10)
    main(ap.parse_args())
