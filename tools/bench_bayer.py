#!/usr/bin/env python
"""Bayer raw frames -> backbone input (fvp_ingest_bayer, fvp_demosaic_bayer; diagnostics).  One job, HIP events, the routes
alternating window by window (protocol of tools/bench_ingest.py --nv12), inputs rotated over more than 600 MB:

  (a) fvp_ingest_bayer, bf16 only and bf16 + fp32;
  (b) fvp_demosaic_bayer + fvp_ingest_frames: the two launches it replaces (an RGB frame written and read back);
  (c) fvp_ingest_frames alone on RGB frames of that size, for scale;
  (d) the formulas of include/fvp.h as torch ops + fvp_ingest_frames: what a user had before;
  fvp_demosaic_bayer alone, against the copy rate.

The routes' outputs are compared bit for bit at the timed size before anything is timed.  Then images -> joints from
BayerFrames next to uint8 frames, in the same job."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import fvp_synthetic as S  # noqa: E402
from faster_voxelpose_amd import _capi as capi  # noqa: E402
from faster_voxelpose_amd.core import config as CFG  # noqa: E402
from faster_voxelpose_amd.dataset import images as IMG  # noqa: E402
from faster_voxelpose_amd.models import faster_voxelpose as FV, resnet as RN  # noqa: E402
from faster_voxelpose_amd.utils.transforms import get_resize_transform  # noqa: E402

HBM_PEAK, COPY_PEAK = 8.0e12, 6.29e12          # bytes/s: data sheet, and the copy rate the tree's other figures use


def demosaic_torch(raw, pattern):
    """(d)'s first step: include/fvp.h with torch ops.  raw [N,Hs,Ws] uint8 (a strided view) -> uint8 [N,Hs,Ws,3]."""
    rx, ry = pattern & 1, pattern >> 1
    n, hs, ws = raw.shape
    p = torch.nn.functional.pad(raw.float()[:, None], (2, 2, 2, 2), mode="reflect")[:, 0].int()

    def at(dy, dx):
        return p[:, 2 + dy:2 + dy + hs, 2 + dx:2 + dx + ws]

    c = at(0, 0)
    h1, v1 = at(0, -1) + at(0, 1), at(-1, 0) + at(1, 0)
    d = at(-1, -1) + at(-1, 1) + at(1, -1) + at(1, 1)
    h2, v2 = at(0, -2) + at(0, 2), at(-2, 0) + at(2, 0)
    own, green = 16 * c, 8 * c + 4 * (h1 + v1) - 2 * (h2 + v2)
    third = 12 * c + 4 * d - 3 * (h2 + v2)
    row, col = 10 * c + 8 * h1 - 2 * d - 2 * h2 + v2, 10 * c + 8 * v1 - 2 * d - 2 * v2 + h2
    xr = ((torch.arange(ws, device=raw.device) & 1) == rx)[None, None, :]
    yr = ((torch.arange(hs, device=raw.device) & 1) == ry)[None, :, None]
    red, blue = xr & yr, ~xr & ~yr
    r = torch.where(red, own, torch.where(blue, third, torch.where(yr, row, col)))
    g = torch.where(red | blue, green, own)
    b = torch.where(blue, own, torch.where(red, third, torch.where(yr, col, row)))
    return ((torch.stack([r, g, b], dim=-1) + 8) >> 4).clamp_(0, 255).to(torch.uint8)


def section(lib, N, src, dst, a):
    (Ws, Hs), (W, H) = src, dst
    fwd = torch.as_tensor(get_resize_transform(src, dst))
    pitch = -(-Ws // 256) * 256
    nraw = max(2, -(-(600 << 20) // (N * Hs * Ws)))              # rotate inputs: > 2 x the 256 MiB Infinity Cache
    nrgb = max(2, -(-(600 << 20) // (N * Hs * Ws * 3)))
    pattern = capi.BAYER_GRBG
    bufs = [torch.randint(0, 256, (N, Hs, pitch), dtype=torch.uint8, device="cuda") for _ in range(nraw)]
    fr = [IMG.BayerFrames(b[..., :Ws], "grbg") for b in bufs]
    rgb = [torch.empty((N, Hs, Ws, 3), dtype=torch.uint8, device="cuda") for _ in range(nrgb)]
    for t in rgb[1:]:
        t.random_(0, 256)
    work = torch.empty((N, Hs, Ws, 3), dtype=torch.uint8, device="cuda")     # (b)'s RGB frame
    o16 = torch.empty((N, H, W // 2, 8), dtype=torch.bfloat16, device="cuda")
    o32 = torch.empty((N, 3, H, W), dtype=torch.float32, device="cuda")
    print(f"\n== Bayer: {N} frames {Hs}x{Ws} (pitch {pitch}) -> {H}x{W}  ({nraw} mosaics / {nrgb} RGB buffers in rotation)")
    # the routes compute the same bits (checked at this size before anything is timed)
    MS = (IMG.IMAGENET_MEAN, IMG.IMAGENET_STD)
    IMG.launch_bayer(lib, fr[0], fwd, (W, H), *MS, o16, o32)
    k16, k32 = o16.clone(), o32.clone()
    IMG.demosaic_bayer(fr[0], out=rgb[0])
    IMG.launch(lib, rgb[0], fwd, (W, H), False, *MS, o16, o32)
    torch.cuda.synchronize()
    same = torch.equal(k16.view(torch.int16), o16.view(torch.int16)) and torch.equal(k32.view(torch.int32), o32.view(torch.int32))
    step = max(1, N // 4)
    same_t = all(torch.equal(demosaic_torch(fr[0].raw[i:i + step], pattern), rgb[0][i:i + step]) for i in range(0, N, step))
    print(f"fvp_ingest_bayer == fvp_demosaic_bayer + fvp_ingest_frames, both outputs, bit for bit: {same}")
    print(f"fvp_demosaic_bayer == the torch-op demosaic, every byte: {same_t}")
    assert same and same_t
    k = [0]

    def nxt(lst):
        k[0] += 1
        return lst[k[0] % len(lst)]

    def a_bf16():
        IMG.launch_bayer(lib, nxt(fr), fwd, (W, H), *MS, o16, None)

    def a_both():
        IMG.launch_bayer(lib, nxt(fr), fwd, (W, H), *MS, o16, o32)

    def b_two():
        IMG.demosaic_bayer(nxt(fr), out=work)
        IMG.launch(lib, work, fwd, (W, H), False, *MS, o16, None)

    def b_two_both():
        IMG.demosaic_bayer(nxt(fr), out=work)
        IMG.launch(lib, work, fwd, (W, H), False, *MS, o16, o32)

    def c_rgb():
        IMG.launch(lib, nxt(rgb), fwd, (W, H), False, *MS, o16, None)

    def d_torch():
        f = nxt(fr)
        IMG.launch(lib, demosaic_torch(f.raw, pattern), fwd, (W, H), False, *MS, o16, None)

    def dem():
        IMG.demosaic_bayer(nxt(fr), out=work)

    raw_b, rgb_b, d16, d32 = N * Hs * Ws, N * Hs * Ws * 3, N * 8 * H * W, N * 12 * H * W
    routes = [("(a) fvp_ingest_bayer bf16", a_bf16, a.iters, raw_b + d16),
              ("(b) fvp_demosaic_bayer + fvp_ingest_frames bf16", b_two, a.iters, raw_b + 2 * rgb_b + d16),
              ("(a) fvp_ingest_bayer bf16+fp32", a_both, a.iters, raw_b + d16 + d32),
              ("(b) demosaic + ingest_frames bf16+fp32", b_two_both, a.iters, raw_b + 2 * rgb_b + d16 + d32),
              ("(c) fvp_ingest_frames RGB bf16", c_rgb, a.iters, rgb_b + d16),
              ("fvp_demosaic_bayer alone", dem, a.iters, raw_b + rgb_b),
              ("(d) torch-op demosaic + fvp_ingest_frames bf16", d_torch, max(1, a.iters // 10), None)]
    for _, fn, _, _ in routes:
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _, _, _ in routes}
    for _ in range(a.repeats):                                   # alternate the routes window by window
        for name, fn, iters, _ in routes:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) / iters)
    for name, _, _, nbytes in routes:
        t = times[name]
        med = statistics.median(t)
        line = f"{name:50s} {med * 1e3:8.1f} us  (min {min(t) * 1e3:.1f}, max {max(t) * 1e3:.1f})"
        if nbytes is not None:
            bw = nbytes / (med * 1e-3)
            line += (f"  {nbytes / 1e6:7.1f} MB  {bw / 1e12:5.2f} TB/s = {100 * bw / HBM_PEAK:4.1f}% of 8.0 TB/s, "
                     f"{100 * bw / COPY_PEAK:4.1f}% of the 6.29 TB/s copy rate")
        print(line)
    ta, tb = times[routes[0][0]], times[routes[1][0]]
    print(f"decision rule: (a) median {statistics.median(ta) * 1e3:.1f} us against (b) median {statistics.median(tb) * 1e3:.1f} us, "
          f"(b)'s window spread {(max(tb) - min(tb)) * 1e3:.1f} us")


def e2e_section(a):
    cfg = S.make_cfg("panoptic", device="cuda:0", min_score=-1.0)
    cams, seq = S.load_cameras("panoptic")
    rt = S.resize_transform(cfg).cuda()
    model = FV.get(cfg).to("cuda:0")
    model.load_state_dict(S.fill_state_dict(model.state_dict(), seed=7))
    bb = RN.get(CFG.default_config()).to("cuda:0")
    bb.load_state_dict(S.fill_backbone_state_dict(bb.state_dict(), seed=3))
    B, V = a.batch, cfg.DATASET.CAMERA_NUM
    Ws, Hs = cfg.DATASET.ORI_IMAGE_SIZE
    frames = torch.randint(0, 256, (B, V, Hs, Ws, 3), dtype=torch.uint8, device="cuda")
    bayer = IMG.BayerFrames(torch.randint(0, 256, (B, V, Hs, Ws), dtype=torch.uint8, device="cuda"), "grbg")
    meta = {"seq": [seq] * B}
    print(f"\n== images -> joints, {B} frames x {V} views per step, eager, one stream")

    def timed(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        out = []
        for _ in range(a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.e2e_iters):
                fn()
            e1.record()
            e1.synchronize()
            out.append(e0.elapsed_time(e1) / a.e2e_iters)
        return statistics.median(out), min(out), max(out)

    with torch.no_grad():
        res = {}
        for _ in range(2):                                   # alternate the inputs: same job, same protocol
            for name, v, flag in ((f"uint8 frames [B,V,{Hs},{Ws},3]", frames, False),
                                  (f"BayerFrames [B,V,{Hs},{Ws}]", bayer, False),
                                  ("BayerFrames, model.bayer_rgb = True", bayer, True)):
                model.bayer_rgb = flag
                res.setdefault(name, []).append(timed(lambda: model(backbone=bb, views=v, meta=meta, cameras=cams,
                                                                    resize_transform=rt)))
        for name, rows in res.items():
            for med, lo, hi in rows:
                print(f"{name:38s} {med:7.3f} ms/step (min {lo:.3f}, max {hi:.3f})  {B / (med * 1e-3):7.1f} frames/s")


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--e2e-iters", type=int, default=10)
    ap.add_argument("--no-e2e", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_bayer.py needs the MI355X"
    lib = capi.load()
    print(torch.cuda.get_device_name(0))
    section(lib, a.frames, (1920, 1080), (960, 512), a)
    section(lib, a.frames, (960, 512), (960, 512), a)
    if not a.no_e2e:
        e2e_section(a)


if __name__ == "__main__":
    main()
