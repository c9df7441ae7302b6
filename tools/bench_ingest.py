#!/usr/bin/env python
"""Camera frames -> backbone input (fvp_ingest_frames, diagnostics): the kernel alone - bf16 only and bf16 + fp32 -
next to the same conversion with torch ops + fvp_bb_input, and the images -> joints step from
uint8 frames next to the fp32-input step.  HIP-event timed, protocol of tools/bench_backbone.py; bytes moved are
computed from the shapes (3 Hs Ws read, 8 H W bf16 [+ 12 H W fp32] written per image).

--nv12: fvp_ingest_nv12 (a decoder's NV12 surface, 1.5 Hs Ws bytes read per image) instead, in the same job and
alternating window by window with (a) fvp_ingest_frames on RGB frames of the same size and (b) the two-step route a
user had before: NV12 -> RGB with torch ops (the integer formula of include/fvp.h, so its result is checked bit for
bit against the kernel) followed by fvp_ingest_frames."""
import argparse
import ctypes as C
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


def timed(fn, iters, repeats, warmup):
    """ms per call: (median, min, max) over `repeats` windows of `iters` calls."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / iters)
    return statistics.median(out), min(out), max(out)


def torch_yardstick(lib, frames, inv, W, H, out16):
    """What the tree could do before fvp_ingest_frames: torch ops (permute / float, grid_sample bilinear with zero padding
    on the affine grid of the same matrix, normalise) + fvp_bb_input."""
    N, Hs, Ws, _ = frames.shape
    dev = frames.device
    mean = torch.tensor(IMG.IMAGENET_MEAN, device=dev).view(1, 3, 1, 1)
    std = torch.tensor(IMG.IMAGENET_STD, device=dev).view(1, 3, 1, 1)
    a = torch.tensor(inv, dtype=torch.float32, device=dev).view(2, 3)
    ys, xs = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32),
                            torch.arange(W, device=dev, dtype=torch.float32), indexing="ij")
    sx = a[0, 0] * xs + a[0, 1] * ys + a[0, 2]
    sy = a[1, 0] * xs + a[1, 1] * ys + a[1, 2]
    grid = torch.stack([(2 * sx + 1) / Ws - 1, (2 * sy + 1) / Hs - 1], dim=-1)[None].expand(N, H, W, 2).contiguous()
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def run():
        x = frames.permute(0, 3, 1, 2).flip(1).float()
        x = torch.nn.functional.grid_sample(x, grid, mode="bilinear", padding_mode="zeros", align_corners=False)
        x = ((x / 255) - mean) / std
        capi.check(lib, lib.fvp_bb_input(C.c_void_p(x.data_ptr()), C.c_void_p(out16.data_ptr()), N, 3, H, W, s),
                   "fvp_bb_input")
    return run


def kernel_section(lib, N, src, dst, a):
    (Ws, Hs), (W, H) = src, dst
    fwd = torch.as_tensor(get_resize_transform(src, dst))       # a tensor: its inverse is cached per identity
    inv = IMG.invert_affine(fwd)
    nbuf = max(2, -(-(600 << 20) // (N * Hs * Ws * 3)))          # rotate inputs: > 2 x the 256 MiB Infinity Cache
    bufs = [torch.randint(0, 256, (N, Hs, Ws, 3), dtype=torch.uint8, device="cuda") for _ in range(nbuf)]
    o16 = torch.empty((N, H, W // 2, 8), dtype=torch.bfloat16, device="cuda")
    o32 = torch.empty((N, 3, H, W), dtype=torch.float32, device="cuda")
    print(f"\n== {N} frames {Hs}x{Ws} -> {H}x{W}  (inverse {[round(float(v), 6) for v in inv]}, {nbuf} input buffers in rotation)")
    k = [0]
    for outs, f32out in (("bf16", None), ("bf16+fp32", o32)):
        def run():
            k[0] += 1
            IMG.launch(lib, bufs[k[0] % nbuf], fwd, (W, H), True, IMG.IMAGENET_MEAN, IMG.IMAGENET_STD, o16, f32out)
        med, lo, hi = timed(run, a.iters, a.repeats, a.warmup)
        nbytes = N * (3 * Hs * Ws + 8 * H * W + (12 * H * W if f32out is not None else 0))
        bw = nbytes / (med * 1e-3)
        print(f"k_ingest_gather {outs:10s} {med * 1e3:8.1f} us  (min {lo * 1e3:.1f}, max {hi * 1e3:.1f})  {nbytes / 1e6:7.1f} MB"
              f"  {bw / 1e12:5.2f} TB/s = {100 * bw / HBM_PEAK:4.1f}% of 8.0 TB/s, {100 * bw / COPY_PEAK:4.1f}% of the 6.29 TB/s copy rate")
    ya = torch_yardstick(lib, bufs[0], inv, W, H, o16)
    med, lo, hi = timed(ya, max(1, a.iters // 4), a.repeats, a.warmup)
    print(f"torch ops + fvp_bb_input (yardstick, bf16 out) {med * 1e3:8.1f} us  (min {lo * 1e3:.1f}, max {hi * 1e3:.1f})")
    # the yardstick computes the same picture (fp32 torch arithmetic: values agree to rounding, not bit for bit)
    ref = o16.clone()
    IMG.launch(lib, bufs[0], fwd, (W, H), True, IMG.IMAGENET_MEAN, IMG.IMAGENET_STD, o16, None)
    torch.cuda.synchronize()
    d = (ref.float() - o16.float()).abs().max().item()
    print(f"max |yardstick - kernel| over the bf16 outputs: {d:.3e}")


def nv12_to_rgb_torch(y, uv, standard):
    """(b)'s first step: the integer formula of include/fvp.h with torch ops, y [N,Hs,Ws], uv [N,Hs/2,Ws/2,2] (strided
    views) -> uint8 [N,Hs,Ws,3] RGB."""
    yoff, cy, crv, cgu, cgv, cbu = YUV_COEFFS[standard]
    c = (y.int() - yoff).clamp_(min=0) * cy + (1 << 19)
    up = uv.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2).int() - 128
    d, e = up[..., 0], up[..., 1]
    rgb = torch.stack([c + crv * e, c + cgu * d + cgv * e, c + cbu * d], dim=-1)
    return (rgb >> 20).clamp_(0, 255).to(torch.uint8)


YUV_COEFFS = {0: (16, 1220945, 1673555, -410793, -852458, 2115221), 1: (16, 1220945, 1879825, -223607, -558796, 2215014),
              2: (0, 1048576, 1470104, -360853, -748826, 1858077), 3: (0, 1048576, 1651297, -196424, -490864, 1945738)}


def nv12_section(lib, N, src, dst, a):
    (Ws, Hs), (W, H) = src, dst
    fwd = torch.as_tensor(get_resize_transform(src, dst))
    pitch = -(-Ws // 256) * 256                                  # what a decoder allocates: 1920 -> 2048, 960 -> 1024
    nbuf = max(2, -(-(600 << 20) // (N * Hs * Ws * 3 // 2)))     # rotate inputs: > 2 x the 256 MiB Infinity Cache
    nrgb = max(2, -(-(600 << 20) // (N * Hs * Ws * 3)))
    surf = [torch.randint(0, 256, (N, Hs * 3 // 2, pitch), dtype=torch.uint8, device="cuda") for _ in range(nbuf)]
    nv = [IMG.Nv12Frames.from_buffer(b, Hs, Ws) for b in surf]
    rgb = [nv12_to_rgb_torch(nv[0].y, nv[0].uv, nv[0].standard)]
    rgb += [torch.randint(0, 256, (N, Hs, Ws, 3), dtype=torch.uint8, device="cuda") for _ in range(nrgb - 1)]
    o16 = torch.empty((N, H, W // 2, 8), dtype=torch.bfloat16, device="cuda")
    o32 = torch.empty((N, 3, H, W), dtype=torch.float32, device="cuda")
    print(f"\n== NV12: {N} frames {Hs}x{Ws} (pitch {pitch}) -> {H}x{W}  ({nbuf} surfaces / {nrgb} RGB buffers in rotation)")
    # the three routes compute the same bits (checked at this size before anything is timed)
    IMG.launch_nv12(lib, nv[0], fwd, (W, H), IMG.IMAGENET_MEAN, IMG.IMAGENET_STD, o16, o32)
    k16, k32 = o16.clone(), o32.clone()
    IMG.launch(lib, rgb[0], fwd, (W, H), False, IMG.IMAGENET_MEAN, IMG.IMAGENET_STD, o16, o32)
    torch.cuda.synchronize()
    same = torch.equal(k16.view(torch.int16), o16.view(torch.int16)) and torch.equal(k32.view(torch.int32), o32.view(torch.int32))
    print(f"fvp_ingest_nv12 == torch-op conversion + fvp_ingest_frames, both outputs, bit for bit: {same}")
    assert same
    k = [0]

    def nv12_bf16():
        k[0] += 1
        IMG.launch_nv12(lib, nv[k[0] % nbuf], fwd, (W, H), IMG.IMAGENET_MEAN, IMG.IMAGENET_STD, o16, None)

    def nv12_both():
        k[0] += 1
        IMG.launch_nv12(lib, nv[k[0] % nbuf], fwd, (W, H), IMG.IMAGENET_MEAN, IMG.IMAGENET_STD, o16, o32)

    def rgb_bf16():
        k[0] += 1
        IMG.launch(lib, rgb[k[0] % nrgb], fwd, (W, H), False, IMG.IMAGENET_MEAN, IMG.IMAGENET_STD, o16, None)

    def rgb_both():
        k[0] += 1
        IMG.launch(lib, rgb[k[0] % nrgb], fwd, (W, H), False, IMG.IMAGENET_MEAN, IMG.IMAGENET_STD, o16, o32)

    def two_step():
        k[0] += 1
        f = nv[k[0] % nbuf]
        IMG.launch(lib, nv12_to_rgb_torch(f.y, f.uv, f.standard), fwd, (W, H), False, IMG.IMAGENET_MEAN, IMG.IMAGENET_STD,
                   o16, None)

    src_nv12, src_rgb, d16, d32 = N * Hs * Ws * 3 // 2, N * Hs * Ws * 3, N * 8 * H * W, N * 12 * H * W
    routes = [("k_ingest_nv12 bf16", nv12_bf16, a.iters, src_nv12 + d16),
              ("(a) k_ingest_gather RGB bf16", rgb_bf16, a.iters, src_rgb + d16),
              ("k_ingest_nv12 bf16+fp32", nv12_both, a.iters, src_nv12 + d16 + d32),
              ("(a) k_ingest_gather RGB bf16+fp32", rgb_both, a.iters, src_rgb + d16 + d32),
              ("(b) torch NV12->RGB + k_ingest_gather bf16", two_step, max(1, a.iters // 10), None)]
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
        line = f"{name:44s} {med * 1e3:8.1f} us  (min {min(t) * 1e3:.1f}, max {max(t) * 1e3:.1f})"
        if nbytes is not None:
            bw = nbytes / (med * 1e-3)
            line += f"  {nbytes / 1e6:7.1f} MB  {bw / 1e12:5.2f} TB/s = {100 * bw / HBM_PEAK:4.1f}% of 8.0 TB/s"
        print(line)


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
    W, H = cfg.DATASET.IMAGE_SIZE
    frames = torch.randint(0, 256, (B, V, Hs, Ws, 3), dtype=torch.uint8, device="cuda")
    views = IMG.ingest_frames(frames, rt, (W, H))
    meta = {"seq": [seq] * B}
    print(f"\n== images -> joints, {B} frames x {V} views per step, eager, one stream")
    with torch.no_grad():
        res = {}
        for _ in range(2):                                   # alternate the two inputs: same job, same protocol
            for name, v in (("fp32 views [B,V,3,512,960]", views), ("uint8 frames [B,V,1080,1920,3]", frames)):
                med, lo, hi = timed(lambda: model(backbone=bb, views=v, meta=meta, cameras=cams, resize_transform=rt),
                                    a.e2e_iters, a.repeats, 3)
                res.setdefault(name, []).append((med, lo, hi))
        for name, rows in res.items():
            for med, lo, hi in rows:
                print(f"{name:32s} {med:7.3f} ms/step (min {lo:.3f}, max {hi:.3f})  {B / (med * 1e-3):7.1f} frames/s")


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--e2e-iters", type=int, default=10)
    ap.add_argument("--no-e2e", action="store_true")
    ap.add_argument("--nv12", action="store_true", help="time fvp_ingest_nv12 against the RGB kernel and the two-step route")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_ingest.py needs the MI355X"
    lib = capi.load()
    print(torch.cuda.get_device_name(0))
    if a.nv12:
        nv12_section(lib, a.frames, (1920, 1080), (960, 512), a)
        nv12_section(lib, a.frames, (960, 512), (960, 512), a)
        return
    kernel_section(lib, a.frames, (1920, 1080), (960, 512), a)
    kernel_section(lib, a.frames, (960, 512), (960, 512), a)
    if not a.no_e2e:
        e2e_section(a)


if __name__ == "__main__":
    main()
