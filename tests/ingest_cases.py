"""Shared by tests/test_ingest_emu.py (CPU emulator) and tests/test_ingest_gpu.py (the shipped library on the card):
the cases, a numpy-float32 restatement of fvp_ingest_frames' arithmetic (include/fvp.h), an exact float64 bilinear,
and a runner that calls the entry point on numpy (emulator) or torch-GPU memory."""
import ctypes as C

import numpy as np
import torch

from faster_voxelpose_amd import _capi as capi
from faster_voxelpose_amd.dataset.images import IMAGENET_MEAN, IMAGENET_STD, invert_affine
from faster_voxelpose_amd.utils.transforms import get_affine_transform, get_resize_transform

f32 = np.float32
MEAN32 = np.array(IMAGENET_MEAN, f32)
STD32 = np.array(IMAGENET_STD, f32)
IDENTITY = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])


def _rotated(src, dst, deg):
    ws, hs = src
    return get_affine_transform(np.array([ws / 2.0, hs / 2.0]), np.array([ws, hs], f32) / 200.0 * 0.8, deg, dst)


# name -> (source (Ws, Hs), network (W, H), forward 2x3 camera -> network, N, swap_rb)
CASES = {
    # the Panoptic geometry scaled down (1920x1080 -> 960x512 letter-boxes in y; this one in x): border taps occur
    "panoptic_small": ((96, 54), (48, 26), get_resize_transform((96, 54), (48, 26)), 3, True),
    "panoptic_small_noswap": ((96, 54), (48, 26), get_resize_transform((96, 54), (48, 26)), 1, False),
    # tall source into a wide network image: a 14-pixel border left and right
    "tall_source": ((30, 40), (48, 26), get_resize_transform((30, 40), (48, 26)), 1, False),
    # up-scale; 3 * 47 = 141 bytes per source row: no row but the first starts on a 4-byte boundary
    "upscale_odd_ws": ((47, 23), (64, 32), get_resize_transform((47, 23), (64, 32)), 3, True),
    "identity": ((40, 24), (40, 24), IDENTITY, 3, True),
    "identity_noswap": ((40, 24), (40, 24), IDENTITY, 1, False),
    "same_size_resize": ((40, 24), (40, 24), get_resize_transform((40, 24), (40, 24)), 1, True),
    # a wide row (more than one workgroup per row), taps outside on every side, 3 * 301 = 903 bytes per row
    "wide_shifted": ((301, 19), (262, 10), np.array([[0.9, 0.0, -3.3], [0.0, 0.55, 1.2]]), 1, True),
    "mirror": ((33, 9), (34, 8), np.array([[-1.0, 0.0, 33.0], [0.0, 1.0, 0.0]]), 1, False),
    "rotation": ((50, 37), (32, 20), _rotated((50, 37), (32, 20), 20.0), 1, True),
    "source_1x1": ((1, 1), (8, 4), np.array([[4.0, 0.0, 2.0], [0.0, 4.0, 0.0]]), 3, True),
    "source_2x2": ((2, 2), (6, 4), get_resize_transform((2, 2), (6, 4)), 1, False),
    "source_2x1": ((2, 1), (6, 4), np.array([[3.0, 0.0, 0.25], [0.0, 3.0, 1.5]]), 1, True),
}
AXIS_ALIGNED = [k for k in CASES if k != "rotation"]


def make_frames(name, seed=0):
    (ws, hs), _, _, n, _ = CASES[name]
    rng = np.random.default_rng([seed, sum(name.encode())])
    fr = rng.integers(0, 256, size=(n, hs, ws, 3), dtype=np.uint8)
    fr.reshape(-1)[:2] = (0, 255)                       # the full range is present whatever the generator drew
    return fr


def bf16_rne(x):
    u = np.ascontiguousarray(x, f32).view(np.uint32).astype(np.uint64)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF).astype(np.uint16)


def pack_nhwc8(out):
    """fp32 [N,3,H,W] -> uint16 [N,H,W/2,8]: pixel pairs of 4 channels, channel 3 zero (fvp_bb_input's layout)."""
    n, _, h, w = out.shape
    px = np.zeros((n, h, w, 4), np.uint16)
    px[..., :3] = bf16_rne(out).transpose(0, 2, 3, 1)
    return px.reshape(n, h, w // 2, 8)


def _taps(frames, y0, x0, ch):
    """frames [N,Hs,Ws,3], integer index planes y0 / x0 [H,W] -> bytes [N,H,W] of channel ch, 0 outside the frame."""
    _, hs, ws, _ = frames.shape
    ok = (y0 >= 0) & (y0 < hs) & (x0 >= 0) & (x0 < ws)
    v = frames[:, np.clip(y0, 0, hs - 1), np.clip(x0, 0, ws - 1), ch]
    return np.where(ok[None], v, 0)


def reference_f32(frames, inv, W, H, swap, mean=MEAN32, std=STD32):
    """The arithmetic of include/fvp.h op by op in numpy float32 (numpy rounds every ufunc result to float32)."""
    inv = np.asarray(inv, f32).reshape(6)
    mean, std = np.asarray(mean, f32), np.asarray(std, f32)
    hs, ws = frames.shape[1:3]
    x = np.arange(W, dtype=f32)[None, :]
    y = np.arange(H, dtype=f32)[:, None]
    sx = ((inv[0] * x) + (inv[1] * y)) + inv[2]
    sy = ((inv[3] * x) + (inv[4] * y)) + inv[5]
    assert sx.dtype == f32 and sx.shape == (H, W)
    flx, fly = np.floor(sx), np.floor(sy)
    fx, fy = sx - flx, sy - fly
    x0 = np.clip(flx, -2, ws).astype(np.int64)
    y0 = np.clip(fly, -2, hs).astype(np.int64)
    gx, gy = f32(1) - fx, f32(1) - fy
    out = np.empty((frames.shape[0], 3, H, W), f32)
    for c in range(3):
        sc = 2 - c if swap else c
        p00, p01 = _taps(frames, y0, x0, sc).astype(f32), _taps(frames, y0, x0 + 1, sc).astype(f32)
        p10, p11 = _taps(frames, y0 + 1, x0, sc).astype(f32), _taps(frames, y0 + 1, x0 + 1, sc).astype(f32)
        v = (gy * ((gx * p00) + (fx * p01))) + (fy * ((gx * p10) + (fx * p11)))
        o = ((v / f32(255)) - mean[c]) / std[c]
        assert o.dtype == f32
        out[:, c] = o
    return out


def reference_f64(frames, forward, W, H, swap, mean=MEAN32, std=STD32):
    """Exact bilinear with a zero border in float64; coordinates from the float64 inverse of ``forward`` (never rounded
    to fp32).  mean / std are the fp32 constants the kernel receives, widened."""
    t = np.asarray(forward, np.float64).reshape(2, 3)
    a = np.linalg.inv(t[:, :2])
    b = -a @ t[:, 2]
    hs, ws = frames.shape[1:3]
    x = np.arange(W, dtype=np.float64)[None, :]
    y = np.arange(H, dtype=np.float64)[:, None]
    sx = a[0, 0] * x + a[0, 1] * y + b[0]
    sy = a[1, 0] * x + a[1, 1] * y + b[1]
    flx, fly = np.floor(sx), np.floor(sy)
    fx, fy = sx - flx, sy - fly
    x0 = np.clip(flx, -2, ws).astype(np.int64)
    y0 = np.clip(fly, -2, hs).astype(np.int64)
    out = np.empty((frames.shape[0], 3, H, W), np.float64)
    for c in range(3):
        sc = 2 - c if swap else c
        p = [_taps(frames, y0 + dy, x0 + dx, sc).astype(np.float64) for dy in (0, 1) for dx in (0, 1)]
        v = (1 - fy) * ((1 - fx) * p[0] + fx * p[1]) + fy * ((1 - fx) * p[2] + fx * p[3])
        out[:, c] = (v / 255.0 - np.float64(mean[c])) / np.float64(std[c])
    return out


def _fa(v):
    v = [float(x) for x in v]
    return (C.c_float * len(v))(*v)


def call(lib, frames_ptr, n, hs, ws, inv, H, W, flags, nhwc8_ptr, nchw_ptr, mean=MEAN32, std=STD32, stream=None):
    return lib.fvp_ingest_frames(frames_ptr, n, hs, ws, _fa(inv), _fa(mean), _fa(std), H, W, flags, nhwc8_ptr, nchw_ptr,
                                 stream)


def run(lib, frames, forward, W, H, swap, general, device=None, want_bf16=True, want_nchw=True):
    """frames: numpy uint8 [N,Hs,Ws,3].  device None: numpy memory (the emulator); else torch memory on that device.
    Returns (nhwc8 uint16 [N,H,W/2,8] or None, nchw fp32 [N,3,H,W] or None) as numpy arrays."""
    n, hs, ws, _ = frames.shape
    inv = invert_affine(forward)
    flags = (capi.INGEST_SWAP_RB if swap else 0) | (capi.INGEST_GENERAL if general else 0)
    if device is None:
        fr = np.ascontiguousarray(frames)
        # poisoned outputs: a pixel the kernel leaves out shows
        o16 = np.full((n, H, W // 2, 8), 0xDEAD, np.uint16) if want_bf16 else None
        o32 = np.full((n, 3, H, W), np.nan, f32) if want_nchw else None
        rc = call(lib, fr.ctypes.data, n, hs, ws, inv, H, W, flags, o16.ctypes.data if want_bf16 else None,
                  o32.ctypes.data if want_nchw else None)
        assert rc == 0, rc
        return o16, o32
    fr = torch.from_numpy(np.ascontiguousarray(frames)).to(device)
    o16 = torch.full((n, H, W // 2, 8), -8531, dtype=torch.int16, device=device) if want_bf16 else None
    o32 = torch.full((n, 3, H, W), float("nan"), dtype=torch.float32, device=device) if want_nchw else None
    rc = call(lib, fr.data_ptr(), n, hs, ws, inv, H, W, flags, o16.data_ptr() if want_bf16 else None,
              o32.data_ptr() if want_nchw else None, stream=C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, rc
    torch.cuda.synchronize()
    return (o16.cpu().numpy().view(np.uint16) if want_bf16 else None), (o32.cpu().numpy() if want_nchw else None)


def torch_loader_f32(frames_rgb):
    """ToTensor + Normalize of the reference's loader (run/validate.py:44-52) on the CPU in fp32: uint8 [N,H,W,3] ->
    [N,3,H,W]."""
    t = torch.from_numpy(np.ascontiguousarray(frames_rgb)).permute(0, 3, 1, 2).float()
    mean = torch.tensor(IMAGENET_MEAN, dtype=torch.float32).view(1, 3, 1, 1)
    std = torch.tensor(IMAGENET_STD, dtype=torch.float32).view(1, 3, 1, 1)
    return (((t / 255) - mean) / std).contiguous()


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def f64_bound(forward, hs, ws, W, H, std=STD32, mean=MEAN32):
    """Bound on |fp32 kernel - exact float64 bilinear| (see test_against_exact_bilinear_in_float64's docstring)."""
    u = 2.0 ** -24                                              # fp32 unit roundoff
    inv = np.abs(invert_affine(forward).astype(np.float64)).reshape(2, 3)
    m = float(max(inv[r, 0] * (W - 1) + inv[r, 1] * (H - 1) + inv[r, 2] for r in range(2)))
    m = max(m, float(max(hs, ws)))
    d_coord = 8 * u * m                                         # 3 rounded coefficients + 4 rounded operations, <= 8 u m
    d_v = 255.0 * 2 * d_coord + 10 * u * 255.0                  # Lipschitz 255 per axis; 1-fx, 1-fy, 6 products, 3 sums (<= 10)
    smin, mmax = float(np.min(std)), float(np.max(mean))
    return d_v / (255.0 * smin) + 4 * u * (1.0 + mmax) / smin   # / 255, - mean, / std at magnitude <= (1 + mean) / std
