"""Shared by tests/test_ingest_nv12_emu.py (CPU emulator) and tests/test_ingest_nv12_gpu.py (the shipped library on the
card): the NV12 cases, the integer colour conversion of include/fvp.h restated in numpy int64, a seeded generator of
pitched surfaces whose padding is random, and a runner that calls fvp_ingest_nv12 on numpy (emulator) or torch-GPU
memory.  The float side (reference_f32, pack_nhwc8, bits, invert_affine) is that of tests/ingest_cases.py, unchanged."""
import ctypes as C

import numpy as np
import torch

from ingest_cases import IDENTITY, MEAN32, STD32, _fa, _rotated, bits, invert_affine, pack_nhwc8, reference_f32  # noqa: F401
from faster_voxelpose_amd.utils.transforms import get_resize_transform

BT601_LIMITED, BT709_LIMITED, BT601_FULL, BT709_FULL = 0, 1, 2, 3
# standard -> (yoff, CY, CRV, CGU, CGV, CBU): the table of the issue / include/fvp.h, typed in a second time here
# (test_header_coefficients compares the header's literals with these and with float64 recomputed from Kr, Kb)
COEFFS = {
    BT601_LIMITED: (16, 1220945, 1673555, -410793, -852458, 2115221),
    BT709_LIMITED: (16, 1220945, 1879825, -223607, -558796, 2215014),
    BT601_FULL: (0, 1048576, 1470104, -360853, -748826, 1858077),
    BT709_FULL: (0, 1048576, 1651297, -196424, -490864, 1945738),
}
KR_KB = {BT601_LIMITED: (0.299, 0.114, True), BT709_LIMITED: (0.2126, 0.0722, True),
         BT601_FULL: (0.299, 0.114, False), BT709_FULL: (0.2126, 0.0722, False)}

# name -> dict(src (Ws, Hs), dst (W, H), fwd 2x3 camera -> network, n, y_pitch, uv_pitch (None: Ws), split (UV plane in
# an allocation of its own), gap (bytes between the end of a plane and the next frame's), standard)
_L = get_resize_transform((96, 54), (48, 26))


def _c(src, dst, fwd, n, standard, y_pitch=None, uv_pitch=None, split=False, gap=0):
    return dict(src=src, dst=dst, fwd=fwd, n=n, standard=standard, y_pitch=y_pitch or src[0], uv_pitch=uv_pitch or src[0],
                split=split, gap=gap)


CASES = {
    # the Panoptic geometry scaled down (letter-box: border taps occur); pitch == Ws, one contiguous NV12 buffer per frame
    "letterbox": _c((96, 54), (48, 26), _L, 3, BT601_LIMITED),
    # the same geometry on a pitched surface: odd luma pitch, another (even) chroma pitch, the UV plane allocated apart,
    # frames further apart than a plane is long
    "letterbox_pitched": _c((96, 54), (48, 26), _L, 3, BT709_LIMITED, y_pitch=101, uv_pitch=98, split=True, gap=38),
    # tall source into a wide network image: a wide border left and right
    "tall_source": _c((30, 40), (48, 26), get_resize_transform((30, 40), (48, 26)), 1, BT601_FULL, y_pitch=32, uv_pitch=32),
    "upscale": _c((46, 22), (64, 32), get_resize_transform((46, 22), (64, 32)), 3, BT709_FULL, y_pitch=64, uv_pitch=48,
                  split=True),
    "identity": _c((40, 24), (40, 24), IDENTITY, 3, BT601_LIMITED, y_pitch=48, uv_pitch=48),
    # a wide row (more than one wave of pixel pairs per row), shifted and scaled per axis: taps above the frame
    "wide_shifted": _c((302, 20), (262, 10), np.array([[0.9, 0.0, -3.3], [0.0, 0.55, 1.2]]), 1, BT709_LIMITED, y_pitch=320,
                       uv_pitch=320),
    "mirror": _c((34, 10), (34, 8), np.array([[-1.0, 0.0, 33.0], [0.0, 1.0, 0.0]]), 1, BT601_FULL),
    "rotation": _c((50, 38), (32, 20), _rotated((50, 38), (32, 20), 20.0), 1, BT709_FULL, y_pitch=53, uv_pitch=52, split=True,
                   gap=2),
    # the smallest frame: one chroma sample per frame, so two frames carry the two clipping pairs
    "smallest": _c((2, 2), (6, 4), get_resize_transform((2, 2), (6, 4)), 2, BT601_LIMITED),
}


def unclipped_rgb(y, uv, standard, chroma_at_luma=False, swap_uv=False, no_floor=False):
    """The integer formula of include/fvp.h in int64 before the clip: y [N,Hs,Ws], uv [N,Hs/2,Ws/2,2] -> [N,Hs,Ws,3].
    The three switches are the faults of test_reference_sees_the_faults, never used for an expected value."""
    yoff, cy, crv, cgu, cgv, cbu = COEFFS[standard]
    hs, ws = y.shape[1:]
    yi, xi = np.arange(hs)[:, None], np.arange(ws)[None, :]
    if chroma_at_luma:
        cyi, cxi = np.minimum(yi, hs // 2 - 1), np.minimum(xi, ws // 2 - 1)
    else:
        cyi, cxi = yi >> 1, xi >> 1
    u = uv[:, cyi, cxi, 1 if swap_uv else 0].astype(np.int64)
    v = uv[:, cyi, cxi, 0 if swap_uv else 1].astype(np.int64)
    c = y.astype(np.int64) - yoff
    if not no_floor:
        c = np.maximum(0, c)
    d, e = u - 128, v - 128
    half = 1 << 19
    r = (cy * c + crv * e + half) >> 20                      # numpy's >> on int64 is arithmetic: floor
    g = (cy * c + cgu * d + cgv * e + half) >> 20
    b = (cy * c + cbu * d + half) >> 20
    assert max(abs(cy * c).max(), abs(cgu * d + cgv * e).max(), abs(cbu * d).max()) < 5.8e8
    return np.stack([r, g, b], axis=-1)


def nv12_to_rgb(y, uv, standard, **fault):
    return np.clip(unclipped_rgb(y, uv, standard, **fault), 0, 255).astype(np.uint8)


class Surface:
    """The raw allocations of one case and where its planes lie in them."""

    def __init__(self, name, seed=0):
        c = CASES[name]
        (ws, hs), n = c["src"], c["n"]
        self.case, self.n, self.hs, self.ws, self.standard = c, n, hs, ws, c["standard"]
        self.y_pitch, self.uv_pitch = c["y_pitch"], c["uv_pitch"]
        rng = np.random.default_rng([seed, sum(name.encode())])
        ylen, uvlen = hs * self.y_pitch, (hs // 2) * self.uv_pitch
        if c["split"]:
            self.y_frame, self.uv_frame = ylen + c["gap"], uvlen + c["gap"]
            self.ybuf = rng.integers(1, 256, size=n * self.y_frame, dtype=np.uint8)       # padding: random, never 0
            self.uvbuf = rng.integers(1, 256, size=n * self.uv_frame, dtype=np.uint8)
            self.y_off, self.uv_off = 0, 0
        else:
            assert self.y_pitch == self.uv_pitch and c["gap"] % 2 == 0
            self.y_frame = self.uv_frame = ylen + uvlen + c["gap"]
            self.ybuf = self.uvbuf = rng.integers(1, 256, size=n * self.y_frame, dtype=np.uint8)
            self.y_off, self.uv_off = 0, ylen                  # uv = y + Hs * pitch: the contiguous NV12 buffer
        y, uv = self.planes()
        y[...] = rng.integers(0, 256, size=y.shape, dtype=np.uint8)
        uv[...] = rng.integers(0, 256, size=uv.shape, dtype=np.uint8)
        # extremes all over the frame, so that the taps the warp actually reads clip too
        ey = rng.random(y.shape)
        y[ey < 1 / 16] = 0
        y[ey > 15 / 16] = 255
        eu = rng.random(uv.shape[:-1])
        uv[eu < 1 / 16] = (0, 0)
        uv[eu > 15 / 16] = (255, 255)
        # forced whatever the generator drew: Y = 0 and Y = 255 under (255, 255) [R, B clip high; G low] in the first
        # quad of the first frame and under (0, 0) [G high; R, B low] in the last quad of the last frame
        y[0, 0, 0], y[0, 0, 1], uv[0, 0, 0] = 0, 255, (255, 255)
        y[-1, -1, -1], y[-1, -1, -2], uv[-1, -1, -1] = 0, 255, (0, 0)

    def planes(self, y_pitch=None, uv_pitch=None):
        """Strided numpy views [N,Hs,Ws] and [N,Hs/2,Ws/2,2] of the allocations (writable)."""
        st = np.lib.stride_tricks.as_strided
        y = st(self.ybuf[self.y_off:], (self.n, self.hs, self.ws), (self.y_frame, y_pitch or self.y_pitch, 1))
        uv = st(self.uvbuf[self.uv_off:], (self.n, self.hs // 2, self.ws // 2, 2),
                (self.uv_frame, uv_pitch or self.uv_pitch, 2, 1))
        return y, uv

    def rgb(self):
        y, uv = self.planes()
        return nv12_to_rgb(y, uv, self.standard)

    def torch_frames(self, device=None, lead=None):
        """The same surface as dataset.images.Nv12Frames over torch memory (CPU: aliases the numpy allocations)."""
        from faster_voxelpose_amd.dataset.images import Nv12Frames
        yb, ub = torch.from_numpy(self.ybuf), torch.from_numpy(self.uvbuf)
        if device is not None:
            yb = yb.to(device)
            ub = yb if self.uvbuf is self.ybuf else ub.to(device)
        y = torch.as_strided(yb, (self.n, self.hs, self.ws), (self.y_frame, self.y_pitch, 1), self.y_off)
        uv = torch.as_strided(ub, (self.n, self.hs // 2, self.ws // 2, 2), (self.uv_frame, self.uv_pitch, 2, 1), self.uv_off)
        if lead is not None:
            y, uv = y.unflatten(0, lead), uv.unflatten(0, lead)
        std = {0: ("bt601", False), 1: ("bt709", False), 2: ("bt601", True), 3: ("bt709", True)}[self.standard]
        return Nv12Frames(y, uv, standard=std[0], full_range=std[1])


def call(lib, y_ptr, uv_ptr, n, hs, ws, y_pitch, uv_pitch, y_frame, uv_frame, standard, inv, H, W, nhwc8_ptr, nchw_ptr,
         mean=MEAN32, std=STD32, stream=None):
    return lib.fvp_ingest_nv12(y_ptr, uv_ptr, n, hs, ws, y_pitch, uv_pitch, y_frame, uv_frame, standard, _fa(inv), _fa(mean),
                               _fa(std), H, W, nhwc8_ptr, nchw_ptr, stream)


def run(lib, surf, device=None, want_bf16=True, want_nchw=True):
    """fvp_ingest_nv12 on a Surface.  device None: numpy memory (the emulator); else torch memory on that device.
    Returns (nhwc8 uint16 [N,H,W/2,8] or None, nchw fp32 [N,3,H,W] or None) as numpy arrays; outputs start poisoned."""
    c = surf.case
    (W, H), n = c["dst"], surf.n
    inv = invert_affine(c["fwd"])
    geo = (n, surf.hs, surf.ws, surf.y_pitch, surf.uv_pitch, surf.y_frame, surf.uv_frame, surf.standard, inv, H, W)
    if device is None:
        o16 = np.full((n, H, W // 2, 8), 0xDEAD, np.uint16) if want_bf16 else None
        o32 = np.full((n, 3, H, W), np.nan, np.float32) if want_nchw else None
        rc = call(lib, surf.ybuf.ctypes.data + surf.y_off, surf.uvbuf.ctypes.data + surf.uv_off, *geo,
                  o16.ctypes.data if want_bf16 else None, o32.ctypes.data if want_nchw else None)
        assert rc == 0, rc
        return o16, o32
    yb = torch.from_numpy(surf.ybuf).to(device)
    ub = yb if surf.uvbuf is surf.ybuf else torch.from_numpy(surf.uvbuf).to(device)
    o16 = torch.full((n, H, W // 2, 8), -8531, dtype=torch.int16, device=device) if want_bf16 else None
    o32 = torch.full((n, 3, H, W), float("nan"), dtype=torch.float32, device=device) if want_nchw else None
    rc = call(lib, yb.data_ptr() + surf.y_off, ub.data_ptr() + surf.uv_off, *geo, o16.data_ptr() if want_bf16 else None,
              o32.data_ptr() if want_nchw else None, stream=C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, rc
    torch.cuda.synchronize()
    return (o16.cpu().numpy().view(np.uint16) if want_bf16 else None), (o32.cpu().numpy() if want_nchw else None)
