"""Shared by tests/test_bayer_emu.py (CPU emulator) and tests/test_bayer_gpu.py (the shipped library on the card): the
Bayer cases, the integer demosaic of include/fvp.h restated in numpy int64 (typed from the header's text), a seeded
generator of pitched mosaics whose padding is random and never 0, and runners that call fvp_demosaic_bayer and
fvp_ingest_bayer on numpy (emulator) or torch-GPU memory.  The float side (reference_f32, pack_nhwc8, bits,
invert_affine) is that of tests/ingest_cases.py, unchanged; the geometry is that of ingest_nv12_cases.CASES."""
import ctypes as C

import numpy as np
import torch

from ingest_cases import IDENTITY, MEAN32, STD32, _fa, _rotated, bits, invert_affine, pack_nhwc8, reference_f32  # noqa: F401
from faster_voxelpose_amd.utils.transforms import get_affine_transform, get_resize_transform

RGGB, GRBG, GBRG, BGGR = 0, 1, 2, 3
RED_AT = {RGGB: (0, 0), GRBG: (1, 0), GBRG: (0, 1), BGGR: (1, 1)}        # pattern -> (rx, ry), the header's table
NAMES = {RGGB: "rggb", GRBG: "grbg", GBRG: "gbrg", BGGR: "bggr"}
GUARD = 64                                                               # poisoned bytes either side of an RGB output

# the shipped kernels' tiles: k_demosaic_bayer owns 256 x 8 pixels per workgroup, k_ingest_bayer_lds 64 x 8 destination pixels
DEMOSAIC_TILE = (256, 8)
INGEST_TILE = (64, 8)


def _c(src, dst, fwd, n, pattern, pitch=None, gap=0, tone=False, form="lds"):
    return dict(src=src, dst=dst, fwd=fwd, n=n, pattern=pattern, pitch=pitch or src[0], gap=gap, tone=tone, form=form)


def _rotated_wide(src, dst, deg):
    """ingest_cases._rotated with a window 1.3 times the frame instead of 0.8: the border is sampled too."""
    ws, hs = src
    return get_affine_transform(np.array([ws / 2.0, hs / 2.0]), np.array([ws, hs], np.float32) / 200.0 * 1.3, deg, dst)


_L = get_resize_transform((96, 54), (48, 26))
_S = get_resize_transform((4, 4), (6, 4))
CASES = {}
for _p in (RGGB, GRBG, GBRG, BGGR):
    CASES[f"letterbox_{NAMES[_p]}"] = _c((96, 54), (48, 26), _L, 3, _p)
CASES.update({
    # odd pitch, frames further apart than a frame is long, a non-identity tone table
    "letterbox_pitched": _c((96, 54), (48, 26), _L, 3, GRBG, pitch=101, gap=38, tone=True),
    "tall_source": _c((30, 40), (48, 26), get_resize_transform((30, 40), (48, 26)), 1, GBRG, pitch=32),
    "upscale": _c((46, 22), (64, 32), get_resize_transform((46, 22), (64, 32)), 3, BGGR, pitch=64),
    "identity": _c((40, 24), (40, 24), IDENTITY, 3, RGGB, pitch=48, tone=True),
    # a row longer than one wave of pixel pairs and several destination tiles; taps above the frame
    "wide_shifted": _c((302, 20), (262, 10), np.array([[0.9, 0.0, -3.3], [0.0, 0.55, 1.2]]), 1, GRBG, pitch=320),
    "mirror": _c((34, 10), (34, 8), np.array([[-1.0, 0.0, 33.0], [0.0, 1.0, 0.0]]), 1, GBRG),
    "rotation": _c((50, 38), (32, 20), _rotated((50, 38), (32, 20), 20.0), 1, BGGR, pitch=53, gap=2),
    # the other side of the dispatch rule: a destination tile of 64 x 8 spans 1072 x 120 source pixels, far beyond the LDS
    # budget, so the gather kernel runs (odd pitch and a tone table there too)
    "steep_downscale": _c((1100, 124), (66, 8), np.array([[1.0 / 17.0, 0.0, 0.4], [0.0, 1.0 / 17.0, 0.3]]), 1, GRBG,
                          pitch=1101, tone=True, form="gather"),
    # the gather kernel under a rotation, the frame's corners and borders inside the network image
    "rotated_downscale": _c((420, 300), (64, 16), _rotated_wide((420, 300), (64, 16), 30.0), 1, BGGR, pitch=424,
                            form="gather"),
})
for _p in (RGGB, GRBG, GBRG, BGGR):
    CASES[f"smallest_{NAMES[_p]}"] = _c((4, 4), (6, 4), _S, 2, _p)      # every neighbour of every pixel is reflected

# demosaic-only sizes (Ws, Hs) around the shipped tile: the tile, the tile +- 2 in each direction, and 6 x 4
DEMOSAIC_SIZES = [(256, 8), (254, 8), (258, 8), (256, 6), (256, 10), (6, 4)]


def lds_plan(inv, H, W, Hs, Ws):
    """The dispatch rule of fvp_ingest_bayer restated: a function of inv, H, W, Hs, Ws only.  Returns (fits, RW, RH)."""
    inv = np.asarray(inv, np.float32).astype(np.float64)
    tw, th = min(W, INGEST_TILE[0]) - 1, min(H, INGEST_TILE[1]) - 1
    dims = []
    for a, n in ((0, Ws), (1, Hs)):
        ka, kb, kc = abs(inv[3 * a]), abs(inv[3 * a + 1]), abs(inv[3 * a + 2])
        m = ka * (W - 1) + kb * (H - 1) + kc
        e = np.floor(ka * tw + kb * th + 2.0 * (5.0 * m * 2.0 ** -24)) + 3.0
        dims.append(int(e) if e < n else n)
    rw, rh = (dims[0] + 6) & ~3, (dims[1] + 2) & ~1
    return rh * rw * 4 + (rh + 4) * (rw + 8) <= 47 * 1024, rw, rh


def _reflect(i, n, clamp=False):
    if clamp:                                           # the fault "a clamped border instead of a reflected one"
        return np.clip(i, 0, n - 1)
    i = np.where(i < 0, -i, i)
    return np.where(i >= n, 2 * (n - 1) - i, i)


def sixteenths(raw, pattern, shift_pattern=False, clamp_border=False, swap_h2v2=False):
    """include/fvp.h in numpy int64 before rounding: raw [N,Hs,Ws] uint8 -> X16 [N,Hs,Ws,3] (R, G, B).  The switches are
    the faults of test_reference_sees_the_faults, never used for an expected value."""
    raw = np.asarray(raw)
    n, hs, ws = raw.shape
    rx, ry = RED_AT[pattern]
    if shift_pattern:
        rx ^= 1
    v = raw.astype(np.int64)
    yi, xi = np.arange(hs)[:, None], np.arange(ws)[None, :]

    def at(dy, dx):
        return v[:, _reflect(yi + dy, hs, clamp_border), _reflect(xi + dx, ws, clamp_border)]

    c = at(0, 0)
    h1 = at(0, -1) + at(0, 1)
    v1 = at(-1, 0) + at(1, 0)
    d = at(-1, -1) + at(-1, 1) + at(1, -1) + at(1, 1)
    h2 = at(0, -2) + at(0, 2)
    v2 = at(-2, 0) + at(2, 0)
    own = 16 * c
    green_at_rb = 8 * c + 4 * (h1 + v1) - 2 * (h2 + v2)
    third = 12 * c + 4 * d - 3 * (h2 + v2)
    if swap_h2v2:
        row_nb = 10 * c + 8 * h1 - 2 * d - 2 * v2 + h2
        col_nb = 10 * c + 8 * v1 - 2 * d - 2 * h2 + v2
    else:
        row_nb = 10 * c + 8 * h1 - 2 * d - 2 * h2 + v2
        col_nb = 10 * c + 8 * v1 - 2 * d - 2 * v2 + h2
    xr, yr = ((xi & 1) == rx)[None], ((yi & 1) == ry)[None]
    red, blue = xr & yr, ~xr & ~yr
    green_red_row, green_blue_row = ~xr & yr, xr & ~yr
    out = np.empty(raw.shape + (3,), np.int64)
    out[..., 0] = np.where(red, own, np.where(blue, third, np.where(green_red_row, row_nb, col_nb)))
    out[..., 1] = np.where(red | blue, green_at_rb, own)
    out[..., 2] = np.where(blue, own, np.where(red, third, np.where(green_blue_row, row_nb, col_nb)))
    assert (red | blue | green_red_row | green_blue_row).all() and out.min() >= -3060 and out.max() <= 7140
    return out


def demosaic(raw, pattern, tone=None, no_round=False, **fault):
    """The SOURCE RGB PIXELS of include/fvp.h: uint8 [N,Hs,Ws,3]."""
    x16 = sixteenths(raw, pattern, **fault)
    rgb = np.clip((x16 + (0 if no_round else 8)) >> 4, 0, 255)         # numpy's >> on int64 is arithmetic: floor
    if tone is not None:
        rgb = np.stack([np.asarray(tone)[ch][rgb[..., ch]] for ch in range(3)], axis=-1)
    return rgb.astype(np.uint8)


def tone_formula(gains, gamma, black):
    """BayerFrames.tone_table's formula typed a second time, element by element in Python floats (float64)."""
    lut = np.empty((3, 256), np.uint8)
    for ch in range(3):
        for v in range(256):
            lin = min(max((v - black) * gains[ch] / (255 - black), 0.0), 1.0)
            lut[ch, v] = int(min(max(np.rint(255 * lin ** (1 / gamma)), 0), 255))
    return lut


TONE_ARGS = dict(gains=(1.9, 1.0, 1.6), gamma=2.2, black=16)


class Mosaic:
    """The raw allocation of one case (or of a demosaic-only size) and where its frames lie in it."""

    def __init__(self, name, case=None, seed=0):
        c = case or CASES[name]
        (ws, hs), n = c["src"], c["n"]
        self.case, self.n, self.hs, self.ws, self.pattern, self.pitch = c, n, hs, ws, c["pattern"], c["pitch"]
        rng = np.random.default_rng([seed, sum(name.encode())])
        self.frame = hs * self.pitch + c["gap"]
        self.buf = rng.integers(1, 256, size=n * self.frame, dtype=np.uint8)               # padding: random, never 0
        raw = self.frames()
        raw[...] = rng.integers(0, 256, size=raw.shape, dtype=np.uint8)
        for _ in range(10000 if hs * ws < 30 * 22 else 0):
            # too small for uniform bytes to clip at both ends of every channel on their own: extremes all over the
            # frame, drawn again until the restated formulas clip (seeded, so the same mosaic every time)
            v = (sixteenths(raw, self.pattern) + 8) >> 4
            if (v.reshape(-1, 3).min(0) < 0).all() and (v.reshape(-1, 3).max(0) > 255).all():
                break
            raw[...] = rng.integers(0, 256, size=raw.shape, dtype=np.uint8)
            e = rng.random(raw.shape)
            raw[e < 1 / 4] = 0
            raw[e > 3 / 4] = 255
        self.tone = tone_formula(**TONE_ARGS) if c["tone"] else None

    def frames(self, pitch=None):
        """Strided numpy view [N,Hs,Ws] of the allocation (writable)."""
        return np.lib.stride_tricks.as_strided(self.buf, (self.n, self.hs, self.ws), (self.frame, pitch or self.pitch, 1))

    def rgb(self, **fault):
        return demosaic(self.frames(), self.pattern, self.tone, **fault)

    def torch_frames(self, device=None, lead=None):
        """The same mosaic as dataset.images.BayerFrames over torch memory (CPU: aliases the numpy allocation)."""
        from faster_voxelpose_amd.dataset.images import BayerFrames
        b = torch.from_numpy(self.buf)
        tone = torch.from_numpy(self.tone) if self.tone is not None else None
        if device is not None:
            b, tone = b.to(device), (tone.to(device) if tone is not None else None)
        raw = torch.as_strided(b, (self.n, self.hs, self.ws), (self.frame, self.pitch, 1))
        if lead is not None:
            raw = raw.unflatten(0, lead)
        return BayerFrames(raw, NAMES[self.pattern], tone)


def sized(ws, hs, pattern=GRBG, n=2, pitch=None, gap=0, tone=False):
    return Mosaic(f"size_{ws}x{hs}", _c((ws, hs), (ws, hs), IDENTITY, n, pattern, pitch=pitch, gap=gap, tone=tone))


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def call_demosaic(lib, raw_ptr, n, hs, ws, pitch, frame, pattern, tone_ptr, flags, rgb_ptr, stream=None):
    return lib.fvp_demosaic_bayer(raw_ptr, n, hs, ws, pitch, frame, pattern, tone_ptr, flags, rgb_ptr, stream)


def call_ingest(lib, raw_ptr, n, hs, ws, pitch, frame, pattern, tone_ptr, inv, H, W, nhwc8_ptr, nchw_ptr, mean=MEAN32,
                std=STD32, stream=None):
    return lib.fvp_ingest_bayer(raw_ptr, n, hs, ws, pitch, frame, pattern, tone_ptr, _fa(inv), _fa(mean), _fa(std), H, W,
                                nhwc8_ptr, nchw_ptr, stream)


def run_demosaic(lib, m, device=None):
    """fvp_demosaic_bayer on a Mosaic -> (rgb uint8 [N,Hs,Ws,3], guards_intact).  The output starts poisoned between two
    guard bands."""
    size = m.n * m.hs * m.ws * 3
    geo = (m.n, m.hs, m.ws, m.pitch, m.frame, m.pattern)
    if device is None:
        out = np.full(size + 2 * GUARD, 0xA5, np.uint8)
        rc = call_demosaic(lib, m.buf.ctypes.data, *geo, m.tone.ctypes.data if m.tone is not None else None, 0,
                           out.ctypes.data + GUARD)
        assert rc == 0, rc
    else:
        buf = torch.from_numpy(m.buf).to(device)
        tone = torch.from_numpy(m.tone).to(device) if m.tone is not None else None
        o = torch.full((size + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=device)
        rc = call_demosaic(lib, buf.data_ptr(), *geo, tone.data_ptr() if tone is not None else None, 0,
                           o.data_ptr() + GUARD, stream=_stream())
        assert rc == 0, rc
        torch.cuda.synchronize()
        out = o.cpu().numpy()
    ok = bool((out[:GUARD] == 0xA5).all() and (out[-GUARD:] == 0xA5).all())
    return out[GUARD:-GUARD].reshape(m.n, m.hs, m.ws, 3), ok


def run_ingest(lib, m, device=None, want_bf16=True, want_nchw=True):
    """fvp_ingest_bayer on a Mosaic.  Returns (nhwc8 uint16 [N,H,W/2,8] or None, nchw fp32 [N,3,H,W] or None) as numpy
    arrays; outputs start poisoned."""
    c = m.case
    (W, H), n = c["dst"], m.n
    inv = invert_affine(c["fwd"])
    geo = (n, m.hs, m.ws, m.pitch, m.frame, m.pattern)
    if device is None:
        o16 = np.full((n, H, W // 2, 8), 0xDEAD, np.uint16) if want_bf16 else None
        o32 = np.full((n, 3, H, W), np.nan, np.float32) if want_nchw else None
        rc = call_ingest(lib, m.buf.ctypes.data, *geo, m.tone.ctypes.data if m.tone is not None else None, inv, H, W,
                         o16.ctypes.data if want_bf16 else None, o32.ctypes.data if want_nchw else None)
        assert rc == 0, rc
        return o16, o32
    buf = torch.from_numpy(m.buf).to(device)
    tone = torch.from_numpy(m.tone).to(device) if m.tone is not None else None
    o16 = torch.full((n, H, W // 2, 8), -8531, dtype=torch.int16, device=device) if want_bf16 else None
    o32 = torch.full((n, 3, H, W), float("nan"), dtype=torch.float32, device=device) if want_nchw else None
    rc = call_ingest(lib, buf.data_ptr(), *geo, tone.data_ptr() if tone is not None else None, inv, H, W,
                     o16.data_ptr() if want_bf16 else None, o32.data_ptr() if want_nchw else None, stream=_stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return (o16.cpu().numpy().view(np.uint16) if want_bf16 else None), (o32.cpu().numpy() if want_nchw else None)
