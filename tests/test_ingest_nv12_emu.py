"""fvp_ingest_nv12 (NV12 decoder surface -> backbone input) on the CPU emulator: the unmodified kernel source of
csrc/fvp_heatmap.hip compiled for the host (tests/hipemu).  The defining property of include/fvp.h is tested bit for
bit: the outputs equal fvp_ingest_frames applied to the RGB frame obtained by converting every source pixel with the
integer formula.  tests/test_ingest_nv12_gpu.py repeats the value checks on the shipped library."""
import os
import re

import numpy as np
import pytest
import torch

import ingest_cases as IC
import ingest_nv12_cases as NC
from faster_voxelpose_amd import _capi as capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = 10001


@pytest.fixture(scope="module")
def surfaces():
    """Every case's surface and its float32 reference, computed once and never written to."""
    out = {}
    for name, c in NC.CASES.items():
        s = NC.Surface(name)
        W, H = c["dst"]
        rgb = s.rgb()
        ref = NC.reference_f32(rgb, NC.invert_affine(c["fwd"]), W, H, False)
        out[name] = (s, rgb, ref)
    return out


@pytest.mark.parametrize("name", list(NC.CASES))
def test_bit_equal_to_the_restatement(emu_lib, surfaces, name):
    """Both outputs, every pixel (they start poisoned), against nv12_to_rgb (numpy int64) followed by the float32
    restatement of fvp_ingest_frames with swap = 0; then each output requested alone."""
    s, rgb, ref = surfaces[name]
    o16, o32 = NC.run(emu_lib, s)
    bad = int((NC.bits(o32) != NC.bits(ref)).sum())
    assert bad == 0, f"{bad} of {ref.size} fp32 values differ"
    assert np.array_equal(o16, NC.pack_nhwc8(ref))
    only16, none32 = NC.run(emu_lib, s, want_nchw=False)
    assert none32 is None and np.array_equal(only16, o16)
    none16, only32 = NC.run(emu_lib, s, want_bf16=False)
    assert none16 is None and np.array_equal(NC.bits(only32), NC.bits(o32))


@pytest.mark.parametrize("name", list(NC.CASES))
def test_equals_ingest_frames_on_the_converted_frame(emu_lib, surfaces, name):
    """The defining property: == fvp_ingest_frames (same emulated library, flags = 0) on the RGB uint8 frame."""
    s, rgb, _ = surfaces[name]
    c = s.case
    W, H = c["dst"]
    r16, r32 = IC.run(emu_lib, rgb, c["fwd"], W, H, False, False)
    o16, o32 = NC.run(emu_lib, s)
    assert np.array_equal(o16, r16) and np.array_equal(NC.bits(o32), NC.bits(r32))


def _header_rows():
    text = open(os.path.join(ROOT, "include", "fvp.h")).read()
    rows = {m.group(1): tuple(int(v) for v in m.group(2).split(","))
            for m in re.finditer(r"#define FVP_YUV_(\w+)_COEFFS \{([^}]*)\}", text)}
    enum = {m.group(1): int(m.group(2)) for m in re.finditer(r"FVP_YUV_(BT\d+_\w+?) = (\d)", text)}
    return rows, enum


def test_header_coefficients():
    """The four rows of include/fvp.h == round(k * 2^20) recomputed in float64 from Kr and Kb, and == the table the
    numpy conversion of these tests uses; the enum values are 0..3 in the documented order."""
    rows, enum = _header_rows()
    assert enum == {"BT601_LIMITED": 0, "BT709_LIMITED": 1, "BT601_FULL": 2, "BT709_FULL": 3}
    assert (capi.YUV_BT601_LIMITED, capi.YUV_BT709_LIMITED, capi.YUV_BT601_FULL, capi.YUV_BT709_FULL) == (0, 1, 2, 3)
    assert sorted(rows) == sorted(enum)
    for name, std in enum.items():
        kr, kb, limited = NC.KR_KB[std]
        kg = 1.0 - kr - kb
        gy, g = (255.0 / 219.0, 255.0 / 224.0) if limited else (1.0, 1.0)
        crv, cbu = 2.0 * (1.0 - kr) * g, 2.0 * (1.0 - kb) * g
        want = (16 if limited else 0,) + tuple(int(round(k * 2.0 ** 20)) for k in (gy, crv, -cbu * kb / kg, -crv * kr / kg, cbu))
        assert rows[name] == want, name
        assert NC.COEFFS[std] == want, name


@pytest.mark.parametrize("standard", sorted(NC.COEFFS))
def test_grey_stays_grey(emu_lib, standard):
    """U = V = 128: R = G = B for every luma value, in the numpy formula and in the kernel (identity warp, mean 0, std 1:
    the three fp32 planes are equal bit for bit)."""
    y = np.arange(256, dtype=np.uint8).reshape(1, 8, 32)
    uv = np.full((1, 4, 16, 2), 128, np.uint8)
    rgb = NC.nv12_to_rgb(y, uv, standard)
    assert np.array_equal(rgb[..., 0], rgb[..., 1]) and np.array_equal(rgb[..., 1], rgb[..., 2])
    assert rgb.min() == 0 and rgb.max() == 255
    o32 = np.full((1, 3, 8, 32), np.nan, np.float32)
    rc = NC.call(emu_lib, y.ctypes.data, uv.ctypes.data, 1, 8, 32, 32, 32, 256, 128, standard, NC.invert_affine(NC.IDENTITY),
                 8, 32, None, o32.ctypes.data, mean=(0, 0, 0), std=(1, 1, 1))
    assert rc == 0
    assert np.array_equal(NC.bits(o32[0, 0]), NC.bits(o32[0, 1])) and np.array_equal(NC.bits(o32[0, 1]), NC.bits(o32[0, 2]))
    assert np.array_equal(o32[0, 0], rgb[0, ..., 0].astype(np.float32) / np.float32(255))


def test_cases_cover_what_their_comments_say(surfaces):
    """Border taps occur, an odd pitch and pitches larger than the width are present, planes both contiguous and apart,
    a frame stride larger than the plane, every standard in at least two cases, the extreme luma values in every case,
    and clipping at both ends of every channel in every case."""
    sides = {}
    for name, k in NC.CASES.items():
        inv = NC.invert_affine(k["fwd"]).astype(np.float64)
        (ws, hs), (W, H) = k["src"], k["dst"]
        x, y = np.meshgrid(np.arange(W), np.arange(H))
        sx, sy = inv[0] * x + inv[1] * y + inv[2], inv[3] * x + inv[4] * y + inv[5]
        sides[name] = {side for side, hit in (("left", sx.min() < 0), ("right", sx.max() > ws - 1), ("top", sy.min() < 0),
                                              ("bottom", sy.max() > hs - 1)) if hit}
    assert sides["letterbox"] and sides["letterbox"] == sides["letterbox_pitched"]
    assert sides["tall_source"] >= {"left", "right"} and "top" in sides["wide_shifted"]
    assert set().union(*sides.values()) == {"left", "right", "top", "bottom"}
    assert NC.CASES["wide_shifted"]["dst"][0] // 2 > 64               # a row is more than one wave of pixel pairs
    cases = NC.CASES.values()
    assert any(k["y_pitch"] % 2 for k in cases)
    assert any(k["y_pitch"] > k["src"][0] for k in cases) and any(k["uv_pitch"] > k["src"][0] for k in cases)
    assert any(k["y_pitch"] == k["src"][0] and not k["split"] for k in cases)
    assert any(k["y_pitch"] != k["uv_pitch"] for k in cases)
    assert any(k["split"] and k["gap"] > 0 for k in cases)
    assert {k["src"] for k in cases} >= {(2, 2)} and {k["n"] for k in cases} >= {1, 3}
    for std in NC.COEFFS:
        assert sum(k["standard"] == std for k in cases) >= 2, std
    rot = NC.invert_affine(NC.CASES["rotation"]["fwd"])
    assert abs(rot[1]) > 0.1 and abs(rot[3]) > 0.1
    for name, (s, rgb, _) in surfaces.items():
        y, uv = s.planes()
        assert y.min() == 0 and y.max() == 255, name
        raw = NC.unclipped_rgb(y, uv, s.standard)
        for ch in range(3):
            assert raw[..., ch].min() < 0 and raw[..., ch].max() > 255, (name, "RGB"[ch])
        # the padding is random and not zero
        if s.y_pitch > s.ws:
            pad = np.lib.stride_tricks.as_strided(s.ybuf[s.y_off + s.ws:], (s.n, s.hs, s.y_pitch - s.ws),
                                                  (s.y_frame, s.y_pitch, 1))
            assert pad.min() > 0 and len(np.unique(pad)) > 8, name


def test_reference_sees_the_faults(surfaces):
    """Mutation check of the reference, pure numpy: each fault a kernel could have changes the expected output on at
    least one case, so the cases can see it."""
    def ref_of(s, rgb):
        c = s.case
        return NC.bits(NC.reference_f32(rgb, NC.invert_affine(c["fwd"]), c["dst"][0], c["dst"][1], False))

    faults = {
        "chroma from (xi, yi) instead of (xi >> 1, yi >> 1)": lambda s: NC.nv12_to_rgb(*s.planes(), s.standard, chroma_at_luma=True),
        "U and V swapped": lambda s: NC.nv12_to_rgb(*s.planes(), s.standard, swap_uv=True),
        "max(0, .) dropped": lambda s: NC.nv12_to_rgb(*s.planes(), s.standard, no_floor=True),
        "the width used as the pitch": lambda s: NC.nv12_to_rgb(*s.planes(y_pitch=s.ws, uv_pitch=s.ws), s.standard),
    }
    for what, make in faults.items():
        seen = [name for name, (s, rgb, ref) in surfaces.items() if not np.array_equal(ref_of(s, make(s)), NC.bits(ref))]
        print(f"{what}: seen by {seen}")
        assert seen, what


def test_argument_errors(emu_lib):
    y = np.full((1, 4, 8), 90, np.uint8)
    uvbuf = np.full(2 * 8 + 2, 128, np.uint8)
    o16 = np.zeros((1, 4, 2, 8), np.uint16)
    o32 = np.zeros((1, 3, 4, 4), np.float32)
    inv = NC.invert_affine(NC.IDENTITY)
    yp, up, p16, p32 = y.ctypes.data, uvbuf.ctypes.data, o16.ctypes.data, o32.ctypes.data
    assert up % 2 == 0

    def go(y_=yp, uv_=up, n=1, hs=4, ws=4, ypitch=8, uvpitch=8, yfs=32, uvfs=16, std=0, inv_=inv, H=4, W=4, a16=p16, a32=p32,
           mean=NC.MEAN32, sd=NC.STD32):
        return NC.call(emu_lib, y_, uv_, n, hs, ws, ypitch, uvpitch, yfs, uvfs, std, inv_, H, W, a16, a32, mean=mean, std=sd)

    assert go() == 0
    assert go(y_=None) == EINVAL and go(uv_=None) == EINVAL               # null planes
    assert go(a16=None, a32=None) == EINVAL                                # no output
    assert go(a32=None) == 0 and go(a16=None) == 0
    assert go(hs=3) == EINVAL and go(ws=3) == EINVAL                       # odd source
    assert go(W=3) == EINVAL                                               # odd W
    assert go(hs=0) == EINVAL and go(ws=0) == EINVAL and go(n=-1) == EINVAL and go(H=0) == EINVAL
    assert go(ypitch=3) == EINVAL and go(uvpitch=2) == EINVAL              # pitch < Ws
    assert go(ypitch=5) == 0                                               # an odd luma pitch is fine
    assert go(uvpitch=5) == EINVAL                                         # odd chroma pitch
    assert go(uv_=up + 1) == EINVAL                                        # odd chroma address
    assert go(uvfs=17) == EINVAL                                           # odd chroma frame stride
    assert go(yfs=33) == 0
    assert go(std=4) == EINVAL and go(std=-1) == EINVAL                    # unknown standard
    for bad in (np.nan, np.inf):
        broken = inv.copy()
        broken[2] = bad
        assert go(inv_=broken) == EINVAL
        assert go(mean=(bad, 0, 0)) == EINVAL and go(sd=(1, bad, 1)) == EINVAL
    assert go(sd=(1, 1, 0)) == EINVAL                                      # stdv == 0
    assert go(ws=1 << 24, ypitch=1 << 24, uvpitch=1 << 24) == 10002        # FVP_ELIMIT as fvp_ingest_frames
    before = o16.copy()
    o16[...] = 7
    assert go(n=0) == 0 and (o16 == 7).all()                               # N == 0: no launch
    del before


def test_python_surface(emu_lib, surfaces):
    """dataset.images.Nv12Frames / ingest_nv12 / from_buffer without a GPU: strides become pitch and frame stride (checked
    by running the emulated library through the wrapper), and wrong inputs are refused."""
    from faster_voxelpose_amd import dataset as DS
    from faster_voxelpose_amd.dataset import images as IMG
    assert DS.Nv12Frames is IMG.Nv12Frames and DS.ingest_nv12 is IMG.ingest_nv12
    for name in ("letterbox", "letterbox_pitched", "rotation"):
        s, rgb, ref = surfaces[name]
        fr = s.torch_frames()
        assert (fr.N, fr.Hs, fr.Ws, fr.y_pitch, fr.uv_pitch, fr.standard) == (s.n, s.hs, s.ws, s.y_pitch, s.uv_pitch, s.standard)
        if s.n > 1:
            assert (fr.y_frame_stride, fr.uv_frame_stride) == (s.y_frame, s.uv_frame)
        out = IMG.ingest_nv12(fr, s.case["fwd"], s.case["dst"], _lib=emu_lib)
        assert out.shape == ref.shape and np.array_equal(NC.bits(out.numpy()), NC.bits(ref))
        with pytest.raises(capi.FvpError):
            IMG.ingest_nv12(fr, s.case["fwd"], s.case["dst"])                           # CPU tensors: no fallback
    # leading dimensions [B, V] flatten to one frame stride; the result carries them
    s, rgb, ref = surfaces["letterbox"]
    fr = s.torch_frames(lead=(1, 3))
    assert fr.lead == (1, 3) and fr.N == 3 and fr.y_frame_stride == s.y_frame
    out = IMG.ingest_nv12(fr, s.case["fwd"], s.case["dst"], _lib=emu_lib)
    assert out.shape == (1, 3) + ref.shape[1:] and np.array_equal(NC.bits(out.numpy().reshape(ref.shape)), NC.bits(ref))

    # from_buffer: the decoder's layout; the views alias the buffer
    hs, ws, pitch = 6, 8, 16
    buf = torch.randint(1, 256, (2, 3, hs * 3 // 2, pitch), dtype=torch.uint8)
    fb = IMG.Nv12Frames.from_buffer(buf, hs, ws)
    assert fb.lead == (2, 3) and (fb.y_pitch, fb.uv_pitch) == (pitch, pitch)
    assert fb.y_frame_stride == fb.uv_frame_stride == hs * 3 // 2 * pitch
    assert fb.y.shape == (2, 3, hs, ws) and fb.uv.shape == (2, 3, hs // 2, ws // 2, 2)
    assert fb.y.data_ptr() == buf.data_ptr() and fb.uv.data_ptr() == buf.data_ptr() + hs * pitch
    buf[1, 2, 1, 3] = 201
    buf[1, 2, hs + 1, 5] = 77                                                           # chroma row 1, pair 2, V
    assert fb.y[1, 2, 1, 3] == 201 and fb.uv[1, 2, 1, 2, 1] == 77
    flat = IMG.Nv12Frames.from_buffer(buf.reshape(2, 3, -1), hs, ws, pitch=pitch)
    assert flat.y.data_ptr() == buf.data_ptr() and flat.y_pitch == pitch and flat.lead == (2, 3)
    want = NC.reference_f32(NC.nv12_to_rgb(fb.y.reshape(6, hs, ws).numpy(), fb.uv.reshape(6, hs // 2, ws // 2, 2).numpy(), 3),
                            NC.invert_affine(NC.IDENTITY), ws, hs, False)
    got = IMG.ingest_nv12(IMG.Nv12Frames.from_buffer(buf, hs, ws, standard="bt709", full_range=True), NC.IDENTITY, (ws, hs),
                          _lib=emu_lib)
    assert np.array_equal(NC.bits(got.numpy().reshape(want.shape)), NC.bits(want))
    with pytest.raises(capi.FvpError):
        IMG.Nv12Frames.from_buffer(buf, hs + 2, ws)                                     # not Hs * 3 / 2 rows
    with pytest.raises(capi.FvpError):
        IMG.Nv12Frames.from_buffer(buf, hs, 2 * pitch)                                  # rows shorter than the width

    y = torch.zeros(2, 3, 4, 8, dtype=torch.uint8)
    uv = torch.zeros(2, 3, 2, 4, 2, dtype=torch.uint8)
    IMG.Nv12Frames(y, uv)
    with pytest.raises(capi.FvpError):
        IMG.Nv12Frames(y, uv[:1])                                                       # mismatched leading dimensions
    with pytest.raises(capi.FvpError):
        IMG.Nv12Frames(y[:, :2], uv)
    with pytest.raises(capi.FvpError):
        IMG.Nv12Frames(torch.zeros(2, 3, 4, 16, dtype=torch.uint8)[..., ::2], uv)       # luma row not dense
    with pytest.raises(capi.FvpError):
        IMG.Nv12Frames(y, torch.zeros(2, 3, 2, 8, 2, dtype=torch.uint8)[..., ::2, :])   # chroma pairs not dense
    with pytest.raises(capi.FvpError):
        IMG.Nv12Frames(y, torch.zeros(2, 3, 2, 4, 4, dtype=torch.uint8)[..., ::2])      # U, V not adjacent
    with pytest.raises(capi.FvpError):
        IMG.Nv12Frames(y.transpose(0, 1), uv.transpose(0, 1))                           # no constant frame stride
    with pytest.raises(capi.FvpError):
        IMG.Nv12Frames(y.float(), uv)
    with pytest.raises(capi.FvpError):
        IMG.Nv12Frames(y[..., :3, :], uv)                                               # odd height
    with pytest.raises(capi.FvpError):
        IMG.Nv12Frames(y, uv, standard="bt2020")
    assert IMG.Nv12Frames(y, uv, "bt709", True).standard == capi.YUV_BT709_FULL
    # a [B,V] slice of a larger batch keeps one frame stride; an expanded (stride 0) batch does too
    big = torch.zeros(4, 3, 6, 16, dtype=torch.uint8)
    part = IMG.Nv12Frames.from_buffer(big[1:3], 4, 8)
    assert part.N == 6 and part.y_frame_stride == 6 * 16


def test_swap_rb_is_refused_with_nv12():
    """PoseResNet._run / forward_frames: swap_rb given together with NV12 frames is an error (checked before any GPU work)."""
    from faster_voxelpose_amd.dataset.images import Nv12Frames
    from faster_voxelpose_amd.models.resnet import PoseResNet
    fr = Nv12Frames(torch.zeros(1, 4, 8, dtype=torch.uint8), torch.zeros(1, 2, 4, 2, dtype=torch.uint8))
    bb = PoseResNet.__new__(PoseResNet)                      # the check needs no parameters and no library
    bb.__dict__["image_size"] = (32, 32)
    for swap in (True, False):
        with pytest.raises(capi.FvpError, match="swap_rb"):
            bb.forward_frames(fr, NC.IDENTITY, swap_rb=swap)
    with pytest.raises(capi.FvpError, match="resize_transform"):
        bb._run(fr, False, True)
