"""fvp_demosaic_bayer and fvp_ingest_bayer (8-bit Bayer mosaic -> RGB frame / backbone input, include/fvp.h ABI 24) on the
CPU emulator: the unmodified kernel source of csrc/fvp_heatmap.hip compiled for the host (tests/hipemu).  Everything is
compared bit for bit: the demosaic with the numpy int64 restatement of the header (tests/bayer_cases.py), the ingest
with that restatement followed by the float32 restatement of fvp_ingest_frames, and with fvp_ingest_frames of the same
library on the demosaiced frame (the defining property).  tests/test_bayer_gpu.py repeats the value checks on the
shipped library."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import bayer_cases as BC
import ingest_cases as IC
from faster_voxelpose_amd import _capi as capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ELIMIT = 10001, 10002


@pytest.fixture(scope="module")
def mosaics():
    """Every case's mosaic, its demosaiced frame and its float32 reference, computed once and never written to."""
    out = {}
    for name, c in BC.CASES.items():
        m = BC.Mosaic(name)
        W, H = c["dst"]
        rgb = m.rgb()
        out[name] = (m, rgb, BC.reference_f32(rgb, BC.invert_affine(c["fwd"]), W, H, False))
    return out


def _launch_log(lib_path=os.path.join(ROOT, "tests", "hipemu", "libfvp_emu.so")):
    so = ctypes.CDLL(lib_path)
    so.hipemu_launch_log.restype = ctypes.c_char_p
    return so


@pytest.mark.parametrize("name", list(BC.CASES))
def test_demosaic_equals_the_restatement(emu_lib, mosaics, name):
    m, rgb, _ = mosaics[name]
    got, guards = BC.run_demosaic(emu_lib, m)
    assert guards, "bytes outside the RGB output were written"
    bad = int((got != rgb).sum())
    assert bad == 0, f"{bad} of {rgb.size} bytes differ"


@pytest.mark.parametrize("size", BC.DEMOSAIC_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("pitch_extra, tone", [(0, False), (5, True)])
def test_demosaic_around_the_tile(emu_lib, size, pitch_extra, tone):
    """The workgroup's 256 x 8 pixels, two more and two fewer in each direction, and 6 x 4; dense rows (dword reads) and
    an odd pitch (rows that start on any byte)."""
    for pattern in (BC.RGGB, BC.BGGR) if pitch_extra else (BC.GRBG, BC.GBRG):
        m = BC.sized(*size, pattern=pattern, pitch=size[0] + pitch_extra, gap=3 * bool(pitch_extra), tone=tone)
        got, guards = BC.run_demosaic(emu_lib, m)
        assert guards and np.array_equal(got, m.rgb())


@pytest.mark.parametrize("name", list(BC.CASES))
def test_ingest_bit_equal_to_the_restatement(emu_lib, mosaics, name):
    """Both outputs, every pixel (they start poisoned); then each output requested alone."""
    m, rgb, ref = mosaics[name]
    o16, o32 = BC.run_ingest(emu_lib, m)
    bad = int((BC.bits(o32) != BC.bits(ref)).sum())
    assert bad == 0, f"{bad} of {ref.size} fp32 values differ"
    assert np.array_equal(o16, BC.pack_nhwc8(ref))
    only16, none32 = BC.run_ingest(emu_lib, m, want_nchw=False)
    assert none32 is None and np.array_equal(only16, o16)
    none16, only32 = BC.run_ingest(emu_lib, m, want_bf16=False)
    assert none16 is None and np.array_equal(BC.bits(only32), BC.bits(o32))


@pytest.mark.parametrize("name", list(BC.CASES))
def test_ingest_equals_ingest_frames_on_the_demosaiced_frame(emu_lib, mosaics, name):
    """The defining property, within one library: == fvp_ingest_frames(flags = 0) on fvp_demosaic_bayer's output."""
    m, _, _ = mosaics[name]
    c = m.case
    W, H = c["dst"]
    frame, _ = BC.run_demosaic(emu_lib, m)
    r16, r32 = IC.run(emu_lib, frame, c["fwd"], W, H, False, False)
    o16, o32 = BC.run_ingest(emu_lib, m)
    assert np.array_equal(o16, r16) and np.array_equal(BC.bits(o32), BC.bits(r32))


def test_dispatch_rule_and_which_kernel_ran(emu_lib, mosaics):
    """Cases sit on both sides of the dispatch rule; the rule restated in bayer_cases.lds_plan names the kernel that the
    launch log shows, for every case."""
    so = _launch_log()
    forms = set()
    for name, (m, _, _) in mosaics.items():
        c = m.case
        W, H = c["dst"]
        fits, rw, rh = BC.lds_plan(BC.invert_affine(c["fwd"]), H, W, m.hs, m.ws)
        assert fits == (c["form"] == "lds"), (name, rw, rh)
        so.hipemu_launch_log_reset()
        BC.run_ingest(emu_lib, m)
        log = so.hipemu_launch_log().decode()
        ran = "lds" if "k_ingest_bayer_lds" in log else "gather" if "k_ingest_bayer_gather" in log else log
        assert ran == c["form"], (name, log)
        forms.add(ran)
    assert forms == {"lds", "gather"}


def test_header_enum_and_constants():
    text = open(os.path.join(ROOT, "include", "fvp.h")).read()
    enum = {m.group(1): int(m.group(2)) for m in re.finditer(r"FVP_BAYER_([RGB]{4}) = (\d)", text)}
    assert enum == {"RGGB": 0, "GRBG": 1, "GBRG": 2, "BGGR": 3}
    assert (capi.BAYER_RGGB, capi.BAYER_GRBG, capi.BAYER_GBRG, capi.BAYER_BGGR) == (0, 1, 2, 3)
    assert re.search(r"#define FVP_ABI_VERSION 24\b", text) and capi.ABI_VERSION == 24
    # the pattern's name spells its cell: the letter at (rx, ry) is R
    for name, value in enum.items():
        rx, ry = BC.RED_AT[value]
        assert name[2 * ry + rx] == "R" and name[2 * (1 - ry) + (1 - rx)] == "B"


def test_version(emu_lib):
    assert emu_lib.fvp_version() == 24


# ---- asserted on the restatement, not on the kernel: the cases can tell right from wrong --------------------------------
def test_flat_frame_stays_flat():
    for pattern in BC.RED_AT:
        for v in (0, 1, 77, 255):
            assert (BC.demosaic(np.full((1, 8, 10), v, np.uint8), pattern) == v).all()


def test_grey_ramp_is_reproduced_inside_the_border():
    """The filter is exact on linear images: a grey ramp comes back exactly two pixels inside the border."""
    y, x = np.mgrid[0:14, 0:18]
    ramp = (20 + 3 * x + 5 * y).astype(np.uint8)[None]
    assert ramp.max() < 255
    for pattern in BC.RED_AT:
        rgb = BC.demosaic(ramp, pattern)
        assert (rgb[0, 2:-2, 2:-2] == ramp[0, 2:-2, 2:-2, None]).all()


@pytest.mark.parametrize("hs, ws", [(4, 4), (6, 10), (12, 8)])
def test_one_colour_lit_gives_that_colour_everywhere(hs, ws):
    """Only the red sites lit: pure red at every pixel, all borders included (the reflection keeps the parity), in all four
    patterns; the same for blue."""
    y, x = np.mgrid[0:hs, 0:ws]
    for pattern, (rx, ry) in BC.RED_AT.items():
        for ch, (cx, cy) in ((0, (rx, ry)), (2, (1 - rx, 1 - ry))):
            raw = np.where(((x & 1) == cx) & ((y & 1) == cy), 200, 0).astype(np.uint8)[None]
            rgb = BC.demosaic(raw, pattern)
            assert (rgb[..., ch] == 200).all(), (pattern, ch)
            assert (rgb[..., 1] == 0).all() and (rgb[..., 2 - ch] == 0).all(), (pattern, ch)


def test_cases_cover_what_their_comments_say(mosaics):
    for name, (m, rgb, _) in mosaics.items():
        raw = m.frames()
        if m.pitch > m.ws:                                         # the padding is random and never 0
            pad = np.lib.stride_tricks.as_strided(m.buf[m.ws:], (m.n, m.hs, m.pitch - m.ws), (m.frame, m.pitch, 1))
            assert pad.min() > 0 and len(np.unique(pad)) > 2, name
        x16 = BC.sixteenths(raw, m.pattern)
        v = (x16 + 8) >> 4
        for ch in range(3):                                        # clips at both ends in every channel
            assert v[..., ch].min() < 0 and v[..., ch].max() > 255, (name, "RGB"[ch])
    cases = BC.CASES.values()
    assert {c["pattern"] for c in cases if c["src"] == (96, 54)} == set(BC.RED_AT)
    assert {c["pattern"] for c in cases if c["src"] == (4, 4)} == set(BC.RED_AT)
    assert any(c["pitch"] % 2 and c["gap"] and c["tone"] for c in cases)
    assert any(c["pitch"] == c["src"][0] and not c["gap"] for c in cases)
    assert {c["form"] for c in cases} == {"lds", "gather"}
    assert BC.CASES["wide_shifted"]["dst"][0] > 4 * BC.INGEST_TILE[0]      # several destination tiles in a row
    assert BC.CASES["upscale"]["dst"][1] > BC.INGEST_TILE[1]               # and more than one tile row
    tone = BC.tone_formula(**BC.TONE_ARGS)
    assert not np.array_equal(tone, np.tile(np.arange(256, dtype=np.uint8), (3, 1))) and len({bytes(t) for t in tone}) == 3


def test_reference_sees_the_faults(mosaics):
    """Four deliberate faults each change the expected output of EVERY case."""
    def ref_of(m, rgb):
        c = m.case
        return BC.bits(BC.reference_f32(rgb, BC.invert_affine(c["fwd"]), c["dst"][0], c["dst"][1], False))

    faults = {
        "the pattern shifted by one column": dict(shift_pattern=True),
        "a clamped border instead of a reflected one": dict(clamp_border=True),
        "the + 8 dropped": dict(no_round=True),
        "H2 and V2 exchanged in the two green-site formulas": dict(swap_h2v2=True),
    }
    for what, kw in faults.items():
        for name, (m, rgb, ref) in mosaics.items():
            wrong = m.rgb(**kw)
            assert not np.array_equal(wrong, rgb), (what, name, "demosaic")
            assert not np.array_equal(ref_of(m, wrong), BC.bits(ref)), (what, name, "ingest")


# ---- arguments ------------------------------------------------------------------------------------------------------------
def test_argument_errors(emu_lib):
    raw = np.full(2 * 8 * 16 + 8, 90, np.uint8)
    tone = np.tile(np.arange(256, dtype=np.uint8), (3, 1)).copy()
    rgb = np.full((2, 8, 8, 3), 7, np.uint8)
    o16 = np.full((2, 4, 2, 8), 7, np.uint16)
    o32 = np.full((2, 3, 4, 4), 7, np.float32)
    inv = BC.invert_affine(BC.IDENTITY)
    rp, tp, gp, p16, p32 = (a.ctypes.data for a in (raw, tone, rgb, o16, o32))

    def dem(raw_=rp, n=2, hs=8, ws=8, pitch=16, frame=128, pattern=0, tone_=tp, flags=0, rgb_=gp):
        return BC.call_demosaic(emu_lib, raw_, n, hs, ws, pitch, frame, pattern, tone_, flags, rgb_)

    def ing(raw_=rp, n=2, hs=8, ws=8, pitch=16, frame=128, pattern=0, tone_=tp, inv_=inv, H=4, W=4, a16=p16, a32=p32,
            mean=BC.MEAN32, sd=BC.STD32):
        return BC.call_ingest(emu_lib, raw_, n, hs, ws, pitch, frame, pattern, tone_, inv_, H, W, a16, a32, mean=mean, std=sd)

    def untouched():
        return (rgb == 7).all() and (o16 == 7).all() and (o32 == 7).all()

    # every refusal first, so that "nothing is written when an error is returned" covers them all
    for f in (dem, ing):
        assert f(raw_=None) == EINVAL
        assert f(n=-1) == EINVAL
        assert f(hs=7) == EINVAL and f(ws=7) == EINVAL                     # odd
        assert f(hs=2) == EINVAL and f(ws=2) == EINVAL                     # < 4
        assert f(hs=0) == EINVAL and f(ws=-4) == EINVAL
        assert f(pitch=7) == EINVAL                                        # pitch < Ws
        assert f(pattern=4) == EINVAL and f(pattern=-1) == EINVAL
    assert dem(rgb_=None) == EINVAL
    assert dem(flags=1) == EINVAL and dem(flags=-1) == EINVAL
    assert dem(hs=16386, frame=16386 * 16) == ELIMIT and dem(ws=16386, pitch=16386) == ELIMIT   # one step past 16384
    assert ing(a16=None, a32=None) == EINVAL
    assert ing(W=3) == EINVAL and ing(W=0) == EINVAL and ing(H=0) == EINVAL
    for bad in (np.nan, np.inf):
        broken = inv.copy()
        broken[2] = bad
        assert ing(inv_=broken) == EINVAL
        assert ing(mean=(bad, 0, 0)) == EINVAL and ing(sd=(1, bad, 1)) == EINVAL
    assert ing(sd=(1, 1, 0)) == EINVAL
    assert ing(ws=1 << 24, pitch=1 << 24) == ELIMIT                        # the limits of fvp_ingest_frames
    assert ing(W=1 << 24) == ELIMIT
    assert untouched()
    assert dem(n=0) == 0 and ing(n=0) == 0 and untouched()                 # N == 0: no launch
    # and the accepted edges
    assert dem(hs=4, ws=4) == 0 and dem(pitch=9, frame=81) == 0 and dem(tone_=None) == 0
    assert ing(a32=None) == 0 and ing(a16=None) == 0 and ing(pitch=9, frame=81, tone_=None) == 0
    assert not untouched()


def test_null_host_arrays_are_refused(emu_lib):
    """inv, mean and stdv are host pointers: a null one is FVP_EINVAL (passed as raw pointers, past the list helper)."""
    raw = np.full(8 * 8, 90, np.uint8)
    o32 = np.full((1, 3, 4, 4), 7, np.float32)
    three = (ctypes.c_float * 3)(1, 1, 1)
    six = (ctypes.c_float * 6)(1, 0, 0, 0, 1, 0)
    for a in range(3):
        args = [six, three, three]
        args[a] = None
        assert emu_lib.fvp_ingest_bayer(raw.ctypes.data, 1, 8, 8, 8, 64, 0, None, *args, 4, 4, None, o32.ctypes.data,
                                        None) == EINVAL
    assert (o32 == 7).all()


# ---- the Python surface -----------------------------------------------------------------------------------------------------
def test_tone_table():
    from faster_voxelpose_amd.dataset.images import BayerFrames
    ident = BayerFrames.tone_table()
    assert ident.dtype == torch.uint8 and tuple(ident.shape) == (3, 256)
    assert np.array_equal(ident.numpy(), np.tile(np.arange(256, dtype=np.uint8), (3, 1)))
    for kw in (BC.TONE_ARGS, dict(gains=(0.5, 2.5, 1.0), gamma=0.45, black=0), dict(gains=(1, 1, 1), gamma=1.0, black=64)):
        assert np.array_equal(BayerFrames.tone_table(**kw).numpy(), BC.tone_formula(**kw)), kw
    with pytest.raises(capi.FvpError):
        BayerFrames.tone_table(gamma=0.0)
    with pytest.raises(capi.FvpError):
        BayerFrames.tone_table(black=255)


def test_python_surface(emu_lib, mosaics):
    """dataset.images.BayerFrames / ingest_bayer / demosaic_bayer / to_rgb without a GPU: strides become pitch and frame
    stride (checked by running the emulated library through the wrappers), and wrong inputs are refused."""
    from faster_voxelpose_amd import dataset as DS
    from faster_voxelpose_amd.dataset import images as IMG
    assert DS.BayerFrames is IMG.BayerFrames and DS.ingest_bayer is IMG.ingest_bayer and DS.demosaic_bayer is IMG.demosaic_bayer
    for name in ("letterbox_grbg", "letterbox_pitched", "rotation"):
        m, rgb, ref = mosaics[name]
        fr = m.torch_frames()
        assert (fr.N, fr.Hs, fr.Ws, fr.pitch, fr.pattern) == (m.n, m.hs, m.ws, m.pitch, m.pattern)
        if m.n > 1:
            assert fr.frame_stride == m.frame
        out = IMG.ingest_bayer(fr, m.case["fwd"], m.case["dst"], _lib=emu_lib)
        assert out.shape == ref.shape and np.array_equal(BC.bits(out.numpy()), BC.bits(ref))
        assert np.array_equal(fr.to_rgb(_lib=emu_lib).numpy(), rgb)
        with pytest.raises(capi.FvpError):
            IMG.ingest_bayer(fr, m.case["fwd"], m.case["dst"])                          # CPU tensors: no fallback
        with pytest.raises(capi.FvpError):
            IMG.demosaic_bayer(fr)
    # leading dimensions [B, V] flatten to one frame stride; the results carry them; out= is written in place
    m, rgb, ref = mosaics["letterbox_pitched"]
    fr = m.torch_frames(lead=(1, 3))
    assert fr.lead == (1, 3) and fr.N == 3 and fr.frame_stride == m.frame
    out = IMG.ingest_bayer(fr, m.case["fwd"], m.case["dst"], _lib=emu_lib)
    assert out.shape == (1, 3) + ref.shape[1:] and np.array_equal(BC.bits(out.numpy().reshape(ref.shape)), BC.bits(ref))
    mine = torch.zeros(1, 3, m.hs, m.ws, 3, dtype=torch.uint8)
    got = IMG.demosaic_bayer(fr, out=mine, _lib=emu_lib)
    assert got.data_ptr() == mine.data_ptr() and np.array_equal(mine.numpy().reshape(rgb.shape), rgb)
    with pytest.raises(capi.FvpError):
        IMG.demosaic_bayer(fr, out=mine[..., :2], _lib=emu_lib)

    raw = torch.zeros(2, 3, 8, 12, dtype=torch.uint8)
    IMG.BayerFrames(raw)
    assert IMG.BayerFrames(raw, "BGGR").pattern == capi.BAYER_BGGR
    part = IMG.BayerFrames(torch.zeros(4, 3, 8, 16, dtype=torch.uint8)[1:3, :, :, :12])  # a slice keeps one frame stride
    assert part.N == 6 and part.pitch == 16 and part.frame_stride == 8 * 16
    for bad in (raw.float(), raw[..., :7, :], raw[..., :, :7], raw[..., :2, :], raw[..., ::2], raw.transpose(0, 1),
                raw[0, 0, 0]):
        with pytest.raises(capi.FvpError):
            IMG.BayerFrames(bad)
    with pytest.raises(capi.FvpError):
        IMG.BayerFrames(raw, "rgbg")
    with pytest.raises(capi.FvpError):
        IMG.BayerFrames(raw, tone=torch.zeros(3, 255, dtype=torch.uint8))
    with pytest.raises(capi.FvpError):
        IMG.BayerFrames(raw, tone=torch.zeros(3, 256))
    with pytest.raises(capi.FvpError):
        IMG.launch_bayer(emu_lib, raw, BC.IDENTITY, (12, 8), IMG.IMAGENET_MEAN, IMG.IMAGENET_STD, None, None)


def test_swap_rb_is_refused_with_bayer():
    """PoseResNet._run / forward_frames: swap_rb given together with Bayer frames is an error (checked before any GPU work)."""
    from faster_voxelpose_amd.dataset.images import BayerFrames
    from faster_voxelpose_amd.models.resnet import PoseResNet
    fr = BayerFrames(torch.zeros(1, 4, 8, dtype=torch.uint8))
    bb = PoseResNet.__new__(PoseResNet)                      # the check needs no parameters and no library
    bb.__dict__["image_size"] = (32, 32)
    for swap in (True, False):
        with pytest.raises(capi.FvpError, match="swap_rb"):
            bb.forward_frames(fr, BC.IDENTITY, swap_rb=swap)
    with pytest.raises(capi.FvpError, match="resize_transform"):
        bb._run(fr, False, True)


def test_model_refuses_frame_stages_without_bayer_rgb():
    """A stage that needs frames, Bayer views and model.bayer_rgb False: the new remedy, before any launch."""
    import fvp_synthetic as S
    from faster_voxelpose_amd.dataset.images import BayerFrames
    from faster_voxelpose_amd.models import faster_voxelpose as FV
    model = FV.FasterVoxelPoseNet(S.make_cfg("tiny", device="cpu"), _lib=object())
    assert model.bayer_rgb is False and model.last_frames is None
    model.evidence, model.overlay = True, object()
    fr = BayerFrames(torch.zeros(1, 2, 8, 8, dtype=torch.uint8))
    with pytest.raises(capi.FvpError, match=r"model\.overlay draws into the camera frames: set model\.bayer_rgb = True"):
        model(views=fr, meta=None, cameras=None, resize_transform=BC.IDENTITY)
    model.overlay, model.crops = None, object()
    with pytest.raises(capi.FvpError, match=r"model\.crops .*set model\.bayer_rgb = True"):
        model(views=fr, meta=None, cameras=None, resize_transform=BC.IDENTITY)
    model.crops = None
    with pytest.raises(capi.FvpError, match=r"leading dimensions \[B,V\]"):
        model(views=BayerFrames(torch.zeros(2, 8, 8, dtype=torch.uint8)), resize_transform=BC.IDENTITY)
    with pytest.raises(capi.FvpError, match="resize_transform"):
        model(views=fr)
