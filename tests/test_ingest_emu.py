"""fvp_ingest_frames (camera frames -> backbone input) on the CPU emulator: the unmodified kernel source of
csrc/fvp_heatmap.hip compiled for the host (tests/hipemu), so the arithmetic, the border handling and the argument
checks are tested without a GPU.  tests/test_ingest_gpu.py repeats the value checks on the
shipped library."""
import ctypes as C

import numpy as np
import pytest
import torch

import ingest_cases as IC
from faster_voxelpose_amd import _capi as capi


def _case(name):
    (ws, hs), (W, H), fwd, n, swap = IC.CASES[name]
    return IC.make_frames(name), fwd, W, H, swap


@pytest.mark.parametrize("general", [False, True], ids=["default", "general"])
@pytest.mark.parametrize("name", list(IC.CASES))
def test_bit_equal_to_the_float32_restatement(emu_lib, name, general):
    """Both outputs, every pixel (the outputs start poisoned), against the arithmetic of include/fvp.h restated op by op
    in numpy float32; with and without FVP_INGEST_GENERAL (a no-op since the staged form was dropped)."""
    frames, fwd, W, H, swap = _case(name)
    assert frames.min() == 0 and frames.max() == 255
    ref = IC.reference_f32(frames, IC.invert_affine(fwd), W, H, swap)
    o16, o32 = IC.run(emu_lib, frames, fwd, W, H, swap, general)
    assert np.array_equal(IC.bits(o32), IC.bits(ref)), f"{int((IC.bits(o32) != IC.bits(ref)).sum())} fp32 values differ"
    assert np.array_equal(o16, IC.pack_nhwc8(ref))
    # one output at a time gives the same values
    only16, none32 = IC.run(emu_lib, frames, fwd, W, H, swap, general, want_nchw=False)
    assert none32 is None and np.array_equal(only16, o16)
    none16, only32 = IC.run(emu_lib, frames, fwd, W, H, swap, general, want_bf16=False)
    assert none16 is None and np.array_equal(IC.bits(only32), IC.bits(o32))


def test_cases_cover_the_border_and_unaligned_rows():
    """The case list does what its comments say: border taps occur, a source row length that is no multiple of 4 bytes,
    sources of 1 and 2 pixels, N of 1 and 3, both swap settings."""
    (ws, hs), (W, H), fwd, _, _ = IC.CASES["panoptic_small"]
    inv = IC.invert_affine(fwd)
    sx = inv[0] * np.arange(W) + inv[2]
    assert sx.min() < 0 and sx.max() > ws - 1                       # letter-box: taps left and right of the frame
    assert any((3 * c[0][0]) % 4 for c in IC.CASES.values())
    assert {c[0] for c in IC.CASES.values()} >= {(1, 1), (2, 2)}
    assert {c[3] for c in IC.CASES.values()} == {1, 3} and {c[4] for c in IC.CASES.values()} == {True, False}
    rot = IC.invert_affine(IC.CASES["rotation"][2])
    assert abs(rot[1]) > 0.1 and abs(rot[3]) > 0.1


STAGED_FORM_DROPPED = ("the LDS-staged form was dropped on the measurement the issue asked for: 257 us against 192 us of "
                       "the general form for 40 frames 1080p -> 512x960, 159 against 167 us at 512x960 -> 512x960 "
                       "(profiles/ingest_kernel.txt); one form ships and FVP_INGEST_GENERAL is a no-op")


@pytest.mark.parametrize("name", IC.AXIS_ALIGNED)
def test_forms_agree(emu_lib, name):
    """Default dispatch == FVP_INGEST_GENERAL, bit for bit, both outputs - for a staged form, should one return."""
    pytest.skip(STAGED_FORM_DROPPED)
    frames, fwd, W, H, swap = _case(name)
    a16, a32 = IC.run(emu_lib, frames, fwd, W, H, swap, False)
    b16, b32 = IC.run(emu_lib, frames, fwd, W, H, swap, True)
    assert np.array_equal(a16, b16) and np.array_equal(IC.bits(a32), IC.bits(b32))


@pytest.mark.parametrize("general", [False, True], ids=["default", "general"])
@pytest.mark.parametrize("name", ["identity", "identity_noswap"])
def test_identity_equals_the_loader_path(emu_lib, name, general):
    """Identity transform, same size: nchw == ToTensor + Normalize computed by torch in fp32, and nhwc8 == what
    fvp_bb_input writes for that tensor - the path float views take today - bit for bit."""
    frames, fwd, W, H, swap = _case(name)
    rgb = frames[..., ::-1] if swap else frames
    t = IC.torch_loader_f32(rgb)
    o16, o32 = IC.run(emu_lib, frames, fwd, W, H, swap, general)
    assert np.array_equal(IC.bits(o32), IC.bits(t.numpy()))
    n = frames.shape[0]
    today = np.full((n, H, W // 2, 8), 0xDEAD, np.uint16)
    assert emu_lib.fvp_bb_input(t.data_ptr(), today.ctypes.data, n, 3, H, W, None) == 0
    assert np.array_equal(o16, today)


@pytest.mark.parametrize("name", list(IC.CASES))
def test_against_exact_bilinear_in_float64(emu_lib, name):
    """Independent of the fp32 restatement: coordinates from the float64 inverse of the forward matrix, float64 blend.
    Bound, derived (ingest_cases.f64_bound computes it from Hs, Ws, the matrix and std; u = 2^-24):
      * a source coordinate is a*x + b*y + c with three coefficients rounded to fp32 and four rounded operations, each
        an error of at most u times the magnitude m of the terms (m = max(Hs, Ws, |a|(W-1) + |b|(H-1) + |c|)):
        |d coord| <= 8 u m;
      * zero-padded bilinear interpolation is continuous and changes by at most the largest neighbour difference, 255,
        per unit of either coordinate: |d v| <= 255 * 2 * 8 u m - this also covers a pixel whose fp32 and float64
        floor() differ, which sits within |d coord| of an integer; fx = sx - floor(sx) is exact;
      * the blend itself (1-fx, 1-fy, six products, three sums on values <= 255): <= 10 u * 255;
      * / 255, - mean, / std: |d v| / (255 min std) plus three roundings at magnitude <= (1 + max mean) / min std.
    Every pixel counts; the measured maximum is printed."""
    frames, fwd, W, H, swap = _case(name)
    hs, ws = frames.shape[1:3]
    _, o32 = IC.run(emu_lib, frames, fwd, W, H, swap, False, want_bf16=False)
    ref = IC.reference_f64(frames, fwd, W, H, swap)
    err = float(np.abs(o32.astype(np.float64) - ref).max())
    bound = IC.f64_bound(fwd, hs, ws, W, H)
    print(f"{name}: max |fp32 - exact| = {err:.3e}, bound {bound:.3e}")
    assert np.isfinite(o32).all() and err <= bound


def test_argument_errors(emu_lib):
    frames = np.zeros((1, 4, 4, 3), np.uint8)
    o16 = np.zeros((1, 4, 2, 8), np.uint16)
    o32 = np.zeros((1, 3, 4, 4), np.float32)
    inv = IC.invert_affine(IC.IDENTITY)
    ok = IC.call(emu_lib, frames.ctypes.data, 1, 4, 4, inv, 4, 4, 0, o16.ctypes.data, o32.ctypes.data)
    assert ok == 0
    einval = 10001
    assert IC.call(emu_lib, None, 1, 4, 4, inv, 4, 4, 0, o16.ctypes.data, o32.ctypes.data) == einval      # null frames
    assert IC.call(emu_lib, frames.ctypes.data, 1, 4, 4, inv, 4, 4, 0, None, None) == einval              # no output
    assert IC.call(emu_lib, frames.ctypes.data, 1, 4, 4, inv, 4, 3, 0, o16.ctypes.data, None) == einval   # odd W
    assert IC.call(emu_lib, frames.ctypes.data, 1, 0, 4, inv, 4, 4, 0, o16.ctypes.data, None) == einval   # empty source
    assert IC.call(emu_lib, frames.ctypes.data, -1, 4, 4, inv, 4, 4, 0, o16.ctypes.data, None) == einval
    assert IC.call(emu_lib, frames.ctypes.data, 1, 4, 4, inv, 4, 4, 4, o16.ctypes.data, None) == einval   # unknown flag
    before = o16.copy()
    assert IC.call(emu_lib, frames.ctypes.data, 0, 4, 4, inv, 4, 4, 0, o16.ctypes.data, None) == 0        # N == 0: no launch
    assert np.array_equal(o16, before)


def test_python_surface_checks_its_inputs():
    """dataset.images without a GPU: the inverse is float64 -> fp32 once; wrong dtypes / layouts are refused."""
    from faster_voxelpose_amd.dataset import images as IMG
    from faster_voxelpose_amd.utils.transforms import get_resize_transform
    rt = get_resize_transform((1920, 1080), (960, 512))
    inv = IMG.invert_affine(rt)
    assert inv.dtype == np.float32 and inv.shape == (6,)
    full = np.vstack([rt, [0, 0, 1]])
    assert np.array_equal(inv, np.linalg.inv(full)[:2].reshape(6).astype(np.float32)) or \
        np.allclose(inv, np.linalg.inv(full)[:2].reshape(6), rtol=1e-7, atol=1e-12)
    assert np.array_equal(IMG.invert_affine(torch.as_tensor(rt)), inv)
    with pytest.raises(capi.FvpError):
        IMG.invert_affine(np.zeros((2, 3)))
    with pytest.raises(capi.FvpError):
        IMG.ingest_frames(torch.zeros(1, 4, 4, 3, dtype=torch.uint8), rt, (4, 4))       # CPU tensor: no fallback
    assert C.sizeof(C.c_float) == 4 and capi.INGEST_SWAP_RB == 1 and capi.INGEST_GENERAL == 2
