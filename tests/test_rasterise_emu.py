"""fvp_rasterise_heatmaps (2-D detections -> input heatmaps) on the CPU emulator: the unmodified k_rasterise of
csrc/fvp_heatmap.hip compiled for the host (tests/hipemu), against the float64 oracle, bit for bit - every band form (4, 2, 1 rows
per workgroup), the ragged last band, the three limits at and past their edge, the count clamping, every argument check and
non-finite joints (tests/rasterise_cases.py; tests/test_rasterise_gpu.py repeats the checks on the shipped library) - and the
Python wrapper dataset/heatmaps.py."""
import types

import numpy as np
import pytest

import rasterise_cases as RC
from faster_voxelpose_amd import _capi as capi

DEV = "cpu"


def test_fixture_conditions():
    """What the case list promises, asserted on the oracle's output and on the window arithmetic restated in float64 (never on
    the kernel): each case has windows clipped at each of the four image sides and windows entirely outside the image on each
    side, a joint whose quotient lies in (-1, 0) (truncation toward zero differs from floor), people on both human-scale clamps
    and between them, extents of exactly 48 and 192, a cell under two people's windows where the later person's value is the
    smaller (the element-wise max matters), and a non-zero value in every band.  The cases launch RB = 4, 2 and 1 and both
    ragged tails (3 rows of 4, 1 row of 2)."""
    rbs, tails = {}, set()
    for name in RC.CASES:
        J, W, H = RC.CASES[name][:3]
        rep, rb = RC.fixture_report(name)
        rbs[name] = rb
        print(f"{name}: J*W = {J * W}, RB = {rb}, bands = {(H + rb - 1) // rb}, last band of {H - (H - 1) // rb * rb} rows")
        if rep.pop("ragged_last_band"):
            tails.add((rb, H % rb))
        for cond, ok in rep.items():
            assert ok, f"{name}: the fixture does not contain the condition '{cond}'"
    assert set(rbs.values()) == {1, 2, 4}, rbs
    assert (rbs["rb4_ragged"], rbs["rb2_ragged"], rbs["rb1"], rbs["rb1_limit"]) == (4, 2, 1, 1)
    assert {(4, 3), (2, 1)} <= tails, tails
    # just above the switches of the host's rule
    assert RC.band_rows(1, 2816) == 4 and RC.band_rows(1, 2817) == 2 and RC.band_rows(1, 5632) == 2 and RC.band_rows(1, 5633) == 1
    assert 2816 < 19 * 150 <= 2816 + 150 and 5632 < 24 * 240 <= 5632 + 240
    assert RC.jp_of(19) == 20 and RC.jp_of(32) == 32
    # a window of `tall` spans more than 3 bands of 4 rows
    J, W, H, P, (sx, sy), sigma, _ = RC.CASES["tall"]
    joints, counts = RC.make_case("tall")
    assert any(min(br1, H) - max(ul1, 0) > 3 * 4 for *_, ul0, ul1, br0, br1, _ in RC.windows(joints[0], sx, sy, sigma)
               if ul0 < W and br0 >= 0)


@pytest.mark.parametrize("name", list(RC.CASES))
def test_bit_equal_to_the_float64_oracle(emu_lib, name):
    RC.check_case(emu_lib, DEV, name, exact=True)


@pytest.mark.parametrize("form", RC.OUTPUT_FORMS)
@pytest.mark.parametrize("name", ["rb4_ragged", "rb2_ragged"])
def test_output_forms(emu_lib, name, form):
    RC.check_output_forms(emu_lib, DEV, name, form)


def test_counts_are_clamped(emu_lib):
    RC.check_counts(emu_lib, DEV, exact=True)


def test_limits(emu_lib):
    RC.check_limits(emu_lib, DEV)


def test_arguments(emu_lib):
    RC.check_arguments(emu_lib, DEV)


def test_determinism_and_batching(emu_lib):
    RC.check_determinism_and_batching(emu_lib, DEV)


def test_non_finite_joints_stamp_nothing(emu_lib):
    """include/fvp.h: a joint with a non-finite coordinate stamps nothing and is left out of the person's extent; finite
    coordinates of any magnitude behave as the reference's Python integers do."""
    RC.check_nonfinite(emu_lib, DEV, exact=True)


# ---- dataset/heatmaps.py ---------------------------------------------------------------------------------------------------
J_, W_, H_ = 5, 40, 7


def _cfg():
    ns = types.SimpleNamespace
    return ns(DEVICE="cpu", DATASET=ns(NUM_JOINTS=J_, HEATMAP_SIZE=[W_, H_], IMAGE_SIZE=[4 * W_, 4 * H_]), NETWORK=ns(SIGMA=3))


RT = np.array([[0.5, 0.0, 3.0], [0.0, 0.5, -2.0]])          # original-image pixels -> network-image pixels


def _people(n, seed, cols=2):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        p = np.concatenate([rng.uniform(0, 8 * W_, (J_, 1)), rng.uniform(0, 8 * H_, (J_, 1)), rng.random((J_, 1))], axis=1)
        out.append(p[:, :cols])
    return out


def _wrapper(lib, preds, **kw):
    from faster_voxelpose_amd.dataset import generate_input_heatmaps
    return generate_input_heatmaps(preds, RT, _cfg(), device="cpu", _lib=lib, **kw)


def test_wrapper_frame_of_empty_views(emu_lib):
    hm = _wrapper(emu_lib, [[], [], []])
    assert tuple(hm.shape) == (3, J_, H_, W_) and not hm.numpy().view(np.uint32).any()
    hm, cl = _wrapper(emu_lib, [[[], []], [[], []]], channels_last=True)
    assert tuple(hm.shape) == (2, 2, J_, H_, W_) and tuple(cl.shape) == (2, 2, H_ * W_, 8)
    assert not hm.numpy().view(np.uint32).any() and not cl.numpy().view(np.uint32).any()


def test_wrapper_batched_input_with_an_empty_first_view(emu_lib):
    """[B][V][people]: the first frame's first view is empty, and so is a whole frame; still recognised as batched, and the
    batched result equals the per-frame results."""
    import fvp_oracle as O
    frames = [[[], _people(2, 1)], [_people(1, 2), _people(3, 3)], [[], []]]
    hm = _wrapper(emu_lib, frames)
    assert tuple(hm.shape) == (3, 2, J_, H_, W_)
    for b, frame in enumerate(frames):
        one = _wrapper(emu_lib, frame)
        assert tuple(one.shape) == (2, J_, H_, W_)
        assert np.array_equal(hm[b].numpy().view(np.uint32), one.numpy().view(np.uint32)), f"frame {b}"
        for v, preds in enumerate(frame):
            want = O.input_heatmaps_from_pred2d([preds], RT, (4 * W_, 4 * H_), (W_, H_), 3)[0].numpy() if preds \
                else np.zeros((J_, H_, W_), np.float32)
            assert np.array_equal(one[v].numpy().view(np.uint32), want.view(np.uint32)), f"frame {b} view {v}"
    assert (hm[0, 1] > 0).any() and (hm[1, 0] > 0).any()


def test_wrapper_accepts_people_as_tuples_and_nested_lists(emu_lib):
    """A frame whose views are tuples and whose people are nested lists is one frame, not a batch."""
    frame = [_people(2, 4), _people(1, 5)]
    want = _wrapper(emu_lib, frame)
    as_lists = [tuple(p.tolist() for p in v) for v in frame]
    got = _wrapper(emu_lib, as_lists)
    assert got.shape == want.shape and np.array_equal(got.numpy().view(np.uint32), want.numpy().view(np.uint32))
    got = _wrapper(emu_lib, (as_lists, as_lists))
    assert tuple(got.shape) == (2,) + tuple(want.shape)
    assert np.array_equal(got[1].numpy().view(np.uint32), want.numpy().view(np.uint32))


def test_wrapper_ignores_a_confidence_column(emu_lib):
    three = [_people(2, 6, cols=3), _people(1, 7, cols=3)]
    two = [[p[:, :2] for p in v] for v in three]
    a, b = _wrapper(emu_lib, three), _wrapper(emu_lib, two)
    assert (a > 0).any() and np.array_equal(a.numpy().view(np.uint32), b.numpy().view(np.uint32))


def test_wrapper_refuses_65_people_in_a_view(emu_lib):
    with pytest.raises(capi.FvpError, match="fvp_rasterise_heatmaps"):
        _wrapper(emu_lib, [_people(65, 8), _people(1, 9)])
    assert tuple(_wrapper(emu_lib, [_people(64, 8), _people(1, 9)]).shape) == (2, J_, H_, W_)
