"""Shared by tests/test_rasterise_emu.py (CPU emulator) and tests/test_rasterise_gpu.py (the shipped library on the card):
fvp_rasterise_heatmaps (k_rasterise, csrc/fvp_heatmap.hip) called directly on caller-owned, guarded, poisoned buffers, against
oracle.fvp_oracle.generate_input_heatmap (float64 scalar arithmetic, one rounding to float32) per image.

The cases are the smallest shapes that reach every path of the launch code: the host picks RB = 4, 2 or 1 rows per workgroup
from J * RB * W * 4 <= 44 KB (band_rows() restates the rule), a last band is ragged when H % RB != 0, and the limits are
J * W * 4 <= 32 KB, P <= 64 and P * J <= 1024.  ``exact`` is True on the emulator (same libm as the oracle: bit-equal) and False
on the card (the device exp(double) may differ in its last float64 bit: <= 1 ulp of float32, rtol 1.2e-7)."""
import ctypes as C
import functools
import math

import numpy as np
import torch

import fvp_oracle as O
from common import POISON_BITS, POISON_GUARD

EINVAL, ELIMIT = 10001, 10002
GUARD = POISON_GUARD              # floats of guard before and after each output: more than the rows a ragged last band lacks
                                  # in any case (at most 3 * 64 * 16 floats), so a kernel that writes that band in full lands in it
RTOL_CARD = 1.2e-7                # at most 1 ulp of float32
LO2, HI2 = 1.0 / 4 * 96 ** 2, 4.0 * 96 ** 2          # compute_human_scale's clamps on the squared extent
EXTENTS = (10, 48, 120, 192, 400)                    # heatmap pixels: below the low clamp, at it, between, at the high one, above

# name -> J, W, H, P, (stride x, stride y), sigma, seed (chosen so that test_fixture_conditions holds)
CASES = {
    "rb4_ragged": (5, 40, 7, 5, (4.0, 4.0), 3.0, 0),        # RB 4, last band of 3 rows, J < 4 waves' worth + 1
    "rb2_ragged": (19, 150, 7, 5, (4.0, 4.0), 3.0, 0),      # RB 2 just above the 2816 switch, last band of 1 row, JP 20
    "rb1": (24, 240, 5, 5, (4.0, 4.0), 2.0, 0),             # RB 1 just above the 5632 switch
    "rb1_limit": (32, 256, 3, 5, (4.0, 3.5), 3.0, 0),       # J * W * 4 == 32 KB, unequal strides, JP == J
    "full_tables": (16, 64, 9, 64, (4.0, 4.0), 1.0, 0),     # P == 64 and P * J == 1024: every q[] and prm[] slot is used
    "tall": (7, 33, 130, 6, (4.0, 4.0), 3.0, 0),            # 33 bands, odd W, windows over > 3 bands, wave 3 one joint short
}
OUTPUT_FORMS = ("both", "nchw_only", "cl_only", "wide_jp")


def band_rows(J, W):
    """The host's rule for RB, restated (fvp_rasterise_heatmaps)."""
    rb = 4
    while rb > 1 and J * rb * W * 4 > 44 * 1024:
        rb >>= 1
    return rb


def jp_of(J):
    return (J + 3) // 4 * 4


def _person(rng, J, W, H, ext, axis, exact):
    """[J,2] in heatmap pixels: the larger side of the joints' box is ``ext`` along ``axis`` (two joints sit on its ends), the
    centre uniform in [-8, W+8] x [-8, H+8]; the free joints are drawn inside the box where it meets the image's surroundings.
    ``exact``: every coordinate an integer, so the extent is ``ext`` with no rounding."""
    c = np.array([rng.uniform(-8, W + 8), rng.uniform(-8, H + 8)])
    half = np.array([ext / 2.0, ext / 2.0])
    half[1 - axis] *= rng.uniform(0.3, 1.0)
    if exact:
        c, half = np.rint(c), np.array([ext // 2, ext // 2], np.float64)
        half[1 - axis] = np.floor(half[1 - axis] * rng.uniform(0.3, 1.0))
    lim = np.array([W, H], np.float64)
    lo, hi = np.maximum(c - half, -12.0), np.minimum(c + half, lim + 12.0)
    q = rng.uniform(lo, hi, size=(J, 2))
    if exact:
        q = np.clip(np.rint(q), c - half, c + half)
    a, b = rng.choice(J, 2, replace=False)
    q[a, axis], q[b, axis] = c[axis] - half[axis], c[axis] + half[axis]
    return q


@functools.lru_cache(maxsize=None)
def make_case(name):
    """(joints [3,P,J,2] float64 in network-image pixels, num_people [3] int32 = [P, P-2, 0]).  Every slot of ``joints`` holds a
    person, also those past an image's count: a kernel that ignores the count shows."""
    J, W, H, P, (sx, sy), sigma, seed = CASES[name]
    rng = np.random.default_rng([seed, sum(name.encode())])
    joints = np.empty((3, P, J, 2), np.float64)
    for i in range(3):
        for n in range(P):
            ext = EXTENTS[(n + 2 * i) % len(EXTENTS)]
            joints[i, n] = _person(rng, J, W, H, ext, (n + i) % 2, exact=ext in (48, 192)) * np.array([sx, sy])
    counts = np.array([P, P - 2, 0], np.int32)
    joints.setflags(write=False)
    counts.setflags(write=False)
    return joints, counts


def oracle_image(people, J, W, H, sx, sy, sigma):
    """The yardstick for one image: ``people`` [n,J,2] -> [J,H,W] float32."""
    if len(people) == 0:
        return np.zeros((J, H, W), np.float32)
    image_size = (W * sx, H * sy)
    assert tuple(np.array(image_size) / np.array((W, H))) == (sx, sy)       # the oracle derives the strides from the sizes
    with np.errstate(over="ignore"):                                       # extent^2 of a far-away joint: inf, then clipped
        return O.generate_input_heatmap([np.asarray(p, np.float64) for p in people], image_size, (W, H), sigma)


def oracle_batch(joints, counts, J, W, H, sx, sy, sigma):
    P = joints.shape[1]
    return np.stack([oracle_image(joints[i, :min(max(int(counts[i]), 0), P)], J, W, H, sx, sy, sigma)
                     for i in range(joints.shape[0])])


@functools.lru_cache(maxsize=None)
def want_of(name):
    J, W, H, P, (sx, sy), sigma, _ = CASES[name]
    joints, counts = make_case(name)
    w = oracle_batch(joints, counts, J, W, H, sx, sy, sigma)
    w.setflags(write=False)
    return w


# ---- the runner ------------------------------------------------------------------------------------------------------------
class Guarded:
    """n floats of POISON_BITS between two guards of POISON_BITS."""

    def __init__(self, n, dev):
        self.n = n
        self.flat = torch.full((n + 2 * GUARD,), POISON_BITS, dtype=torch.int32, device=dev)
        self.ptr = self.flat.data_ptr() + 4 * GUARD

    def guards_untouched(self):
        b = self.flat.cpu().numpy()
        return bool((b[:GUARD] == POISON_BITS).all() and (b[GUARD + self.n:] == POISON_BITS).all())

    def bits(self):
        return self.flat.cpu().numpy()[GUARD:GUARD + self.n].copy()

    def floats(self):
        return self.bits().view(np.float32)


def run(lib, dev, joints, counts, J, W, H, sx, sy, sigma, *, form="both", JP=None, nimg=None, P=None, expect=0,
        null_joints=False, null_counts=False):
    """One call of fvp_rasterise_heatmaps.  joints [nimg,P,J,2] float64, counts [nimg] int32 (numpy); ``dev``: "cpu" (the
    emulator) or a GPU device.  form: which outputs are passed (OUTPUT_FORMS; "none": neither).  Asserts the return code, that
    the guards of both outputs are untouched, and that a requested output holds no poison after a success and nothing but
    poison after a refusal.  Returns (nchw [nimg,J,H,W] or None, cl [nimg,H*W,JP] or None) as numpy float32."""
    joints = np.array(joints, np.float64)            # copies: the cases' arrays are read-only
    counts = np.array(counts, np.int32)
    nimg = joints.shape[0] if nimg is None else nimg
    P = joints.shape[1] if P is None else P
    if JP is None:
        JP = jp_of(J) + (8 if form == "wide_jp" else 0)
    n_img = max(nimg, 1)
    jd = torch.from_numpy(joints).to(dev)
    cd = torch.from_numpy(counts).to(dev)
    o_n = Guarded(n_img * max(J, 1) * max(H, 1) * max(W, 1), dev) if form not in ("cl_only", "none") else None
    o_c = Guarded(n_img * max(H, 1) * max(W, 1) * max(JP, J, 1), dev) if form not in ("nchw_only", "none") else None
    cuda = torch.device(dev).type == "cuda"
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream) if cuda else None
    rc = lib.fvp_rasterise_heatmaps(None if null_joints else jd.data_ptr(), None if null_counts else cd.data_ptr(), nimg, P, J,
                                    W, H, sx, sy, sigma, o_n.ptr if o_n else None, o_c.ptr if o_c else None, JP, stream)
    if cuda:
        torch.cuda.synchronize()
    assert rc == expect, f"fvp_rasterise_heatmaps returned {rc}, expected {expect}"
    out = []
    for o, shape, what in ((o_n, (nimg, J, H, W), "heat_nchw"), (o_c, (nimg, H * W, JP), "heat_cl")):
        if o is None:
            out.append(None)
            continue
        assert o.guards_untouched(), f"{what}: guard words changed (out-of-bounds write)"
        b = o.bits()
        if rc != 0 or nimg == 0:
            assert (b == POISON_BITS).all(), f"{what}: written although the call returned {rc} (nimg {nimg})"
            out.append(None)
            continue
        used = int(np.prod(shape))
        assert not (b[:used] == POISON_BITS).any(), f"{what}: {int((b[:used] == POISON_BITS).sum())} elements were not written"
        assert (b[used:] == POISON_BITS).all(), f"{what}: written past the requested output"
        out.append(b[:used].view(np.float32).reshape(shape))
    return tuple(out)


def run_case(lib, dev, name, **kw):
    J, W, H, P, (sx, sy), sigma, _ = CASES[name]
    joints, counts = make_case(name)
    return run(lib, dev, joints, counts, J, W, H, sx, sy, sigma, **kw)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- comparison rules ------------------------------------------------------------------------------------------------------
def compare(got, want, exact, what=""):
    """Placement exact; values bit-equal (emulator) or within 1 ulp of float32 (card)."""
    assert got.shape == want.shape and got.dtype == np.float32
    assert np.isfinite(got).all(), f"{what}: non-finite values"
    assert np.array_equal(got > 0, want > 0), f"{what}: window placement differs in {int(((got > 0) != (want > 0)).sum())} cells"
    nz = want > 0
    rel = float((np.abs(got[nz].astype(np.float64) - want[nz]) / want[nz]).max()) if nz.any() else 0.0
    print(f"{what}: {int(nz.sum())} non-zero cells, max relative difference {rel:.3e}, "
          f"{int((bits(got) != bits(want)).sum())} cells differ in bits")
    if exact:
        assert np.array_equal(bits(got), bits(want)), f"{what}: {int((bits(got) != bits(want)).sum())} values differ in bits"
    else:
        np.testing.assert_allclose(got, want, rtol=RTOL_CARD, atol=0, err_msg=what)
        assert not np.signbit(got[~nz]).any(), f"{what}: -0.0 where nothing is stamped"


def compare_cl(cl, nchw, J, what=""):
    """cl[..., :J] is the NCHW output permuted, bit for bit; the padding channels are +0.0."""
    nimg, _, H, W = nchw.shape
    assert np.array_equal(bits(cl[..., :J]), bits(nchw.reshape(nimg, J, H * W).transpose(0, 2, 1))), \
        f"{what}: channels-last copy differs from the NCHW output"
    assert not bits(cl[..., J:]).any(), f"{what}: padding channels are not +0.0"


def check_case(lib, dev, name, exact):
    J = CASES[name][0]
    nchw, cl = run_case(lib, dev, name)
    compare(nchw, want_of(name), exact, name)
    compare_cl(cl, nchw, J, name)


def check_output_forms(lib, dev, name, form):
    """Both outputs, NCHW only, channels-last only, JP > J + 3: the output that is there equals the two-output call's bits."""
    J = CASES[name][0]
    nchw, cl = run_case(lib, dev, name)
    n2, c2 = run_case(lib, dev, name, form=form)
    if form == "nchw_only":
        assert c2 is None and np.array_equal(bits(n2), bits(nchw))
    elif form == "cl_only":
        assert n2 is None and np.array_equal(bits(c2), bits(cl))
    else:
        assert np.array_equal(bits(n2), bits(nchw))
        assert c2.shape[-1] == (jp_of(J) + 8 if form == "wide_jp" else jp_of(J)) and c2.shape[-1] >= J
        compare_cl(c2, nchw, J, f"{name} {form}")


# ---- counts, limits, arguments ---------------------------------------------------------------------------------------------
def check_counts(lib, dev, exact):
    """num_people = [9, -3] with P = 2: image 0 is the oracle on exactly 2 people, image 1 is all +0.0 and fully written."""
    J, W, H, _, (sx, sy), sigma, _ = CASES["rb4_ragged"]
    joints = make_case("rb4_ragged")[0][:2, 1:3]                     # two people per image, the exact-48 one among them
    nchw, cl = run(lib, dev, joints, np.array([9, -3], np.int32), J, W, H, sx, sy, sigma)
    want = oracle_batch(joints, np.array([2, 0]), J, W, H, sx, sy, sigma)
    assert (want[0] > 0).any()
    compare(nchw, want, exact, "counts [9, -3]")
    assert not bits(nchw[1]).any() and not bits(cl[1]).any(), "an image with a negative count is not all +0.0"
    compare_cl(cl, nchw, J, "counts")


def check_limits(lib, dev):
    """One step past each limit: FVP_ELIMIT and both outputs still poison (run() asserts that).  The companions AT the limit
    are the cases rb1_limit (J * W * 4 == 32 KB) and full_tables (P == 64, P * J == 1024)."""
    assert CASES["rb1_limit"][0] * CASES["rb1_limit"][1] * 4 == 32 * 1024
    assert CASES["full_tables"][3] == 64 and CASES["full_tables"][3] * CASES["full_tables"][0] == 1024
    for J, W, P in ((33, 256, 1), (4, 16, 65), (17, 16, 64)):
        joints = np.full((1, P, J, 2), 8.0)
        run(lib, dev, joints, np.array([P], np.int32), J, W, 3, 4.0, 4.0, 3.0, expect=ELIMIT)


def check_arguments(lib, dev):
    """Every FVP_EINVAL condition, outputs untouched; nimg == 0 returns 0 before any limit check and writes nothing."""
    J, W, H, P = 4, 16, 3, 2
    joints = np.full((1, P, J, 2), 8.0)
    counts = np.array([P], np.int32)
    base = dict(J=J, W=W, H=H, sx=4.0, sy=4.0, sigma=3.0)

    def call(expect=EINVAL, **over):
        a = dict(base)
        kw = {k: over.pop(k) for k in list(over) if k not in a}
        a.update(over)
        return run(lib, dev, joints, counts, a["J"], a["W"], a["H"], a["sx"], a["sy"], a["sigma"], expect=expect, **kw)

    nchw, _ = call(expect=0)
    assert (nchw > 0).any()
    call(null_joints=True)
    call(null_counts=True)
    call(form="none")
    call(JP=J - 1)
    call(JP=J - 1, form="cl_only")
    assert call(expect=0, JP=J - 1, form="nchw_only")[0] is not None            # JP is not looked at without heat_cl
    for bad in (0.0, -4.0, float("nan"), float("inf")):
        call(sx=bad)
        call(sy=bad)
        call(sigma=bad)
    for dim in ("J", "W", "H"):
        call(**{dim: 0})
        call(**{dim: -1})
    call(nimg=-1)
    call(P=-1)
    # nimg == 0: success, nothing written, even with sizes beyond every limit
    run(lib, dev, joints, counts, 33, 256, H, 4.0, 4.0, 3.0, nimg=0, P=65, expect=0)


def check_determinism_and_batching(lib, dev, name="rb2_ragged"):
    """Two calls on the same inputs give the same bits; a call on nimg = 3 equals three calls on nimg = 1."""
    J, W, H, P, (sx, sy), sigma, _ = CASES[name]
    joints, counts = make_case(name)
    a_n, a_c = run_case(lib, dev, name)
    b_n, b_c = run_case(lib, dev, name)
    assert np.array_equal(bits(a_n), bits(b_n)) and np.array_equal(bits(a_c), bits(b_c)), "two calls differ"
    for i in range(3):
        n1, c1 = run(lib, dev, joints[i:i + 1], counts[i:i + 1], J, W, H, sx, sy, sigma)
        assert np.array_equal(bits(n1[0]), bits(a_n[i])) and np.array_equal(bits(c1[0]), bits(a_c[i])), f"image {i} alone differs"


# ---- non-finite joints -----------------------------------------------------------------------------------------------------
NONFINITE = ("nan_x", "inf_y", "neg_inf_x", "all_nan", "huge_finite")


def nonfinite_inputs():
    """rb4_ragged's shape, one person per image (NONFINITE names the images).  Returns (joints [5,1,J,2], counts, zeroed:
    per image the joints whose map must be +0.0, want [5,J,H,W]).  The yardstick is the oracle on the finite joints: a
    non-finite joint is replaced by a copy of a finite one (which leaves the person's extent as it is) and its map zeroed."""
    J, W, H, _, (sx, sy), sigma, _ = CASES["rb4_ragged"]
    nan, inf = float("nan"), float("inf")
    base = np.array([[30.0, 12.0], [70.0, 8.0], [110.0, 20.0], [50.0, 16.0], [150.0, 4.0]])      # network pixels, all inside
    assert base.shape == (J, 2)
    joints = np.repeat(base[None, None], len(NONFINITE), axis=0)
    joints[0, 0, 1] = (nan, 12.0)              # hardware double -> int32 gives 0 for NaN: a blob at column 0, row 3
    joints[1, 0, 2] = (40.0, inf)
    joints[2, 0, 3] = (-inf, 10.0)
    joints[3, 0] = nan
    joints[4, 0, 0, 0] = 3e9                   # finite: part of the extent; its window lies beyond the image
    joints[4, 0, 4, 1] = -1e300
    zeroed = [[1], [2], [3], list(range(J)), [0, 4]]
    want = np.zeros((len(NONFINITE), J, H, W), np.float32)
    for i in range(len(NONFINITE)):
        p = joints[i, 0].copy()
        bad = ~np.isfinite(p).all(axis=1)
        if bad.all():
            continue
        p[bad] = p[~bad][0]
        want[i] = oracle_image(p[None], J, W, H, sx, sy, sigma)
        want[i, bad] = 0.0
        if NONFINITE[i] == "huge_finite":
            assert not want[i, zeroed[i]].any()          # the oracle itself skips the windows beyond the image
        else:
            assert bad.tolist() == [j in zeroed[i] for j in range(J)]
        assert all((want[i, j] > 0).any() for j in range(J) if j not in zeroed[i])
    return joints, np.ones(len(NONFINITE), np.int32), zeroed, want


def check_nonfinite(lib, dev, exact):
    J, W, H, _, (sx, sy), sigma, _ = CASES["rb4_ragged"]
    joints, counts, zeroed, want = nonfinite_inputs()
    nchw, cl = run(lib, dev, joints, counts, J, W, H, sx, sy, sigma)
    assert np.isfinite(nchw).all() and np.isfinite(cl).all(), "a non-finite joint gave a non-finite map"
    nan_map = nchw[0, 1]
    assert not nan_map[:, 0].any() and not nan_map[0, :].any(), \
        f"the NaN joint stamped column 0 / row 0 (max {float(nan_map.max()):.3g} at {np.unravel_index(nan_map.argmax(), nan_map.shape)})"
    for i, name in enumerate(NONFINITE):
        for j in zeroed[i]:
            assert not bits(nchw[i, j]).any(), f"{name}: the map of joint {j} is not +0.0 (max {float(nchw[i, j].max()):.3g})"
        compare(nchw[i], want[i], exact, name)
    compare_cl(cl, nchw, J, "non-finite joints")


# ---- what the fixtures contain (asserted on the oracle and on the window arithmetic in float64, never on the kernel) --------
def windows(people, sx, sy, sigma):
    """JointsDataset.generate_input_heatmap's window arithmetic for people [n,J,2], in Python floats and ints:
    rows (person, joint, q_x, q_y, ul0, ul1, br0, br1, squared extent)."""
    rows = []
    for n, p in enumerate(people):
        q = np.asarray(p, np.float64) / np.array([sx, sy])
        e2 = float(max(q[:, 1].max() - q[:, 1].min(), q[:, 0].max() - q[:, 0].min())) ** 2
        tmp = 3 * (sigma * math.sqrt(2 * min(max(e2, LO2), HI2) / (96.0 * 96.0)))
        for j in range(q.shape[0]):
            mx, my = int(q[j, 0]), int(q[j, 1])
            rows.append((n, j, float(q[j, 0]), float(q[j, 1]), int(mx - tmp), int(my - tmp), int(mx + tmp + 1), int(my + tmp + 1), e2))
    return rows


def fixture_report(name):
    """The conditions of the case list as {condition: bool}."""
    J, W, H, P, (sx, sy), sigma, _ = CASES[name]
    joints, counts = make_case(name)
    rep = {k: False for k in ("clipped_left", "clipped_top", "clipped_right", "clipped_bottom", "outside_right", "outside_below",
                              "outside_left", "outside_above", "q_between_minus_one_and_zero", "low_clamp", "no_clamp",
                              "high_clamp", "extent_exactly_48", "extent_exactly_192", "later_person_smaller_under_overlap")}
    for i in range(3):
        people = joints[i, :counts[i]]
        for n, j, qx, qy, ul0, ul1, br0, br1, e2 in windows(people, sx, sy, sigma):
            rep["low_clamp"] |= e2 < LO2
            rep["high_clamp"] |= e2 > HI2
            rep["no_clamp"] |= LO2 < e2 < HI2
            rep["extent_exactly_48"] |= e2 == 48.0 ** 2
            rep["extent_exactly_192"] |= e2 == 192.0 ** 2
            rep["outside_right"] |= ul0 >= W
            rep["outside_below"] |= ul1 >= H
            rep["outside_left"] |= br0 < 0
            rep["outside_above"] |= br1 < 0
            if ul0 >= W or ul1 >= H or br0 < 0 or br1 < 0:
                continue
            rep["clipped_left"] |= ul0 < 0
            rep["clipped_top"] |= ul1 < 0
            rep["clipped_right"] |= br0 > W
            rep["clipped_bottom"] |= br1 > H
            rep["q_between_minus_one_and_zero"] |= -1 < qx < 0 or -1 < qy < 0
        # element-wise max: a cell under the windows of two people where the later one's value is the smaller
        single = [oracle_image(people[n:n + 1], J, W, H, sx, sy, sigma) for n in range(len(people))]
        for b in range(1, len(single)):
            first = np.maximum.reduce(single[:b])
            rep["later_person_smaller_under_overlap"] |= bool(((single[b] > 0) & (first > 0) & (single[b] < first)).any())
    rb = band_rows(J, W)
    rows_hit = (want_of(name) > 0).any(axis=(0, 1, 3))                                   # [H]
    bands = [bool(rows_hit[b * rb:(b + 1) * rb].any()) for b in range((H + rb - 1) // rb)]
    rep["every_band_non_zero"] = all(bands)
    rep["ragged_last_band"] = H % rb != 0
    return rep, rb
