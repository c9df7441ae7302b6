"""Cases and the yardstick of fvp_draw_poses (include/fvp.h, ABI 14), shared by tests/test_overlay_emu.py (CPU emulation of
the kernel) and tests/test_overlay_gpu.py (the shipped library on the MI355X).

The yardstick ``reference`` restates the definition independently of the product: Python integers (unbounded, so no
product is ever split), numpy float32 for the three compares and the product by 16, plain loops - person by person over
the whole frame, primitive by primitive over the pixels its box can reach - where the kernel goes tile by tile and pixel by
pixel.  The whole frame is compared byte for byte.  ``MUTANTS`` are six wrong readings of the definition;
test_overlay_emu.py asserts that the case set tells each from the true one.
"""
import ctypes as C
import functools

import numpy as np
import torch

EINVAL, ELIMIT = 10001, 10002
LIMBS15 = [[0, 1], [0, 2], [0, 3], [3, 4], [4, 5], [0, 9], [9, 10], [10, 11], [2, 6], [2, 12], [6, 7], [7, 8], [12, 13],
           [13, 14]]
LIMBS17 = [[0, 1], [0, 2], [1, 2], [1, 3], [2, 4], [3, 5], [4, 6], [5, 7], [7, 9], [6, 8], [8, 10], [5, 11], [11, 13],
           [13, 15], [6, 12], [12, 14], [14, 16], [5, 6], [11, 12]]
PAL3 = [[255, 0, 0], [0, 255, 0], [10, 20, 250]]
PAL16 = [[(37 * i + 11) % 256, (91 * i + 200) % 256, (53 * i + 77) % 256] for i in range(16)]
MUTANTS = ("disc_lt", "perp_lt", "trunc", "descending", "per_primitive", "no_half")
F32 = np.float32
NAN, INF = float("nan"), float("inf")
ABOVE = float(np.nextafter(F32(32768), F32(np.inf)))


# ---- the yardstick ---------------------------------------------------------------------------------------------------
def _q4(v, mut):
    p = F32(v) * F32(16)
    return int(np.trunc(p)) if mut == "trunc" else int(np.rint(p))          # np.rint: round-half-even


def _joint(views, conf, conf_min, b, v, n, j, mut):
    """Q4 position of a drawable joint, else None."""
    px, py, depth = (F32(views[b, v, n, j, k]) for k in range(3))
    if not depth > F32(0):
        return None
    if not (np.abs(px) <= F32(32768) and np.abs(py) <= F32(32768)):
        return None
    if conf is not None and not F32(conf[b, n, j]) >= F32(conf_min):
        return None
    return _q4(px, mut), _q4(py, mut)


def _disc(p, q, R, mut):
    d2 = (p[0] - q[0]) ** 2 + (p[1] - q[1]) ** 2
    return d2 < R * R if mut == "disc_lt" else d2 <= R * R


def _capsule(p, a, b, W, mut):
    dx, dy, wx, wy = b[0] - a[0], b[1] - a[1], p[0] - a[0], p[1] - a[1]
    t, dd = wx * dx + wy * dy, dx * dx + dy * dy
    if t <= 0:
        return wx * wx + wy * wy <= W * W
    if t >= dd:
        return (p[0] - b[0]) ** 2 + (p[1] - b[1]) ** 2 <= W * W
    cross2 = (wx * dy - wy * dx) ** 2
    return cross2 < W * W * dd if mut == "perp_lt" else cross2 <= W * W * dd


def _reach(lo, hi, n):
    """Pixel indices whose centres 16 i lie in [lo, hi], clipped to [0, n)."""
    return range(max(-(-lo // 16), 0), min(hi // 16, n - 1) + 1)


def reference(case, mut=None):
    """The frames after fvp_draw_poses, as a new array."""
    out = case["frames"].copy()
    views, ids, conf = case["views"], case["ids"], case["conf"]
    B, V, N, J = views.shape[:4]
    Hs, Ws = out.shape[2:4]
    R, W, alpha, pal = case["R"], case["W"], case["alpha"], case["palette"]
    half = 0 if mut == "no_half" else 128
    order = range(N - 1, -1, -1) if mut == "descending" else range(N)
    for b in range(B):
        for v in range(V):
            for n in order:
                if ids is not None and ids[b, n] < 0:
                    continue
                colour = pal[(int(ids[b, n]) if ids is not None else n) % len(pal)]
                q = [_joint(views, conf, case["conf_min"], b, v, n, j, mut) for j in range(J)]
                prims = [(q[j], q[j], R, True) for j in range(J) if q[j] is not None]
                prims += [(q[i], q[k], W, False) for i, k in case["limbs"] if q[i] is not None and q[k] is not None]
                hits = []                                # one entry per (primitive, covered pixel)
                for a, e, rad, disc in prims:
                    for y in _reach(min(a[1], e[1]) - rad, max(a[1], e[1]) + rad, Hs):
                        for x in _reach(min(a[0], e[0]) - rad, max(a[0], e[0]) + rad, Ws):
                            p = (16 * x, 16 * y)
                            if _disc(p, a, rad, mut) if disc else _capsule(p, a, e, rad, mut):
                                hits.append((y, x))
                for y, x in (hits if mut == "per_primitive" else sorted(set(hits))):
                    for c in range(3):
                        out[b, v, y, x, c] = (colour[c] * alpha + int(out[b, v, y, x, c]) * (256 - alpha) + half) >> 8
    return out


# ---- building cases --------------------------------------------------------------------------------------------------
def _frames(B, V, Hs, Ws, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(B, V, Hs, Ws, 3), dtype=np.uint8)


def _case(frames, N, J, limbs=(), palette=PAL16, R=80, W=32, alpha=256, conf_min=0.0, ids=None, conf=None):
    B, V = frames.shape[:2]
    return dict(frames=frames, views=np.zeros((B, V, N, J, 4), F32), ids=ids, conf=conf, limbs=[list(ab) for ab in limbs],
                palette=palette, R=R, W=W, alpha=alpha, conf_min=conf_min)


def _put(case, n, j, px, py, depth=1.0, b=None, v=None):
    """Joint (n, j) at pixel (px, py) in every frame (or frame b / view v)."""
    bs = slice(None) if b is None else b
    vs = slice(None) if v is None else v
    case["views"][bs, vs, n, j] = (px, py, depth, 0.5)


def _skeletons(case, seed, spread=1.3):
    """Random joints in and around the frame for every (b, v, n, j); a few joints behind the camera."""
    views = case["views"]
    Hs, Ws = case["frames"].shape[2:4]
    rng = np.random.default_rng(seed)
    B, V, N, J = views.shape[:4]
    centre = rng.uniform([0, 0], [Ws, Hs], size=(B, V, N, 1, 2))
    xy = centre + rng.normal(0, spread * min(Hs, Ws) / 2, size=(B, V, N, J, 2))
    views[..., :2] = (np.round(xy * 32) / 32).astype(F32)          # fractional Q4 positions, ties included
    views[..., 2] = np.where(rng.random((B, V, N, J)) < 0.1, -1.0, 1.0 + rng.random((B, V, N, J)))
    views[..., 3] = rng.random((B, V, N, J))


def disc_edges():
    c = _case(_frames(1, 1, 37, 150, 1), 1, 15)
    _put(c, 0, 0, 20.0, 10.0)                # on a pixel centre: (25, 10) and the 3-4-5 pixel (23, 14) lie at exactly R
    _put(c, 0, 1, 60.5, 20.5)                # at a half-pixel position
    _put(c, 0, 2, 100.0, 17.9375)            # (105, 18) lies at R^2 + 1 on the squared test: not covered
    _put(c, 0, 3, 59.96875, 31.0)            # 959.5 sixteenths: a tie, rounds to the even 960 = pixel 60, so (65, 31) is at R
    _put(c, 0, 4, 130.03125, 8.0)            # 2080.5 -> 2080
    return c


def disc_radius_zero():
    c = _case(_frames(2, 2, 37, 150, 2), 1, 15, R=0)
    _put(c, 0, 0, 20.0, 10.0)                # one pixel
    _put(c, 0, 1, 60.5, 20.5)                # no pixel centre at distance 0
    _put(c, 0, 2, 149.0, 36.0)               # the last pixel of the frame
    return c


def capsules():
    limbs = [(0, 1), (2, 3), (4, 5), (6, 7), (8, 9), (10, 11)]
    c = _case(_frames(1, 1, 37, 150, 3), 1, 15, limbs=limbs, R=0, W=32)
    _put(c, 0, 0, 5.0, 5.0), _put(c, 0, 1, 40.0, 5.0)                   # horizontal, both end caps inside
    _put(c, 0, 2, 100.0, 3.0), _put(c, 0, 3, 100.0, 30.0)               # vertical, across a tile border
    _put(c, 0, 4, 50.0, 10.0), _put(c, 0, 5, 80.0, 25.0)                # diagonal across four tiles (x = 64, y = 16)
    _put(c, 0, 6, 120.0, 20.0), _put(c, 0, 7, 120.0, 20.0)              # a == b
    _put(c, 0, 8, 20.0, 18.0), _put(c, 0, 9, 23.0, 22.0)                # d = (48, 64): (24, 20) has |cross| = W * 80, (25, 20) more
    _put(c, 0, 10, 130.25, 12.5), _put(c, 0, 11, 141.8125, 33.4375)     # fractional ends
    return c


def capsule_ends_outside():
    limbs = [(0, 1), (2, 3), (4, 5), (6, 7), (8, 9)]
    c = _case(_frames(1, 2, 37, 150, 4), 1, 15, limbs=limbs, R=48, W=24)
    _put(c, 0, 0, -20.0, -10.0), _put(c, 0, 1, 30.0, 20.0)              # left / top
    _put(c, 0, 2, 140.0, 30.0), _put(c, 0, 3, 170.0, 50.0)              # right / bottom
    _put(c, 0, 4, 75.0, -40.0), _put(c, 0, 5, 75.0, 80.0)               # through the frame, both ends outside
    _put(c, 0, 6, -30.0, 18.0), _put(c, 0, 7, 200.0, 18.5)              # the whole width
    _put(c, 0, 8, 155.0, 5.0), _put(c, 0, 9, 149.0, 0.0)                # one end outside, its cap reaches in
    return c


def limb_wholly_outside():
    limbs = [(0, 1), (2, 3), (4, 5)]
    c = _case(_frames(1, 1, 37, 150, 5), 1, 15, limbs=limbs, R=32, W=32)
    _put(c, 0, 0, -50.0, -5.0), _put(c, 0, 1, 200.0, -5.0)              # above: 3 pixels away with a reach of 2
    _put(c, 0, 2, 153.0, -40.0), _put(c, 0, 3, 153.0, 90.0)             # right of the frame
    _put(c, 0, 4, -3.0, 40.0), _put(c, 0, 5, 20.0, 60.0)                # below left
    c["unchanged"] = True
    return c


def range_limit():
    limbs = [(0, 1), (2, 3), (4, 5), (6, 7)]
    c = _case(_frames(1, 1, 37, 150, 6), 1, 15, limbs=limbs, R=32, W=24)
    _put(c, 0, 0, 32768.0, 18.0), _put(c, 0, 1, 100.0, 18.0)            # px = 32768: drawn
    _put(c, 0, 2, 32768.0, 32768.0), _put(c, 0, 3, 30.0, 5.0)           # the widest products
    _put(c, 0, 4, -32768.0, 32768.0), _put(c, 0, 5, 60.0, 30.0)
    _put(c, 0, 6, 32768.0, -32768.0), _put(c, 0, 7, -32768.0, 32767.9375)    # both ends far outside, passes the frame
    return c


def not_drawn_joints():
    """Each bad joint ends a limb whose other joint is fine: that joint's disc is drawn, the limb is not."""
    bad = [(ABOVE, 18.0, 1.0), (18.0, -ABOVE, 1.0), (NAN, 18.0, 1.0), (70.0, NAN, 1.0), (INF, 18.0, 1.0),
           (70.0, -INF, 1.0), (70.0, 18.0, 0.0), (70.0, 18.0, -1.0), (70.0, 18.0, NAN)]
    c = _case(_frames(1, 1, 37, 150, 7), 2, 17, limbs=[(2 * i, 2 * i + 1) for i in range(8)] + [(15, 16)], R=32, W=24)
    for i, (px, py, depth) in enumerate(bad[:8]):
        _put(c, 0, 2 * i, 10.0 + 17 * i, 8.0)
        _put(c, 0, 2 * i + 1, px, py, depth)
    _put(c, 1, 15, 20.0, 30.0), _put(c, 1, 16, *bad[8])
    _put(c, 1, 0, 60.0, 30.0), _put(c, 1, 1, 90.0, 31.0)                # a good limb beside them
    return c


def confidence(null_conf=False):
    c = _case(_frames(1, 2, 37, 150, 8), 1, 15, limbs=[(0, 1), (1, 2), (2, 3), (3, 4)], R=40, W=16, conf_min=0.3)
    for j in range(5):
        _put(c, 0, j, 15.0 + 28 * j, 10.0 + 4 * j)
    if not null_conf:
        conf = np.ones((1, 1, 15), F32)
        conf[0, 0, :5] = [0.3, np.nextafter(F32(0.3), F32(0)), 0.9, NAN, F32(0.3)]
        c["conf"] = conf
    return c


def identity_slot_keys():
    c = _case(_frames(1, 1, 37, 150, 9), 3, 15, limbs=LIMBS15, palette=PAL3, R=32, W=16)
    _skeletons(c, 90, spread=0.5)
    return c


def identity_left_out_and_wrap():
    c = _case(_frames(2, 2, 37, 150, 10), 3, 17, limbs=LIMBS17, palette=PAL3, R=32, W=16,
              ids=np.array([[7, -1, 4], [-1, 2 ** 31 - 1, 0]], np.int32))
    _skeletons(c, 100, spread=0.5)
    return c


def identity_permuted_slots():
    """The same three people (ids 5, 6, 40) in other slots in batch 1, on the same picture, apart from each other: both
    frames come out equal (the test asserts it)."""
    fr = _frames(1, 1, 37, 150, 11)
    c = _case(np.concatenate([fr, fr]), 3, 15, limbs=[(0, 1)], R=40, W=24, ids=np.array([[5, 6, 40], [40, 5, 6]], np.int32))
    where = {5: ((10.0, 10.0), (30.0, 25.0)), 6: ((60.0, 8.0), (85.0, 30.0)), 40: ((115.0, 28.0), (140.0, 6.0))}
    for b in range(2):
        for n in range(3):
            a, e = where[int(c["ids"][b, n])]
            _put(c, n, 0, *a, b=b), _put(c, n, 1, *e, b=b)
    c["batches_equal"] = True
    return c


def blending(alpha):
    """Three people crossing in one spot; person 0's joint disc lies over its own limb."""
    c = _case(_frames(1, 1, 37, 150, 12), 3, 15, limbs=[(0, 1)], palette=PAL3, R=64, W=32, alpha=alpha)
    _put(c, 0, 0, 60.0, 18.0), _put(c, 0, 1, 90.0, 18.0)
    _put(c, 1, 0, 75.0, 2.0), _put(c, 1, 1, 75.0, 34.0)
    _put(c, 2, 0, 62.0, 6.0), _put(c, 2, 1, 88.0, 30.0)
    return c


def nothing_drawable():
    c = _case(_frames(2, 2, 37, 150, 13), 3, 17, limbs=LIMBS17, conf_min=0.5, ids=np.array([[0, 1, -1], [2, 3, 4]], np.int32))
    _skeletons(c, 130)
    c["ids"][0, 2] = -1
    c["conf"] = np.full((2, 3, 17), 0.25, F32)
    c["conf"][0, 2] = 1.0                                               # the confident person is the one left out
    c["unchanged"] = True
    return c


def one_pixel_frame():
    c = _case(_frames(2, 2, 1, 1, 14), 1, 15, limbs=LIMBS15, R=8, W=8, alpha=128)
    _put(c, 0, 0, 0.25, -0.25, b=0)                                     # batch 1 stays empty
    return c


def whole_tiles(seed=15):
    c = _case(_frames(2, 2, 16, 64, seed), 1, 15, limbs=LIMBS15, R=24, W=12, alpha=200,
              ids=np.array([[3], [19]], np.int32))
    _skeletons(c, 150)
    return c


def crowd():
    c = _case(_frames(2, 2, 37, 150, 16), 3, 17, limbs=LIMBS17, R=40, W=20, alpha=160,
              ids=np.array([[2, 0, 1], [17, 33, 1]], np.int32), conf_min=0.2)
    _skeletons(c, 160, spread=0.6)
    c["conf"] = np.random.default_rng(161).random((2, 3, 17)).astype(F32)
    return c


CASES = {
    "disc_edges": disc_edges, "disc_radius_zero": disc_radius_zero, "capsules": capsules,
    "capsule_ends_outside": capsule_ends_outside, "limb_wholly_outside": limb_wholly_outside, "range_limit": range_limit,
    "not_drawn_joints": not_drawn_joints, "confidence": confidence,
    "confidence_null": functools.partial(confidence, null_conf=True), "identity_slot_keys": identity_slot_keys,
    "identity_left_out_and_wrap": identity_left_out_and_wrap, "identity_permuted_slots": identity_permuted_slots,
    "blend_256": functools.partial(blending, 256), "blend_128": functools.partial(blending, 128),
    "blend_1": functools.partial(blending, 1), "nothing_drawable": nothing_drawable, "one_pixel_frame": one_pixel_frame,
    "whole_tiles": whole_tiles, "crowd": crowd,
}


@functools.lru_cache(maxsize=None)
def expected(name):
    """(case, reference frames): computed once and shared; neither is modified by a test."""
    case = CASES[name]()
    want = reference(case)
    want.setflags(write=False)
    case["frames"].setflags(write=False)
    return case, want


# ---- running the product ---------------------------------------------------------------------------------------------
def _dev(a, device):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def call(lib, device, t_frames, t_views, ids, conf, case, **over):
    """One fvp_draw_poses on device tensors; ``over`` replaces scalar arguments (argument-error tests).  Returns the code."""
    B, V, Hs, Ws = t_frames.shape[:4]
    N, J = t_views.shape[2:4]
    a = dict(B=B, V=V, Hs=Hs, Ws=Ws, N=N, J=J, L=len(case["limbs"]), P=len(case["palette"]), R=case["R"], W=case["W"],
             alpha=case["alpha"], conf_min=case["conf_min"], limbs=case["limbs"], palette=case["palette"],
             frames=_ptr(t_frames), views=_ptr(t_views))
    a.update(over)
    flat = [j for ab in a["limbs"] for j in ab] if a["limbs"] is not None else None
    limbs = None if flat is None else (C.c_int32 * max(len(flat), 1))(*flat)
    pal = None if a["palette"] is None else (C.c_uint8 * (3 * len(a["palette"])))(*[v for c in a["palette"] for v in c])
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream) if str(device).startswith("cuda") else None
    return lib.fvp_draw_poses(a["frames"], a["B"], a["V"], a["Hs"], a["Ws"], a["views"], _ptr(ids), _ptr(conf), a["N"],
                              a["J"], limbs, a["L"], pal, a["P"], a["R"], a["W"], a["alpha"], a["conf_min"], stream)


def run(lib, device, case, fence=False):
    """The frames after fvp_draw_poses on ``device`` as a numpy array (and, with ``fence``, the emulator's count of reads
    of frame bytes)."""
    frames, views = _dev(case["frames"].copy(), device), _dev(case["views"], device)
    ids, conf = _dev(case["ids"], device), _dev(case["conf"], device)
    if fence:
        lib.hipemu_fence.argtypes = [C.c_void_p, C.c_size_t]
        lib.hipemu_fenced_reads.restype = C.c_long
        lib.hipemu_fences_clear()
        lib.hipemu_fence(C.c_void_p(frames.data_ptr()), frames.numel())
    rc = call(lib, device, frames, views, ids, conf, case)
    reads = None
    if fence:
        reads = int(lib.hipemu_fenced_reads())
        lib.hipemu_fences_clear()
    assert rc == 0, rc
    if str(device).startswith("cuda"):
        torch.cuda.synchronize()
    return (frames.cpu().numpy(), reads) if fence else frames.cpu().numpy()


def check_case(lib, device, name):
    case, want = expected(name)
    got = run(lib, device, case)
    bad = int((got != want).any(axis=-1).sum())
    assert bad == 0, f"{name}: {bad} of {want[..., 0].size} pixels differ from the yardstick"
    changed = int((want != case["frames"]).any(axis=-1).sum())
    if case.get("unchanged"):
        assert changed == 0
    else:
        assert changed > 0, f"{name}: the case draws nothing"
    if case.get("batches_equal"):
        assert np.array_equal(got[0], got[1])


# (what is wrong, expected code); every call must leave a sentinel-filled frame untouched
ARGUMENT_ERRORS = [
    (dict(frames=None), EINVAL), (dict(views=None), EINVAL), (dict(palette=None), EINVAL), (dict(limbs=None), EINVAL),
    (dict(B=-1), EINVAL), (dict(V=-1), EINVAL), (dict(N=0), EINVAL), (dict(J=0), EINVAL), (dict(Hs=0), EINVAL),
    (dict(Ws=0), EINVAL), (dict(P=0), EINVAL), (dict(L=-1), EINVAL), (dict(limbs=[[0, 15]], L=1), EINVAL),
    (dict(limbs=[[-1, 2]], L=1), EINVAL), (dict(alpha=0), EINVAL), (dict(alpha=257), EINVAL), (dict(R=-1), EINVAL),
    (dict(R=1025), EINVAL), (dict(W=-1), EINVAL), (dict(W=1025), EINVAL), (dict(conf_min=NAN), EINVAL),
    (dict(N=33), ELIMIT), (dict(J=33, limbs=[], L=0), ELIMIT), (dict(V=9), ELIMIT),
    (dict(L=65, limbs=[[0, 1]] * 65), ELIMIT), (dict(P=65, palette=[[1, 2, 3]] * 65), ELIMIT), (dict(Hs=16385), ELIMIT),
    (dict(Ws=16385), ELIMIT),
]


def case_argument_errors(lib, device):
    """Every error of include/fvp.h: the code comes back and the frame - its joints all drawable - keeps its sentinel.
    The shape arguments that are over their limit are never used to address memory: no launch happens."""
    case = _case(np.full((1, 1, 37, 150, 3), 0xA5, np.uint8), 1, 15, limbs=LIMBS15)
    _skeletons(case, 170, spread=0.4)
    case["views"][..., 2] = 1.0
    frames, views = _dev(case["frames"].copy(), device), _dev(case["views"], device)
    for over, code in ARGUMENT_ERRORS:
        rc = call(lib, device, frames, views, None, None, case, **over)
        assert rc == code, f"{over}: returned {rc}, expected {code}"
    for over in (dict(B=0), dict(V=0)):                                  # nothing to do: 0, no launch
        assert call(lib, device, frames, views, None, None, case, **over) == 0
    if str(device).startswith("cuda"):
        torch.cuda.synchronize()
    assert (frames.cpu().numpy() == 0xA5).all()
    assert call(lib, device, frames, views, None, None, case) == 0       # and the same arguments, valid, do draw
    assert (frames.cpu().numpy() != 0xA5).any()
