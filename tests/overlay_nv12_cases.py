"""Cases and the yardstick of fvp_draw_poses_nv12 (include/fvp.h, ABI 15), shared by tests/test_overlay_nv12_emu.py (CPU
emulation of the kernel) and tests/test_overlay_nv12_gpu.py (the shipped library on the MI355X).

The yardstick ``reference`` restates the definition independently of the product, in Python integers: it derives the colour
constants itself from Kr and Kb in float64, takes the per-person coverage of a luma pixel from the yardstick geometry of
tests/overlay_cases.py (the same rule, by definition), and paints person by person over the whole frame - luma pixel by
pixel, chroma quad by quad with the count of covered pixels.  A surface is one or two flat allocations filled with seeded
random bytes, planes at byte offsets with their own pitches and frame strides; the WHOLE allocation is compared byte for
byte: both planes, the pitch padding, the gaps between frames and the bytes before and behind.  ``MUTANTS`` are seven wrong
readings of the definition; test_overlay_nv12_emu.py asserts that the case set tells each from the true one.
"""
import ctypes as C
import functools

import numpy as np
import torch

import overlay_cases as OC

EINVAL, ELIMIT = OC.EINVAL, OC.ELIMIT
F32 = np.float32
# utils/overlay.py::PALETTE, restated: the 16 default colours
PALETTE16 = [(230, 25, 75), (60, 180, 75), (255, 225, 25), (0, 130, 200), (245, 130, 48), (145, 30, 180), (70, 240, 240),
             (240, 50, 230), (210, 245, 60), (250, 190, 212), (0, 128, 128), (220, 190, 255), (170, 110, 40), (255, 250, 200),
             (128, 0, 0), (170, 255, 195)]
EXTREMES = [(0, 0, 0), (255, 255, 255), (255, 0, 0), (0, 255, 0), (0, 0, 255)]
MUTANTS = ("chroma_all_or_nothing", "chroma_per_pixel", "chroma_top_left", "uv_swapped", "descending", "no_half", "shift8")
# FVP_YUV_*: (Kr, Kb, full range)
STANDARDS = {0: (0.299, 0.114, False), 1: (0.2126, 0.0722, False), 2: (0.299, 0.114, True), 3: (0.2126, 0.0722, True)}
STANDARD_NAMES = {0: "BT601_LIMITED", 1: "BT709_LIMITED", 2: "BT601_FULL", 3: "BT709_FULL"}


# ---- the yardstick: colour --------------------------------------------------------------------------------------------
def colour_constants(standard):
    """The twelve constants (YOFF, CYR, CYG, CYB, UOFF, CUR, CUG, CUB, VOFF, CVR, CVG, CVB) from Kr, Kb in float64."""
    kr, kb, full = STANDARDS[standard]
    kg = 1.0 - kr - kb
    sy, sc, yoff = (1.0, 1.0, 0) if full else (219.0 / 255.0, 224.0 / 255.0, 16)
    q = lambda k: int(round(k * 65536.0))                                       # noqa: E731
    return ([yoff] + [q(k * sy) for k in (kr, kg, kb)]
            + [128] + [q(k / (2.0 * (1.0 - kb)) * sc) for k in (-kr, -kg, 1.0 - kb)]
            + [128] + [q(k / (2.0 * (1.0 - kr)) * sc) for k in (1.0 - kr, -kg, -kb)])


def yuv_of(rgb, standard, clip=True):
    """(Yc, Uc, Vc) of an RGB colour; Python's >> on integers is arithmetic."""
    k = colour_constants(standard)
    r, g, b = (int(c) for c in rgb)
    out = []
    for c in range(3):
        v = k[4 * c] + ((k[4 * c + 1] * r + k[4 * c + 2] * g + k[4 * c + 3] * b + 32768) >> 16)
        out.append(min(max(v, 0), 255) if clip else v)
    return tuple(out)


# ---- surfaces ---------------------------------------------------------------------------------------------------------
class Surface:
    """B x V NV12 frames of Hs x Ws inside flat uint8 allocations of seeded random bytes.  ``bufs``: one allocation
    (``contiguous``: per frame Hs rows of luma, then Hs/2 rows of chroma, one pitch - the layout of
    Nv12Frames.from_buffer) or two (a plane each, ``lead`` random bytes before the first frame and some behind the last).
    ``y`` / ``uv``: (index into bufs, byte offset)."""

    def __init__(self, B, V, Hs, Ws, y_pad=7, uv_pad=6, y_gap=13, uv_gap=10, lead=(3, 4), contiguous=False, standard=0, seed=0):
        self.B, self.V, self.Hs, self.Ws, self.standard, self.contiguous = B, V, Hs, Ws, standard, contiguous
        rng = np.random.default_rng(1000 + seed)
        F = B * V
        if contiguous:
            pitch = Ws + uv_pad
            self.y_pitch = self.uv_pitch = pitch
            self.y_fs = self.uv_fs = (Hs * 3 // 2) * pitch
            self.y, self.uv = (0, 0), (0, Hs * pitch)
            self.bufs = [rng.integers(0, 256, size=F * self.y_fs, dtype=np.uint8)]
        else:
            self.y_pitch, self.uv_pitch = Ws + y_pad, Ws + uv_pad
            self.y_fs, self.uv_fs = Hs * self.y_pitch + y_gap, (Hs // 2) * self.uv_pitch + uv_gap
            self.y, self.uv = (0, lead[0]), (1, lead[1])
            self.bufs = [rng.integers(0, 256, size=lead[0] + F * self.y_fs + 5, dtype=np.uint8),
                         rng.integers(0, 256, size=lead[1] + F * self.uv_fs + 6, dtype=np.uint8)]
        assert self.uv[1] % 2 == 0 and self.uv_pitch % 2 == 0 and self.uv_fs % 2 == 0

    def y_at(self, f, y, x):
        return self.y[1] + f * self.y_fs + y * self.y_pitch + x

    def uv_at(self, f, cy, cx):
        return self.uv[1] + f * self.uv_fs + cy * self.uv_pitch + 2 * cx

    def planes(self, bufs):
        """(Y [B,V,Hs,Ws], UV [B,V,Hs/2,Ws/2,2]) gathered out of ``bufs`` (copies)."""
        B, V, Hs, Ws = self.B, self.V, self.Hs, self.Ws
        yb, ub = bufs[self.y[0]], bufs[self.uv[0]]
        Y = np.stack([np.stack([yb[self.y_at(f, r, 0):self.y_at(f, r, 0) + Ws] for r in range(Hs)]) for f in range(B * V)])
        U = np.stack([np.stack([ub[self.uv_at(f, r, 0):self.uv_at(f, r, 0) + Ws] for r in range(Hs // 2)]) for f in range(B * V)])
        return Y.reshape(B, V, Hs, Ws), U.reshape(B, V, Hs // 2, Ws // 2, 2)

    def padding(self):
        """Per allocation, the [begin, end) byte ranges no plane byte lies in."""
        used = [np.zeros(len(b), bool) for b in self.bufs]
        for f in range(self.B * self.V):
            for r in range(self.Hs):
                used[self.y[0]][self.y_at(f, r, 0):self.y_at(f, r, 0) + self.Ws] = True
            for r in range(self.Hs // 2):
                used[self.uv[0]][self.uv_at(f, r, 0):self.uv_at(f, r, 0) + self.Ws] = True
        out = []
        for u in used:
            edge = np.flatnonzero(np.diff(np.concatenate([[True], u, [True]]).astype(np.int8)))
            out.append([(int(a), int(e)) for a, e in zip(edge[0::2], edge[1::2])])
        return out


# ---- the yardstick: paint ---------------------------------------------------------------------------------------------
def coverage(case, b, v, n, mut=None):
    """The set of luma pixels (y, x) person n covers in frame (b, v): the rule of fvp_draw_poses, through the yardstick
    geometry of tests/overlay_cases.py."""
    views, conf, s = case["views"], case["conf"], case["surface"]
    J = views.shape[3]
    q = [OC._joint(views, conf, case["conf_min"], b, v, n, j, None) for j in range(J)]
    prims = [(q[j], q[j], case["R"], True) for j in range(J) if q[j] is not None]
    prims += [(q[i], q[k], case["W"], False) for i, k in case["limbs"] if q[i] is not None and q[k] is not None]
    hits = set()
    for a, e, rad, disc in prims:
        for y in OC._reach(min(a[1], e[1]) - rad, max(a[1], e[1]) + rad, s.Hs):
            for x in OC._reach(min(a[0], e[0]) - rad, max(a[0], e[0]) + rad, s.Ws):
                p = (16 * x, 16 * y)
                if OC._disc(p, a, rad, None) if disc else OC._capsule(p, a, e, rad, None):
                    hits.add((y, x))
    return hits


def reference(case, mut=None, counts=None):
    """The allocations after fvp_draw_poses_nv12, as new arrays.  ``counts``: a dict that receives the number of covered
    luma bytes and of quads with any coverage (what the kernel may read)."""
    s = case["surface"]
    bufs = [b.copy() for b in s.bufs]
    yb, ub = bufs[s.y[0]], bufs[s.uv[0]]
    ids, pal, alpha = case["ids"], case["palette"], case["alpha"]
    B, V, N = case["views"].shape[:3]
    half8, half10 = (0, 0) if mut == "no_half" else (128, 512)
    order = range(N - 1, -1, -1) if mut == "descending" else range(N)
    luma_bytes, quads = set(), set()
    for b in range(B):
        for v in range(V):
            f = b * V + v
            for n in order:
                if ids is not None and ids[b, n] < 0:
                    continue
                yc, uc, vc = yuv_of(pal[(int(ids[b, n]) if ids is not None else n) % len(pal)], s.standard)
                if mut == "uv_swapped":
                    uc, vc = vc, uc
                hits = coverage(case, b, v, n)
                k = {}
                for y, x in sorted(hits):
                    at = s.y_at(f, y, x)
                    yb[at] = (yc * alpha + int(yb[at]) * (256 - alpha) + half8) >> 8
                    luma_bytes.add(at)
                    k[(y >> 1, x >> 1)] = k.get((y >> 1, x >> 1), 0) + 1
                for (cy, cx), kn in sorted(k.items()):
                    at = s.uv_at(f, cy, cx)
                    quads.add(at)
                    for c, col in ((0, uc), (1, vc)):
                        old = int(ub[at + c])
                        if mut == "chroma_all_or_nothing":
                            kn = 4
                        if mut == "chroma_top_left":
                            if (2 * cy, 2 * cx) not in hits:
                                continue
                            kn = 4
                        a = alpha * kn
                        if mut == "chroma_per_pixel":
                            for _ in range(kn):
                                old = (col * alpha + old * (256 - alpha) + 128) >> 8
                            ub[at + c] = old
                        elif mut == "shift8":
                            ub[at + c] = ((col * a + old * (1024 - a) + 512) >> 8) & 255
                        else:
                            ub[at + c] = (col * a + old * (1024 - a) + half10) >> 10
    if counts is not None:
        counts["luma"], counts["quads"] = len(luma_bytes), len(quads)
    return bufs


# ---- building cases ---------------------------------------------------------------------------------------------------
def _even(n):
    return n + (n & 1)


def _case(surface, N, J, limbs=(), palette=OC.PAL16, R=80, W=32, alpha=256, conf_min=0.0, ids=None, conf=None):
    return dict(surface=surface, views=np.zeros((surface.B, surface.V, N, J, 4), F32), ids=ids, conf=conf,
                limbs=[list(ab) for ab in limbs], palette=[list(c) for c in palette], R=R, W=W, alpha=alpha, conf_min=conf_min)


def carried_over(name):
    """Case ``name`` of overlay_cases.CASES on an NV12 surface of the same size made even (37 x 150 -> 38 x 150, the 1 x 1
    frame -> 2 x 2), random contents, padded pitches and frame gaps; the standards take turns."""
    i = list(OC.CASES).index(name)
    c = OC.CASES[name]()
    B, V, Hs, Ws = c["frames"].shape[:4]
    c["surface"] = Surface(B, V, _even(Hs), _even(Ws), standard=i % 4, seed=i, y_pad=7 + 2 * (i % 3), uv_pad=6 + 2 * (i % 2))
    del c["frames"]
    if name == "identity_permuted_slots":                        # both batches start from the same picture, as there
        s = c["surface"]
        for r in range(s.Hs):
            s.bufs[0][s.y_at(1, r, 0):s.y_at(1, r, 0) + s.Ws] = s.bufs[0][s.y_at(0, r, 0):s.y_at(0, r, 0) + s.Ws]
        for r in range(s.Hs // 2):
            s.bufs[1][s.uv_at(1, r, 0):s.uv_at(1, r, 0) + s.Ws] = s.bufs[1][s.uv_at(0, r, 0):s.uv_at(0, r, 0) + s.Ws]
    return c


def chroma_quads(alpha, standard=0):
    """Discs of radius 0 (one pixel each) of one person: quads with k = 1 (its bottom-right pixel), 2 (a row), 2 (a
    diagonal), 3 and 4 covered pixels; a second person with k = 1 whose pixel is the top-right one."""
    c = _case(Surface(1, 1, 40, 96, standard=standard, seed=40), 2, 15, R=0, alpha=alpha, palette=OC.PAL3)
    px = [(11, 11), (20, 10), (21, 10), (30, 10), (31, 11), (40, 10), (41, 10), (40, 11), (50, 10), (51, 10), (50, 11), (51, 11)]
    for j, (x, y) in enumerate(px):
        OC._put(c, 0, j, float(x), float(y))
    OC._put(c, 1, 0, 71.0, 20.0)
    return c


QUADS = {1: (5, 5), 2: (5, 10), 3: (5, 20), 4: (5, 25)}          # k -> (cy, cx) of chroma_quads' person 0 (k = 2: the row)


def chroma_disc_edge():
    """One disc of radius 5 pixels around a half-pixel centre at odd coordinates: its edge cuts quads at every k."""
    c = _case(Surface(1, 1, 40, 96, standard=1, seed=41), 1, 15, R=80, alpha=200)
    OC._put(c, 0, 0, 47.5, 19.5)
    OC._put(c, 0, 1, 70.0, 33.0)                                 # crosses the tile borders x = 64 and y = 32
    return c


def chroma_two_persons(alpha=128):
    """Two persons in one quad with different k: person 0 covers its top-right pixel, person 1 three pixels (the shared one
    among them); a second quad the other way round.  The blends do not commute: the slot order shows."""
    c = _case(Surface(1, 1, 40, 96, standard=2, seed=42), 2, 15, R=0, alpha=alpha, palette=[[255, 0, 0], [0, 0, 255]])
    OC._put(c, 0, 0, 31.0, 10.0)
    for j, (x, y) in enumerate([(31, 10), (30, 11), (31, 11)]):
        OC._put(c, 1, j, float(x), float(y))
    for j, (x, y) in enumerate([(60, 20), (61, 20), (61, 21)]):
        OC._put(c, 0, 1 + j, float(x), float(y))
    OC._put(c, 1, 3, 60.0, 21.0)
    return c


def layout(contiguous, B=2, V=2, Hs=40, Ws=96, seed=43):
    """One scene (three people, ids, confidences) on surfaces of different layouts with the same plane contents: 96 x 40 is
    no multiple of the 64 x 16 tile.  Not contiguous: an odd y_pitch, an even uv_pitch, gaps between frames, y at an odd
    address."""
    s = Surface(B, V, Hs, Ws, contiguous=contiguous, standard=3, seed=seed, y_pad=9, uv_pad=12, y_gap=31, uv_gap=18, lead=(5, 2))
    rng = np.random.default_rng(seed)                            # the planes' contents: the same in every layout
    Y, U = rng.integers(0, 256, size=(B * V, Hs, Ws), dtype=np.uint8), rng.integers(0, 256, size=(B * V, Hs // 2, Ws), dtype=np.uint8)
    for f in range(B * V):
        for r in range(Hs):
            s.bufs[s.y[0]][s.y_at(f, r, 0):s.y_at(f, r, 0) + Ws] = Y[f, r]
        for r in range(Hs // 2):
            s.bufs[s.uv[0]][s.uv_at(f, r, 0):s.uv_at(f, r, 0) + Ws] = U[f, r]
    c = _case(s, 3, 17, limbs=OC.LIMBS17, R=40, W=20, alpha=160, ids=np.array([[2, 0, 1], [17, 33, 1]], np.int32)[:B], conf_min=0.2)
    c["views"][:] = _skeleton_views(B, V, 3, 17, Hs, Ws, seed + 1)
    c["conf"] = np.random.default_rng(seed + 2).random((B, 3, 17)).astype(F32)
    return c


def _skeleton_views(B, V, N, J, Hs, Ws, seed, spread=0.6):
    tmp = dict(views=np.zeros((B, V, N, J, 4), F32), frames=np.zeros((B, V, Hs, Ws, 3), np.uint8))
    OC._skeletons(tmp, seed, spread=spread)
    return tmp["views"]


def largest():
    """2 x 2 frames of 160 x 48: three tile columns with a partial one, three whole tile rows."""
    c = layout(False, Hs=48, Ws=160, seed=44)
    return c


def colours(standard, palette=tuple(PALETTE16) + tuple(EXTREMES)):
    """Every colour paints one aligned quad, opaque: person n's four radius-0 discs fill the quad (4 n, 4): the surface then
    holds (Yc, Uc, Vc) itself."""
    P = len(palette)
    c = _case(Surface(1, 1, 16, 96, standard=standard, seed=50 + standard), P, 4, R=0, alpha=256, palette=palette)
    for n in range(P):
        for j in range(4):
            OC._put(c, n, j, float(4 * n + (j & 1)), float(4 + (j >> 1)))
    return c


CASES = {f"carried_{name}": functools.partial(carried_over, name) for name in OC.CASES}
CASES.update({
    "chroma_quads_256": functools.partial(chroma_quads, 256), "chroma_quads_128": functools.partial(chroma_quads, 128),
    "chroma_disc_edge": chroma_disc_edge, "chroma_two_persons": chroma_two_persons,
    "layout_planes": functools.partial(layout, False), "layout_contiguous": functools.partial(layout, True), "largest": largest,
    "colours_0": functools.partial(colours, 0), "colours_1": functools.partial(colours, 1),
    "colours_2": functools.partial(colours, 2), "colours_3": functools.partial(colours, 3),
})
TIE_CASES = ("carried_capsules", "carried_blend_128", "carried_crowd")


@functools.lru_cache(maxsize=None)
def expected(name):
    """(case, reference allocations, counts): computed once and shared; none is modified by a test."""
    case = CASES[name]()
    counts = {}
    want = reference(case, counts=counts)
    for b in want + case["surface"].bufs:
        b.setflags(write=False)
    return case, want, counts


# ---- running the product ----------------------------------------------------------------------------------------------
_dev, _ptr = OC._dev, OC._ptr


def _stream(device):
    return C.c_void_p(torch.cuda.current_stream().cuda_stream) if str(device).startswith("cuda") else None


def call(lib, device, t_bufs, t_views, ids, conf, case, **over):
    """One fvp_draw_poses_nv12 on device tensors; ``over`` replaces arguments (argument-error tests).  Returns the code."""
    s = case["surface"]
    N, J = t_views.shape[2:4]
    a = dict(B=s.B, V=s.V, Hs=s.Hs, Ws=s.Ws, y_pitch=s.y_pitch, uv_pitch=s.uv_pitch, y_fs=s.y_fs, uv_fs=s.uv_fs,
             standard=s.standard, N=N, J=J, L=len(case["limbs"]), P=len(case["palette"]), R=case["R"], W=case["W"],
             alpha=case["alpha"], conf_min=case["conf_min"], limbs=case["limbs"], palette=case["palette"],
             y=t_bufs[s.y[0]].data_ptr() + s.y[1], uv=t_bufs[s.uv[0]].data_ptr() + s.uv[1], views=_ptr(t_views))
    a.update(over)
    flat = [j for ab in a["limbs"] for j in ab] if a["limbs"] is not None else None
    limbs = None if flat is None else (C.c_int32 * max(len(flat), 1))(*flat)
    pal = None if a["palette"] is None else (C.c_uint8 * (3 * len(a["palette"])))(*[v for c in a["palette"] for v in c])
    y, uv = (None if a[k] is None else C.c_void_p(a[k]) for k in ("y", "uv"))
    return lib.fvp_draw_poses_nv12(y, uv, a["B"], a["V"], a["Hs"], a["Ws"], a["y_pitch"], a["uv_pitch"], a["y_fs"], a["uv_fs"],
                                   a["standard"], a["views"], _ptr(ids), _ptr(conf), a["N"], a["J"], limbs, a["L"], pal,
                                   a["P"], a["R"], a["W"], a["alpha"], a["conf_min"], _stream(device))


def run(lib, device, case, fences=None):
    """The allocations after fvp_draw_poses_nv12 on ``device`` as numpy arrays (and, with ``fences`` - per allocation a list
    of [begin, end) byte ranges - the emulator's count of reads inside them)."""
    s = case["surface"]
    bufs = [_dev(b.copy(), device) for b in s.bufs]
    views, ids, conf = _dev(case["views"], device), _dev(case["ids"], device), _dev(case["conf"], device)
    if fences is not None:
        lib.hipemu_fence.argtypes = [C.c_void_p, C.c_size_t]
        lib.hipemu_fenced_reads.restype = C.c_long
        lib.hipemu_fences_clear()
        for t, ranges in zip(bufs, fences):
            for a, e in ranges:
                lib.hipemu_fence(C.c_void_p(t.data_ptr() + a), e - a)
    rc = call(lib, device, bufs, views, ids, conf, case)
    reads = None
    if fences is not None:
        reads = int(lib.hipemu_fenced_reads())
        lib.hipemu_fences_clear()
    assert rc == 0, rc
    if str(device).startswith("cuda"):
        torch.cuda.synchronize()
    out = [t.cpu().numpy() for t in bufs]
    return (out, reads) if fences is not None else out


def changed_bytes(case, want):
    return sum(int((w != b).sum()) for w, b in zip(want, case["surface"].bufs))


def check_case(lib, device, name):
    case, want, counts = expected(name)
    got = run(lib, device, case)
    for i, (g, w) in enumerate(zip(got, want)):
        bad = int((g != w).sum())
        assert bad == 0, f"{name}: {bad} of {w.size} bytes of allocation {i} differ from the yardstick (first at {int(np.flatnonzero(g != w)[0])})"
    base = name[len("carried_"):] if name.startswith("carried_") else None
    unchanged = base in ("limb_wholly_outside", "nothing_drawable")
    if unchanged:
        assert changed_bytes(case, want) == 0 and counts["luma"] == counts["quads"] == 0
    else:
        assert changed_bytes(case, want) > 0 and counts["luma"] > 0, f"{name}: the case draws nothing"
    if base == "identity_permuted_slots":
        Y, U = case["surface"].planes(got)
        assert np.array_equal(Y[0], Y[1]) and np.array_equal(U[0], U[1])


def check_tie_to_rgb(lib, device, name):
    """The Y plane after fvp_draw_poses_nv12 equals channel 0 after fvp_draw_poses on an RGB frame whose channel 0 holds the
    same luma and whose palette entries are (Yc, Yc, Yc): the two kernels share their coverage.  No yardstick paint."""
    case, _, _ = expected(name)
    s = case["surface"]
    Y = s.planes(run(lib, device, case))[0]
    luma = s.planes(s.bufs)[0]
    rng = np.random.default_rng(7)
    frames = np.stack([luma, rng.integers(0, 256, luma.shape, dtype=np.uint8), rng.integers(0, 256, luma.shape, dtype=np.uint8)], -1)
    grey = [[yuv_of(c, s.standard)[0]] * 3 for c in case["palette"]]
    rgb = OC.run(lib, device, dict(case, frames=frames, palette=grey))
    assert np.array_equal(rgb[..., 0], Y) and not np.array_equal(Y, luma)


def check_layouts_agree(lib, device):
    """A contiguous from_buffer surface and separately allocated, padded planes with the same contents: the same planes
    after the call."""
    ca, cb = expected("layout_planes")[0], expected("layout_contiguous")[0]
    pa, pb = ca["surface"].planes(run(lib, device, ca)), cb["surface"].planes(run(lib, device, cb))
    assert np.array_equal(pa[0], pb[0]) and np.array_equal(pa[1], pb[1])
    assert not np.array_equal(pa[0], ca["surface"].planes(ca["surface"].bufs)[0])


def check_colours(lib, device, standard):
    """The quads of ``colours`` hold the yardstick's (Yc, Uc, Vc) of the 16 default colours, black, white, pure R, G, B."""
    case, want, _ = expected(f"colours_{standard}")
    Y, U = case["surface"].planes(run(lib, device, case))
    for n, rgb in enumerate(case["palette"]):
        yc, uc, vc = yuv_of(rgb, standard)
        assert (Y[0, 0, 4:6, 4 * n:4 * n + 2] == yc).all() and tuple(U[0, 0, 2, 2 * n]) == (uc, vc), (standard, rgb)


def check_round_trip(lib, device, standard):
    """``colours`` drawn, then read back through fvp_ingest_nv12 with the identity transform, mean 0 and std 1: the pixels of
    the painted quads come back within 2 / 255 of the palette's RGB on every channel (the measured maximum of the two
    integer conversions over the 16 default colours: 1, 1, 2, 1 for the four standards)."""
    case = CASES[f"colours_{standard}"]()
    case["palette"] = case["palette"][:16]
    case["views"] = case["views"][:, :, :16].copy()
    s = case["surface"]
    bufs = [_dev(b.copy(), device) for b in s.bufs]
    assert call(lib, device, bufs, _dev(case["views"], device), None, None, case) == 0
    out = torch.zeros((1, 3, s.Hs, s.Ws), dtype=torch.float32, device=device)
    f3 = lambda *v: (C.c_float * len(v))(*v)                                      # noqa: E731
    rc = lib.fvp_ingest_nv12(C.c_void_p(bufs[s.y[0]].data_ptr() + s.y[1]), C.c_void_p(bufs[s.uv[0]].data_ptr() + s.uv[1]), 1,
                             s.Hs, s.Ws, s.y_pitch, s.uv_pitch, s.y_fs, s.uv_fs, standard, f3(1, 0, 0, 0, 1, 0), f3(0, 0, 0),
                             f3(1, 1, 1), s.Hs, s.Ws, None, _ptr(out), _stream(device))
    assert rc == 0, rc
    if str(device).startswith("cuda"):
        torch.cuda.synchronize()
    back = np.rint(out.cpu().numpy()[0] * 255.0).astype(int)                       # [3, Hs, Ws]
    worst = 0
    for n, rgb in enumerate(case["palette"]):
        quad = back[:, 4:6, 4 * n:4 * n + 2]
        worst = max(worst, int(np.abs(quad - np.array(rgb).reshape(3, 1, 1)).max()))
    print(f"round trip, standard {standard}: worst channel error {worst} / 255")
    assert worst <= 2, worst


# ---- argument errors --------------------------------------------------------------------------------------------------
# (what is wrong, expected code); every call must leave the allocations untouched
ARGUMENT_ERRORS = [
    # those of fvp_draw_poses
    (dict(y=None), EINVAL), (dict(uv=None), EINVAL), (dict(views=None), EINVAL), (dict(palette=None), EINVAL),
    (dict(limbs=None), EINVAL), (dict(B=-1), EINVAL), (dict(V=-1), EINVAL), (dict(N=0), EINVAL), (dict(J=0), EINVAL),
    (dict(Hs=0), EINVAL), (dict(Ws=0), EINVAL), (dict(P=0), EINVAL), (dict(L=-1), EINVAL), (dict(limbs=[[0, 15]], L=1), EINVAL),
    (dict(limbs=[[-1, 2]], L=1), EINVAL), (dict(alpha=0), EINVAL), (dict(alpha=257), EINVAL), (dict(R=-1), EINVAL),
    (dict(R=1025), EINVAL), (dict(W=-1), EINVAL), (dict(W=1025), EINVAL), (dict(conf_min=OC.NAN), EINVAL),
    (dict(N=33), ELIMIT), (dict(J=33, limbs=[], L=0), ELIMIT), (dict(V=9), ELIMIT),
    (dict(L=65, limbs=[[0, 1]] * 65), ELIMIT), (dict(P=65, palette=[[1, 2, 3]] * 65), ELIMIT),
    (dict(Hs=16386, y_fs=1 << 30, uv_fs=1 << 30), ELIMIT), (dict(Ws=16386, y_pitch=16386, uv_pitch=16386), ELIMIT),
    (dict(B=8192, V=8), ELIMIT),
    # those of the surface
    (dict(Hs=39), EINVAL), (dict(Ws=95), EINVAL), (dict(y_pitch=95), EINVAL), (dict(uv_pitch=94), EINVAL),
    (dict(uv_pitch=103), EINVAL), (dict(uv_fs=2051), EINVAL), (dict(uv="odd"), EINVAL), (dict(standard=4), EINVAL),
    (dict(standard=-1), EINVAL), (dict(y_fs=39 * 103 + 95), EINVAL), (dict(uv_fs=19 * 102 + 94), EINVAL),
    (dict(y_fs=0), EINVAL), (dict(uv_fs=-2), EINVAL),
]


def case_argument_errors(lib, device):
    """Every error of include/fvp.h: the code comes back and the surface - its joints all drawable - keeps its bytes.  No
    launch happens, so arguments over their limit are never used to address memory."""
    s = Surface(1, 2, 40, 96, seed=60)
    assert (s.y_pitch, s.uv_pitch) == (103, 102)
    case = _case(s, 1, 15, limbs=OC.LIMBS15)
    case["views"][:] = _skeleton_views(1, 2, 1, 15, 40, 96, 170, spread=0.4)
    case["views"][..., 2] = 1.0
    bufs, views = [_dev(b.copy(), device) for b in s.bufs], _dev(case["views"], device)
    for over, code in ARGUMENT_ERRORS:
        if over.get("uv") == "odd":
            over = dict(uv=bufs[s.uv[0]].data_ptr() + s.uv[1] + 1)
        rc = call(lib, device, bufs, views, None, None, case, **over)
        assert rc == code, f"{over}: returned {rc}, expected {code}"
    for over in (dict(B=0), dict(V=0)):                                  # nothing to do: 0, no launch
        assert call(lib, device, bufs, views, None, None, case, **over) == 0
    # a single frame needs no frame stride at all
    one = dict(case, views=case["views"][:, :1].copy())
    if str(device).startswith("cuda"):
        torch.cuda.synchronize()
    assert all(np.array_equal(t.cpu().numpy(), b) for t, b in zip(bufs, s.bufs))
    assert call(lib, device, bufs, _dev(one["views"], device), None, None, one, V=1, y_fs=0, uv_fs=0) == 0
    assert call(lib, device, bufs, views, None, None, case) == 0          # and the same arguments, valid, do draw
    assert any(not np.array_equal(t.cpu().numpy(), b) for t, b in zip(bufs, s.bufs))


# ---- Nv12Frames over a Surface ------------------------------------------------------------------------------------------
def nv12_frames(surface, t_bufs):
    """The product's Nv12Frames [B,V] over the tensors ``t_bufs`` that hold ``surface.bufs`` (views, no copy)."""
    from faster_voxelpose_amd.dataset.images import Nv12Frames
    s = surface
    kr_name = "bt601" if s.standard in (0, 2) else "bt709"
    if s.contiguous:
        buf = t_bufs[0].view(s.B, s.V, s.Hs * 3 // 2, s.y_pitch)
        return Nv12Frames.from_buffer(buf, s.Hs, s.Ws, standard=kr_name, full_range=s.standard >= 2)
    y = t_bufs[0].as_strided((s.B, s.V, s.Hs, s.Ws), (s.V * s.y_fs, s.y_fs, s.y_pitch, 1), s.y[1])
    uv = t_bufs[1].as_strided((s.B, s.V, s.Hs // 2, s.Ws // 2, 2), (s.V * s.uv_fs, s.uv_fs, s.uv_pitch, 2, 1), s.uv[1])
    return Nv12Frames(y, uv, standard=kr_name, full_range=s.standard >= 2)
