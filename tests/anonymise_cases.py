"""Cases and the yardstick of fvp_anonymise_rois and fvp_anonymise_rois_nv12 (include/fvp.h, ABI 23), shared by
tests/test_anonymise_emu.py (CPU emulator) and tests/test_anonymise_gpu.py (the shipped library on the card): an independent
numpy restatement of the header's text - coverage in float32, operation by operation (numpy float32 arrays and scalars round
every result to float32), the cell means in int64 - over seeded frames and pitched NV12 surfaces that sit in guarded, poisoned
allocations; the wrong readings of the definition (mutants) the case set must tell apart; and a runner that calls the entry
points on torch memory (CPU for the emulator, the card otherwise).  Whole allocations are compared byte for byte - guards,
pitch padding and the gaps between frames included: no tolerance anywhere."""
import ctypes as C

import numpy as np
import torch

f32 = np.float32
NAN, INF = float("nan"), float("inf")
EINVAL, ELIMIT = 10001, 10002
RECT, ELLIPSE, MOSAIC, FILL = 0, 1, 0, 1
CELLS = (2, 4, 8, 16, 32)
TILE_W, TILE_H = 64, 32                                  # what one workgroup owns (include/fvp.h)
GUARD = 64                                               # poisoned bytes in front of and behind every plane
MUTANTS = ("no_half", "box_anchored", "covered_mean", "trunc_mean", "x1_inclusive", "wrong_frame", "chroma_topleft")
# standard -> (YOFF, CYR, CYG, CYB, UOFF, CUR, CUG, CUB, VOFF, CVR, CVG, CVB): the FVP_RGB2YUV_* tables of include/fvp.h
RGB2YUV = {0: (16, 16829, 33039, 6416, 128, -9714, -19071, 28784, 128, 28784, -24103, -4681),
           1: (16, 11966, 40254, 4064, 128, -6596, -22189, 28784, 128, 28784, -26145, -2639),
           2: (0, 19595, 38470, 7471, 128, -11058, -21710, 32768, 128, 32768, -27439, -5329),
           3: (0, 13933, 46871, 4732, 128, -7509, -25259, 32768, 128, 32768, -29763, -3005)}
BEYOND = float(np.nextafter(f32(65536), f32(INF)))       # one step beyond the bound of an active ROI

# The boxes, for frames of 38 x 70 (two tiles each way): name -> (x0, y0, x1, y1)
BOXES = {
    "inside_cell": (16.2, 8.1, 17.9, 9.9),                # pixels 16..17 x 8..9: inside one cell of every size
    "across_tile": (58.3, 27.6, 69.2, 35.4),              # over x = 64 and y = 32, the tile borders
    "over_left": (-5.5, 12.0, 3.4, 20.0),
    "over_top": (30.0, -4.0, 41.0, 2.6),
    "over_right": (66.5, 5.0, 75.0, 12.0),
    "over_bottom": (20.0, 33.3, 29.0, 45.0),
    "outside_right": (80.0, 5.0, 90.0, 15.0),
    "outside_above": (10.0, -40.0, 20.0, -21.0),
    "outside_far": (60000.0, 60000.0, 65000.0, 65000.0),
    "x1_eq_x0": (5.0, 5.0, 5.0, 9.0),
    "x1_lt_x0": (9.0, 5.0, 5.0, 9.0),
    "y1_eq_y0": (5.0, 7.0, 9.0, 7.0),
    "nan": (NAN, 1.0, 5.0, 9.0),
    "nan_y1": (1.0, 1.0, 5.0, NAN),
    "inf": (1.0, 1.0, INF, 9.0),
    "minus_inf": (1.0, -INF, 5.0, 9.0),
    "zeros": (0.0, 0.0, 0.0, 0.0),                         # an invalid box of fvp_person_rois
    "at_bound": (-65536.0, 23.2, 2.7, 26.1),               # |x0| == 65536: active
    "beyond_bound": (-BEYOND, 28.2, 2.7, 31.1),            # one step more: inactive
    "on_centres": (40.5, 20.5, 43.5, 22.5),                # x0 on a pixel centre (<=: in), x1 on one (<: out)
    "ellipse_exact": (30.5, 10.5, 40.5, 16.5),             # centre (35.5, 13.5), hw 5, hh 3: (40.5, 13.5) lies ON the ellipse
    "overlap_a": (44.3, 3.2, 56.8, 12.9),
    "overlap_b": (50.1, 8.4, 62.7, 18.2),
    "inner": (8.0, 22.0, 15.0, 30.0),
}
INACTIVE = ("x1_eq_x0", "x1_lt_x0", "y1_eq_y0", "nan", "nan_y1", "inf", "minus_inf", "zeros", "beyond_bound")
NOTHING = INACTIVE + ("outside_right", "outside_above", "outside_far")
ZERO_BOX = (0.0, 0.0, 0.0, 0.0)
TINY_BOX = (0.0, 0.0, 1e-25, 1e-25)                      # hw * hw and hh * hh underflow to 0: the ellipse test reads 0 <= 0


def active(roi):
    """Active ROI of include/fvp.h, in float32."""
    v = np.array(roi, f32)
    with np.errstate(invalid="ignore"):
        return bool(np.all(np.abs(v) <= f32(65536))) and bool(v[2] > v[0]) and bool(v[3] > v[1])


def ellipse_sides(roi, x, y):
    """(lhs, rhs) of the ellipse test for pixel (x, y), float32 scalars, operation by operation."""
    x0, y0, x1, y1 = (f32(t) for t in roi)
    cx, hw = f32(f32(x0 + x1) * f32(0.5)), f32(f32(x1 - x0) * f32(0.5))
    cy, hh = f32(f32(y0 + y1) * f32(0.5)), f32(f32(y1 - y0) * f32(0.5))
    dx, dy = f32(f32(f32(x) + f32(0.5)) - cx), f32(f32(f32(y) + f32(0.5)) - cy)
    hw2, hh2 = f32(hw * hw), f32(hh * hh)
    return f32(f32(f32(dx * dx) * hh2) + f32(f32(dy * dy) * hw2)), f32(hw2 * hh2)


def roi_coverage(roi, hs, ws, shape, mutant=None):
    """bool [hs,ws]: the pixels one ROI covers."""
    if not active(roi):
        return np.zeros((hs, ws), bool)
    x0, y0, x1, y1 = (f32(t) for t in roi)
    half = f32(0.0 if mutant == "no_half" else 0.5)
    xc, yc = np.arange(ws, dtype=f32)[None, :] + half, np.arange(hs, dtype=f32)[:, None] + half
    with np.errstate(under="ignore"):
        if shape == RECT:
            right = (xc <= x1) if mutant == "x1_inclusive" else (xc < x1)
            return (x0 <= xc) & right & (y0 <= yc) & (yc < y1)
        cx, hw = f32(f32(x0 + x1) * f32(0.5)), f32(f32(x1 - x0) * f32(0.5))
        cy, hh = f32(f32(y0 + y1) * f32(0.5)), f32(f32(y1 - y0) * f32(0.5))
        dx, dy = xc - cx, yc - cy
        hw2, hh2 = f32(hw * hw), f32(hh * hh)
        lhs = ((dx * dx) * hh2) + ((dy * dy) * hw2)
        assert lhs.dtype == f32 and lhs.shape == (hs, ws)
        if mutant == "x1_inclusive":                       # the ellipse has no exclusive edge: its equality case instead
            return lhs < f32(hw2 * hh2)
        return lhs <= f32(hw2 * hh2)


def frame_rois(c, f, mutant=None):
    rpf, F = c["rpf"], c["F"]
    if mutant == "wrong_frame":                            # ROI r read as belonging to frame r % F
        return [c["rois"][r] for r in range(F * rpf) if r % F == f]
    return list(c["rois"][f * rpf:(f + 1) * rpf])


def coverage(c, mutant=None):
    """bool [F,hs,ws]: the union over every frame's ROIs."""
    cov = np.zeros((c["F"], c["hs"], c["ws"]), bool)
    for f in range(c["F"]):
        for roi in frame_rois(c, f, mutant):
            cov[f] |= roi_coverage(roi, c["hs"], c["ws"], c["shape"], mutant)
    return cov


def _mean(vals, mutant):
    S, n = int(np.sum(vals, dtype=np.int64)), int(vals.size)
    return S // n if mutant == "trunc_mean" else (2 * S + n) // (2 * n)


def _mosaic_plane(src, pcov, cell, mutant, origin=(0, 0)):
    """One channel [h,w] (read-only original) -> its mosaic where ``pcov`` (the plane's own covered samples) says so; a cell is
    touched iff it holds a covered sample.  Returns (out, touched samples bool [h,w])."""
    h, w = src.shape
    out, read = src.copy(), np.zeros((h, w), bool)
    oy, ox = origin
    for j0 in range(oy - cell if oy else 0, h, cell):
        for i0 in range(ox - cell if ox else 0, w, cell):
            ys, xs = slice(max(j0, 0), min(j0 + cell, h)), slice(max(i0, 0), min(i0 + cell, w))
            k = pcov[ys, xs]
            if not k.any():
                continue
            read[ys, xs] = True
            block = src[ys, xs]
            m = _mean(block[k] if mutant == "covered_mean" else block, mutant)
            out[ys, xs][k] = m
    return out, read


def yuv_of(colour, standard):
    k = RGB2YUV[standard]
    r, g, b = (int(t) for t in colour)
    return tuple(min(255, max(0, k[4 * i] + ((k[4 * i + 1] * r + k[4 * i + 2] * g + k[4 * i + 3] * b + 32768) >> 16))) for i in range(3))


def reference(c, mutant=None):
    """(expected allocations, loads, bytes a kernel may read per allocation) of a case by the definition.  ``loads``: one per
    RGB pixel, luma byte and (U, V) pair of a touched cell."""
    bufs = [b.copy() for b in c["bufs"]]
    may_read = [np.zeros(len(b), bool) for b in bufs]
    cov = coverage(c, mutant)
    loads = 0
    F, hs, ws, cell = c["F"], c["hs"], c["ws"], c["cell"]
    if c["kind"] == "rgb":
        src, dst = rgb_view(c, c["bufs"]), rgb_view(c, bufs)
        rd = rgb_view(c, may_read)
        for f in range(F):
            if c["mode"] == FILL:
                dst[f][cov[f]] = c["colour"]
                continue
            if mutant == "box_anchored":                   # cells anchored at each box's corner, box after box
                for roi in frame_rois(c, f):
                    k = roi_coverage(roi, hs, ws, c["shape"])
                    if k.any():
                        org = (int(np.floor(roi[1])) % cell, int(np.floor(roi[0])) % cell)
                        for ch in range(3):
                            dst[f, :, :, ch] = _mosaic_plane(dst[f, :, :, ch].copy(), k, cell, None, org)[0]
                continue
            for ch in range(3):
                dst[f, :, :, ch], read = _mosaic_plane(src[f, :, :, ch], cov[f], cell, mutant)
            rd[f][read] = True
            loads += int(read.sum())
        return bufs, loads, may_read
    (sy, suv), (dy, duv), (ry, ruv) = nv12_views(c, c["bufs"]), nv12_views(c, bufs), nv12_views(c, may_read)
    for f in range(F):
        k = cov[f]
        pair = k[0::2, 0::2] if mutant == "chroma_topleft" else k[0::2, 0::2] | k[0::2, 1::2] | k[1::2, 0::2] | k[1::2, 1::2]
        if c["mode"] == FILL:
            yc, uc, vc = yuv_of(c["colour"], c["standard"])
            dy[f][k] = yc
            duv[f][pair] = (uc, vc)
            continue
        dy[f], read = _mosaic_plane(sy[f], k, cell, mutant)
        ry[f][read] = True
        loads += int(read.sum())
        full = k[0::2, 0::2] | k[0::2, 1::2] | k[1::2, 0::2] | k[1::2, 1::2]      # a chroma cell is read iff its luma cell is touched
        for ch in range(2):
            duv[f, :, :, ch], read = _mosaic_plane(suv[f, :, :, ch], full, cell // 2, mutant)
            if mutant == "chroma_topleft":
                duv[f, :, :, ch][~pair] = suv[f, :, :, ch][~pair]
        ruv[f][read] = True
        loads += int(read.sum())
    return bufs, loads, may_read


# ---- layouts -----------------------------------------------------------------------------------------------------------
def rgb_view(c, bufs):
    F, hs, ws = c["F"], c["hs"], c["ws"]
    return bufs[0][GUARD:GUARD + F * hs * ws * 3].reshape(F, hs, ws, 3)


def nv12_views(c, bufs):
    """Strided numpy views [F,hs,ws] and [F,hs/2,ws/2,2] of the allocations (writable); bool masks work as well."""
    st = np.lib.stride_tricks.as_strided
    y = st(bufs[c["y"][0]][c["y"][1]:], (c["F"], c["hs"], c["ws"]), (c["y_fs"], c["y_pitch"], 1))
    uv = st(bufs[c["uv"][0]][c["uv"][1]:], (c["F"], c["hs"] // 2, c["ws"] // 2, 2), (c["uv_fs"], c["uv_pitch"], 2, 1))
    return y, uv


def _case(kind, cell, shape, mode, rpf, per_frame, seed, hs=38, ws=70, colour=(0, 0, 0), standard=0, y_pitch=None,
          uv_pitch=None, split=False, gap=0):
    """``per_frame``: for every frame the names (or tuples) of its boxes; padded to ``rpf`` with all-zero boxes."""
    F = len(per_frame)
    rois = []
    for names in per_frame:
        boxes = [BOXES[n] if isinstance(n, str) else n for n in names]
        assert len(boxes) <= rpf
        rois += boxes + [ZERO_BOX] * (rpf - len(boxes))
    c = dict(kind=kind, cell=cell, shape=shape, mode=mode, rpf=rpf, F=F, hs=hs, ws=ws, colour=tuple(colour), standard=standard,
             rois=np.array(rois, f32), seed=seed)
    rng = np.random.default_rng([seed, hs, ws, cell])
    if kind == "rgb":
        buf = rng.integers(0, 256, size=2 * GUARD + F * hs * ws * 3, dtype=np.uint8)
        c["bufs"] = [buf]
        return c
    yp, up = y_pitch or ws, uv_pitch or ws
    c["y_pitch"], c["uv_pitch"] = yp, up
    ylen, uvlen = hs * yp, (hs // 2) * up
    if split:                                              # planes in allocations of their own, an odd luma frame stride
        c["y_fs"], c["uv_fs"] = ylen + gap + 1, uvlen + gap
        sizes = [2 * GUARD + F * c["y_fs"], 2 * GUARD + F * c["uv_fs"]]
        c["y"], c["uv"] = (0, GUARD), (1, GUARD)
    else:                                                  # one buffer: a frame's chroma rows behind its luma rows
        off = ylen + (ylen & 1)                            # chroma at an even address
        c["y_fs"] = c["uv_fs"] = off + uvlen + gap
        assert c["y_fs"] % 2 == 0
        sizes = [2 * GUARD + F * c["y_fs"]]
        c["y"], c["uv"] = (0, GUARD), (0, GUARD + off)
    c["bufs"] = [rng.integers(0, 256, size=n, dtype=np.uint8) for n in sizes]
    return c


def used_bytes(c):
    """Per allocation, bool: the bytes that belong to a pixel of some frame (everything else is guard, padding or gap)."""
    used = [np.zeros(len(b), bool) for b in c["bufs"]]
    if c["kind"] == "rgb":
        rgb_view(c, used)[...] = True
    else:
        y, uv = nv12_views(c, used)
        y[...] = True
        uv[...] = True
    return used


def runs(mask):
    """[begin, end) runs of True in a bool vector."""
    edges = np.flatnonzero(np.diff(np.concatenate([[False], mask, [False]]).astype(np.int8)))
    return [(int(a), int(e)) for a, e in zip(edges[::2], edges[1::2])]


def forbidden_fences(may_read):
    """The emulator's fence counts a load at address p when [p, p + 4) meets the fenced range: a fence that begins three
    bytes into a run of bytes that must not be loaded counts every load that starts in the run and none that starts in front
    of it.  Runs of up to three bytes cannot be fenced."""
    return [[(a + 3, e) for a, e in runs(~m) if e - a > 3] for m in may_read]


FOUR = ("inside_cell", "across_tile", "over_left"), ("over_top", "over_right", "over_bottom"), \
       ("on_centres", "ellipse_exact", "overlap_a"), ("overlap_b", "overlap_a", "at_bound")
ALL = list(BOXES)


def _quarters():
    """Four frames for rois_per_frame = 64: frame f holds every box but each fourth (another quarter per frame)."""
    return [[n for i, n in enumerate(ALL) if i % 4 != f] for f in range(4)]


BUILDERS = {
    # RGB, frames of 38 x 70: every cell size, both shapes, rois_per_frame 1, 3 and 64
    "rgb_c2_rect_r3": lambda: _case("rgb", 2, RECT, MOSAIC, 3, FOUR, 1),
    "rgb_c4_ellipse_r3": lambda: _case("rgb", 4, ELLIPSE, MOSAIC, 3, FOUR, 2),
    "rgb_c8_rect_r64": lambda: _case("rgb", 8, RECT, MOSAIC, 64, _quarters(), 3),
    "rgb_c8_ellipse_r3": lambda: _case("rgb", 8, ELLIPSE, MOSAIC, 3, FOUR, 4),
    "rgb_c16_ellipse_r1": lambda: _case("rgb", 16, ELLIPSE, MOSAIC, 1, [["across_tile"], ["ellipse_exact"], ["zeros"], ["over_left"]], 5),
    "rgb_c16_rect_r3": lambda: _case("rgb", 16, RECT, MOSAIC, 3, FOUR, 6),
    "rgb_c32_rect_r3": lambda: _case("rgb", 32, RECT, MOSAIC, 3, FOUR, 7),
    "rgb_c32_ellipse_r64": lambda: _case("rgb", 32, ELLIPSE, MOSAIC, 64, _quarters(), 8),
    "rgb_fill_rect_r3": lambda: _case("rgb", 8, RECT, FILL, 3, FOUR, 9, colour=(200, 30, 90)),
    "rgb_fill_ellipse_r64": lambda: _case("rgb", 2, ELLIPSE, FILL, 64, _quarters(), 10, colour=(1, 255, 0)),
    # a frame smaller than a cell
    "rgb_small_c32": lambda: _case("rgb", 32, ELLIPSE, MOSAIC, 1, [[(1.0, 0.5, 8.5, 5.0)], [ZERO_BOX], [(-3.0, 2.0, 4.0, 9.0)], [(2.2, 1.1, 3.9, 2.6)]], 11, hs=6, ws=10),
    # nothing to do: every box inactive or wholly outside
    "rgb_nothing": lambda: _case("rgb", 8, RECT, MOSAIC, 3, [NOTHING[0:3], NOTHING[3:6], NOTHING[6:9], NOTHING[9:12]], 12),
    "rgb_inactive": lambda: _case("rgb", 8, ELLIPSE, MOSAIC, 3, [INACTIVE[0:3], INACTIVE[3:6], INACTIVE[6:9], ["zeros"]], 13),
    # hw * hw == hh * hh == 0: the ellipse test, taken literally, covers the whole frame (frame 1 only)
    "rgb_underflow": lambda: _case("rgb", 8, ELLIPSE, MOSAIC, 1, [["inner"], [TINY_BOX], ["zeros"], ["inside_cell"]], 14),
    # NV12, 38 x 70: an odd luma pitch, a frame stride with a gap; planes in one buffer and in two
    "nv12_c2_ellipse_r3": lambda: _case("nv12", 2, ELLIPSE, MOSAIC, 3, FOUR, 21, y_pitch=77, uv_pitch=78, gap=6),
    "nv12_c4_rect_r3_planes": lambda: _case("nv12", 4, RECT, MOSAIC, 3, FOUR, 22, standard=1, y_pitch=75, uv_pitch=72, split=True, gap=38),
    "nv12_c8_rect_r3": lambda: _case("nv12", 8, RECT, MOSAIC, 3, FOUR, 23, standard=2, y_pitch=77, uv_pitch=78, gap=6),
    "nv12_c8_ellipse_r64_planes": lambda: _case("nv12", 8, ELLIPSE, MOSAIC, 64, _quarters(), 24, standard=3, y_pitch=71, uv_pitch=74, split=True, gap=10),
    "nv12_c16_ellipse_r1": lambda: _case("nv12", 16, ELLIPSE, MOSAIC, 1, [["across_tile"], ["ellipse_exact"], ["zeros"], ["over_left"]], 25, y_pitch=77, uv_pitch=78, gap=2),
    "nv12_c32_rect_r64_planes": lambda: _case("nv12", 32, RECT, MOSAIC, 64, _quarters(), 26, y_pitch=73, uv_pitch=70, split=True, gap=4),
    "nv12_c32_ellipse_r3": lambda: _case("nv12", 32, ELLIPSE, MOSAIC, 3, FOUR, 27, y_pitch=70, uv_pitch=70),
    # FILL under the four standards; pure blue / pure red reach 256 in full range: the clip
    "nv12_fill_601l": lambda: _case("nv12", 8, ELLIPSE, FILL, 3, FOUR, 31, colour=(200, 30, 90), standard=0, y_pitch=77, uv_pitch=78, gap=6),
    "nv12_fill_709l_planes": lambda: _case("nv12", 8, RECT, FILL, 3, FOUR, 32, colour=(12, 250, 77), standard=1, y_pitch=75, uv_pitch=72, split=True, gap=38),
    "nv12_fill_601f": lambda: _case("nv12", 8, RECT, FILL, 64, _quarters(), 33, colour=(0, 0, 255), standard=2, y_pitch=77, uv_pitch=78, gap=6),
    "nv12_fill_709f_planes": lambda: _case("nv12", 8, ELLIPSE, FILL, 3, FOUR, 34, colour=(255, 0, 0), standard=3, y_pitch=71, uv_pitch=74, split=True, gap=10),
    "nv12_small_c32": lambda: _case("nv12", 32, RECT, MOSAIC, 1, [[(1.0, 0.5, 8.5, 5.0)], [ZERO_BOX], [(-3.0, 2.0, 4.0, 9.0)], [(2.2, 1.1, 3.9, 2.6)]], 35, hs=6, ws=10, y_pitch=11, uv_pitch=12, gap=2),
    "nv12_inactive": lambda: _case("nv12", 8, ELLIPSE, MOSAIC, 3, [INACTIVE[0:3], INACTIVE[3:6], INACTIVE[6:9], ["zeros"]], 36, y_pitch=77, uv_pitch=78, gap=6),
}
CASES = list(BUILDERS)
_cache = {}


def case(name):
    """(case, (expected allocations, loads, bytes that may be read)) - computed once, shared, never modified."""
    if name not in _cache:
        c = BUILDERS[name]()
        _cache[name] = (c, reference(c))
    return _cache[name]


def reversed_rois(c):
    """The same case with every frame's ROI list in reversed order."""
    r = dict(c)
    r["rois"] = c["rois"].reshape(c["F"], c["rpf"], 4)[:, ::-1].reshape(-1, 4).copy()
    return r


def permuted_within_cells(c, seed=99):
    """An RGB case whose source pixels are shuffled inside every frame-anchored cell (whole pixels, all three channels)."""
    assert c["kind"] == "rgb"
    p = dict(c)
    p["bufs"] = [c["bufs"][0].copy()]
    v = rgb_view(p, p["bufs"])
    rng = np.random.default_rng(seed)
    cell = c["cell"]
    for f in range(c["F"]):
        for j0 in range(0, c["hs"], cell):
            for i0 in range(0, c["ws"], cell):
                block = v[f, j0:j0 + cell, i0:i0 + cell]
                flat = block.reshape(-1, 3)
                v[f, j0:j0 + cell, i0:i0 + cell] = flat[rng.permutation(len(flat))].reshape(block.shape)
    return p


# ---- runner ------------------------------------------------------------------------------------------------------------
def _dev(a, device):
    t = torch.from_numpy(np.ascontiguousarray(a).copy())
    return t if str(device) == "cpu" else t.to(device)


def _ptr(t, off=0):
    return C.c_void_p(t.data_ptr() + off)


def _stream(device):
    return C.c_void_p(torch.cuda.current_stream().cuda_stream) if str(device).startswith("cuda") else None


def _fence(lib, ranges_per_buf, bufs):
    lib.hipemu_fence.argtypes = [C.c_void_p, C.c_size_t]
    lib.hipemu_fenced_reads.restype = C.c_long
    lib.hipemu_fences_clear()
    for t, ranges in zip(bufs, ranges_per_buf):
        for a, e in ranges:
            lib.hipemu_fence(C.c_void_p(t.data_ptr() + a), e - a)


def call(lib, device, c, fences=None, **over):
    """fvp_anonymise_rois / fvp_anonymise_rois_nv12 on ``device``: (rc, the allocations afterwards as numpy[, fenced loads]).
    ``over`` replaces arguments (the error tests)."""
    a = dict(c)
    a.update(over)
    bufs = [_dev(b, device) for b in c["bufs"]]
    rois = _dev(c["rois"], device)
    col = None if a.get("null_colour") else (C.c_uint8 * 3)(*a["colour"])
    tail = (None if a.get("null_rois") else _ptr(rois), a.get("R", len(c["rois"])), a["rpf"], a["cell"], a["shape"], a["mode"], col,
            _stream(device))
    if fences is not None:
        _fence(lib, fences, bufs)
    if c["kind"] == "rgb":
        rc = lib.fvp_anonymise_rois(None if a.get("null_frames") else _ptr(bufs[0], GUARD), a["F"], a["hs"], a["ws"], *tail)
    else:
        rc = lib.fvp_anonymise_rois_nv12(None if a.get("null_frames") else _ptr(bufs[c["y"][0]], c["y"][1]),
                                         None if a.get("null_uv") else _ptr(bufs[c["uv"][0]], c["uv"][1] + a.get("uv_shift", 0)),
                                         a["F"], a["hs"], a["ws"], a["y_pitch"], a["uv_pitch"], a["y_fs"], a["uv_fs"],
                                         a["standard"], *tail)
    if str(device).startswith("cuda"):
        torch.cuda.synchronize()
    res = (rc, [t.cpu().numpy() for t in bufs])
    if fences is not None:
        res += (int(lib.hipemu_fenced_reads()),)
        lib.hipemu_fences_clear()
    return res


def same(got, want):
    return len(got) == len(want) and all(np.array_equal(g, w) for g, w in zip(got, want))


def check(lib, device, name):
    """Every allocation equals the yardstick's, byte for byte: the covered pixels hold the definition's values and nothing
    else - uncovered pixels, pitch padding, frame gaps, guards - has changed."""
    c, (want, _, _) = case(name)
    rc, got = call(lib, device, c)
    assert rc == 0, (name, rc)
    for g, w in zip(got, want):
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, (name, bad[:8], g[bad[:8]], w[bad[:8]])


def check_reversed(lib, device, name):
    c, (want, _, _) = case(name)
    rc, got = call(lib, device, reversed_rois(c))
    assert rc == 0 and same(got, want), name


def argument_errors(lib, device):
    """Every refusal of the two calls; nothing is written when an error is returned."""
    for name in ("rgb_c8_ellipse_r3", "nv12_c4_rect_r3_planes", "rgb_fill_rect_r3", "nv12_fill_601l"):
        c, _ = case(name)
        R = len(c["rois"])
        bad = [dict(null_frames=True), dict(null_rois=True), dict(F=-1), dict(R=-1), dict(F=-1, R=-3), dict(rpf=0), dict(rpf=-3),
               dict(R=R - 1), dict(F=c["F"] + 1), dict(rpf=2), dict(cell=0), dict(cell=1), dict(cell=3), dict(cell=6), dict(cell=64),
               dict(cell=-8), dict(shape=2), dict(shape=-1), dict(mode=2), dict(mode=-1), dict(hs=0), dict(ws=0), dict(hs=-2)]
        if c["mode"] == FILL:
            bad += [dict(null_colour=True)]
        if c["kind"] == "nv12":
            bad += [dict(null_uv=True), dict(hs=37), dict(ws=69), dict(y_pitch=69), dict(uv_pitch=68), dict(uv_pitch=c["uv_pitch"] + 1),
                    dict(uv_fs=c["uv_fs"] + 1), dict(uv_shift=1), dict(standard=4), dict(standard=-1),
                    dict(y_fs=(c["hs"] - 1) * c["y_pitch"] + c["ws"] - 1), dict(uv_fs=(c["hs"] // 2 - 1) * c["uv_pitch"] + c["ws"] - 2)]
        for over in bad:
            rc, got = call(lib, device, c, **over)
            assert rc == EINVAL, (name, over, rc)
            assert same(got, c["bufs"]), (name, over)
        wide = dict(ws=16386, y_pitch=16386, uv_pitch=16386) if c["kind"] == "nv12" else dict(ws=16385)
        for over in (dict(rpf=65, R=65 * c["F"]), dict(hs=16386), wide, dict(F=65536, R=65536 * c["rpf"])):
            rc, got = call(lib, device, c, **over)
            assert rc == ELIMIT, (name, over, rc)
            assert same(got, c["bufs"]), (name, over)
        rc, got = call(lib, device, c, F=0, R=0)                                       # no launch: nothing written
        assert rc == 0 and same(got, c["bufs"])
        if c["mode"] == MOSAIC:                                                        # colour is FILL's alone
            rc, got = call(lib, device, c, null_colour=True)
            assert rc == 0 and same(got, case(name)[1][0])


# ---- host side -----------------------------------------------------------------------------------------------------------
def torch_frames(c, bufs, lead):
    """The frames of a case over torch allocations laid out as ``c`` describes: uint8 [*lead,hs,ws,3] or Nv12Frames."""
    if c["kind"] == "rgb":
        n = c["F"] * c["hs"] * c["ws"] * 3
        return bufs[0][GUARD:GUARD + n].view(*lead, c["hs"], c["ws"], 3)
    from faster_voxelpose_amd.dataset.images import Nv12Frames
    y = torch.as_strided(bufs[c["y"][0]], (c["F"], c["hs"], c["ws"]), (c["y_fs"], c["y_pitch"], 1), c["y"][1])
    uv = torch.as_strided(bufs[c["uv"][0]], (c["F"], c["hs"] // 2, c["ws"] // 2, 2), (c["uv_fs"], c["uv_pitch"], 2, 1), c["uv"][1])
    std = {0: ("bt601", False), 1: ("bt709", False), 2: ("bt601", True), 3: ("bt709", True)}[c["standard"]]
    return Nv12Frames(y.unflatten(0, lead), uv.unflatten(0, lead), standard=std[0], full_range=std[1])


def head_scene(J, joints, hs, ws, seed, B=2, V=2, N=3):
    """views [B,V,N,J,4], ids [B,N], conf [B,N,J]: heads of a few pixels inside and partly outside a frame of hs x ws."""
    rng = np.random.default_rng([seed, J, hs, ws])
    v = np.empty((B, V, N, J, 4), f32)
    v[..., 0] = rng.uniform(-ws, 2 * ws, (B, V, N, J))                            # the body: anywhere
    v[..., 1] = rng.uniform(-hs, 2 * hs, (B, V, N, J))
    cx = rng.uniform(0.0, ws, (B, V, N, 1))
    cy = rng.uniform(0.0, hs, (B, V, N, 1))
    v[..., joints, 0] = cx + rng.uniform(-2.5, 2.5, (B, V, N, len(joints)))
    v[..., joints, 1] = cy + rng.uniform(-2.0, 2.0, (B, V, N, len(joints)))
    v[..., 2] = rng.uniform(1.0, 5.0, (B, V, N, J))
    v[..., 3] = rng.uniform(0.0, 1.0, (B, V, N, J))
    v[0, 1, 2, :, 2] = -1.0                                                       # one person behind one camera: no box there
    ids = np.array([[4, -1, 9], [0, 1, 2]], np.int32)
    conf = rng.uniform(0.2, 1.0, (B, N, J)).astype(f32)
    return v, ids, conf


def head_rois(views, ids, conf, joints, scale, pad_px, min_joints, aspect, conf_min):
    """fvp_person_rois by its definition (include/fvp.h) for the joints of a head: the restatement of tests/crop_cases.py."""
    from crop_cases import roi_reference
    mask = 0
    for j in joints:
        mask |= 1 << j
    return roi_reference(dict(views=views, ids=ids, conf=conf, mask=mask, min_joints=min_joints, scale=scale, pad_px=pad_px,
                              aspect=aspect, conf_min=conf_min))[:3]
