"""The back-projection kernels (csrc/fvp_project.hip, fvp_project_lds.h, fvp_geom.h) against a float64 reference that
carries its own error bound, over the ranges include/fvp.h promises: V 1 .. 8, J 1 .. 32, Z <= 256, power-of-two cubes
4 .. 128, any W, H >= 2.  Shared by the emulator suite (test_projection_emu.py) and the GPU suite
(test_projection_gpu.py): every check takes the bound C-ABI library and a device string and calls the ABI directly.

THE RIG.  Eight cameras written out below (RIG), the first V of which serve a case with V views; set B is set A shifted.
  0 .. 4  a ring around the space looking at its centre, each with its own roll, focal lengths and principal point;
          1 and 3 are distorted (k[0..2], p[0..1] non-zero)
  5       INSIDE the space: part of every grid is behind it, and voxels lie on both sides of its den = 0 plane
  6       outside, looking AWAY: every voxel is behind it.  The camera model has no behind-camera test, so the mirrored
          projections count like any other
  7       a long lens aimed off-centre: the image border cuts through the projected grid
The resize transform has a rotation term and a translation chosen so that each clamp of the chain lands where it changes
the tap pattern (heat map 26 x 19, clamp_max 660):
  pixel x clamped at -1        -> x = -1.54 heat pixels -> the -1.1 clamp -> every tap outside
  pixel x clamped at clamp_max -> x in (25, 26): the east taps outside
  pixel y clamped at -1        -> y in (-1, 0): the north taps outside
  pixel y clamped at clamp_max -> the +1.1 clamp -> y = 18.9: the south taps outside
so that 0, 1, 2 and 4 taps inside all occur.  (Exactly 3 taps inside cannot occur for any camera: the taps are the
product of two x columns and two y rows, each of which is inside or not, so the count is 0, 1, 2 or 4.  coverage()
asserts that 3 never occurs.)
Heat maps are sums of three Gaussians with amplitudes in [-0.6, 1.8] and centres up to 2 pixels outside the map: the
view mean leaves [0, 1] on both sides (a narrow strong peak on a broad negative floor per map), and the maps are smooth:
their steepest step is the cut at the border of the zero padding, below 2.5 per pixel.

THE REFERENCE.  Plain numpy float64 from the fp32 input values, written from the camera model's formulas, sharing no
code with oracle/fvp_oracle.py or the kernels.  Class EV carries a value and a first-order bound of the error of the
fp32 chain beside it: every rounded operation adds U |result| (U = 2^-24), operand errors propagate through the partial
derivatives, a division divides by |b| - err(b) (infinite once the denominator's error reaches it: the bound grows on its
own near den = 0, no mask), clamps pass the error through - except where the whole interval value +- error lies beyond
the limit: there the fp32 chain and the exact one both return the limit itself and the error is zero (without this the
saturated pixels of the inside camera, whose distortion polynomial multiplies their error, would carry errors of
hundreds of pixels through the clamp that pins them, and 17 % of that camera's samples would be vacuous).
  (a) coordinates: fvp_sample_grid against the float64 pixel coordinates, error / bound <= 1; and bit-equal to
      O.sample_grid, the contract fvp_geom.h states.
  (b) values, tight: the fp32 pixel coordinates of the kernel's own grid (formed as O.bilinear_mean forms them) as
      inputs, taps / weights / mean / clamp in float64.  Bound K U sum_v sum_taps |h w| / V + U with K = V + 7 roundings:
        3  a weight: two subtractions (x1 - ix, y1 - iy or their complements) and their product
        4  the tap chain: one multiplication h w and three fused multiply-adds
        V - 1  the additions of the views
        1  the division by V
      (every rounding is relative to a partial sum that sum |h w| bounds; the clamp is exact; + U absorbs the
      second-order terms.)  This bar is of order 1e-7 and is the one that catches a wrong tap order, weight or sum.
  (c) values, end to end: everything in float64, bound sum_v (Lx err(ix) + Ly err(iy)) / V + the bound of (b), with Lx,
      Ly the largest horizontal / vertical difference of the zero-padded map of that (view, joint): the bilinear
      interpolant of the zero-padded map is continuous and piecewise linear with those slopes.  Loose (median 1e-5), kept
      as the backstop that shares nothing with the oracle.  VACUITY CAP: at most 2 % of the checked voxels of a case may
      have a bound above 1e-3.
MUTANTS (discrimination, no kernel): align_corners=False, x / y weights swapped, border padding, one view dropped, a 0.01
pixel shift must each exceed the bound of (c) on >= 10 % of voxels; transposed taps and a mean over V - 1 that of (b).

THE CASES.  WHOLE_CASES: a covering set over the grids (Z = 1, 3, 20, 129, 200, 256: cpb = 256 / Z with idle lanes and a
partly full last workgroup), B in {1, 3, 8, 16} (frames alternate between the camera sets, B % 8 == 0 takes the XCD-major
index decode), V in {1, 2, 4, 6, 8} (empty quad lanes below 3, the tail loop above 4), J in {1 .. 32}, one at W x H = 2 x 3;
per case the cubes against (a) (b) (c), the fused z-max, fvp_zmax, fvp_project_columns, the single-output calls and the
Z = 257 refusal.  The lane-per-voxel form runs in a child process (projection_child.py).  PERSON_CASES: cubes 4 .. 128, every
JP from 4 to 32, V in {1, 2, 8}, windows generated from C (windows()); the materialised cubes against the reference and
exactly zero outside the window, fvp_triplane_max, and the fused planes against the materialised ones.  The fused planes
are compared AS FLOATS: a negative view mean clamps to a zero whose sign the materialised path may keep, while the fused
forms merge integer maxima onto the caller's +0.0 fill; the two zeros are the same number to everything downstream (the
conv stack adds and multiplies them), so a sign difference is counted and reported, not failed.  (None occurred, on the
emulator or on the MI355X.)  Staging, fvp_person_boxes and the proposal glue are exact."""
import ctypes as C
import types

import numpy as np
import torch

import fvp_oracle as O
from faster_voxelpose_amd import _capi as capi
from faster_voxelpose_amd.engine import _ptr

U = 2.0 ** -24
F32 = np.float32
INF = np.inf

# ---------------------------------------------------------------------------------------------------------------------
# value + first-order error bound of the fp32 chain


class EV:
    __slots__ = ("v", "e")

    def __init__(self, v, e=None):
        self.v = np.asarray(v, np.float64)
        self.e = np.zeros_like(self.v) if e is None else np.asarray(e, np.float64)


def _ev(x):
    return x if isinstance(x, EV) else EV(np.float64(F32(x)))


def _rnd(v, e):
    with np.errstate(invalid="ignore"):
        e = e + U * np.abs(v)
    return EV(v, np.where(np.isnan(e), INF, e))


def add(a, b):
    a, b = _ev(a), _ev(b)
    return _rnd(a.v + b.v, a.e + b.e)


def sub(a, b):
    a, b = _ev(a), _ev(b)
    return _rnd(a.v - b.v, a.e + b.e)


def _prod_err(a, b):
    with np.errstate(invalid="ignore"):
        e = np.abs(a.v) * b.e + np.abs(b.v) * a.e
    return np.where(np.isnan(e), INF, e)


def mul(a, b):
    a, b = _ev(a), _ev(b)
    return _rnd(a.v * b.v, _prod_err(a, b))


def fma(a, b, c):
    a, b, c = _ev(a), _ev(b), _ev(c)
    return _rnd(a.v * b.v + c.v, _prod_err(a, b) + c.e)


def div(a, b):
    a, b = _ev(a), _ev(b)
    with np.errstate(divide="ignore", invalid="ignore"):
        v = a.v / b.v
        d = np.abs(b.v) - b.e
        e = np.where(d > 0, (a.e + np.abs(v) * b.e) / np.where(d > 0, d, 1.0), INF)
    return _rnd(v, np.where(np.isnan(e), INF, e))


def clamp(a, lo, hi):
    """The error passes through, except where the whole interval v +- e lies beyond a limit: there the fp32 chain and
    the exact one both return that limit, and the error is zero."""
    lo, hi = np.float64(F32(lo)), np.float64(F32(hi))
    beyond = (a.v - a.e > hi) | (a.v + a.e < lo)
    return EV(np.clip(a.v, lo, hi), np.where(beyond, 0.0, a.e))


# ---------------------------------------------------------------------------------------------------------------------
# the rig

SPACE_CENTER = (300.0, -500.0, 900.0)
SPACE_SIZE = (4000.0, 3600.0, 2000.0)
ORI_SIZE = (660, 480)
SIZES = {(26, 19): dict(image=(208, 152), rt=(0.325, 0.004, -12.0, -0.003, 0.3167, -2.6)),
         (2, 3): dict(image=(16, 24), rt=(0.025, 0.001, -0.6, -0.002, 0.05, -0.7))}


def _look_at(pos, target, roll):
    """Rows of R = the camera's x (right), y (down), z (forward) axes in the world; x_cam = R (x - T), T = the position."""
    pos, target = np.asarray(pos, np.float64), np.asarray(target, np.float64)
    z = (target - pos) / np.linalg.norm(target - pos)
    x = np.cross(z, np.array([0.0, 0.0, 1.0]))
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    c, s = np.cos(roll), np.sin(roll)
    return np.stack([c * x + s * y, -s * x + c * y, z])


def _cam(pos, target, roll, f, c, k=(0.0, 0.0, 0.0), p=(0.0, 0.0)):
    r32 = lambda a: [float(F32(v)) for v in np.asarray(a, np.float64).reshape(-1)]
    return dict(R=np.asarray(r32(_look_at(pos, target, roll))).reshape(3, 3).tolist(), T=[[v] for v in r32(pos)],
                fx=r32(f)[0], fy=r32(f)[1], cx=r32(c)[0], cy=r32(c)[1], k=r32(k), p=r32(p))


def _ring(i):
    th = 2.0 * np.pi * i / 5.0 + 0.3
    cx, cy, cz = SPACE_CENTER
    pos = (cx + 5200.0 * np.cos(th), cy + 5200.0 * np.sin(th), 2400.0 + 150.0 * i)
    tgt = (cx + 40.0 * i, cy - 30.0 * i, cz - 100.0 + 60.0 * i)
    dist = {1: dict(k=(-0.12, 0.05, -0.01), p=(0.002, -0.001)), 3: dict(k=(0.08, -0.02, 0.004), p=(-0.0015, 0.0025))}
    return _cam(pos, tgt, (-0.2, 0.1, 0.35, -0.05, 0.15)[i], (520.0 + 25.0 * i, 530.0 + 20.0 * i),
                (330.0 + 7.0 * i, 240.0 - 5.0 * i), **dist.get(i, {}))


def _rig(shift):
    sh = np.asarray(shift, np.float64)
    cx, cy, cz = SPACE_CENTER
    cams = [_ring(i) for i in range(5)]
    # inside the space, off every voxel plane (den = 0 on a voxel centre would make the reference itself infinite there)
    cams.append(_cam((cx + 613.7, cy - 287.3, cz + 391.1), (cx - 900.0, cy + 1400.0, cz - 350.0), 0.25, (300.0, 310.0),
                     (325.0, 236.0), k=(-0.05, 0.01, 0.0), p=(0.001, 0.0005)))
    # outside, looking away from the space: every voxel has den < 0
    cams.append(_cam((cx + 3900.0, cy + 2800.0, cz + 700.0), (cx + 9000.0, cy + 7000.0, cz + 1500.0), -0.1, (380.0, 370.0),
                     (318.0, 250.0)))
    # a long lens aimed beside the space: the image border cuts through the projected grid
    cams.append(_cam((cx - 4700.0, cy + 3100.0, cz + 2100.0), (cx - 1100.0, cy + 1300.0, cz + 500.0), 0.3, (1150.0, 1120.0),
                     (340.0, 228.0)))
    for cam in cams:
        cam["T"] = [[float(F32(v[0] + s))] for v, s in zip(cam["T"], sh)]
    return cams


RIG = {"a": _rig((0.0, 0.0, 0.0)), "b": _rig((231.0, -187.0, 95.0))}


def cam_rows(which, V):
    """[V][24] fp32: R[9] T[3] f[2] c[2] k[3] p[2] pad[3] (FVP_CAM_FLOATS)."""
    rows = np.zeros((V, capi.FVP_CAM_FLOATS), F32)
    for v, cam in enumerate(RIG[which][:V]):
        rows[v, 0:9] = np.asarray(cam["R"]).reshape(9)
        rows[v, 9:12] = np.asarray(cam["T"]).reshape(3)
        rows[v, 12:16] = [cam["fx"], cam["fy"], cam["cx"], cam["cy"]]
        rows[v, 16:19] = cam["k"]
        rows[v, 19:21] = cam["p"]
    return rows


def oracle_cfg(W, H):
    ds = types.SimpleNamespace(HEATMAP_SIZE=[W, H], ORI_IMAGE_SIZE=list(ORI_SIZE), IMAGE_SIZE=list(SIZES[(W, H)]["image"]))
    return types.SimpleNamespace(DATASET=ds)


def make_geom(W, H, V, J):
    g = capi.FvpGeom()
    g.clamp_max = float(max(ORI_SIZE))
    for i, v in enumerate(SIZES[(W, H)]["rt"]):
        g.rt[i] = v
    g.hm_w, g.hm_h = float(W), float(H)
    g.img_w, g.img_h = (float(v) for v in SIZES[(W, H)]["image"])
    g.W, g.H, g.V, g.J, g.JP = W, H, V, J, (J + 3) // 4 * 4
    return g


def axes(nbins):
    """Voxel-centre coordinates of a grid over the space, fp32 (linspace + centre, as the engine forms them)."""
    return [(torch.linspace(-SPACE_SIZE[a] / 2, SPACE_SIZE[a] / 2, int(nbins[a])) + SPACE_CENTER[a]).numpy() if nbins[a] > 1
            else np.asarray([SPACE_CENTER[a] + 137.0 * (a + 1)], F32) for a in range(3)]


def points(ax3):
    mx, my, mz = np.meshgrid(*ax3, indexing="ij")
    return np.stack([mx.reshape(-1), my.reshape(-1), mz.reshape(-1)], axis=1).astype(F32)


def heatmaps(B, V, J, W, H, seed):
    """[B][V][J][H][W] fp32: three Gaussians per map, amplitudes in [-0.6, 1.8], centres up to 2 pixels outside."""
    rs = np.random.RandomState(seed)
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    amp = rs.uniform(-0.6, 1.8, (B, V, J, 3))
    amp[..., 0] = rs.uniform(1.3, 1.8, (B, V, J))          # one strong positive lobe and one negative one per map
    amp[..., 1] = rs.uniform(-0.6, -0.3, (B, V, J))
    cx = rs.uniform(-2.0, W + 1.0, (B, V, J, 3))
    cy = rs.uniform(-2.0, H + 1.0, (B, V, J, 3))
    sg = rs.uniform(0.3, 0.5, (B, V, J, 3)) * min(W, H) + 1.0
    sg[..., 0] = rs.uniform(0.15, 0.3, (B, V, J)) * min(W, H) + 0.7     # (narrow peaks on a broad negative floor)
    sg[..., 1] = rs.uniform(0.6, 0.9, (B, V, J)) * min(W, H) + 1.0
    out = np.zeros((B, V, J, H, W))
    for i in range(3):
        d2 = (xs - cx[..., i, None, None]) ** 2 + (ys - cy[..., i, None, None]) ** 2
        out += amp[..., i, None, None] * np.exp(-d2 / (2.0 * sg[..., i, None, None] ** 2))
    return out.astype(F32)


# ---------------------------------------------------------------------------------------------------------------------
# the float64 reference


def pixel_coords64(row, g, pts, mutant=None):
    """One camera (24 fp32 values), points [N][3] fp32 -> (ix, iy) EV heat-map pixel coordinates and den (float64)."""
    r = [np.float64(v) for v in row]
    R, T, f, c, k, p = r[0:9], r[9:12], r[12:14], r[14:16], r[16:19], r[19:21]
    w = [EV(pts[:, a]) for a in range(3)]
    d = [sub(w[a], T[a]) for a in range(3)]
    xc = [fma(R[3 * i + 2], d[2], fma(R[3 * i + 1], d[1], mul(R[3 * i], d[0]))) for i in range(3)]
    den = add(xc[2], 1e-5)
    y0, y1 = div(xc[0], den), div(xc[1], den)
    rr = add(mul(y0, y0), mul(y1, y1))
    dd = add(1.0, mul(k[0], rr))
    dd = add(dd, mul(mul(k[1], rr), rr))
    dd = add(dd, mul(mul(mul(k[2], rr), rr), rr))
    u = add(mul(y0, dd), mul(mul(mul(2.0, p[0]), y0), y1))
    u = add(u, mul(p[1], add(rr, mul(mul(2.0, y0), y0))))
    v = add(mul(y1, dd), mul(mul(mul(2.0, p[1]), y0), y1))
    v = add(v, mul(p[0], add(rr, mul(mul(2.0, y1), y1))))
    px, py = add(mul(f[0], u), c[0]), add(mul(f[1], v), c[1])
    lo_x, hi_x = px.v < -1.0, px.v > g.clamp_max
    lo_y, hi_y = py.v < -1.0, py.v > g.clamp_max
    px, py = clamp(px, -1.0, g.clamp_max), clamp(py, -1.0, g.clamp_max)
    ax_ = fma(g.rt[2], 1.0, fma(g.rt[1], py, mul(g.rt[0], px)))
    ay_ = fma(g.rt[5], 1.0, fma(g.rt[4], py, mul(g.rt[3], px)))
    sx = div(mul(ax_, g.hm_w), g.img_w)
    sy = div(mul(ay_, g.hm_h), g.img_h)
    sx = sub(mul(div(sx, g.hm_w - 1.0), 2.0), 1.0)
    sy = sub(mul(div(sy, g.hm_h - 1.0), 2.0), 1.0)
    sat = (np.abs(sx.v) > np.float64(F32(1.1))) | (np.abs(sy.v) > np.float64(F32(1.1)))
    gx, gy = clamp(sx, -1.1, 1.1), clamp(sy, -1.1, 1.1)
    if mutant == "align_corners_false":
        ix = EV(((gx.v + 1.0) * g.W - 1.0) / 2.0, gx.e * g.W / 2.0)
        iy = EV(((gy.v + 1.0) * g.H - 1.0) / 2.0, gy.e * g.H / 2.0)
    else:
        ix, iy = mul(add(gx, 1.0), 0.5 * (g.W - 1)), mul(add(gy, 1.0), 0.5 * (g.H - 1))
    if mutant == "shift":
        ix = EV(ix.v + 0.01, ix.e)
    flags = dict(den_neg=den.v < 0, pix_lo=lo_x | lo_y, pix_hi=hi_x | hi_y, sat=sat)
    return ix, iy, gx, gy, flags


def coords64(rows, g, pts, mutant=None):
    """All views: ix, iy, their bounds [V][N] and the coverage flags."""
    per = [pixel_coords64(rows[v], g, pts, mutant) for v in range(rows.shape[0])]
    st = lambda f: np.stack([f(p) for p in per])
    out = dict(ix=st(lambda p: p[0].v), iy=st(lambda p: p[1].v), eix=st(lambda p: p[0].e), eiy=st(lambda p: p[1].e),
               gx=st(lambda p: p[2].v), gy=st(lambda p: p[3].v), egx=st(lambda p: p[2].e), egy=st(lambda p: p[3].e))
    for name in per[0][4]:
        out[name] = np.stack([p[4][name] for p in per])
    return out


def bilinear64(heat, ix, iy, mutant=None):
    """heat [V][J][H][W], ix / iy [V][N] -> clamp01(mean over the views of the bilinear samples) [J][N] in float64 (zero
    padding, align_corners=True is already in ix / iy), sum_v sum_taps |h w| [J][N], and the taps-inside count [V][N]."""
    heat = np.asarray(heat, np.float64)
    V, J, H, W = heat.shape
    ix, iy = np.asarray(ix, np.float64), np.asarray(iy, np.float64)
    total = np.zeros((J, ix.shape[1]))
    absum = np.zeros_like(total)
    count = np.zeros(ix.shape, np.int64)
    for v in range(V - 1 if mutant == "drop_view" else V):
        x0, y0 = np.floor(ix[v]), np.floor(iy[v])
        fx, fy = ix[v] - x0, iy[v] - y0
        if mutant == "swap_weights":
            fx, fy = fy, fx
        wts = [(1.0 - fx) * (1.0 - fy), fx * (1.0 - fy), (1.0 - fx) * fy, fx * fy]
        if mutant == "transposed_taps":
            wts = [wts[0], wts[2], wts[1], wts[3]]
        flat = heat[v].reshape(J, H * W)
        for (dx, dy), wt in zip(((0, 0), (1, 0), (0, 1), (1, 1)), wts):
            xx, yy = (x0 + dx).astype(np.int64), (y0 + dy).astype(np.int64)
            inside = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
            count[v] += inside
            val = flat[:, np.clip(yy, 0, H - 1) * W + np.clip(xx, 0, W - 1)]
            if mutant != "border_padding":
                val = val * inside
            total += val * wt
            absum += np.abs(val * wt)
    nv = V - 1 if mutant == "mean_vm1" else V
    return np.clip(total / nv, 0.0, 1.0), absum / V, count, total / nv


def lipschitz(heat):
    """Largest horizontal / vertical difference of each zero-padded map: [V][J] each."""
    h = np.pad(np.asarray(heat, np.float64), ((0, 0), (0, 0), (1, 1), (1, 1)))
    return np.abs(np.diff(h, axis=3)).max(axis=(2, 3)), np.abs(np.diff(h, axis=2)).max(axis=(2, 3))


def k_roundings(V):
    """Roundings between the fp32 pixel coordinates and the stored value: 3 (a weight) + 4 (mul + three fmas) + V - 1 (view
    additions) + 1 (division)."""
    return 3 + 4 + (V - 1) + 1


def bound_b(absum, V):
    return k_roundings(V) * U * absum + U


def reference(rows, g, pts, heat):
    """Everything the checks need for one (camera set, points, frame): (c) value and bound, coordinates and bounds."""
    V = rows.shape[0]
    co = coords64(rows, g, pts)
    val, absum, count, raw = bilinear64(heat, co["ix"], co["iy"])
    lx, ly = lipschitz(heat)
    with np.errstate(invalid="ignore"):
        geo = (lx[:, :, None] * co["eix"][:, None, :] + ly[:, :, None] * co["eiy"][:, None, :]).sum(axis=0) / V
    geo = np.where(np.isnan(geo), INF, geo)
    co.update(val=val, bound_c=geo + bound_b(absum, V), count=count, raw=raw)
    return co


def tight(grid32, g, heat):
    """(b): the kernel's own fp32 grid [V][N][2] -> float64 values from fp32 pixel coordinates formed as O.bilinear_mean
    forms them, and the bound."""
    gt = torch.as_tensor(grid32)
    ix = ((gt[..., 0] + 1) * ((g.W - 1) / 2)).numpy()
    iy = ((gt[..., 1] + 1) * ((g.H - 1) / 2)).numpy()
    val, absum, _, _ = bilinear64(heat, ix, iy)
    return val, bound_b(absum, heat.shape[0])


# ---------------------------------------------------------------------------------------------------------------------
# self-tests of the fixture (CPU, no kernel)

COVER_GRID = (12, 10, 8)
W0, H0 = 26, 19


def coverage():
    """Fractions of (voxel, view) samples of the coverage grid, all eight cameras of both sets, in each tap / clamp class;
    asserts the floor of 1 % each on the float64 reference."""
    g = make_geom(W0, H0, 8, 5)
    pts = points(axes(COVER_GRID))
    heat = heatmaps(1, 8, 5, W0, H0, seed=1)[0]
    cnt, flags = [], {}
    for which in ("a", "b"):
        ref = reference(cam_rows(which, 8), g, pts, heat)
        cnt.append(ref["count"])
        for k in ("den_neg", "pix_lo", "pix_hi", "sat"):
            flags.setdefault(k, []).append(ref[k])
    cnt = np.concatenate(cnt, axis=1)
    fl = {k: np.concatenate(v, axis=1) for k, v in flags.items()}
    frac = {"taps_%d" % n: float((cnt == n).mean()) for n in range(5)}
    frac["all_out_through_the_1.1_clamp"] = float(((cnt == 0) & fl["sat"]).mean())
    frac["pixel_clamp_low"] = float(fl["pix_lo"].mean())
    frac["pixel_clamp_high"] = float(fl["pix_hi"].mean())
    frac["den_negative"] = float(fl["den_neg"].mean())
    assert frac["taps_3"] == 0.0, frac          # two columns x two rows: 0, 1, 2 or 4 taps, never 3
    for k, v in frac.items():
        if k not in ("taps_3", "taps_0"):
            assert v >= 0.01, (k, frac)
    return frac


def mean_clamp_fractions(V, J, seed, nbins=COVER_GRID):
    """Fraction of (voxel, joint) values of one frame whose view mean is clamped at 0 / at 1."""
    g = make_geom(W0, H0, V, J)
    ref = reference(cam_rows("a", V), g, points(axes(nbins)), heatmaps(1, V, J, W0, H0, seed)[0])
    return float((ref["raw"] < 0).mean()), float((ref["raw"] > 1).mean())


MUTANTS_C = ("align_corners_false", "swap_weights", "border_padding", "drop_view", "shift")
MUTANTS_B = ("transposed_taps", "mean_vm1")


def discrimination(V=8, J=5):
    """Fraction of (voxel, joint) values on which each mutated reference leaves the bound: of (c) for MUTANTS_C, of (b) for
    MUTANTS_B.  Also the vacuity figure of the same case."""
    g = make_geom(W0, H0, V, J)
    rows, pts = cam_rows("a", V), points(axes(COVER_GRID))
    heat = heatmaps(1, V, J, W0, H0, seed=2)[0]
    ref = reference(rows, g, pts, heat)
    out = {"vacuous": float((ref["bound_c"] > 1e-3).mean())}
    for m in MUTANTS_C:
        if m in ("align_corners_false", "shift"):
            co = coords64(rows, g, pts, m)
            val = bilinear64(heat, co["ix"], co["iy"])[0]
        else:
            val = bilinear64(heat, ref["ix"], ref["iy"], m)[0]
        out[m] = float((np.abs(val - ref["val"]) > ref["bound_c"]).mean())
    ix32, iy32 = ref["ix"].astype(F32), ref["iy"].astype(F32)
    good, absum, _, _ = bilinear64(heat, ix32, iy32)
    for m in MUTANTS_B:
        val = bilinear64(heat, ix32, iy32, m)[0]
        out[m] = float((np.abs(val - good) > bound_b(absum, V)).mean())
    return out


# ---------------------------------------------------------------------------------------------------------------------
# calling the library


class Ctx:
    """One bound library on one device."""

    def __init__(self, lib, dev):
        self.lib, self.dev = lib, dev
        self._hold = []

    def call(self, name, *args):
        capi.check(self.lib, self.rc(name, *args), name)

    def rc(self, name, *args):
        try:
            return getattr(self.lib, name)(*args)
        finally:
            self._hold.clear()              # (launched: the allocator hands the blocks on in stream order)

    def p(self, a, dtype=None):
        """Upload an argument and return its pointer; the tensor lives until the call it is an argument of has been issued
        (a bare _ptr(up(a)) would free it before the next argument is uploaded - into the same block)."""
        self._hold.append(self.up(a, dtype))
        return _ptr(self._hold[-1])

    def stream(self):
        if self.dev != "cpu":
            return C.c_void_p(torch.cuda.current_stream(torch.device(self.dev)).cuda_stream)
        return None

    def up(self, a, dtype=None):
        t = torch.as_tensor(np.ascontiguousarray(a) if isinstance(a, np.ndarray) else a)
        return (t.to(dtype) if dtype is not None else t).contiguous().to(self.dev)

    def full(self, shape, value, dtype=torch.float32):
        return torch.full(shape, value, dtype=dtype, device=self.dev)


def _ratio(err, bound):
    """max err / bound; 0 / 0 counts as 0, an infinite bound as 0 (the vacuity cap counts those)."""
    err, bound = np.asarray(err, np.float64), np.asarray(bound, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    assert not np.isnan(r).any()
    return float(r.max()) if r.size else 0.0


def grid_of(cx, ax3, rows, g):
    """fvp_sample_grid on the grid of three axis tables: [V][n][2] fp32 (numpy)."""
    V = rows.shape[0]
    dims = [len(a) for a in ax3]
    out = cx.full((V, dims[0] * dims[1] * dims[2], 2), float("nan"))
    dax = [cx.up(a, torch.float32) for a in ax3]
    cx.call("fvp_sample_grid", _ptr(dax[0]), _ptr(dax[1]), _ptr(dax[2]), dims[0], dims[1], dims[2], cx.p(rows), C.byref(g),
            _ptr(out), cx.stream())
    return out.cpu().numpy()


def check_coords(grid32, rows, g, pts, which, what, oracle_stride=1):
    """(a): the kernel's grid against the float64 coordinates (normalised and in heat-map pixels) and, bit for bit, against
    O.sample_grid.  Returns the largest error / bound."""
    co = coords64(rows, g, pts)
    gt = torch.as_tensor(grid32)
    ix32 = ((gt[..., 0] + 1) * ((g.W - 1) / 2)).numpy().astype(np.float64)
    iy32 = ((gt[..., 1] + 1) * ((g.H - 1) / 2)).numpy().astype(np.float64)
    worst = max(_ratio(np.abs(grid32[..., 0] - co["gx"]), co["egx"]), _ratio(np.abs(grid32[..., 1] - co["gy"]), co["egy"]),
                _ratio(np.abs(ix32 - co["ix"]), co["eix"]), _ratio(np.abs(iy32 - co["iy"]), co["eiy"]))
    assert np.isfinite(grid32).all(), what
    assert worst <= 1.0, "%s: coordinates leave the fp32 bound: error / bound = %.3f" % (what, worst)
    cfg = oracle_cfg(g.W, g.H)
    sub_pts = torch.as_tensor(pts[::oracle_stride])
    rt = np.asarray(SIZES[(g.W, g.H)]["rt"], F32).reshape(2, 3)
    for v in range(rows.shape[0]):
        want = O.sample_grid(sub_pts, RIG[which][v], cfg, rt).numpy()
        assert np.array_equal(grid32[v, ::oracle_stride].view(np.int32), want.view(np.int32)), \
            "%s: view %d differs from O.sample_grid in %d coordinates" % (what, v, int((grid32[v, ::oracle_stride] != want).sum()))
    return worst


def check_values(got, grid32, rows, g, pts, heat, what, sample=None):
    """(b) and (c) for one frame: got [J][N] (or [J][len(sample)]) against the two references.  Returns the two ratios and the
    vacuous fraction of (c)."""
    if sample is not None:
        grid32, pts = grid32[:, sample], pts[sample]
    got = np.asarray(got, np.float64)
    val_b, bnd_b = tight(grid32, g, heat)
    rb = _ratio(np.abs(got - val_b), bnd_b)
    ref = reference(rows, g, pts, heat)
    rc = _ratio(np.abs(got - ref["val"]), ref["bound_c"])
    vac = float((ref["bound_c"] > 1e-3).mean())
    assert rb <= 1.0, "%s: (b) values from the kernel's own coordinates: error / bound = %.3f (K = %d)" % (what, rb, k_roundings(g.V))
    assert rc <= 1.0, "%s: (c) values end to end: error / bound = %.3f" % (what, rc)
    return rb, rc, vac, ref


def _feq(a, b):
    """Equal as floats (-0.0 == +0.0), no NaN."""
    return bool(torch.equal(a, b)) and not bool(torch.isnan(a).any())


# ---------------------------------------------------------------------------------------------------------------------
# staging

# (J, W, H): H * W = 6, 494, 256 (one full block of the kernel's 256 pixels) and 258 = one block + 2.  (257 is prime: it would
# need a side of 1, which the geometry check refuses - check_staging_refusal.)
STAGING = [(1, 2, 3), (3, 26, 19), (4, 16, 16), (5, 129, 2), (17, 26, 19), (21, 2, 3), (32, 16, 16), (32, 2, 129)]


def _staging_geom(J, W, H, V):
    g = make_geom(W0, H0, V, J)
    g.W, g.H, g.hm_w, g.hm_h = W, H, float(W), float(H)
    return g


def check_staging(cx, J, W, H, B=2, V=3):
    """fvp_heatmaps_to_cl against a permute: padding channels exactly zero, guard bands untouched."""
    g = _staging_geom(J, W, H, V)
    heat = np.random.RandomState(J * 1000 + W).uniform(-1, 1, (B, V, J, H, W)).astype(F32)
    guard, n = 64, B * V * H * W * g.JP
    buf = cx.full((n + 2 * guard,), -3.0)
    out = buf[guard:guard + n]
    cx.call("fvp_heatmaps_to_cl", cx.p(heat), _ptr(out), B, C.byref(g), cx.stream())
    buf = buf.cpu()
    assert bool((buf[:guard] == -3.0).all()) and bool((buf[guard + n:] == -3.0).all()), "guard band written"
    got = buf[guard:guard + n].view(B, V, H, W, g.JP)
    want = torch.zeros(B, V, H, W, g.JP)
    want[..., :J] = torch.as_tensor(heat).permute(0, 1, 3, 4, 2)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (J, W, H)


def check_staging_refusal(cx):
    """A heat map with a side of 1 (H * W = 257) is refused and nothing is written."""
    g = _staging_geom(5, 257, 1, 1)
    buf = cx.full((257 * g.JP,), -3.0)
    rc = cx.rc("fvp_heatmaps_to_cl", cx.p(np.zeros((1, 1, 5, 1, 257), F32)), _ptr(buf), 1, C.byref(g), cx.stream())
    assert rc == 10001 and bool((buf.cpu() == -3.0).all()), rc


def stage(cx, heat, g):
    B, V, J, H, W = heat.shape
    out = cx.full((B, V, H, W, g.JP), float("nan"))
    cx.call("fvp_heatmaps_to_cl", cx.p(heat), _ptr(out), B, C.byref(g), cx.stream())
    return out


# ---------------------------------------------------------------------------------------------------------------------
# whole space

#              name                  grid (X, Y, Z)  B   V  J   (W, H)
WHOLE_CASES = [("g5x7x20_B3_V4_J5", (5, 7, 20), 3, 4, 5, (26, 19)),
               ("g3x3x1_B1_V1_J1", (3, 3, 1), 1, 1, 1, (26, 19)),
               ("g2x3x256_B1_V2_J4", (2, 3, 256), 1, 2, 4, (26, 19)),
               ("g4x5x3_B8_V6_J17", (4, 5, 3), 8, 6, 17, (26, 19)),
               ("g3x2x200_B3_V8_J21", (3, 2, 200), 3, 8, 21, (26, 19)),
               ("g2x2x129_B1_V8_J32", (2, 2, 129), 1, 8, 32, (26, 19)),
               ("g5x7x20_B16_V2_J16", (5, 7, 20), 16, 2, 16, (26, 19)),
               ("g4x5x3_B3_V1_J32", (4, 5, 3), 3, 1, 32, (26, 19)),
               ("g3x3x1_B8_V8_J21", (3, 3, 1), 8, 8, 21, (26, 19)),
               ("g5x7x20_B1_V6_J4", (5, 7, 20), 1, 6, 4, (26, 19)),
               ("g4x5x3_B3_V4_J16_hm2x3", (4, 5, 3), 3, 4, 16, (2, 3)),
               ("g2x2x129_B3_V2_J17", (2, 2, 129), 3, 2, 17, (26, 19))]
WHOLE_BY_NAME = {c[0]: c for c in WHOLE_CASES}
_WHOLE_REF = {}


def whole_inputs(name):
    _, grid, B, V, J, (W, H) = WHOLE_BY_NAME[name]
    g = make_geom(W, H, V, J)
    ax3 = axes(grid)
    heat = heatmaps(B, V, J, W, H, seed=100 + sum(ord(c) for c in name))
    return g, ax3, points(ax3), heat, np.stack([cam_rows("a", V), cam_rows("b", V)]), np.arange(B, dtype=np.int32) % 2


def project_whole(cx, g, ax3, heat_cl, cams, frame_set, B, cubes=True, zmax=True, Z=None):
    X, Y, Zn = (len(a) for a in ax3)
    dax = [cx.up(a, torch.float32) for a in ax3]
    c = cx.full((B, g.J, X, Y, Zn), -5.0) if cubes else None
    z = cx.full((B, g.J, X, Y), -5.0) if zmax else None
    rc = cx.rc("fvp_project_whole", _ptr(heat_cl), cx.p(cams), cx.p(frame_set), _ptr(dax[0]), _ptr(dax[1]),
               _ptr(dax[2]), X, Y, Zn if Z is None else Z, B, C.byref(g), _ptr(c), _ptr(z), cx.stream())
    return rc, (c.cpu() if cubes else None), (z.cpu() if zmax else None)


def check_whole(cx, name, lane_form=False):
    """One whole-space case: cubes against (a), (b), (c); the fused z-max, fvp_zmax, fvp_project_columns, the single-output
    calls and the Z limit.  Returns the figures of the summary."""
    _, grid, B, V, J, (W, H) = WHOLE_BY_NAME[name]
    g, ax3, pts, heat, cams, frame_set = whole_inputs(name)
    X, Y, Z = grid
    n = X * Y * Z
    heat_cl = stage(cx, heat, g)
    rc, cubes, zmax = project_whole(cx, g, ax3, heat_cl, cams, frame_set, B)
    assert rc == 0, rc
    out = dict(a=0.0, b=0.0, c=0.0, vacuous=0.0, low=0.0, high=0.0)
    grids = {}
    for s, which in enumerate("ab"[:min(B, 2)]):
        grids[s] = grid_of(cx, ax3, cams[s], g)
        out["a"] = max(out["a"], check_coords(grids[s], cams[s], g, pts, which, "%s set %s" % (name, which)))
    vac = []
    for b in range(B):
        s = int(frame_set[b])
        rb, rcc, v, ref = check_values(cubes[b].reshape(J, n).numpy(), grids[s], cams[s], g, pts, heat[b], "%s frame %d" % (name, b))
        out["b"], out["c"] = max(out["b"], rb), max(out["c"], rcc)
        out["low"], out["high"] = max(out["low"], float((ref["raw"] < 0).mean())), max(out["high"], float((ref["raw"] > 1).mean()))
        vac.append(v)
    out["vacuous"] = float(np.mean(vac))
    assert out["vacuous"] <= 0.02, "%s: %.1f %% of the voxels have an end-to-end bound above 1e-3" % (name, 100 * out["vacuous"])
    # ---- z-max: fused, single-output calls, fvp_zmax
    want_z = cubes.max(dim=4)[0]
    assert _feq(zmax, want_z), "%s: fused z-max differs from the max over the cubes" % name
    if not lane_form:
        _, c_only, _ = project_whole(cx, g, ax3, heat_cl, cams, frame_set, B, zmax=False)
        _, _, z_only = project_whole(cx, g, ax3, heat_cl, cams, frame_set, B, cubes=False)
        assert torch.equal(c_only.view(torch.int32), cubes.view(torch.int32)), "%s: cubes-only call differs" % name
        assert torch.equal(z_only.view(torch.int32), zmax.view(torch.int32)), "%s: z-max-only call differs" % name
        zm = cx.full((B, J, X, Y), -5.0)
        cx.call("fvp_zmax", cx.p(cubes), _ptr(zm), B * J * X * Y, Z, cx.stream())
        assert _feq(zm.cpu(), want_z), "%s: fvp_zmax differs" % name
    # ---- proposal columns: duplicates, the first and the last column, indices outside the map
    flat = np.array([[0, X * Y - 1, (3 + b) % (X * Y), 0, -1, X * Y, X * Y - 1] for b in range(B)], np.int64)
    N = flat.shape[1]
    feat = cx.full((B * N, J, Z), -5.0)
    dax = [cx.up(a, torch.float32) for a in ax3]
    cx.call("fvp_project_columns", _ptr(heat_cl), cx.p(cams), cx.p(frame_set), _ptr(dax[0]), _ptr(dax[1]), _ptr(dax[2]),
            X, Y, Z, B, C.byref(g), cx.p(flat), N, _ptr(feat), cx.stream())
    feat = feat.cpu().view(B, N, J, Z)
    cols = cubes.view(B, J, X * Y, Z)
    for b in range(B):
        for k in range(N):
            f = int(flat[b, k])
            if 0 <= f < X * Y:
                assert torch.equal(feat[b, k].view(torch.int32), cols[b, :, f].contiguous().view(torch.int32)), (name, "column", b, k)
            else:
                assert float(feat[b, k].abs().max()) == 0.0, (name, "column outside the map", b, k)
    # ---- Z = 257: refused, nothing written
    if not lane_form:
        rc, c257, z257 = project_whole(cx, g, ax3, heat_cl, cams, frame_set, B, Z=257)
        assert rc == 10002, rc               # FVP_ELIMIT
        assert bool((c257 == -5.0).all()) and bool((z257 == -5.0).all()), "%s: a refused call wrote" % name
    return out


# ---------------------------------------------------------------------------------------------------------------------
# per person

N_SLOTS = 4                                                      # person slots per frame, two frames (camera sets a, b)


def fine_dims(Cn):
    return (Cn + Cn // 2 + 3, Cn + Cn // 4 + 2, Cn + 5)


def windows(Cn, two_only=False):
    """[tl, s, e] rows as fvp_person_boxes writes them, from the cube size alone, and the valid flags:
      0 full interior                                4 one x column
      1 interior, x extent C - 2, y C - 3, z C - 3   5 empty in x (s >= e), valid
      2 clipped by the space on the low side         6 empty in y, valid
      3 clipped on the high side                     7 invalid person with a sane box"""
    F = fine_dims(Cn)
    b = lambda tl, s, e: list(tl) + list(s) + list(e)
    full = lambda tl: b(tl, [max(v, 0) for v in tl], [min(v + Cn, f) for v, f in zip(tl, F)])
    h = Cn // 2
    rows = [full((2, 1, 3)),
            b((1, 2, 0), (2, 3 if Cn > 4 else 2, 1), (1 + Cn - 1, 2 + Cn - (2 if Cn > 4 else 1), Cn - 2)),
            full((-(Cn // 4) - 1, -h, -1)),
            full((F[0] - Cn + Cn // 4 + 1, F[1] - Cn + 1, F[2] - Cn + h)),
            b((3, 0, 2), (3 + h, 1, 2), (3 + h + 1, Cn - 1, 2 + Cn)),
            b((2, 2, 0), (2 + h + 1, 2, 0), (2 + h - 1, 2 + Cn, Cn)),
            b((1, 1, 1), (1, 1 + h + 1, 1), (1 + Cn, 1 + h - 1, 1 + Cn)),
            full((3, 2, 1))]
    valid = [1, 1, 1, 1, 1, 1, 1, 0]
    if two_only:
        rows, valid = [rows[1], rows[3]], [1, 1]
    r = np.asarray(rows, np.int32)
    assert (r[:, 3:6] >= r[:, 0:3]).all() and (r[:, 6:9] <= r[:, 0:3] + Cn).all() and (r[:, 3:6] >= 0).all()
    assert (r[:, 6:9] <= np.asarray(F)).all()
    return r, np.asarray(valid, np.uint8)


#               (C, J, V)        JP
PERSON_CASES = [(4, 1, 1),      # 4   C < the z block: a strip of one block
                (4, 17, 2),     # 20  the five-quad form, V < 3
                (8, 5, 8),      # 8
                (8, 29, 2),     # 32
                (16, 9, 2),     # 12
                (16, 21, 1),    # 24
                (16, 13, 8),    # 16
                (16, 25, 8),    # 28
                (64, 25, 2),    # 28  block form (the owned cells exceed 36 KB)
                (64, 17, 8),    # 20  owned
                (64, 32, 1),    # 32  block form
                (128, 5, 2)]    # 8   block form; PER = 64 in fvp_triplane_max; two persons
PERSON_EMU = [c for c in PERSON_CASES if c[0] <= 16]
KB = 1024


def owned_lds(Cn, JP):
    """Bytes of LDS of the owned form (tri_owned_lds of fvp_project_lds.h): it runs where this fits 36 KB."""
    zt = max(Cn, 16)
    return (4 * zt + 2 * 4 * 16) * (JP + 1) * 4 + 4 * 16


def expected_form(Cn, JP):
    return "own" if owned_lds(Cn, JP) <= 36 * KB else "blk"


class Person:
    """One (C, J, V) shape on one library: inputs, the materialised cubes and their planes (checked against the float64
    reference once), and the fused call."""

    def __init__(self, cx, shape, check=True):
        Cn, J, V = shape
        self.cx, self.Cn, self.J, self.V = cx, Cn, J, V
        self.g = g = make_geom(W0, H0, V, J)
        self.F = F = fine_dims(Cn)
        self.ax3 = ax3 = axes(F)
        boxes, valid = windows(Cn, two_only=Cn >= 128)
        self.boxes, self.valid = boxes, valid
        self.nP = nP = boxes.shape[0]
        self.ppf = ppf = nP // 2
        self.heat = heat = heatmaps(2, V, J, W0, H0, seed=7 * Cn + J)
        self.cams = cams = np.stack([cam_rows("a", V), cam_rows("b", V)])
        self.frame_set = np.array([0, 1], np.int32)
        self.person_frame = (np.arange(nP) // ppf).astype(np.int32)
        self.d = dict(hcl=stage(cx, heat, g), cams=cx.up(cams), fs=cx.up(self.frame_set), pf=cx.up(self.person_frame),
                      valid=cx.up(valid), boxes=cx.up(boxes), ax=[cx.up(a, torch.float32) for a in ax3],
                      fine=cx.up(np.asarray(F, np.int32)))
        self.fine_host = (C.c_int32 * 3)(*F)
        self.fgrid = None
        d = self.d
        cubes = cx.full((nP, J, Cn, Cn, Cn), -5.0)
        cx.call("fvp_project_individual", _ptr(d["hcl"]), _ptr(d["cams"]), _ptr(d["fs"]), _ptr(d["pf"]), _ptr(d["valid"]),
                _ptr(d["boxes"]), _ptr(d["ax"][0]), _ptr(d["ax"][1]), _ptr(d["ax"][2]), _ptr(d["fine"]), Cn, nP, C.byref(g),
                _ptr(cubes), cx.stream())
        want = cx.full((nP, 3, J, Cn, Cn), -5.0)
        cx.call("fvp_triplane_max", _ptr(cubes), _ptr(want), nP, J, Cn, cx.stream())
        self.want = want.cpu()
        self.figures = dict(a=0.0, b=0.0, c=0.0, vacuous=0.0)
        if check:
            self._check_cubes(cubes.cpu())
        del cubes

    def _check_cubes(self, cubes):
        Cn, J, g = self.Cn, self.J, self.g
        tri = torch.stack([cubes.max(dim=4)[0], cubes.max(dim=3)[0], cubes.max(dim=2)[0]], dim=1)
        assert _feq(self.want, tri), "fvp_triplane_max differs from the three maxima of the cubes"
        rs = np.random.RandomState(Cn)
        vac = []
        grids = {}
        for p in range(self.nP):
            tl, s, e = self.boxes[p, 0:3], self.boxes[p, 3:6], self.boxes[p, 6:9]
            live = bool(self.valid[p]) and bool((s < e).all())
            inside = np.zeros((Cn, Cn, Cn), bool)
            if live:
                lo, hi = s - tl, e - tl
                inside[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = True
            cube = cubes[p].numpy()
            assert (cube[:, ~inside] == 0.0).all(), "person %d: a voxel outside the window is not zero" % p
            if not live:
                continue
            idx = np.argwhere(inside)
            if idx.shape[0] > 6000:                     # large cubes: the window's corners and a deterministic sample
                corners = np.array([[a, b, c] for a in (lo[0], hi[0] - 1) for b in (lo[1], hi[1] - 1) for c in (lo[2], hi[2] - 1)])
                idx = np.concatenate([corners, idx[rs.choice(idx.shape[0], 6000, replace=False)]])
            set_ = int(self.frame_set[self.person_frame[p]])
            pts = np.stack([self.ax3[a][tl[a] + idx[:, a]] for a in range(3)], axis=1).astype(F32)
            if set_ not in grids:
                grids[set_] = grid_of(self.cx, self.ax3, self.cams[set_], g)
                if grids[set_].shape[1] <= 20000:      # small cubes: (a) on the whole fine grid, not only inside the windows
                    self.figures["a"] = max(self.figures["a"], check_coords(grids[set_], self.cams[set_], g, points(self.ax3),
                                                                            "ab"[set_], "C %d fine grid, set %d" % (Cn, set_)))
            lin = ((tl[0] + idx[:, 0]) * self.F[1] + tl[1] + idx[:, 1]) * self.F[2] + tl[2] + idx[:, 2]
            grid32 = grids[set_][:, lin]
            what = "C %d J %d V %d person %d" % (Cn, J, self.V, p)
            stride = 1 if idx.shape[0] <= 6000 else 7
            ra = check_coords(grid32, self.cams[set_], g, pts, "ab"[set_], what, oracle_stride=stride)
            got = cube[:, idx[:, 0], idx[:, 1], idx[:, 2]]
            rb, rc, v, _ = check_values(got, grid32, self.cams[set_], g, pts, self.heat[self.person_frame[p]], what)
            f = self.figures
            f["a"], f["b"], f["c"] = max(f["a"], ra), max(f["b"], rb), max(f["c"], rc)
            vac.append(v)
        self.figures["vacuous"] = float(np.mean(vac))
        assert self.figures["vacuous"] <= 0.02, self.figures

    def fused(self, cached):
        cx, d = self.cx, self.d
        if cached and self.fgrid is None:
            fg = [torch.as_tensor(grid_of(cx, self.ax3, self.cams[s], self.g)) for s in range(2)]
            self.fgrid = cx.up(torch.stack(fg))
        planes = torch.zeros((self.nP, 3, self.J, self.Cn, self.Cn), device=cx.dev)       # the caller's zero fill
        cx.call("fvp_project_individual_triplane", _ptr(d["hcl"]), _ptr(d["cams"]), _ptr(d["fs"]), _ptr(d["pf"]), _ptr(d["valid"]),
                _ptr(d["boxes"]), _ptr(d["ax"][0]), _ptr(d["ax"][1]), _ptr(d["ax"][2]), self.fine_host, self.Cn, self.nP,
                C.byref(self.g), _ptr(planes), self.ppf, _ptr(self.fgrid if cached else None), cx.stream())
        return planes.cpu()

    def check_fused(self, what):
        """Recomputed and cached coordinates: equal to the materialised planes as floats.  Returns the number of cells whose
        zero differs in sign (the materialised path keeps the -0.0 of a negative mean clamped at 0; the merge through integer
        maxima onto the zero fill keeps +0.0)."""
        signs = 0
        for cached in (False, True):
            got = self.fused(cached)
            assert _feq(got, self.want), "%s, %s coordinates: %d plane cells differ from the materialised path" % (
                what, "cached" if cached else "recomputed", int((got != self.want).sum()))
            signs = max(signs, int((got.view(torch.int32) != self.want.view(torch.int32)).sum()))
        return signs


_PERSON = {}


def person(cx, shape, key):
    if (key, shape) not in _PERSON:
        _PERSON[(key, shape)] = Person(cx, shape)
    return _PERSON[(key, shape)]


# ---------------------------------------------------------------------------------------------------------------------
# fvp_person_boxes against exact integer arithmetic


def check_person_boxes(cx, Cn=16):
    """tl = round_half_even(fl(fl(c * scale) + bias)); margin = trunc(fl(fl(fl(1 - bbox) / 2) * (C - 1))), negatives 0; windows
    clipped to [0, fine].  The reference forms every product and sum in float64 (exact for fp32 operands: 48-bit products,
    sums within range) and rounds to fp32 where the kernel does."""
    fine = (40, 36, 21)
    whole, ind = np.array(SPACE_SIZE, F32), np.array([2000.0, 2000.0, 2000.0], F32)
    scale = np.array([0.5, 0.25, 2.0], F32)                      # powers of two: c * scale exact, ties can be hit exactly
    bias = np.array([3.0, -2.0, 0.5], F32)
    consts = np.concatenate([scale, bias, whole, ind]).astype(F32)
    rows = []
    for cxv, cyv, czv in [(1.0, 2.0, 0.0), (3.0, 6.0, 1.0), (-9.0, 14.0, 0.5), (5.0, -6.0, 0.25), (70.0, 150.0, 9.75),
                          (-13.0, -2.0, -0.75), (60.5, 130.0, 3.3), (17.3, 41.7, 2.2)]:
        for bw, bh in [(1.5, 0.2), (0.0, 1.0), (-0.2, -3.0), (0.9999999, 0.5), (1.0 - (Cn + 0.5) / (Cn - 1), 1.0 - 2.0 / (Cn - 1))]:
            rows.append([cxv, cyv, czv, 0.0, 0.9, bw, bh])
    cen = np.asarray(rows, F32)
    n = cen.shape[0]
    boxes = cx.full((n, 9), -77, dtype=torch.int32)
    offset = cx.full((n, 3), float("nan"))
    fc = (C.c_int32 * 6)(*fine, Cn, Cn, Cn)
    cx.call("fvp_person_boxes", cx.p(cen), n, cx.p(consts), fc, _ptr(boxes), _ptr(offset), cx.stream())
    boxes, offset = boxes.cpu().numpy(), offset.cpu().numpy()
    f32 = lambda x: np.float64(F32(x))
    ties = set()
    for i in range(n):
        tl, m = [], [0, 0, 0]
        for a in range(3):
            v = f32(f32(np.float64(cen[i, a]) * np.float64(scale[a])) + np.float64(bias[a]))
            r = np.floor(v)
            d = v - r
            t = r + (1 if d > 0.5 or (d == 0.5 and int(r) % 2 != 0) else 0)
            if d == 0.5:
                ties.add(int(r) % 2)
            tl.append(int(t))
            o = f32(f32(np.float64(F32(tl[a])) / np.float64(fine[a] - 1)) * np.float64(whole[a]))
            o = f32(f32(o - f32(np.float64(whole[a]) / 2.0)) + f32(np.float64(ind[a]) / 2.0))
            assert offset[i, a] == F32(o), ("offset", i, a, offset[i, a], o)
        for a in range(2):
            r = f32(f32(f32(1.0 - np.float64(cen[i, 5 + a])) / 2.0) * np.float64(Cn - 1))
            m[a] = max(int(np.trunc(r)), 0)
        want = tl + [max(tl[a] + m[a], 0) for a in range(3)] + [min(tl[a] + Cn - m[a], fine[a]) for a in range(3)]
        assert boxes[i].tolist() == want, ("boxes", i, cen[i].tolist(), boxes[i].tolist(), want)
    assert ties == {0, 1}, "fixture: ties of both parities expected"
    m_all = np.array([[max(int(np.trunc(f32(f32(f32(1.0 - np.float64(b)) / 2.0) * (Cn - 1)))), 0) for b in r[5:7]] for r in cen])
    assert (m_all == 0).any() and (m_all == Cn // 2).any() and (m_all > Cn // 2).any() and (boxes[:, 3:6] == 0).any()
    assert any((boxes[:, 6 + a] == fine[a]).any() for a in range(3)), "fixture: a window clipped at fine expected"


# ---------------------------------------------------------------------------------------------------------------------
# proposal glue: small and exact


def check_proposal_glue(cx):
    B, N, J, Z, X, Y = 3, 4, 5, 7, 3, 5
    rs = np.random.RandomState(5)
    bbox_map = rs.uniform(0, 1, (B, 2, X, Y)).astype(F32)
    cubes = rs.uniform(0, 1, (B, J, X, Y, Z)).astype(F32)
    flat = np.array([[0, X * Y - 1, 7, 7], [3, 3, 14, 1], [14, 0, 9, 2]], np.int64)
    for with_cubes in (True, False):
        bf, mb = cx.full((B, X * Y, 2), -5.0), cx.full((B, N, 2), -5.0)
        f1 = cx.full((B * N, J, Z), -5.0)
        cx.call("fvp_gather_proposals", cx.p(bbox_map), cx.p(cubes) if with_cubes else None, cx.p(flat), B, J, X, Y,
                Z, N, _ptr(bf), _ptr(mb), _ptr(f1) if with_cubes else None, cx.stream())
        bm = torch.as_tensor(bbox_map).view(B, 2, X * Y)
        assert torch.equal(bf.cpu(), bm.permute(0, 2, 1).contiguous())
        want_mb = torch.stack([bm[b][:, torch.as_tensor(flat[b])].t() for b in range(B)])
        assert torch.equal(mb.cpu(), want_mb)
        if with_cubes:
            cb = torch.as_tensor(cubes).view(B, J, X * Y, Z)
            want = torch.stack([cb[b][:, int(flat[b, k])] for b in range(B) for k in range(N)])
            assert torch.equal(f1.cpu(), want)
        else:
            assert bool((f1 == -5.0).all())
    # ---- fvp_proposals: first maximum on ties, conf > min_score at equality, two roundings (no fma) for the centres
    hm1d = rs.uniform(0, 0.5, (B * N, Z)).astype(F32)
    hm1d[0, [2, 5]] = 0.75                                         # a tie: the first wins
    hm1d[1, :] = 0.25                                              # all equal: z = 0
    hm1d[2, Z - 1] = 1.0
    hm1d[3, [0, 6]] = 0.5
    conf2d = rs.uniform(0.5, 1.0, (B * N,)).astype(F32)
    conf2d[0] = 0.5                                                # conf = 0.5 * 0.75 = 0.375 = min_score exactly: not valid
    min_score = 0.375
    idx2d = np.stack([rs.randint(0, 80, B * N), rs.randint(0, 80, B * N)], axis=1).astype(np.int64)
    idx2d[0] = (3, 77)
    # scale / bias for which the fused result differs from the twice-rounded one (searched below, asserted to exist)
    sb = np.array([100.1, 33.3333, 7.7, -4000.7, 1234.56, 0.3], F32)
    mbb = rs.uniform(0, 1, (B * N, 2)).astype(F32)
    for null_out in (False, True):
        ti = None if null_out else cx.full((B * N, 3), -9, dtype=torch.int64)
        va = None if null_out else cx.full((B * N,), 9, dtype=torch.uint8)
        cen = cx.full((B * N, 7), float("nan"))
        cx.call("fvp_proposals", cx.p(hm1d), cx.p(conf2d), cx.p(idx2d), cx.p(mbb), cx.p(sb),
                C.c_float(min_score), B, N, Z, _ptr(ti), _ptr(cen), _ptr(va), cx.stream())
        cen = cen.cpu().numpy()
        fma_differs = 0
        for i in range(B * N):
            bz = int(np.argmax(hm1d[i]))                          # numpy: the first maximum
            conf = F32(np.float64(conf2d[i]) * np.float64(hm1d[i, bz]))
            idx = [int(idx2d[i, 0]), int(idx2d[i, 1]), bz]
            for a in range(3):
                prod = np.float64(idx[a]) * np.float64(sb[a])     # exact in float64
                two = F32(np.float64(F32(prod)) + np.float64(sb[3 + a]))
                fused = F32(prod + np.float64(sb[3 + a]))         # (exact sum of two doubles of this size, rounded once)
                fma_differs += int(two != fused)
                assert cen[i, a] == two, ("centre", i, a, cen[i, a], two, fused)
            flag = 0.0 if conf > F32(min_score) else -1.0
            assert cen[i, 3] == flag and cen[i, 4] == conf and cen[i, 5] == mbb[i, 0] and cen[i, 6] == mbb[i, 1], (i, cen[i])
            if not null_out:
                assert ti.cpu()[i].tolist() == idx and int(va.cpu()[i]) == int(flag >= 0), (i, ti.cpu()[i], va.cpu()[i])
        assert cen[0, 3] == -1.0 and cen[0, 4] == F32(0.375), "conf == min_score is not valid"
        assert fma_differs > 0, "fixture: no centre on which an fma would differ"


LANE_CASE = "g3x2x200_B3_V8_J21"                                  # JP = 24: k_project_whole<6>, a partly idle workgroup
