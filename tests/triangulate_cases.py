"""Cases and the yardstick of fvp_triangulate_joints (include/fvp.h, ABI 18), shared by tests/test_triangulate_emu.py (CPU
emulator), tests/test_triangulate_gpu.py (the shipped library on the card), tests/golden/make_triangulate_floor.py and
tools/bench_triangulate.py: an independent numpy restatement of the header's definition, vectorised over (frame, view,
person, joint) - float32 arrays round every result to float32, the fmaf chains are evaluated exactly (product and sum in
float64, rounded to odd, then to float32), the solve runs in float64 as the header says; ``dt=f64`` evaluates everything in
float64 and is the second judge - the constructed scenes with the entries each of them is about, the wrong readings of the
definition (mutants) the scenes must tell apart, seeded random scenes, the floor scenes and a runner that calls the entry
point on torch memory (CPU for the emulator, the card otherwise).  Outputs are compared bit for bit: no tolerance anywhere
but in the floor test, whose bound comes from tests/golden/triangulate_floor.json."""
import ctypes as C
import json
import os

import numpy as np

from visibility_cases import bits, ring_cameras

f32, f64 = np.float32, np.float64
NAN, INF = float("nan"), float("inf")
EINVAL, ELIMIT = 10001, 10002
MAX_JOINTS, MAX_VIEWS, MAX_RADIUS, MAX_ITERS, CAM_FLOATS = 32, 8, 8, 16, 24
FLT_MAX = float(np.finfo(f32).max)
USED, NOT_EVALUATED, OUTSIDE, PEAK_LOW, NOT_ENCLOSED, OCCLUDED, REJECTED, UNSOLVED = 1, 0, -1, -2, -3, -4, -5, -6
OUTPUTS = ("tri_poses", "tri_count", "tri_stats", "obs", "view_state", "cam_resid", "cam_count")
DEFAULTS = dict(radius=3, min_peak=0.3, iters=8, min_views=2, min_det=1e-3, reject_px=0.0)
MUTANTS = ("no_border", "tie_last", "neighbours_clamped", "no_delta_clamp", "unit_weights", "descending_views",
           "no_undistort", "no_rt_inverse", "reject_twice", "ignore_occluder")
HERE = os.path.dirname(os.path.abspath(__file__))


# ======================================================================================================================
# the definition
# ======================================================================================================================
def _fma(a, b, c, dt):
    """fmaf(a, b, c): exact for float32 - the product is exact in float64, the sum is rounded to odd there (TwoSum gives the
    error's sign), so the final rounding to float32 sees no double rounding.  In float64 mode: a*b + c."""
    if dt is f64:
        return a * b + c
    p, c = np.broadcast_arrays(np.asarray(a, f64) * np.asarray(b, f64), np.asarray(c, f64))
    s = np.atleast_1d(p + c)
    t = s - p
    err = (p - (s - t)) + (c - t)
    si = s.view(np.int64)
    fix = np.isfinite(s) & (err != 0) & ((si & 1) == 0)
    step = np.where((err > 0) == (s > 0), 1, -1)                   # towards the error: one more or one less in magnitude
    si = np.where(fix, si + step, si)
    return si.view(f64).astype(f32).reshape(p.shape)


def _clamp(x, lo, hi):
    return np.fmin(np.fmax(x, lo), hi)


def _dot(p0, p1, p2, q0, q1, q2):
    return (p0 * q0 + p1 * q1) + p2 * q2


def _finite(x, dt):
    return np.abs(x) <= dt(FLT_MAX)                                 # a NaN fails


def project_pixel(cm, x0, x1, x2, dt):
    """The camera model of csrc/fvp_geom.h: (px, py, depth).  ``cm``: [..., 24] records, already in ``dt``."""
    R = [cm[..., i] for i in range(9)]
    d0, d1, d2 = x0 - cm[..., 9], x1 - cm[..., 10], x2 - cm[..., 11]
    xc0 = _fma(R[2], d2, _fma(R[1], d1, R[0] * d0, dt), dt)
    xc1 = _fma(R[5], d2, _fma(R[4], d1, R[3] * d0, dt), dt)
    xc2 = _fma(R[8], d2, _fma(R[7], d1, R[6] * d0, dt), dt)
    den = xc2 + dt(f32(1e-5))
    y0, y1 = xc0 / den, xc1 / den
    u, v = _distort(cm, y0, y1, dt)
    return cm[..., 12] * u + cm[..., 14], cm[..., 13] * v + cm[..., 15], xc2


def _poly(cm, y0, y1, dt):
    k0, k1, k2, p0, p1 = (cm[..., i] for i in range(16, 21))
    r = y0 * y0 + y1 * y1
    d = dt(1) + k0 * r
    d = d + (k1 * r) * r
    d = d + ((k2 * r) * r) * r
    t0 = ((dt(2) * p0) * y0) * y1 + p1 * (r + (dt(2) * y0) * y0)
    t1 = ((dt(2) * p1) * y0) * y1 + p0 * (r + (dt(2) * y1) * y1)
    return d, t0, t1, p0, p1, r


def _distort(cm, y0, y1, dt):
    d, _, _, p0, p1, r = _poly(cm, y0, y1, dt)
    u = y0 * d + ((dt(2) * p0) * y0) * y1
    u = u + p1 * (r + (dt(2) * y0) * y0)
    v = y1 * d + ((dt(2) * p1) * y0) * y1
    v = v + p0 * (r + (dt(2) * y1) * y1)
    return u, v


def inverse_transform(geom):
    """Heat-map cell -> original pixel: the inverse of rt and of the heat scale, in double from the float32 fields, rounded to
    float32 once."""
    r = [f64(f32(x)) for x in geom["rt"]]
    sx = f64(f32(geom["img"][0])) / f64(f32(geom["W"]))
    sy = f64(f32(geom["img"][1])) / f64(f32(geom["H"]))
    det = r[0] * r[4] - r[1] * r[3]
    return [f32(r[4] / det * sx), f32(-r[1] / det * sy), f32((r[1] * r[5] - r[4] * r[2]) / det),
            f32(-r[3] / det * sx), f32(r[0] / det * sy), f32((r[3] * r[2] - r[0] * r[5]) / det)]


def heat_coords(case, dt=f32):
    """Step 1: (hx, hy, depth, finite P) [B,V,N,J] and the camera records [B,V,1,1,24] in ``dt``."""
    poses, cams, fset, geom = case["poses"], case["cams"], case["frame_set"], case["geom"]
    nsets = cams.shape[0]
    ok_set = (fset >= 0) & (fset < nsets)
    cm = cams[np.where(ok_set, fset, 0)].astype(dt)[:, :, None, None, :]                 # [B,V,1,1,24]
    X = poses[..., :3].astype(dt)[:, None]                                                 # [B,1,N,J,3]
    fin = _finite(X[..., 0], dt) & _finite(X[..., 1], dt) & _finite(X[..., 2], dt)
    px, py, depth = project_pixel(cm, X[..., 0], X[..., 1], X[..., 2], dt)
    rt = [dt(f32(x)) for x in geom["rt"]]
    ax = _fma(rt[2], dt(1), _fma(rt[1], py, rt[0] * px, dt), dt)
    ay = _fma(rt[5], dt(1), _fma(rt[4], py, rt[3] * px, dt), dt)
    hx = (ax * dt(f32(geom["W"]))) / dt(f32(geom["img"][0]))
    hy = (ay * dt(f32(geom["H"]))) / dt(f32(geom["img"][1]))
    return hx, hy, depth, np.broadcast_to(fin, hx.shape), cm, ok_set


def _solve(mask, ray, w, cm, min_det, order):
    """Step 8 over the views of ``mask`` [B,V,N,J] in ``order``: (not degenerate [B,N,J], X [B,N,J,3] float64)."""
    shp = mask[:, 0].shape
    A = {k: np.zeros(shp, f64) for k in ("00", "01", "02", "11", "12", "22")}
    b = [np.zeros(shp, f64) for _ in range(3)]
    for v in order:
        m = mask[:, v]
        dx, dy, dz = (ray[:, v, ..., i].astype(f64) for i in range(3))
        wv = w[:, v].astype(f64)
        c0, c1, c2 = (cm[:, v, ..., 9 + i].astype(f64) for i in range(3))
        M = {"00": 1.0 - dx * dx, "11": 1.0 - dy * dy, "22": 1.0 - dz * dz, "01": -(dx * dy), "02": -(dx * dz), "12": -(dy * dz)}
        for k in A:
            A[k] = np.where(m, A[k] + wv * M[k], A[k])
        b[0] = np.where(m, b[0] + wv * ((M["00"] * c0 + M["01"] * c1) + M["02"] * c2), b[0])
        b[1] = np.where(m, b[1] + wv * ((M["01"] * c0 + M["11"] * c1) + M["12"] * c2), b[1])
        b[2] = np.where(m, b[2] + wv * ((M["02"] * c0 + M["12"] * c1) + M["22"] * c2), b[2])
    k00, k01, k02 = A["11"] * A["22"] - A["12"] * A["12"], A["02"] * A["12"] - A["01"] * A["22"], A["01"] * A["12"] - A["02"] * A["11"]
    k11, k12, k22 = A["00"] * A["22"] - A["02"] * A["02"], A["01"] * A["02"] - A["00"] * A["12"], A["00"] * A["11"] - A["01"] * A["01"]
    det = (A["00"] * k00 + A["01"] * k01) + A["02"] * k02
    t3 = ((A["00"] + A["11"]) + A["22"]) / 3.0
    ok = det > min_det * ((t3 * t3) * t3)
    X = np.stack([((k00 * b[0] + k01 * b[1]) + k02 * b[2]) / det, ((k01 * b[0] + k11 * b[1]) + k12 * b[2]) / det,
                  ((k02 * b[0] + k12 * b[1]) + k22 * b[2]) / det], axis=-1)
    return ok, X


def _tree_mean(e, used):
    """cam_resid / cam_count of one (frame, view): e, used [N*J]."""
    n = -(-len(e) // 256) * 256
    e = np.concatenate([e, np.zeros(n - len(e), f32)]).reshape(-1, 256)
    u = np.concatenate([used, np.zeros(n - len(used), bool)]).reshape(-1, 256)
    s = np.zeros(256, f32)
    for row, ur in zip(e, u):
        s = np.where(ur, s + row, s).astype(f32)
    h = 128
    while h >= 1:
        s = (s[:h] + s[h:2 * h]).astype(f32)
        h //= 2
    cnt = int(used.sum())
    return (s[0] / f32(cnt) if cnt else f32(0)), cnt


def reference(case, dt=f32, mutant=None):
    """dict of the seven outputs by the definition in include/fvp.h, in ``dt`` (float64: nothing is rounded to float32, the
    float outputs come back as float64)."""
    poses, cams, fset, geom = case["poses"], case["cams"], case["frame_set"], case["geom"]
    heat, ids, occ = case["heat"], case.get("ids"), case.get("occluder")
    prm = {**DEFAULTS, **case.get("params", {})}
    r, iters, min_views = int(prm["radius"]), int(prm["iters"]), int(prm["min_views"])
    if mutant == "no_undistort":
        iters = 0
    min_peak, reject = dt(f32(prm["min_peak"])), dt(f32(prm["reject_px"]))
    min_det = f64(f32(prm["min_det"]))
    B, N, J = poses.shape[:3]
    V, W, H = cams.shape[1], geom["W"], geom["H"]
    zero, one, half = dt(0), dt(1), dt(0.5)
    with np.errstate(all="ignore"):
        hx, hy, depth, fin, cm, ok_set = heat_coords(case, dt)
        present = poses[:, :, 0, 3] >= 0
        if ids is not None:
            present = present & (ids >= 0)
        ev = np.broadcast_to((present & ok_set[:, None])[:, None, :, None], (B, V, N, J))
        state = np.where(ev, USED, NOT_EVALUATED).astype(np.int32)
        cxf, cyf = np.floor(hx + half), np.floor(hy + half)
        inside = fin & (depth > 0) & _finite(hx, dt) & _finite(hy, dt)
        inside = inside & (cxf >= dt(-r)) & (cxf <= dt(W - 1 + r)) & (cyf >= dt(-r)) & (cyf <= dt(H - 1 + r))
        state = np.where(ev & ~inside, OUTSIDE, state)
        live = state == USED
        cx, cy = np.where(live, cxf, 0).astype(np.int64), np.where(live, cyf, 0).astype(np.int64)
        bI, vI, jI = np.arange(B)[:, None, None, None], np.arange(V)[None, :, None, None], np.arange(J)[None, None, None, :]

        def cell(x, y, clamped=False):
            """Channel j at (x, y): the value inside the map, 0 outside (``clamped``: the nearest cell of the map)."""
            inmap = (x >= 0) & (x < W) & (y >= 0) & (y < H)
            val = heat[bI, vI, np.clip(y, 0, H - 1), np.clip(x, 0, W - 1), jI].astype(dt)
            return (val if clamped else np.where(inmap, val, zero)), inmap

        have = np.zeros((B, V, N, J), bool)
        best = np.zeros((B, V, N, J), dt)
        bx, by = np.zeros_like(cx), np.zeros_like(cy)
        for oy_ in range(-r, r + 1):
            for ox_ in range(-r, r + 1):
                val, inmap = cell(cx + ox_, cy + oy_)
                cand = live & inmap & ~np.isnan(val)
                better = cand & (~have | ((val >= best) if mutant == "tie_last" else (val > best)))
                best, bx, by = np.where(better, val, best), np.where(better, cx + ox_, bx), np.where(better, cy + oy_, by)
                have = have | cand
        peak = np.where(live & have, best, zero)
        low = live & ~(have & (best >= min_peak))
        state = np.where(low, PEAK_LOW, state)
        edge = (bx == cx - r) | (bx == cx + r) | (by == cy - r) | (by == cy + r)
        if mutant != "no_border":
            state = np.where((state == USED) & edge, NOT_ENCLOSED, state)
        got = state == USED                                                             # a peak was taken
        clamped = mutant == "neighbours_clamped"

        def refine(m, c, p):
            den = (dt(2) * c - m) - p
            raw = (half * (p - m)) / den
            return np.where(den > 0, raw if mutant == "no_delta_clamp" else _clamp(raw, dt(-0.5), half), zero)

        qx = bx.astype(dt) + refine(cell(bx - 1, by, clamped)[0], best, cell(bx + 1, by, clamped)[0])
        qy = by.astype(dt) + refine(cell(bx, by - 1, clamped)[0], best, cell(bx, by + 1, clamped)[0])
        inv = [dt(x) for x in inverse_transform(geom)]
        if mutant == "no_rt_inverse":
            inv = [dt(f32(geom["img"][0] / geom["W"])), zero, zero, zero, dt(f32(geom["img"][1] / geom["H"])), zero]
        ox = _fma(inv[2], one, _fma(inv[1], qy, inv[0] * qx, dt), dt)
        oy = _fma(inv[5], one, _fma(inv[4], qy, inv[3] * qx, dt), dt)
        cmv = cm
        u0, u1 = (ox - cmv[..., 14]) / cmv[..., 12], (oy - cmv[..., 15]) / cmv[..., 13]
        y0, y1 = u0, u1
        for _ in range(iters):
            d, t0, t1, _, _, _ = _poly(cmv, y0, y1, dt)
            y0, y1 = (u0 - t0) / d, (u1 - t1) / d
        g = [(cmv[..., k] * y0 + cmv[..., 3 + k] * y1) + cmv[..., 6 + k] for k in range(3)]
        ln = np.sqrt(_dot(g[0], g[1], g[2], g[0], g[1], g[2]))
        ray = np.stack([g[0] / ln, g[1] / ln, g[2] / ln], axis=-1)
        w = np.ones_like(peak) if mutant == "unit_weights" else _clamp(peak, zero, one)
        if occ is not None and mutant != "ignore_occluder":
            state = np.where(got & (occ != -1), OCCLUDED, state)
        # ---- steps 7-10 ---------------------------------------------------------------------------------------------
        order = range(V - 1, -1, -1) if mutant == "descending_views" else range(V)
        mask = state == USED
        usable = mask.sum(1)
        enough = ev[:, 0] & (usable >= min_views)
        ok, X64 = _solve(mask, ray, w, cm, min_det, order)
        tri = enough & ok
        X = X64 if dt is f64 else X64.astype(f32)

        def residuals(X, mask):
            qx_, qy_, _ = project_pixel(cmv, X[:, None, ..., 0], X[:, None, ..., 1], X[:, None, ..., 2], dt)
            ex, ey = qx_ - ox, qy_ - oy
            return np.where(mask, np.sqrt(ex * ex + ey * ey), dt(-1))

        e = residuals(X, mask & tri[:, None])
        for _ in range(2 if mutant == "reject_twice" else 1):
            if not reject > 0:
                break
            keep = mask & ~(e > reject)
            ok2, Y64 = _solve(keep, ray, w, cm, min_det, order)
            apply = tri & (keep != mask).any(1) & (keep.sum(1) >= min_views) & ok2
            Y = Y64 if dt is f64 else Y64.astype(f32)
            X = np.where(apply[..., None], Y, X)
            state = np.where(apply[:, None] & mask & ~keep, REJECTED, state)
            mask = np.where(apply[:, None], keep, mask)
            e = residuals(X, mask & tri[:, None])
        P = poses[..., :3].astype(dt)
        count = np.where(tri, mask.sum(1), np.where(enough, -1, np.where(ev[:, 0], usable, -2))).astype(np.int32)
        tri_poses = poses.astype(dt).copy()
        tri_poses[..., :3] = np.where(tri[..., None], X, P)
        s = [X[..., i] - P[..., i] for i in range(3)]
        shift = np.sqrt(_dot(s[0], s[1], s[2], s[0], s[1], s[2]))
        num, den = np.zeros((B, N, J), dt), np.zeros((B, N, J), dt)
        for v in order:
            m = mask[:, v] & tri
            num = np.where(m, num + w[:, v] * (e[:, v] * e[:, v]), num)
            den = np.where(m, den + w[:, v], den)
        stats = np.stack([np.where(tri, shift, zero), np.where(tri, np.sqrt(num / den), zero)], axis=-1)
        state = np.where((state == USED) & ~tri[:, None], UNSOLVED, state)                # usable, but nothing was solved
        in_solve = state == USED
        obs = np.stack([np.where(got, ox, zero), np.where(got, oy, zero), peak, np.where(in_solve, e, dt(-1))], axis=-1)
        resid, cnt = np.zeros((B, V), f32), np.zeros((B, V), np.int32)
        e32 = obs[..., 3].astype(f32)
        for b_ in range(B):
            for v in range(V):
                resid[b_, v], cnt[b_, v] = _tree_mean(e32[b_, v].reshape(-1), in_solve[b_, v].reshape(-1))
    return dict(tri_poses=tri_poses, tri_count=count, tri_stats=stats, obs=obs, view_state=state.astype(np.int32),
                cam_resid=resid, cam_count=cnt)


# ======================================================================================================================
# the rig of the constructed scenes: look-at cameras on a ring, a 192x128 image, a 48x32 heat map
# ======================================================================================================================
W, H = 48, 32
GEOM = dict(rt=[0.5, 0.0, 1.5, 0.0, 0.5, -0.75], W=W, H=H, img=(96.0, 64.0), clamp_max=192.0)
TARGET = (0.0, 0.0, 900.0)


def look_at_cameras(centres, target=TARGET, f=250.0, c=(96.0, 64.0), k=(-0.05, 0.01, 0.0), p=(1e-3, -5e-4)):
    """[nsets][V][3] camera centres -> [nsets,V,24] records: rows of R = right, down, forward (towards ``target``)."""
    centres = np.asarray(centres, f64)
    cams = np.zeros(centres.shape[:2] + (CAM_FLOATS,), f32)
    for s in range(centres.shape[0]):
        for v in range(centres.shape[1]):
            fw = np.asarray(target, f64) - centres[s, v]
            fw /= np.linalg.norm(fw)
            right = np.cross(fw, (0.0, 0.0, 1.0))
            right /= np.linalg.norm(right)
            cams[s, v, :9] = np.stack([right, np.cross(fw, right), fw]).reshape(9)
            cams[s, v, 9:12] = centres[s, v]
            cams[s, v, 12:14], cams[s, v, 14:16], cams[s, v, 16:19], cams[s, v, 19:21] = f, c, k, p
    return cams


def cells_of(case, points):
    """Heat-map coordinates (hx, hy, depth) [B,V,N,J] of ``points`` [B,N,J,3] in float64."""
    p5 = np.zeros(points.shape[:3] + (5,), f64)
    p5[..., :3] = points
    with np.errstate(all="ignore"):
        hx, hy, depth = heat_coords(dict(case, poses=p5), f64)[:3]
    return hx, hy, depth


def centres(case):
    """The window centres (cx, cy) [B,V,N,J] of the case's fused joints, as the definition computes them in float32."""
    with np.errstate(all="ignore"):
        hx, hy = heat_coords(case, f32)[:2]
        return np.floor(hx + f32(0.5)).astype(np.int64), np.floor(hy + f32(0.5)).astype(np.int64)


def blob(case, b, v, j, hx, hy, amp=0.9, a=0.08, shape="paraboloid", sigma=3.0):
    """max-combine a peak at the heat-map point (hx, hy) into channel j of view (b, v): ``amp * max(1 - a*dist^2, 0)``, an
    exact paraboloid for the sub-cell refinement, or ``amp * exp(-dist^2 / (2 sigma^2))``."""
    Hh, Ww = case["heat"].shape[2:4]
    if not (np.isfinite(hx) and np.isfinite(hy)) or not (-8 < hx < Ww + 8 and -8 < hy < Hh + 8):
        return
    reach = 12 if shape == "gaussian" else 6
    x0, x1 = max(int(hx) - reach, 0), min(int(hx) + reach + 1, Ww)
    y0, y1 = max(int(hy) - reach, 0), min(int(hy) + reach + 1, Hh)
    if x0 >= x1 or y0 >= y1:
        return
    ys, xs = np.mgrid[y0:y1, x0:x1].astype(f64)
    d2 = (xs - hx) ** 2 + (ys - hy) ** 2
    val = amp * (np.exp(-d2 / (2 * sigma ** 2)) if shape == "gaussian" else np.maximum(1.0 - a * d2, 0.0))
    tile = case["heat"][b, v, y0:y1, x0:x1, j]
    case["heat"][b, v, y0:y1, x0:x1, j] = np.maximum(tile, val.astype(f32))


def paint(case, truth, amps, skip=(), **kw):
    hx, hy, depth = cells_of(case, truth)
    B, V, N, J = hx.shape
    for idx in np.ndindex(B, V, N, J):
        if depth[idx] > 0 and idx not in skip:
            blob(case, idx[0], idx[1], idx[3], hx[idx], hy[idx], amp=amps[idx], **kw)


def wipe(case, b, v, j, cx, cy, value=0.0, reach=7):
    Hh, Ww = case["heat"].shape[2:4]
    case["heat"][b, v, max(cy - reach, 0):max(cy + reach + 1, 0), max(cx - reach, 0):max(cx + reach + 1, 0), j] = value


def put(case, b, v, j, x, y, value):
    Hh, Ww = case["heat"].shape[2:4]
    assert 0 <= x < Ww and 0 <= y < Hh, (x, y)
    case["heat"][b, v, y, x, j] = value


ROOTS = ((-700.0, -500.0, 900.0), (650.0, 600.0, 900.0))


def scene(V, J, seed, B=2, N=2, nsets=2, offset=15.0, cams=None, truth=None, params=None, frame_set=(1, 0), painted=True):
    """Two people 1.5 m apart, every joint an exact paraboloid at its true projection in every view, amplitudes 0.5..1; the
    fused joints are the truth plus ``offset`` mm in a seeded direction."""
    rng = np.random.default_rng(seed)
    cams = look_at_cameras(ring_cameras(V, nsets)) if cams is None else cams
    if truth is None:
        truth = np.asarray(ROOTS)[None, :N, None, :] + rng.uniform(-250, 250, (B, N, J, 3)) * (1.0, 1.0, 1.6)
    step = rng.standard_normal((B, N, J, 3))
    poses = np.zeros((B, N, J, 5), f32)
    poses[..., :3] = truth + offset * step / np.linalg.norm(step, axis=-1, keepdims=True)
    poses[..., 3] = 0.5
    poses[..., 4] = rng.uniform(0, 1, (B, N, J))
    case = dict(poses=poses, cams=cams, frame_set=np.asarray(frame_set, np.int32)[:B], geom=dict(GEOM), ids=None, occluder=None,
                heat=np.zeros((B, V, H, W, 4 * ((J + 3) // 4)), f32), params=dict(params or {}), truth=truth, expect={})
    case["amps"] = rng.uniform(0.5, 1.0, (B, V, N, J))
    if painted:
        paint(case, truth, case["amps"])
    return case


def _expect(case, **kw):
    case["expect"] = kw
    return case


def _argmax_tie():
    c = scene(3, 3, 1)
    cx, cy = centres(c)
    x, y = int(cx[0, 1, 0, 2]), int(cy[0, 1, 0, 2])
    wipe(c, 0, 1, 2, x, y)
    put(c, 0, 1, 2, x + 1, y, 0.8)
    put(c, 0, 1, 2, x - 1, y + 1, 0.8)                     # the same value later in the (y, x) order
    put(c, 0, 1, 2, x + 2, y + 1, 0.8)
    return _expect(c, view_state={(0, 1, 0, 2): USED}, cell={(0, 1, 0, 2): (x + 1, y)})


def _window_border():
    c = scene(3, 3, 2)
    cx, cy = centres(c)
    x, y = int(cx[1, 0, 1, 0]), int(cy[1, 0, 1, 0])
    wipe(c, 1, 0, 0, x, y)
    put(c, 1, 0, 0, x + 3, y - 1, 0.9)                     # on the border column of the radius-3 window
    put(c, 1, 0, 0, x, y, 0.5)
    return _expect(c, view_state={(1, 0, 1, 0): NOT_ENCLOSED})


def _map_border_row():
    """A joint on the ring's axis, high up: in every view its peak lies on row 0 of the map, the neighbour above is 0."""
    c = scene(3, 3, 3, painted=False)
    z = 2000.0
    for _ in range(60):                                    # the height whose projection lands near hy = 0.3
        t = c["truth"].copy()
        t[0, 0, 1] = (0.0, 0.0, z)
        hy = cells_of(c, t)[1][0, 0, 0, 1]
        z += (hy - 0.3) * 60.0
    c["truth"][0, 0, 1] = (0.0, 0.0, z)
    c["poses"][0, 0, 1, :3] = (4.0, -3.0, z - 5.0)
    paint(c, c["truth"], c["amps"])
    cy = centres(c)[1]
    assert (cy[0, :, 0, 1] == 0).all()
    return _expect(c, view_state={(0, v, 0, 1): USED for v in range(3)}, tri_count={(0, 0, 1): 3})


def _peak_low():
    c = scene(3, 3, 4)
    cx, cy = centres(c)
    c["heat"][1, 2, :, :, 1] *= f32(0.25)                  # every peak of this channel in this view is below 0.3
    return _expect(c, view_state={(1, 2, 0, 1): PEAK_LOW, (1, 2, 1, 1): PEAK_LOW}, tri_count={(1, 0, 1): 2})


def _behind_camera():
    c = scene(4, 3, 5, painted=False)
    cm = c["cams"][1, 2].astype(f64)                       # frame 0 uses set 1
    behind = cm[9:12] - 600.0 * cm[6:9]
    c["truth"][0, 1, 2] = behind
    c["poses"][0, 1, 2, :3] = behind + (5.0, 5.0, 5.0)
    paint(c, c["truth"], c["amps"])
    return _expect(c, view_state={(0, 2, 1, 2): OUTSIDE})


def _window_outside():
    c = scene(4, 3, 6, painted=False)
    cm = c["cams"][0, 1].astype(f64)                       # frame 1 uses set 0: 2.4 m to the right of this camera's axis
    off = np.asarray(TARGET) + 2400.0 * cm[0:3]
    c["truth"][1, 0, 0] = off
    c["poses"][1, 0, 0, :3] = off + (5.0, -5.0, 5.0)
    paint(c, c["truth"], c["amps"])
    hx, hy, depth = cells_of(c, c["truth"])
    assert depth[1, 1, 0, 0] > 0 and hx[1, 1, 0, 0] > W + 4
    return _expect(c, view_state={(1, 1, 0, 0): OUTSIDE})


def _occluded():
    c = scene(4, 3, 7)
    occ = np.full((2, 4, 2, 3), -1, np.int32)
    occ[0, 3, 0, 1] = 1                                    # hidden by person 1
    occ[1, 0, 1, 2] = -2                                   # not evaluated by the visibility test: not usable either
    c["occluder"] = occ
    return _expect(c, view_state={(0, 3, 0, 1): OCCLUDED, (1, 0, 1, 2): OCCLUDED, (0, 1, 0, 1): USED}, tri_count={(1, 1, 2): 3})


def _one_view_short():
    c = scene(3, 3, 8, params=dict(min_views=3))
    c["heat"][0, 1, :, :, 0] = 0.0
    return _expect(c, view_state={(0, 1, 0, 0): PEAK_LOW, (0, 0, 0, 0): UNSOLVED, (0, 2, 0, 0): UNSOLVED},
                   tri_count={(0, 0, 0): 2, (0, 1, 0): 2, (0, 0, 1): 3})


def _collinear():
    """Camera 1 of set 1 stands on the line from camera 0 to the joint, camera 2 does not see channel 0 in frame 0."""
    ring = ring_cameras(3, 2)
    joint = np.asarray(TARGET)
    ring[1, 1] = ring[1, 0] + 0.45 * (joint - ring[1, 0])
    c = scene(3, 3, 9, cams=look_at_cameras(ring), painted=False)
    c["truth"][0, 0, 0] = joint
    c["poses"][0, 0, 0, :3] = joint + (6.0, -4.0, 3.0)
    paint(c, c["truth"], c["amps"])
    c["heat"][0, 2, :, :, 0] = 0.0
    return _expect(c, view_state={(0, 0, 0, 0): UNSOLVED, (0, 1, 0, 0): UNSOLVED, (0, 2, 0, 0): PEAK_LOW},
                   tri_count={(0, 0, 0): -1, (0, 0, 1): 3})


def _flat_top():
    """den == 0: the cells (1 - 2^-24, 1, 1) along x; a NaN neighbour along y of another joint."""
    c = scene(3, 3, 10)
    cx, cy = centres(c)
    x, y = int(cx[0, 0, 1, 1]), int(cy[0, 0, 1, 1])
    wipe(c, 0, 0, 1, x, y)
    put(c, 0, 0, 1, x - 1, y, np.nextafter(f32(1), f32(0)))
    put(c, 0, 0, 1, x, y, 1.0)
    put(c, 0, 0, 1, x + 1, y, 1.0)
    x2, y2 = int(cx[1, 2, 0, 2]), int(cy[1, 2, 0, 2])
    wipe(c, 1, 2, 2, x2, y2)
    put(c, 1, 2, 2, x2, y2, 0.7)
    put(c, 1, 2, 2, x2, y2 + 1, NAN)
    put(c, 1, 2, 2, x2 + 1, y2, 0.6)
    return _expect(c, view_state={(0, 0, 1, 1): USED, (1, 2, 0, 2): USED}, cell={(0, 0, 1, 1): (x, y), (1, 2, 0, 2): (x2 + 0.375, y2)})


def _delta_clamp():
    """min_peak < 0 and a negative peak on row 0 of the map: the neighbour outside the map (0) is larger than the peak."""
    c = _map_border_row()
    c["params"] = dict(min_peak=-1.0)
    cx, cy = centres(c)
    x, y = int(cx[0, 1, 0, 1]), int(cy[0, 1, 0, 1])
    wipe(c, 0, 1, 1, x, y, value=-0.9)
    put(c, 0, 1, 1, x, 0, -0.1)
    put(c, 0, 1, 1, x, 1, -0.5)
    return _expect(c, view_state={(0, 1, 0, 1): USED}, cell={(0, 1, 0, 1): (x, -0.5)})


def _displaced(seed, V, shifts, **params):
    """Joint (0, 0, 0): the peak of view v sits ``shifts[v]`` cells beside the true projection."""
    c = scene(V, 3, seed, params=params, painted=False)
    skip = {(0, v, 0, 0) for v in shifts}
    paint(c, c["truth"], c["amps"], skip=skip)
    hx, hy, _ = cells_of(c, c["truth"])
    for v, (sx, sy) in shifts.items():
        cxy = centres(c)
        wipe(c, 0, v, 0, int(cxy[0][0, v, 0, 0]), int(cxy[1][0, v, 0, 0]))
        blob(c, 0, v, 0, hx[0, v, 0, 0] + sx, hy[0, v, 0, 0] + sy, amp=0.9)
    return c


def _reject_one():
    c = _displaced(11, 5, {2: (1.8, -0.9)}, reject_px=3.0)
    return _expect(c, view_state={(0, 2, 0, 0): REJECTED, (0, 0, 0, 0): USED}, tri_count={(0, 0, 0): 4, (0, 0, 1): 5})


def _reject_cascade():
    """Two displaced peaks: the first round drops the worse one only; a second round - which is not made - would drop the other."""
    c = _displaced(31, 5, {1: (0.0, 2.2), 3: (0.4, 1.5)}, reject_px=3.75)
    return _expect(c, view_state={(0, 1, 0, 0): REJECTED, (0, 3, 0, 0): USED}, tri_count={(0, 0, 0): 4})


def _reject_too_few():
    c = _displaced(13, 3, {0: (1.8, 0.9)}, reject_px=3.0, min_views=3)
    return _expect(c, view_state={(0, v, 0, 0): USED for v in range(3)}, tri_count={(0, 0, 0): 3})


def _absent():
    c = scene(3, 5, 14)
    c["poses"][0, 1, 0, 3] = -1.0
    c["ids"] = np.asarray([[4, 9], [-1, 2]], np.int32)
    vs = {(0, v, 1, j): NOT_EVALUATED for v in range(3) for j in range(5)}
    vs.update({(1, v, 0, j): NOT_EVALUATED for v in range(3) for j in range(5)})
    return _expect(c, view_state=vs, tri_count={(0, 1, 0): -2, (1, 0, 4): -2, (0, 0, 0): 3, (1, 1, 1): 3})


def _nan_joint():
    c = scene(3, 5, 15)
    c["poses"][0, 0, 1, 0] = NAN
    c["poses"][1, 1, 3, 2] = -INF
    c["poses"][1, 0, 4, 1] = 1e30
    return _expect(c, view_state={(0, 1, 0, 1): OUTSIDE, (1, 2, 1, 3): OUTSIDE, (1, 0, 0, 4): OUTSIDE},
                   tri_count={(0, 0, 1): 0, (1, 1, 3): 0, (1, 0, 4): 0})


def _frame_set_range():
    c = scene(3, 3, 16, B=2, frame_set=(2, 1))             # two sets: row 2 is outside the table
    c2 = scene(3, 3, 16, B=2, frame_set=(-1, 0))
    c["poses"][1], c["heat"][1], c["frame_set"] = c2["poses"][1], c2["heat"][1], np.asarray([2, 0], np.int32)
    vs = {(0, v, n, j): NOT_EVALUATED for v in range(3) for n in range(2) for j in range(3)}
    return _expect(c, view_state=vs, tri_count={(0, 0, 0): -2, (1, 0, 0): 3})


def _no_undistortion():
    return _expect(scene(4, 5, 17, params=dict(iters=0)), tri_count={(0, 0, 0): 4})


def random_scene(V, J, seed, B=2, N=2, radius=3, reject_px=2.5, shape=(H, W)):
    """The painted scene, spoiled: displaced and weak peaks, NaN and negative cells, occluded views, absent people."""
    rng = np.random.default_rng(seed)
    c = scene(V, J, seed, B=B, N=N, params=dict(radius=radius, reject_px=reject_px), painted=False,
              frame_set=rng.integers(0, 2, B))
    c["amps"] = rng.uniform(0.1, 1.3, (B, V, N, J))
    hx, hy, depth = cells_of(c, c["truth"])
    for idx in np.ndindex(B, V, N, J):
        if depth[idx] > 0 and rng.uniform() > 0.05:
            d = rng.uniform(-2.5, 2.5, 2) * (rng.uniform() < 0.25)
            blob(c, idx[0], idx[1], idx[3], hx[idx] + d[0], hy[idx] + d[1], amp=c["amps"][idx])
    noise = rng.uniform(size=c["heat"].shape)
    c["heat"] = np.where(noise < 0.003, NAN, np.where(noise < 0.006, -0.5, c["heat"])).astype(f32)
    c["occluder"] = np.where(rng.uniform(size=(B, V, N, J)) < 0.1, rng.integers(-2, N, (B, V, N, J)), -1).astype(np.int32)
    c["ids"] = np.where(rng.uniform(size=(B, N)) < 0.2, -1, rng.integers(0, 50, (B, N))).astype(np.int32)
    c["poses"][..., 0] = np.where(rng.uniform(size=(B, N, J)) < 0.04, rng.choice([NAN, INF, 1e30], (B, N, J)), c["poses"][..., 0])
    return c


BUILDERS = {
    "argmax_tie": _argmax_tie, "window_border": _window_border, "map_border_row": _map_border_row, "peak_low": _peak_low,
    "behind_camera": _behind_camera, "window_outside": _window_outside, "occluded": _occluded,
    "one_view_short": _one_view_short, "collinear": _collinear, "flat_top": _flat_top, "delta_clamp": _delta_clamp,
    "reject_one": _reject_one, "reject_cascade": _reject_cascade, "reject_too_few": _reject_too_few, "absent": _absent,
    "nan_joint": _nan_joint, "frame_set_range": _frame_set_range, "no_undistortion": _no_undistortion,
    "random_v3_j3": lambda: random_scene(3, 3, 21, radius=2), "random_v5_j5": lambda: random_scene(5, 5, 22, B=3),
}
# the scene that tells each wrong reading of the definition from the definition
TELLS = {"no_border": "window_border", "tie_last": "argmax_tie", "neighbours_clamped": "map_border_row",
         "no_delta_clamp": "delta_clamp", "unit_weights": "reject_one", "descending_views": "random_v5_j5",
         "no_undistort": "occluded", "no_rt_inverse": "peak_low", "reject_twice": "reject_cascade", "ignore_occluder": "occluded"}
CASES = list(BUILDERS)
_cache = {}


def get(name):
    """(case, outputs of the yardstick) - computed once, shared, never modified."""
    if name not in _cache:
        case = BUILDERS[name]()
        _cache[name] = (case, reference(case))
    return _cache[name]


def differs(a, b):
    """The names of the outputs whose bits differ."""
    return [k for k in OUTPUTS if not np.array_equal(bits(a[k]) if a[k].dtype.kind == "f" else a[k],
                                                     bits(b[k]) if b[k].dtype.kind == "f" else b[k])]


def check_expectations(name):
    """The yardstick gives every named entry of a constructed scene the value the scene was built for."""
    case, want = get(name)
    exp = case["expect"]
    assert exp, name
    for idx, val in exp.get("view_state", {}).items():
        assert want["view_state"][idx] == val, (name, idx, int(want["view_state"][idx]), val)
    for idx, val in exp.get("tri_count", {}).items():
        assert want["tri_count"][idx] == val, (name, idx, int(want["tri_count"][idx]), val)
    inv = np.asarray(inverse_transform(case["geom"]), f64)
    for idx, (qx, qy) in exp.get("cell", {}).items():      # the refined peak, in heat-map cells
        ox, oy = want["obs"][idx][:2]
        assert abs(inv[0] * qx + inv[1] * qy + inv[2] - ox) < 1e-3 and abs(inv[3] * qx + inv[4] * qy + inv[5] - oy) < 1e-3, \
            (name, idx, (qx, qy), (ox, oy))


# ======================================================================================================================
# runners
# ======================================================================================================================
SHAPES = dict(tri_poses=lambda B, V, N, J: (B, N, J, 5), tri_count=lambda B, V, N, J: (B, N, J),
              tri_stats=lambda B, V, N, J: (B, N, J, 2), obs=lambda B, V, N, J: (B, V, N, J, 4),
              view_state=lambda B, V, N, J: (B, V, N, J), cam_resid=lambda B, V, N, J: (B, V), cam_count=lambda B, V, N, J: (B, V))
INT_FILL = -77
FENCE_CELLS = 4096                                          # floats of 1e30 before and behind the heat maps


def _torch():
    import torch
    return torch


def _dev(a, device):
    if a is None:
        return None
    t = _torch().from_numpy(np.ascontiguousarray(a).copy())
    return t if str(device) == "cpu" else t.to(device)


def _ptr(t, offset=0):
    return None if t is None else C.c_void_p(t.data_ptr() + offset)


def geom_struct(geom, V, J):
    from faster_voxelpose_amd import _capi as capi
    g = capi.FvpGeom()
    g.clamp_max = float(geom["clamp_max"])
    for i in range(6):
        g.rt[i] = float(geom["rt"][i])
    g.hm_w, g.hm_h = float(geom["W"]), float(geom["H"])
    g.img_w, g.img_h = float(geom["img"][0]), float(geom["img"][1])
    g.W, g.H, g.V, g.J, g.JP = geom["W"], geom["H"], V, J, 4 * ((J + 3) // 4)
    return g


def call(lib, device, case, outs=OUTPUTS, fenced=False, **over):
    """fvp_triangulate_joints on ``device``; returns (rc, {name: numpy or None}).  The outputs start filled with sentinels (NaN,
    -77).  ``fenced``: the heat maps sit inside a larger allocation whose margins hold 1e30.  ``over``: arguments that replace
    the case's (B, N, nsets, V, J, JP, W, H, rt, any parameter of DEFAULTS, null=<names of pointers passed as NULL>)."""
    torch = _torch()
    B, N, J = case["poses"].shape[:3]
    V = case["cams"].shape[1]
    heat = case["heat"]
    if fenced:
        heat = np.concatenate([np.full(FENCE_CELLS, 1e30, f32), heat.reshape(-1), np.full(FENCE_CELLS, 1e30, f32)])
    t = dict(heat=_dev(heat, device), cams=_dev(case["cams"], device), frame_set=_dev(case["frame_set"], device),
             poses=_dev(case["poses"], device), ids=_dev(case.get("ids"), device), occluder=_dev(case.get("occluder"), device))
    o = {}
    for k in OUTPUTS:
        shape = SHAPES[k](B, V, N, J)
        fill = np.full(shape, NAN, f32) if k in ("tri_poses", "tri_stats", "obs", "cam_resid") else np.full(shape, INT_FILL, np.int32)
        o[k] = _dev(fill, device) if k in outs else None
    a = dict(heat=_ptr(t["heat"], 4 * FENCE_CELLS if fenced else 0), cams=_ptr(t["cams"]), frame_set=_ptr(t["frame_set"]),
             poses=_ptr(t["poses"]), ids=_ptr(t["ids"]), occluder=_ptr(t["occluder"]))
    for k in over.get("null", ()):
        a[k] = None
    geom = dict(case["geom"], **{k: over[k] for k in ("W", "H", "rt") if k in over})
    g = geom_struct(geom, over.get("V", V), over.get("J", J))
    if "JP" in over:
        g.JP = over["JP"]
    prm = {**DEFAULTS, **case.get("params", {}), **{k: over[k] for k in DEFAULTS if k in over}}
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream) if str(device).startswith("cuda") else None
    rc = lib.fvp_triangulate_joints(a["heat"], a["cams"], over.get("nsets", case["cams"].shape[0]), a["frame_set"], a["poses"],
                                    a["ids"], a["occluder"], over.get("B", B), over.get("N", N),
                                    None if "g" in over.get("null", ()) else C.byref(g), int(prm["radius"]),
                                    float(prm["min_peak"]), int(prm["iters"]), int(prm["min_views"]), float(prm["min_det"]),
                                    float(prm["reject_px"]), *[_ptr(o[k]) for k in OUTPUTS], stream)
    if str(device).startswith("cuda"):
        torch.cuda.synchronize()
    return rc, {k: None if v is None else v.cpu().numpy() for k, v in o.items()}


def assert_equal(got, want, what):
    for k in OUTPUTS:
        if got.get(k) is None:
            continue
        g, w = got[k], want[k]
        same = np.array_equal(bits(g), bits(w)) if w.dtype.kind == "f" else np.array_equal(g, w)
        if not same:
            bad = np.argwhere((bits(g) != bits(w)) if w.dtype.kind == "f" else (g != w))
            raise AssertionError((what, k, len(bad), bad[:4].tolist(), g[tuple(bad[0])], w[tuple(bad[0])]))


def check(lib, device, name):
    case, want = get(name)
    rc, got = call(lib, device, case)
    assert rc == 0, rc
    assert_equal(got, want, name)


def untouched(got):
    return all(v is None or (np.isnan(v).all() if v.dtype.kind == "f" else (v == INT_FILL).all()) for v in got.values())


def check_null_outputs(lib, device):
    """Any output may be NULL, not all of them; cam_resid and cam_count are reduced from obs and view_state and need both.
    Every one of the 127 combinations: the allowed ones give the yardstick's bits in the outputs that are there, the others
    FVP_EINVAL with nothing written."""
    case, want = get("random_v5_j5")
    for m in range(1, 128):
        outs = tuple(k for i, k in enumerate(OUTPUTS) if (m >> i) & 1)
        allowed = not ({"cam_resid", "cam_count"} & set(outs)) or {"obs", "view_state"} <= set(outs)
        rc, got = call(lib, device, case, outs=outs)
        assert [k for k in OUTPUTS if got[k] is not None] == list(outs)
        if allowed:
            assert rc == 0, (outs, rc)
            assert_equal(got, want, outs)
        else:
            assert rc == EINVAL and untouched(got), (outs, rc)
    rc, got = call(lib, device, case, outs=())
    assert rc == EINVAL
    for k in ("ids", "occluder"):                          # both inputs may be NULL: the result is that of the scene without
        rc, got = call(lib, device, case, null=(k,))
        assert rc == 0
        assert_equal(got, reference({**case, k: None}), k + " = NULL")
        assert differs(got, want)


def argument_errors(lib, device):
    """Every FVP_EINVAL / FVP_ELIMIT condition of the header returns its code and leaves pre-filled outputs untouched."""
    case, _ = get("reject_one")
    bad = [dict(null=("heat",)), dict(null=("cams",)), dict(null=("frame_set",)), dict(null=("poses",)), dict(null=("g",)),
           dict(B=-1), dict(N=0), dict(nsets=0), dict(radius=0), dict(radius=-1), dict(min_views=1), dict(min_views=0),
           dict(iters=-1), dict(min_peak=NAN), dict(min_peak=INF), dict(min_det=NAN), dict(min_det=-INF),
           dict(reject_px=NAN), dict(reject_px=INF), dict(JP=12), dict(W=1), dict(H=0),
           dict(rt=[0.5, 0.0, 1.5, 1.0, 0.0, -0.75]), dict(rt=[NAN, 0.0, 1.5, 0.0, 0.5, -0.75])]
    for over in bad:
        rc, got = call(lib, device, case, **over)
        assert rc == EINVAL, (over, rc)
        assert untouched(got), over
    for over in (dict(J=MAX_JOINTS + 1, JP=36), dict(V=MAX_VIEWS + 1), dict(radius=MAX_RADIUS + 1), dict(iters=MAX_ITERS + 1)):
        rc, got = call(lib, device, case, **over)
        assert rc == ELIMIT, (over, rc)
        assert untouched(got), over
    rc, got = call(lib, device, case, B=0)                  # no launch: nothing written
    assert rc == 0 and untouched(got)
    for over in (dict(radius=MAX_RADIUS), dict(iters=MAX_ITERS), dict(reject_px=-1.0)):   # the limits themselves are fine
        rc, got = call(lib, device, case, **over)
        assert rc == 0, over
        assert_equal(got, reference(dict(case, params={**case["params"], **over})), over)


def fence_case():
    """Window centres at the map's four corners, just outside, far outside, and at +-1e30, +-inf and NaN: with 1e30 in the
    allocation around the heat maps, a single cell read outside the map would win its window."""
    c = scene(3, 5, 41, B=1, N=2, frame_set=(0,), painted=False)
    cm = c["cams"][0, 0].astype(f64)
    right, down, fw, centre = cm[0:3], cm[3:6], cm[6:9], cm[9:12]
    dist = np.linalg.norm(np.asarray(TARGET) - centre)

    def at(px, py):                                        # the point at `dist` whose pixel in view 0 is about (px, py)
        return centre + dist * (fw + right * (px - 96.0) / 250.0 + down * (py - 64.0) / 250.0)

    inv = np.asarray(inverse_transform(c["geom"]), f64)
    cells = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (-2, -2), (W + 1, H + 1), (-3.4, 10), (W + 2.4, 10), (-40, -40), (400, 9)]
    pts = [at(inv[0] * x + inv[2], inv[4] * y + inv[5]) for x, y in cells]
    c["truth"] = np.asarray(pts, f64).reshape(1, 2, 5, 3)
    c["poses"][..., :3] = c["truth"]
    paint(c, c["truth"], c["amps"])
    c["heat"][0, 0, 0, 0, :] = c["heat"][0, 0, H - 1, W - 1, :] = 0.95           # a peak in the very corner cells
    far = scene(3, 5, 42, B=1, N=2, frame_set=(0,))
    far["poses"][0, :, :, 0] = np.asarray([[1e30, -1e30, INF, -INF, NAN], [3e38, -3e38, 1e20, -1e20, 1e12]], f32)
    c["poses"], c["heat"] = np.concatenate([c["poses"], far["poses"]]), np.concatenate([c["heat"], far["heat"]])
    c["frame_set"] = np.zeros(2, np.int32)
    return c


BUILDERS["fence"] = fence_case
CASES.append("fence")


def check_fence(lib, device):
    case, want = get("fence")
    vs = want["view_state"]
    assert (vs == OUTSIDE).any() and (vs == USED).any() and (vs[1] == OUTSIDE).sum() >= 3 * 8
    rc, got = call(lib, device, case, fenced=True)
    assert rc == 0
    assert_equal(got, want, "fenced")
    assert not (np.nan_to_num(got["obs"][..., 2]) > 2.0).any()                  # no 1e30 was ever a peak


# ======================================================================================================================
# host side: the class and the model attribute against the yardstick
# ======================================================================================================================
class Cfg:
    """The fields JointTriangulator reads, for the rig of the constructed scenes."""

    def __init__(self, J, geom=GEOM, ori=(192, 128)):
        from types import SimpleNamespace as NS
        self.DATASET = NS(NUM_JOINTS=J, HEATMAP_SIZE=[geom["W"], geom["H"]], IMAGE_SIZE=list(geom["img"]), ORI_IMAGE_SIZE=list(ori))


def triangulator_for(case, lib=None, **kw):
    from faster_voxelpose_amd.utils.triangulate import JointTriangulator
    prm = {**DEFAULTS, **case.get("params", {})}
    return JointTriangulator(Cfg(case["poses"].shape[2], case["geom"]), radius=prm["radius"], min_peak=prm["min_peak"],
                             undistort_iters=prm["iters"], min_views=prm["min_views"], min_det=prm["min_det"],
                             reject_px=prm["reject_px"], resize_transform=np.asarray(case["geom"]["rt"], f32).reshape(2, 3),
                             **({} if lib is None else dict(_lib=lib)), **kw)


KEYS = ("poses", "cams", "frame_set", "heat", "occluder", "ids")


def tensors(case, device):
    return {k: _dev(case.get(k), device) for k in KEYS}


def run_class(tri, t):
    return tri(t["poses"], t["cams"], t["frame_set"], t["heat"], occluder=t["occluder"], ids=t["ids"])


def as_dict(out):
    return {k: None if v is None else v.cpu().numpy() for k, v in zip(OUTPUTS, out)}


def model_case(model, cfg, rt, heat, meta, cams, out, occluder=None):
    """The scene a forward with model.triangulator has just worked on, for the yardstick."""
    V = heat.shape[1]
    g = model.engine.geom(rt)
    g.V = V
    hcl = model.engine.heat_cl(heat, g).cpu().numpy()
    fs = model.engine.frame_sets(meta, cams, V)
    tri = model.triangulator
    ds = cfg.DATASET
    geom = dict(rt=[float(x) for x in np.asarray(rt.cpu(), f32).reshape(6)], W=int(ds.HEATMAP_SIZE[0]), H=int(ds.HEATMAP_SIZE[1]),
                img=(float(ds.IMAGE_SIZE[0]), float(ds.IMAGE_SIZE[1])), clamp_max=float(max(ds.ORI_IMAGE_SIZE)))
    return dict(poses=out[0].cpu().numpy(), cams=model.engine.geo.cams.cpu().numpy(), frame_set=fs.cpu().numpy(), geom=geom,
                heat=hcl, ids=None, occluder=None if occluder is None else occluder.cpu().numpy(),
                params=dict(radius=tri.radius, min_peak=tri.min_peak, iters=tri.undistort_iters, min_views=tri.min_views,
                            min_det=tri.min_det, reject_px=tri.reject_px))


# ======================================================================================================================
# the definition against the truth (tests/golden/make_triangulate_floor.py writes tests/golden/triangulate_floor.json)
# ======================================================================================================================
FLOOR_JSON = os.path.join(HERE, "golden", "triangulate_floor.json")
PANOPTIC = dict(W=240, H=128, img=(960.0, 512.0), ori=(1920, 1080), clamp_max=1920.0)


def panoptic_rig():
    """The five distorted cameras of tests/golden/calibration_panoptic_demo.json as [1,5,24] records and the dataset's geometry
    (heat maps of 240x128 for images of 960x512 cut out of 1920x1080 frames; the resize transform of the dataset:
    scale 0.5, the 28 rows of letterbox taken off)."""
    with open(os.path.join(HERE, "golden", "calibration_panoptic_demo.json")) as f:
        raw = json.load(f)["customized_sequence"]
    cams = np.zeros((1, len(raw), CAM_FLOATS), f32)
    for v, c in enumerate(raw):
        cams[0, v, :9] = np.asarray(c["R"], f64).reshape(9)
        cams[0, v, 9:12] = np.asarray(c["T"], f64).reshape(3)
        cams[0, v, 12:16] = c["fx"], c["fy"], c["cx"], c["cy"]
        cams[0, v, 16:19] = np.asarray(c["k"], f64).reshape(3)
        cams[0, v, 19:21] = np.asarray(c["p"], f64).reshape(2)
    s = 960.0 / 1920.0
    geom = dict(PANOPTIC, rt=[s, 0.0, 0.0, 0.0, s, (512.0 - 1080.0 * s) / 2.0])
    return cams, geom


def floor_scene(seed, shape="paraboloid", N=2, J=15, offset=20.0, radius=3):
    """Points with known 3-D positions inside the true field of view of at least three of the Panoptic cameras (undistorted
    radius^2 below 0.9 - the fixture's radial polynomial folds beyond that - and the pixel inside the frame), every heat-map
    peak an exact paraboloid ``max(1 - a*dist^2, 0)`` (or a Gaussian of sigma 3) at the true projection; the fused input is the
    truth plus ``offset`` mm in a seeded direction."""
    rng = np.random.default_rng(seed)
    cams, geom = panoptic_rig()
    V = cams.shape[1]
    truth = np.zeros((1, N, J, 3))
    cm = cams[0].astype(f64)
    taken = [[] for _ in range(J)]
    for n in range(N):
        for j in range(J):
            while True:
                p = np.asarray([rng.uniform(-1500, 1500), rng.uniform(-1500, 1500), rng.uniform(100, 1800)])
                xc = np.einsum("vik,vk->vi", cm[:, :9].reshape(V, 3, 3), p - cm[:, 9:12])
                y = xc[:, :2] / xc[:, 2:3]
                r2 = (y ** 2).sum(-1)
                px = project_pixel(cm, p[0], p[1], p[2], f64)
                infov = (xc[:, 2] > 0) & (r2 < 0.9) & (px[0] > 40) & (px[0] < 1880) & (px[1] > 40) & (px[1] < 1040)
                hp = cells_of(dict(cams=cams, frame_set=np.zeros(1, np.int32), geom=geom), p.reshape(1, 1, 1, 3))
                hp = np.stack([hp[0], hp[1]], -1).reshape(V, 2)
                # the people share the joint's channel: their peaks stay 16 cells apart in every view
                apart = all(np.abs(hp - q).max(-1).min() >= 16 for q in taken[j])
                if infov.sum() >= 3 and apart:
                    taken[j].append(hp)
                    break
            truth[0, n, j] = p
    step = rng.standard_normal((1, N, J, 3))
    poses = np.zeros((1, N, J, 5), f32)
    poses[..., :3] = truth + offset * step / np.linalg.norm(step, axis=-1, keepdims=True)
    poses[..., 3], poses[..., 4] = 0.5, 0.5
    case = dict(poses=poses, cams=cams, frame_set=np.zeros(1, np.int32), geom=geom, ids=None, occluder=None,
                heat=np.zeros((1, V, geom["H"], geom["W"], 4 * ((J + 3) // 4)), f32), params=dict(radius=radius), truth=truth)
    hx, hy, depth = cells_of(case, truth)
    xc = np.einsum("vik,njvk->vnji", cm[:, :9].reshape(V, 3, 3), truth[0][:, :, None, :] - cm[:, 9:12])
    r2 = ((xc[..., :2] / xc[..., 2:3]) ** 2).sum(-1)[None]
    for idx in np.ndindex(1, V, N, J):
        # a view shows a joint whole or not at all: a peak cut off by the map's border would be taken at the border cell, with
        # the missing neighbour read as 0 (seen in a first version of this scene: 12 mm off the truth)
        if depth[idx] > 0 and r2[idx] < 0.9 and 2 <= hx[idx] <= geom["W"] - 3 and 2 <= hy[idx] <= geom["H"] - 3:
            blob(case, 0, idx[1], idx[3], hx[idx], hy[idx], amp=1.0, a=0.04, shape=shape)
    return case


def floor_figures(case, got_x=None, got_state=None):
    """(largest |X64 - truth|, largest |X32 - X64|, share of joint-views whose state differs between fp32 and fp64, share of
    evaluated joints that are triangulated) over the joints triangulated with the same views in both precisions; ``got_x`` /
    ``got_state``: a kernel's tri_poses / view_state to measure instead of the float32 yardstick's."""
    w64 = reference(case, dt=f64)
    if got_x is None:
        w32 = reference(case)
        got_x, got_state = w32["tri_poses"], w32["view_state"]
    same = (got_state == w64["view_state"]).all(1) & (w64["tri_count"] >= 2)
    x64, x32 = w64["tri_poses"][..., :3], got_x[..., :3].astype(f64)
    d_truth = np.linalg.norm(x64 - case["truth"], axis=-1)[same]
    d_prec = np.linalg.norm(x32 - x64, axis=-1)[same]
    ev = w64["tri_count"] != -2
    return dict(fp64_to_truth_mm=float(d_truth.max()), fp32_to_fp64_mm=float(d_prec.max()),
                kernel_to_truth_mm=float(np.linalg.norm(x32 - case["truth"], axis=-1)[same].max()),
                state_mismatch_share=float((got_state != w64["view_state"]).mean()),
                triangulated_share=float((w64["tri_count"] >= 2)[ev].mean()), joints_compared=int(same.sum()),
                not_enclosed_share=float((w64["view_state"] == NOT_ENCLOSED).mean()))


def floor():
    with open(FLOOR_JSON) as f:
        return json.load(f)


def check_floor(lib, device):
    """The kernel's X within 2 x ((a) + (b)) of the truth, (a) the float64 yardstick's largest distance from the truth and
    (b) the float32 yardstick's largest distance from the float64 one, both measured by the generator on another seed and
    committed; the factor 2 covers only the different rounding of a different seed's sample.  At most 5 % of the joint-views
    are left out because fp32 and fp64 disagree on a state; at least 90 % of the evaluated joints are triangulated."""
    fl = floor()
    for kind in ("paraboloid", "gaussian"):
        case = floor_scene(fl["test_seed"], shape=kind)
        rc, got = call(lib, device, case)
        assert rc == 0
        fig = floor_figures(case, got["tri_poses"], got["view_state"])
        bound = 2.0 * (fl[kind]["fp64_to_truth_mm"] + fl[kind]["fp32_to_fp64_mm"])
        print(f"{kind}: kernel to truth {fig['kernel_to_truth_mm']:.3g} mm, bound {bound:.3g} mm; {fig}")
        assert fig["joints_compared"] >= 20
        assert fig["kernel_to_truth_mm"] <= bound, (kind, fig, bound)
        assert fig["state_mismatch_share"] <= 0.05 and fig["triangulated_share"] >= 0.90, (kind, fig)


def panoptic_scene(B, N, seed, J=15, offset=20.0, radius=3):
    """tools/bench_triangulate.py: B frames of N people in the Panoptic rig, joints uniform in the capture volume, a paraboloid
    wherever a view shows the joint, the people's peaks sharing the joint's channel as they fall."""
    rng = np.random.default_rng(seed)
    cams, geom = panoptic_rig()
    V = cams.shape[1]
    truth = np.stack([rng.uniform(-1500, 1500, (B, N, J)), rng.uniform(-1500, 1500, (B, N, J)), rng.uniform(100, 1800, (B, N, J))], -1)
    step = rng.standard_normal((B, N, J, 3))
    poses = np.zeros((B, N, J, 5), f32)
    poses[..., :3] = truth + offset * step / np.linalg.norm(step, axis=-1, keepdims=True)
    poses[..., 3], poses[..., 4] = 0.5, 0.5
    case = dict(poses=poses, cams=cams, frame_set=np.zeros(B, np.int32), geom=geom, ids=None, occluder=None,
                heat=np.zeros((B, V, geom["H"], geom["W"], 4 * ((J + 3) // 4)), f32), params=dict(radius=radius), truth=truth)
    paint(case, truth, np.ones((B, V, N, J)), a=0.04)
    return case
