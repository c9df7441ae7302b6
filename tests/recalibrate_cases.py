"""Cases and the yardstick of fvp_camera_refit_accumulate / fvp_camera_refit_solve (include/fvp.h, ABI 19), shared by
tests/test_recalibrate_emu.py (CPU emulator), tests/test_recalibrate_gpu.py (the shipped library on the card),
tests/golden/make_refit_floor.py and tools/bench_refit.py: an independent numpy float64 restatement of the header's
definition, vectorised over (frame, view, person, joint) for the accumulation and over the cameras for the solve - every
numpy operation rounds once, as the header demands; the undistortion is the float32 one of tests/triangulate_cases.py - the
constructed scenes with what each of them is about, the wrong readings of the definition (mutants) the scenes must tell
apart, and runners that call the entry points on torch memory (CPU for the emulator, the card otherwise) with guard
elements around every buffer.  Outputs are compared bit for bit: no tolerance anywhere but in the floor test, whose bound
comes from tests/golden/refit_floor.json."""
import ctypes as C
import json
import os

import numpy as np

from triangulate_cases import _poly, look_at_cameras, project_pixel

f32, f64 = np.float32, np.float64
NAN, INF = float("nan"), float("inf")
EINVAL, ELIMIT = 10001, 10002
MAX_JOINTS, MAX_VIEWS, MAX_ITERS, CAM_FLOATS, ACC = 32, 8, 16, 24, 32
FLT_MAX = f32(np.finfo(f32).max)
DBL_MAX = np.finfo(f64).max
USED = 1
OK, CLAMPED, FEW, DEGENERATE = 1, 2, 0, -1
DEFAULTS = dict(iters=8, huber_px=0.0, decay=1.0, min_obs=60, lam=0.0, min_pivot=1e-9, max_angle=np.deg2rad(5.0), max_shift=200.0)
MUTANTS = ("uv_swapped", "tau_sign", "t_from_r", "f_scale_missing", "decay_after_add", "fold_order", "huber_on_e2",
           "unscaled_pivot", "rodrigues")
SOLVE_OUTPUTS = ("cams_out", "cal_stats", "cal_state")
HERE = os.path.dirname(os.path.abspath(__file__))


def bits(a):
    """The bit pattern of a float32 / float64 array."""
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == f64 else np.uint32)


def _prm(case, **over):
    return {**DEFAULTS, **case.get("params", {}), **over}


# ======================================================================================================================
# the definition
# ======================================================================================================================
def _ut(i, k):
    return i * 6 - i * (i - 1) // 2 + (k - i)


def contributions(case, mutant=None):
    """Section 1 of the header: which observations count [B,V,N,J] and their 31 addends [B,V,N,J,31] (float64)."""
    pts, obs, vs, cams, fset = case["points"], case["obs"], case["view_state"], case["cams"], case["frame_set"]
    prm = _prm(case)
    nsets = cams.shape[0]
    ok_set = (fset >= 0) & (fset < nsets)
    with np.errstate(all="ignore"):
        cm32 = cams[np.where(ok_set, fset, 0)][:, :, None, None, :]                          # [B,V,1,1,24]
        X = pts[:, None, :, :, :3]                                                            # [B,1,N,J,3]
        ox, oy, pk = obs[..., 0], obs[..., 1], obs[..., 2]
        fin = (np.abs(X) <= FLT_MAX).all(-1) & (np.abs(ox) <= FLT_MAX) & (np.abs(oy) <= FLT_MAX)
        wf = np.fmin(np.fmax(pk, f32(0)), f32(1))
        u0, u1 = (ox - cm32[..., 14]) / cm32[..., 12], (oy - cm32[..., 15]) / cm32[..., 13]  # step 5, float32
        y0, y1 = u0, u1
        for _ in range(int(prm["iters"])):
            d, t0, t1, _, _, _ = _poly(cm32, y0, y1, f32)
            y0, y1 = (u0 - t0) / d, (u1 - t1) / d
        assert y0.dtype == f32 and wf.dtype == f32
        cm = cm32.astype(f64)
        R = [cm[..., i] for i in range(9)]
        d = [X[..., i].astype(f64) - cm[..., 9 + i] for i in range(3)]
        xc = [(R[3 * k] * d[0] + R[3 * k + 1] * d[1]) + R[3 * k + 2] * d[2] for k in range(3)]
        z = xc[2]
        iz, u, v = 1.0 / z, xc[0] / z, xc[1] / z
        f0, f1 = cm[..., 12], cm[..., 13]
        if mutant == "f_scale_missing":
            r0, r1 = y0.astype(f64) - u, y1.astype(f64) - v
        else:
            r0, r1 = (y0.astype(f64) - u) * f0, (y1.astype(f64) - v) * f1
        zero = np.zeros_like(u)
        Ju = [f0 * (-(u * v)), f0 * (1.0 + u * u), f0 * (-v), f0 * iz, zero, f0 * (-(u * iz))]
        Jv = [f1 * (-(1.0 + v * v)), f1 * (u * v), f1 * u, zero, f1 * iz, f1 * (-(v * iz))]
        if mutant == "uv_swapped":
            Ju, Jv = Jv, Ju
        e2 = r0 * r0 + r1 * r1
        e = np.sqrt(e2)
        hub = f64(f32(prm["huber_px"]))
        if mutant == "huber_on_e2":
            h = np.where((hub > 0) & (e2 > hub), hub / e2, 1.0)
        else:
            h = np.where((hub > 0) & (e > hub), hub / e, 1.0)
        ww = wf.astype(f64) * h
        counts = ok_set[:, None, None, None] & (vs == USED) & fin & (wf > 0) & (z > 1.0)
        terms = [ww * ((Ju[i] * Ju[k]) + (Jv[i] * Jv[k])) for i in range(6) for k in range(i, 6)]
        terms += [ww * ((Ju[i] * r0) + (Jv[i] * r1)) for i in range(6)]
        terms += [ww, ww * e2, np.ones_like(ww), (h < 1.0).astype(f64)]
    return counts, np.stack(terms, axis=-1)


def _fold(vals, mask, mutant=None):
    """The fixed reduction of one camera: vals [Q,31], mask [Q] -> [31]."""
    n = -(-len(mask) // 256) * 256
    vals = np.concatenate([vals, np.zeros((n - len(vals), 31))]).reshape(-1, 256, 31)
    mask = np.concatenate([mask, np.zeros(n - len(mask), bool)]).reshape(-1, 256)
    p = np.zeros((256, 31))
    with np.errstate(all="ignore"):
        for row, m in zip(vals, mask):
            p = np.where(m[:, None], p + row, p)
        if mutant == "fold_order":
            s = p[0]
            for t in range(1, 256):
                s = s + p[t]
            return s
        h = 128
        while h >= 1:
            p = p[:h] + p[h:2 * h]
            h //= 2
    return p[0]


def ref_accumulate(case, acc=None, mutant=None, **over):
    """acc [nsets,V,32] after one call of fvp_camera_refit_accumulate on ``acc`` (default: zeros)."""
    cams, fset = case["cams"], case["frame_set"]
    nsets, V = cams.shape[:2]
    acc = np.zeros((nsets, V, ACC)) if acc is None else acc.copy()
    if case["points"].shape[0] == 0:
        return acc
    counts, terms = contributions(case, mutant)
    decay = f64(f32(_prm(case, **over)["decay"]))
    with np.errstate(all="ignore"):
        for s in range(nsets):
            for v in range(V):
                m = (counts[:, v] & (fset == s)[:, None, None]).reshape(-1)
                p = _fold(terms[:, v].reshape(-1, 31), m, mutant)
                acc[s, v, :31] = (acc[s, v, :31] + p) * decay if mutant == "decay_after_add" else acc[s, v, :31] * decay + p
                acc[s, v, 31] = 0.0
    return acc


def ref_solve(acc, cams, prm=None, mutant=None, pivots=False):
    """Section 2 of the header over every camera: dict(cams_out [nsets,V,24] f32, cal_stats [nsets,V,6] f32, cal_state
    [nsets,V] int32).  ``pivots``: also the scaled pivots [nsets*V,6] and D [nsets*V,6]."""
    prm = {**DEFAULTS, **(prm or {})}
    nsets, V = cams.shape[:2]
    a, cm32 = acc.reshape(-1, ACC), cams.reshape(-1, CAM_FLOATS)
    lam, min_pivot = f64(f32(prm["lam"])), f64(f32(prm["min_pivot"]))
    max_angle, max_shift = f64(f32(prm["max_angle"])), f64(f32(prm["max_shift"]))
    with np.errstate(all="ignore"):
        Hm = lambda i, k: a[:, _ut(min(i, k), max(i, k))]                                    # noqa: E731
        g = [a[:, 21 + i] for i in range(6)]
        sw, se, count = a[:, 27], a[:, 28], a[:, 29]
        few = ~(count >= f64(int(prm["min_obs"])))
        deg = np.zeros(len(a), bool)
        for i in range(6):
            deg |= ~(Hm(i, i) > 0)
        D = [np.sqrt(Hm(i, i)) for i in range(6)]
        A = {(i, k): Hm(i, k) / (D[i] * D[k]) for i in range(6) for k in range(i)}
        for i in range(6):
            A[i, i] = Hm(i, i) / (D[i] * D[i]) + lam
        L, piv_all, minpiv = {}, [], None
        for j in range(6):
            piv = A[j, j]
            for k in range(j):
                piv = piv - L[j, k] * L[j, k]
            piv_all.append(piv)
            deg |= ~((piv * (D[j] * D[j]) if mutant == "unscaled_pivot" else piv) > min_pivot)
            minpiv = piv if j == 0 else np.where(piv < minpiv, piv, minpiv)
            L[j, j] = np.sqrt(piv)
            for i in range(j + 1, 6):
                t = A[i, j]
                for k in range(j):
                    t = t - L[i, k] * L[j, k]
                L[i, j] = t / L[j, j]
        y, zt = [None] * 6, [None] * 6
        for i in range(6):
            t = g[i] / D[i]
            for k in range(i):
                t = t - L[i, k] * y[k]
            y[i] = t / L[i, i]
        for i in range(5, -1, -1):
            t = y[i]
            for k in range(i + 1, 6):
                t = t - L[k, i] * zt[k]
            zt[i] = t / L[i, i]
        dl = [zt[i] / D[i] for i in range(6)]
        theta = np.sqrt((dl[0] * dl[0] + dl[1] * dl[1]) + dl[2] * dl[2])
        sigma = np.sqrt((dl[3] * dl[3] + dl[4] * dl[4]) + dl[5] * dl[5])
        deg |= ~((theta <= DBL_MAX) & (sigma <= DBL_MAX))
        gd = ((((g[0] * dl[0] + g[1] * dl[1]) + g[2] * dl[2]) + g[3] * dl[3]) + g[4] * dl[4]) + g[5] * dl[5]
        left = se - gd
        rms_before = np.where(sw > 0, np.sqrt(se / sw), 0.0)
        rms_pred = np.where(sw > 0, np.sqrt(np.where(left > 0, left, 0.0) / sw), 0.0)
        kappa = np.where(theta > max_angle, max_angle / theta, 1.0)
        k2 = max_shift / sigma
        kappa = np.where((sigma > max_shift) & (k2 < kappa), k2, kappa)
        clamp = kappa < 1.0
        dl = [np.where(clamp, x * kappa, x) for x in dl]
        theta = np.where(clamp, np.sqrt((dl[0] * dl[0] + dl[1] * dl[1]) + dl[2] * dl[2]), theta)
        sigma = np.where(clamp, np.sqrt((dl[3] * dl[3] + dl[4] * dl[4]) + dl[5] * dl[5]), sigma)
        if mutant == "rodrigues":
            th = np.sqrt((dl[0] * dl[0] + dl[1] * dl[1]) + dl[2] * dl[2])
            sa, cb = np.sin(th) / th, (1.0 - np.cos(th)) / (th * th)
            K = [[0 * th, -dl[2], dl[1]], [dl[2], 0 * th, -dl[0]], [-dl[1], dl[0], 0 * th]]
            Cm = [[(1.0 if i == k else 0.0) + sa * K[i][k] + cb * sum(K[i][m] * K[m][k] for m in range(3)) for k in range(3)]
                  for i in range(3)]
        else:
            h0, h1, h2 = 0.5 * dl[0], 0.5 * dl[1], 0.5 * dl[2]
            n = np.sqrt(1.0 + ((h0 * h0 + h1 * h1) + h2 * h2))
            qw, qx, qy, qz = 1.0 / n, h0 / n, h1 / n, h2 / n
            Cm = [[1.0 - 2.0 * (qy * qy + qz * qz), 2.0 * (qx * qy - qz * qw), 2.0 * (qx * qz + qy * qw)],
                  [2.0 * (qx * qy + qz * qw), 1.0 - 2.0 * (qx * qx + qz * qz), 2.0 * (qy * qz - qx * qw)],
                  [2.0 * (qx * qz - qy * qw), 2.0 * (qy * qz + qx * qw), 1.0 - 2.0 * (qx * qx + qy * qy)]]
        cm = cm32.astype(f64)
        R = [[cm[:, 3 * i + k] for k in range(3)] for i in range(3)]
        Rn = [[(Cm[i][0] * R[0][k] + Cm[i][1] * R[1][k]) + Cm[i][2] * R[2][k] for k in range(3)] for i in range(3)]
        Rt = R if mutant == "t_from_r" else Rn
        move = [(Rt[0][k] * dl[3] + Rt[1][k] * dl[4]) + Rt[2][k] * dl[5] for k in range(3)]
        Tn = [cm[:, 9 + k] + move[k] if mutant == "tau_sign" else cm[:, 9 + k] - move[k] for k in range(3)]
        solved = ~few & ~deg
        state = np.where(few, FEW, np.where(deg, DEGENERATE, np.where(clamp, CLAMPED, OK))).astype(np.int32)
        out = cm32.copy()
        new = np.stack([Rn[i][k] for i in range(3) for k in range(3)] + Tn, axis=-1).astype(f32)
        out[:, :12] = np.where(solved[:, None], new, cm32[:, :12])
        z = np.zeros(len(a))
        stats = np.stack([np.where(solved, theta, z), np.where(solved, sigma, z), rms_before, np.where(solved, rms_pred, z),
                          count, np.where(solved, minpiv, z)], axis=-1).astype(f32)
    res = dict(cams_out=out.reshape(nsets, V, CAM_FLOATS), cal_stats=stats.reshape(nsets, V, 6), cal_state=state.reshape(nsets, V))
    if pivots:
        res["pivots"], res["D"] = np.stack(piv_all, -1), np.stack(D, -1)
    return res


def ref_refine(case, iters=3, mutant=None):
    """``iters`` rounds of reset - accumulate - solve, each on the cameras of the round before: the last round's outputs."""
    cams, res = case["cams"], None
    for _ in range(iters):
        acc = ref_accumulate(dict(case, cams=cams), mutant=mutant, decay=1.0)
        res = ref_solve(acc, cams, _prm(case), mutant=mutant)
        cams = res["cams_out"]
    return res


# ======================================================================================================================
# scenes: look-at cameras with lens terms on a ring of 4 m, points in a 3 m x 3 m x 1.8 m volume, observations the exact
# (float64) projections through the TRUE cameras rounded to float32; the table handed to the calls holds bumped cameras
# ======================================================================================================================
def ring(V, nsets=1, radius=4000.0, height=1600.0, phase=0.3, **kw):
    ang = [[phase + s * 0.4 + 2 * np.pi * v / V for v in range(V)] for s in range(nsets)]
    centres = [[(radius * np.cos(a), radius * np.sin(a), height + 150.0 * (v % 3)) for v, a in enumerate(row)] for row in ang]
    return look_at_cameras(centres, f=1100.0, c=(960.0, 540.0), k=(-0.25, 0.15, -0.02), **kw)


def bump(rec, deg, mm, seed):
    """A camera record rotated by ``deg`` degrees about a seeded axis (camera frame) and its centre moved by ``mm``."""
    rng = np.random.default_rng(seed)
    ax = rng.standard_normal(3)
    ax /= np.linalg.norm(ax)
    t = np.deg2rad(deg)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    Rot = np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)
    sh = rng.standard_normal(3)
    out = rec.copy()
    out[:9] = (Rot @ rec[:9].astype(f64).reshape(3, 3)).reshape(9)
    out[9:12] = rec[9:12].astype(f64) + mm * sh / np.linalg.norm(sh)
    return out


def observe(true_cams, frame_set, points, noise=0.0, rng=None):
    """obs [B,V,N,J,4]: the float64 projection of the points through the true cameras, rounded to float32; peak 0.4..1."""
    B, N, J = points.shape[:3]
    nsets, V = true_cams.shape[:2]
    fs = np.where((frame_set >= 0) & (frame_set < nsets), frame_set, 0)
    cm = true_cams[fs].astype(f64)[:, :, None, None, :]
    X = points[:, None, :, :, :3].astype(f64)
    with np.errstate(all="ignore"):
        px, py, _ = project_pixel(cm, X[..., 0], X[..., 1], X[..., 2], f64)
    obs = np.zeros((B, V, N, J, 4), f32)
    rng = rng or np.random.default_rng(0)
    obs[..., 0], obs[..., 1] = px + noise * rng.standard_normal(px.shape), py + noise * rng.standard_normal(py.shape)
    obs[..., 2] = rng.uniform(0.4, 1.0, px.shape)
    obs[..., 3] = rng.uniform(0.0, 2.0, px.shape)                                              # the triangulation's residual: not read
    return obs


def scene(B, V, N, J, seed, nsets=1, frame_set=None, bumped=((0, 0, 1.5, 30.0),), noise=0.0, params=None):
    """``bumped``: (set, view, degrees, mm) of the cameras that moved since calibration."""
    rng = np.random.default_rng(seed)
    true = ring(V, nsets)
    cams = true.copy()
    for i, (s, v, deg, mm) in enumerate(bumped):
        cams[s, v] = bump(true[s, v], deg, mm, seed * 31 + i)
    fs = np.asarray(frame_set if frame_set is not None else [b % nsets for b in range(B)], np.int32)
    pts = np.zeros((B, N, J, 5), f32)
    pts[..., 0], pts[..., 1] = rng.uniform(-1500, 1500, (B, N, J)), rng.uniform(-1500, 1500, (B, N, J))
    pts[..., 2] = rng.uniform(0, 1800, (B, N, J))
    pts[..., 3], pts[..., 4] = 0.5, 0.5
    return dict(points=pts, obs=observe(true, fs, pts, noise, rng), view_state=np.full((B, V, N, J), USED, np.int32), cams=cams,
                true_cams=true, frame_set=fs, params=dict(params or {}), expect={})


def _smallest():
    return scene(1, 2, 1, 6, 3, params=dict(min_obs=6))


def _full_tree():
    c = scene(4, 3, 8, 8, 5)                                   # B*N*J = 256: every thread holds exactly one entry
    assert np.prod(c["points"].shape[:3]) == 256
    return c


def _second_trip():
    return scene(6, 3, 5, 9, 7)                                # 270 entries: threads 0..13 take a second trip


def _two_sets():
    """Two camera sets interleaved, one frame with a set index outside the table (and one negative)."""
    c = scene(8, 3, 5, 5, 9, nsets=2, frame_set=[0, 1, 1, 0, 2, 1, -1, 0], bumped=((0, 1, 1.0, 20.0), (1, 2, 2.0, 40.0)),
              params=dict(min_obs=60))
    c["expect"]["count"] = {(0, 0): 75, (0, 1): 75, (1, 2): 75}
    return c


def _eight_views():
    return scene(2, 8, 4, 5, 11, bumped=((0, 7, 1.0, 25.0), (0, 3, 0.5, 10.0)), params=dict(min_obs=30))


def _rejections():
    """One entry per rule that sets an observation aside, in view 0; view 1 keeps everything."""
    c = scene(2, 2, 3, 6, 13, params=dict(min_obs=6))
    vs, pts = c["view_state"], c["points"]
    for i, st in enumerate((0, -1, -2, -3, -4, -5)):            # every non-USED state of fvp_triangulate_joints
        vs[0, 0, 0, i] = st
    vs[0, 0, 1, 0] = -6
    vs[0, 0, 1, 1] = 2                                           # not a state: not USED either
    pts[0, 1, 2, 0], pts[0, 1, 3, 1], pts[0, 1, 4, 2] = NAN, INF, -INF      # joints (0,1,2..4): both views lose them
    # view 0 becomes an axis-aligned camera, so that a point can lie exactly 1 mm in front of it
    c["cams"][0, 0, :9] = np.asarray([[1, 0, 0], [0, 0, -1], [0, 1, 0]], f32).reshape(9)
    c["cams"][0, 0, 9:12] = np.asarray([100.0, -4000.0, 1000.0], f32)
    c["true_cams"][0, 0] = c["cams"][0, 0]
    c["obs"][:, 0] = observe(c["true_cams"], c["frame_set"], pts)[:, 0]
    obs = c["obs"]
    obs[0, 0, 2, 0, 0], obs[0, 0, 2, 1, 1], obs[0, 0, 2, 2, 0] = NAN, NAN, INF
    obs[0, 0, 2, 3, 2], obs[0, 0, 2, 4, 2], obs[0, 0, 2, 5, 2] = 0.0, -0.5, NAN         # peak 0, clamped to 0, NaN
    pts[1, 0, 0, :3] = (130.0, -3999.0, 1010.0)                  # z = 1.0 exactly in view 0
    pts[1, 0, 1, :3] = (130.0, -3998.5, 1010.0)                  # z = 1.5: counts
    pts[1, 0, 2, :3] = (130.0, -4100.0, 1010.0)                  # behind view 0
    obs[1, 0, 0, 0:3, 0:2] = (960.0, 540.0)
    obs[1, 1, 0, 0:3, 2] = 0.0                                   # (view 1 does not take these three)
    # view 0: 36 entries - 8 states - 3 points - 6 obs - 2 (z = 1, behind); view 1: 36 - 3 points - 3
    c["expect"]["count"] = {(0, 0): 36 - 8 - 3 - 6 - 2, (0, 1): 36 - 3 - 3}
    return c


def _huber(on):
    c = scene(2, 3, 4, 6, 17, bumped=((0, 0, 0.05, 1.0),), params=dict(huber_px=3.0 if on else 0.0, min_obs=40))
    c["obs"][0, 0, 1, 2, 0] += 80.0                              # one outlier in view 0
    c["expect"]["huber_count_min"] = {(0, 0): 1} if on else {}
    c["expect"]["huber_count"] = {} if on else {(0, 0): 0, (0, 1): 0}
    return c


def _few(n):
    c = scene(1, 2, 2, 5, 19, params=dict(min_obs=8))
    c["view_state"][0, 0].reshape(-1)[n:] = -2
    c["expect"]["count"] = {(0, 0): n}
    c["expect"]["state"] = {(0, 0): OK if n >= 8 else FEW}
    return c


def _coincident():
    c = scene(2, 2, 3, 5, 23, params=dict(min_obs=6))
    c["points"][..., :3] = c["points"][0, 0, 0, :3]
    c["obs"] = observe(c["true_cams"], c["frame_set"], c["points"])
    c["expect"]["state"] = {(0, 0): DEGENERATE, (0, 1): DEGENERATE}
    return c


def _zero_diagonal():
    """Every point of view 0 on the optical axis of an axis-aligned camera: u = v = 0, so H_22 (roll) is exactly 0."""
    c = scene(1, 2, 2, 5, 29, params=dict(min_obs=6))
    c["cams"][0, 0, :9] = np.asarray([[1, 0, 0], [0, 0, -1], [0, 1, 0]], f32).reshape(9)
    c["cams"][0, 0, 9:12] = np.asarray([0.0, -4000.0, 1000.0], f32)
    c["points"][..., 0], c["points"][..., 2] = 0.0, 1000.0
    c["points"][..., 1] = np.linspace(-1000, 1000, 10, dtype=f32).reshape(1, 2, 5)
    c["expect"]["state"] = {(0, 0): DEGENERATE}
    c["expect"]["h22_zero"] = (0, 0)
    return c


def _clamped(kind):
    prm = dict(max_angle=np.deg2rad(0.5)) if kind == "angle" else dict(max_shift=10.0)
    c = scene(2, 3, 5, 8, 31, bumped=((0, 0, 1.5, 30.0),), params=dict(min_obs=60, **prm))
    c["expect"]["state"] = {(0, 0): CLAMPED, (0, 1): OK, (0, 2): OK}
    c["expect"]["clamp"] = kind
    return c


def _lambda():
    return scene(2, 3, 5, 8, 37, params=dict(lam=0.05))


def _pivot_scale():
    """min_pivot between the smallest scaled pivot and the smallest unscaled one of camera (0, 0): the threshold is unit-free
    only when it is applied to the scaled matrix."""
    c = scene(2, 2, 5, 8, 41)
    r = ref_solve(ref_accumulate(c), c["cams"], _prm(c), pivots=True)
    a, b = r["pivots"][0].min(), (r["pivots"][0] * r["D"][0] ** 2).min()
    assert max(a, b) / min(a, b) > 2, (a, b)
    c["params"]["min_pivot"] = float(f32(np.sqrt(a * b)))
    assert min(a, b) < c["params"]["min_pivot"] < max(a, b)
    c["expect"]["state"] = {(0, 0): OK if a > b else DEGENERATE}
    return c


def _independent():
    """Two calls that differ only in the observations of view 2: the other cameras' rows keep their bits (checked in
    check_expectations)."""
    return scene(2, 3, 5, 8, 43, bumped=((0, 0, 1.0, 20.0), (0, 2, 0.7, 15.0)))


def random_scene(V, J, seed, B=3, N=4, nsets=2):
    rng = np.random.default_rng(seed)
    c = scene(B, V, N, J, seed, nsets=nsets, frame_set=rng.integers(-1, nsets + 1, B), noise=0.5,
              bumped=tuple((s, int(rng.integers(V)), 1.0, 20.0) for s in range(nsets)), params=dict(huber_px=2.0, min_obs=12, lam=1e-3))
    c["view_state"][rng.uniform(size=c["view_state"].shape) < 0.2] = -2
    c["obs"][..., 2][rng.uniform(size=c["view_state"].shape) < 0.1] = 0.0
    c["points"][..., 0][rng.uniform(size=c["points"].shape[:3]) < 0.05] = NAN
    return c


BUILDERS = {
    "smallest": _smallest, "full_tree_256": _full_tree, "second_trip_270": _second_trip, "two_sets": _two_sets,
    "eight_views_j5": _eight_views, "rejections": _rejections, "huber_on": lambda: _huber(True), "huber_off": lambda: _huber(False),
    "few_7": lambda: _few(7), "few_8": lambda: _few(8), "coincident": _coincident, "zero_diagonal": _zero_diagonal,
    "clamped_angle": lambda: _clamped("angle"), "clamped_shift": lambda: _clamped("shift"), "lambda": _lambda,
    "pivot_scale": _pivot_scale, "independent": _independent, "random_v3_j5": lambda: random_scene(3, 5, 51),
    "random_v5_j7": lambda: random_scene(5, 7, 52, B=5),
}
TELLS = {"uv_swapped": "second_trip_270", "tau_sign": "second_trip_270", "t_from_r": "second_trip_270",
         "f_scale_missing": "smallest", "decay_after_add": "second_trip_270", "fold_order": "full_tree_256",
         "huber_on_e2": "huber_on", "unscaled_pivot": "pivot_scale", "rodrigues": "second_trip_270"}
CASES = list(BUILDERS)
DECAYS = (1.0, 0.5, 0.0)
_cache = {}


def reference(case, mutant=None):
    """What one round gives from zeroed accumulators, then a second accumulation with ``decay`` 0.5 on top (``acc2``): dict of
    acc, acc2, cams_out, cal_stats, cal_state."""
    acc = ref_accumulate(case, mutant=mutant, decay=1.0)
    res = ref_solve(acc, case["cams"], _prm(case), mutant=mutant)
    res["acc"] = acc
    res["acc2"] = ref_accumulate(case, acc=acc, mutant=mutant, decay=0.5)
    return res


def get(name):
    if name not in _cache:
        case = BUILDERS[name]()
        _cache[name] = (case, reference(case))
    return _cache[name]


KEYS = ("acc", "acc2", "cams_out", "cal_stats", "cal_state")


def differs(a, b, keys=KEYS):
    return any(a.get(k) is not None and b.get(k) is not None and not np.array_equal(bits(a[k]) if a[k].dtype.kind == "f" else a[k],
                                                                                      bits(b[k]) if b[k].dtype.kind == "f" else b[k])
               for k in keys)


def assert_equal(got, want, what, keys=KEYS):
    for k in keys:
        if got.get(k) is None or want.get(k) is None:
            continue
        g, w = got[k], want[k]
        same = np.array_equal(bits(g), bits(w)) if w.dtype.kind == "f" else np.array_equal(g, w)
        if not same:
            bad = np.argwhere((bits(g) != bits(w)) if w.dtype.kind == "f" else (g != w))
            raise AssertionError((what, k, len(bad), bad[:4].tolist(), g[tuple(bad[0])], w[tuple(bad[0])]))


def check_expectations(name):
    """What the scene is named after shows in the yardstick's values."""
    case, want = get(name)
    exp = case["expect"]
    acc = want["acc"]
    for (s, v), n in exp.get("count", {}).items():
        assert acc[s, v, 29] == n, (name, s, v, acc[s, v, 29], n)
    for (s, v), n in exp.get("huber_count", {}).items():
        assert acc[s, v, 30] == n, (name, s, v, acc[s, v, 30])
    for (s, v), n in exp.get("huber_count_min", {}).items():
        assert acc[s, v, 30] >= n and acc[s, v, 30] < acc[s, v, 29], (name, s, v, acc[s, v, 30])
    for (s, v), st in exp.get("state", {}).items():
        assert want["cal_state"][s, v] == st, (name, s, v, want["cal_state"][s, v], st)
    assert (acc[..., 31] == 0).all() and (acc[..., 29] == np.round(acc[..., 29])).all()
    solved = want["cal_state"] >= 1
    assert np.isfinite(want["cams_out"]).all() and np.isfinite(want["cal_stats"]).all()
    # a camera that is not solved is copied, and its stats are zeros except rms_before and count
    assert np.array_equal(bits(want["cams_out"][~solved]), bits(case["cams"][~solved]))
    assert (want["cal_stats"][~solved][:, [0, 1, 3, 5]] == 0).all()
    assert np.array_equal(bits(want["cams_out"][..., 12:]), bits(case["cams"][..., 12:]))
    if "h22_zero" in exp:
        assert acc[exp["h22_zero"]][_ut(2, 2)] == 0.0 and acc[exp["h22_zero"]][29] >= 6
    if exp.get("clamp") == "angle":
        assert abs(want["cal_stats"][0, 0, 0] - f32(_prm(case)["max_angle"])) < 1e-6
    if exp.get("clamp") == "shift":
        assert abs(want["cal_stats"][0, 0, 1] - 10.0) < 1e-4
    if name == "huber_on":
        off = get("huber_off")[1]
        assert want["acc"][0, 0, 27] < off["acc"][0, 0, 27]                       # the outlier weighs less
        err = lambda r: np.abs(r["cams_out"][0, 0, 9:12].astype(f64) - case["true_cams"][0, 0, 9:12]).max()   # noqa: E731
        assert err(want) < err(off)                                               # and pulls the camera less
    if name == "lambda":
        plain = ref_solve(want["acc"], case["cams"], _prm(case, lam=0.0))
        assert differs(plain, want, SOLVE_OUTPUTS) and (want["cal_state"] == OK).all()
        assert want["cal_stats"][0, 0, 5] > plain["cal_stats"][0, 0, 5]           # the damping lifts every pivot
    if name == "independent":
        other = {**case, "obs": case["obs"].copy()}
        other["obs"][:, 2, ..., 0] += 3.0
        w2 = reference(other)
        for k in KEYS:
            assert np.array_equal(bits(w2[k][:, :2]) if w2[k].dtype.kind == "f" else w2[k][:, :2],
                                  bits(want[k][:, :2]) if want[k].dtype.kind == "f" else want[k][:, :2]), k
        assert differs({k: v[:, 2:] for k, v in w2.items()}, {k: v[:, 2:] for k, v in want.items()})
    if name == "two_sets":
        assert (acc[..., 29].sum() == 6 * 3 * 25)                                 # frames 4 and 6 count for no camera


# ======================================================================================================================
# runners
# ======================================================================================================================
GUARD = 512                                                  # guard elements in front of and behind every buffer
INT_FILL = -77
# what a read outside a buffer would bring: values that count (a used state, a valid set, finite points and pixels)
GUARD_VALUE = dict(points=f32(100.0), obs=f32(0.7), view_state=np.int32(USED), cams=f32(1.0), frame_set=np.int32(0),
                   acc=f64(1e30), cams_in=f32(1.0))


def _torch():
    import torch
    return torch


class Buf:
    """An array inside a larger allocation with guard elements on both sides, on ``device``."""

    def __init__(self, a, device, guard):
        self.shape, self.dtype = a.shape, a.dtype
        self.n = a.size
        flat = np.concatenate([np.full(GUARD, guard, a.dtype), np.ascontiguousarray(a).reshape(-1), np.full(GUARD, guard, a.dtype)])
        self.before = flat.copy()
        t = _torch().from_numpy(flat)
        self.t = t if str(device) == "cpu" else t.to(device)

    @property
    def ptr(self):
        return C.c_void_p(self.t.data_ptr() + GUARD * self.dtype.itemsize)

    def host(self):
        return self.t.cpu().numpy()

    def value(self):
        return self.host()[GUARD:GUARD + self.n].reshape(self.shape).copy()

    def guards_intact(self):
        h = self.host()
        return np.array_equal(bits(h[:GUARD]), bits(self.before[:GUARD])) and np.array_equal(bits(h[-GUARD:]), bits(self.before[-GUARD:]))

    def untouched(self):
        return np.array_equal(bits(self.host()), bits(self.before))


def _stream(device):
    torch = _torch()
    return C.c_void_p(torch.cuda.current_stream().cuda_stream) if str(device).startswith("cuda") else None


def _sync(device):
    if str(device).startswith("cuda"):
        _torch().cuda.synchronize()


def call_accumulate(lib, device, case, acc=None, **over):
    """fvp_camera_refit_accumulate; returns (rc, acc after the call, the buffers).  ``over``: arguments that replace the
    case's (B, V, N, J, nsets, iters, huber_px, decay, null=<names passed as NULL>)."""
    B, N, J = case["points"].shape[:3]
    nsets, V = case["cams"].shape[:2]
    prm = _prm(case, **{k: v for k, v in over.items() if k in DEFAULTS})
    acc = np.zeros((nsets, V, ACC)) if acc is None else acc
    arrays = dict(points=case["points"], obs=case["obs"], view_state=case["view_state"], cams=case["cams"],
                  frame_set=case["frame_set"], acc=acc)
    bufs = {k: Buf(a, device, GUARD_VALUE[k]) for k, a in arrays.items()}
    p = {k: (None if k in over.get("null", ()) else b.ptr) for k, b in bufs.items()}
    rc = lib.fvp_camera_refit_accumulate(p["points"], p["obs"], p["view_state"], p["cams"], over.get("nsets", nsets),
                                         p["frame_set"], over.get("B", B), over.get("V", V), over.get("N", N), over.get("J", J),
                                         int(prm["iters"]), float(prm["huber_px"]), float(prm["decay"]), p["acc"], _stream(device))
    _sync(device)
    return rc, bufs["acc"].value(), bufs


def call_solve(lib, device, acc, cams, prm=None, outs=SOLVE_OUTPUTS, **over):
    """fvp_camera_refit_solve; returns (rc, {name: numpy or None}, the buffers).  The outputs start filled with NaN / -77."""
    prm = {**DEFAULTS, **(prm or {}), **{k: v for k, v in over.items() if k in DEFAULTS}}
    nsets, V = cams.shape[:2]
    fills = dict(cams_out=np.full((nsets, V, CAM_FLOATS), NAN, f32), cal_stats=np.full((nsets, V, 6), NAN, f32),
                 cal_state=np.full((nsets, V), INT_FILL, np.int32))
    bufs = dict(acc=Buf(acc, device, GUARD_VALUE["acc"]), cams_in=Buf(cams, device, GUARD_VALUE["cams_in"]))
    for k in SOLVE_OUTPUTS:
        if k in outs:
            bufs[k] = Buf(fills[k], device, fills[k].reshape(-1)[0])
    p = {k: (None if k in over.get("null", ()) else b.ptr) for k, b in bufs.items()}
    if over.get("alias"):
        p["cams_out"] = p["cams_in"]
    rc = lib.fvp_camera_refit_solve(p["acc"], p["cams_in"], over.get("nsets", nsets), over.get("V", V), int(prm["min_obs"]),
                                    float(prm["lam"]), float(prm["min_pivot"]), float(prm["max_angle"]), float(prm["max_shift"]),
                                    p.get("cams_out"), p.get("cal_stats"), p.get("cal_state"), _stream(device))
    _sync(device)
    return rc, {k: (bufs[k].value() if k in bufs else None) for k in SOLVE_OUTPUTS}, bufs


def run(lib, device, case):
    """One round from zeroed accumulators, the solve, and a second accumulation with decay 0.5 on top; every guard checked."""
    rc, acc, b1 = call_accumulate(lib, device, case, decay=1.0)
    assert rc == 0, rc
    rc, got, b2 = call_solve(lib, device, acc, case["cams"], _prm(case))
    assert rc == 0, rc
    rc, acc2, b3 = call_accumulate(lib, device, case, acc=acc, decay=0.5)
    assert rc == 0, rc
    for bufs in (b1, b2, b3):
        for k, b in bufs.items():
            assert b.guards_intact(), k
    for bufs in (b1, b3):
        for k in ("points", "obs", "view_state", "cams", "frame_set"):
            assert bufs[k].untouched(), k
    assert b2["acc"].untouched() and b2["cams_in"].untouched()
    return dict(got, acc=acc, acc2=acc2)


def check(lib, device, name):
    case, want = get(name)
    assert_equal(run(lib, device, case), want, name)


def check_decay(lib, device):
    """decay across two calls: 1 accumulates, 0.5 forgets half, 0 replaces."""
    case, want = get("second_trip_270")
    other = scene(2, 3, 5, 9, 8, bumped=((0, 0, 1.5, 30.0),))
    other["cams"] = case["cams"]
    for decay in DECAYS:
        rc, acc, _ = call_accumulate(lib, device, other, acc=want["acc"], decay=decay)
        assert rc == 0
        exp = ref_accumulate(other, acc=want["acc"], decay=decay)
        assert_equal(dict(acc=acc), dict(acc=exp), ("decay", decay))
        if decay == 0.0:
            assert_equal(dict(acc=acc), dict(acc=ref_accumulate(other)), "decay 0 replaces")
        if decay == 1.0:
            assert acc[0, 0, 29] == want["acc"][0, 0, 29] + 90


def check_fence(lib, device):
    """Guard elements that would count sit around every input (a used state, set 0, finite points and pixels, peak 0.7): one
    entry read outside a buffer would change the sums.  The accumulators' and outputs' guards must keep their bits."""
    for name in ("smallest", "second_trip_270", "two_sets"):
        check(lib, device, name)


def check_null_outputs(lib, device):
    case, want = get("random_v3_j5")
    for outs in (("cams_out",), ("cams_out", "cal_stats"), ("cams_out", "cal_state")):
        rc, got, _ = call_solve(lib, device, want["acc"], case["cams"], _prm(case), outs=outs)
        assert rc == 0, outs
        assert_equal(got, want, outs)
        assert [k for k in SOLVE_OUTPUTS if got[k] is not None] == list(outs)


def argument_errors(lib, device):
    """Every FVP_EINVAL / FVP_ELIMIT condition of the header returns its code and leaves every buffer as it was."""
    case, want = get("second_trip_270")
    acc0 = want["acc"]
    bad = [dict(null=(k,)) for k in ("points", "obs", "view_state", "cams", "frame_set", "acc")]
    bad += [dict(B=-1), dict(V=0), dict(N=0), dict(J=0), dict(nsets=0), dict(iters=-1), dict(huber_px=NAN), dict(huber_px=INF),
            dict(decay=-0.1), dict(decay=1.5), dict(decay=NAN)]
    for over in bad:
        rc, acc, bufs = call_accumulate(lib, device, case, acc=acc0, **over)
        assert rc == EINVAL, (over, rc)
        assert all(b.untouched() for b in bufs.values()), over
    for over in (dict(V=MAX_VIEWS + 1), dict(J=MAX_JOINTS + 1), dict(iters=MAX_ITERS + 1), dict(B=1 << 20, N=1 << 10, J=32)):
        rc, acc, bufs = call_accumulate(lib, device, case, acc=acc0, **over)
        assert rc == ELIMIT, (over, rc)
        assert all(b.untouched() for b in bufs.values()), over
    rc, acc, bufs = call_accumulate(lib, device, case, acc=acc0, B=0, decay=0.5)          # no launch: nothing written
    assert rc == 0 and all(b.untouched() for b in bufs.values())
    for over in (dict(iters=MAX_ITERS), dict(iters=0), dict(huber_px=-1.0), dict(decay=0.0)):   # the limits themselves are fine
        rc, acc, _ = call_accumulate(lib, device, case, acc=acc0, **over)
        assert rc == 0, over
        assert_equal(dict(acc=acc), dict(acc=ref_accumulate(dict(case, params={**case["params"], **over}), acc=acc0)), over)
    bad = [dict(null=("acc",)), dict(null=("cams_in",)), dict(null=("cams_out",)), dict(alias=True), dict(nsets=0), dict(V=0),
           dict(min_obs=5), dict(lam=-1e-3), dict(lam=NAN), dict(lam=INF), dict(min_pivot=0.0), dict(min_pivot=-1.0),
           dict(min_pivot=NAN), dict(min_pivot=INF), dict(max_angle=0.0), dict(max_angle=NAN), dict(max_angle=INF),
           dict(max_shift=0.0), dict(max_shift=-5.0), dict(max_shift=NAN), dict(max_shift=INF)]
    for over in bad:
        rc, got, bufs = call_solve(lib, device, acc0, case["cams"], _prm(case), **over)
        assert rc == EINVAL, (over, rc)
        assert all(b.untouched() for b in bufs.values()), over
    rc, got, bufs = call_solve(lib, device, acc0, case["cams"], _prm(case), V=MAX_VIEWS + 1)
    assert rc == ELIMIT and all(b.untouched() for b in bufs.values())
    rc, got, _ = call_solve(lib, device, acc0, case["cams"], _prm(case), min_obs=6)
    assert rc == 0
    assert_equal(got, ref_solve(acc0, case["cams"], _prm(case, min_obs=6)), "min_obs 6")


# ======================================================================================================================
# host side
# ======================================================================================================================
class Cfg:
    """The field CameraRefiner reads."""

    def __init__(self, J):
        from types import SimpleNamespace as NS
        self.DATASET = NS(NUM_JOINTS=J)


def refiner_for(case, lib=None, **kw):
    from faster_voxelpose_amd.utils.recalibrate import CameraRefiner
    prm = _prm(case)
    args = dict(undistort_iters=prm["iters"], huber_px=prm["huber_px"], decay=prm["decay"], min_obs=prm["min_obs"], lam=prm["lam"],
                min_pivot=prm["min_pivot"], max_angle_deg=float(np.rad2deg(prm["max_angle"])), max_shift_mm=prm["max_shift"])
    args.update(kw)
    return CameraRefiner(Cfg(case["points"].shape[2]), **args, **({} if lib is None else dict(_lib=lib)))


TENSORS = ("points", "obs", "view_state", "cams", "frame_set")


def tensors(case, device):
    torch = _torch()
    out = {}
    for k in TENSORS:
        t = torch.from_numpy(np.ascontiguousarray(case[k]).copy())
        out[k] = t if str(device) == "cpu" else t.to(device)
    return out


def as_dict(out):
    return {k: v.cpu().numpy() for k, v in zip(SOLVE_OUTPUTS, out)}


def camera_records(cameras, names):
    """The cameras dict of the forward -> [nsets,V,24] records, the way the engine's table builder packs them."""
    from faster_voxelpose_amd.engine import HotPath
    return np.stack([np.stack([HotPath._cam_row(c) for c in cameras[n]]) for n in names])


# ======================================================================================================================
# against the truth (tests/golden/make_refit_floor.py writes tests/golden/refit_floor.json)
# ======================================================================================================================
FLOOR_JSON = os.path.join(HERE, "golden", "refit_floor.json")
FLOOR_ROUNDS = 3


def floor_scene(seed):
    """A rig of 4 cameras with lens terms, 150 seeded points per camera, camera 0 bumped by 1.5 degrees and 30 mm.  The
    TRUE cameras are float64 records no float32 table represents (orthonormal rotations, centres off the float32 grid); the
    observations are their exact projections rounded to float32; the table handed in is the truth rounded to float32, with
    camera 0 bumped."""
    c = scene(3, 4, 5, 10, seed, bumped=(), params=dict(min_obs=60))
    true = c["true_cams"].astype(f64)
    for v in range(4):
        true[0, v] = bump(true[0, v], 0.01, 0.37, seed * 7 + v)
        U, _, Vt = np.linalg.svd(true[0, v, :9].reshape(3, 3))
        true[0, v, :9] = (U @ Vt).reshape(9)
    c["true_cams"] = true
    c["cams"] = true.astype(f32)
    c["cams"][0, 0] = bump(true[0, 0], 1.5, 30.0, seed * 31).astype(f32)
    c["obs"] = observe(true, c["frame_set"], c["points"], rng=np.random.default_rng(seed + 1))
    return c


def floor_figures(case, res):
    """Centre error (mm) and angle error (degrees) of the bumped camera against the truth, the rms residual (pixels) the last
    round started from, the largest distance of an untouched camera from the truth (mm, degrees)."""
    out, true = res["cams_out"].astype(f64), case["true_cams"].astype(f64)

    def angle(a, b):
        Rd = a[:9].reshape(3, 3) @ b[:9].reshape(3, 3).T
        sk = 0.5 * np.asarray([Rd[2, 1] - Rd[1, 2], Rd[0, 2] - Rd[2, 0], Rd[1, 0] - Rd[0, 1]])
        return float(np.rad2deg(np.arcsin(min(1.0, np.linalg.norm(sk)))))                     # exact for small angles

    others = [(0, v) for v in range(1, out.shape[1])]
    return dict(centre_mm=float(np.linalg.norm(out[0, 0, 9:12] - true[0, 0, 9:12])), angle_deg=angle(out[0, 0], true[0, 0]),
                rms_px=float(res["cal_stats"][0, 0, 2]),
                others_mm=max(float(np.linalg.norm(out[i][9:12] - true[i][9:12])) for i in others),
                others_deg=max(angle(out[i], true[i]) for i in others))


def floor():
    with open(FLOOR_JSON) as f:
        return json.load(f)


def refine_calls(lib, device, case, rounds=FLOOR_ROUNDS):
    cams, got = case["cams"], None
    for _ in range(rounds):
        rc, acc, _ = call_accumulate(lib, device, dict(case, cams=cams), decay=1.0)
        assert rc == 0
        rc, got, _ = call_solve(lib, device, acc, cams, _prm(case))
        assert rc == 0
        got["acc"] = acc
        cams = got["cams_out"]
    return got


def check_floor(lib, device):
    """Three rounds on another seed than the recorded one: the bumped camera lands within 2 x the recorded centre, angle and
    rms figures (the margin covers the seed), reports OK, and the untouched cameras move less than 2 x what they moved in
    the recording.  Every camera has at least min_obs counting observations and none is DEGENERATE."""
    fl = floor()
    case = floor_scene(fl["test_seed"])
    got = refine_calls(lib, device, case)
    assert_equal(got, ref_refine(case, FLOOR_ROUNDS), "three rounds", keys=SOLVE_OUTPUTS)
    fig = floor_figures(case, got)
    print(f"kernel: {fig}; recorded: {fl['figures']}")
    assert (got["acc"][..., 29] >= _prm(case)["min_obs"]).all() and (got["cal_state"] != DEGENERATE).all()
    assert got["cal_state"][0, 0] == OK
    for k in ("centre_mm", "angle_deg", "rms_px", "others_mm", "others_deg"):
        assert fig[k] <= 2.0 * fl["figures"][k], (k, fig, fl["figures"])
