"""Cases and the yardstick of fvp_joint_visibility (include/fvp.h, ABI 17), shared by tests/test_visibility_emu.py (CPU
emulator) and tests/test_visibility_gpu.py (the shipped library on the card): an independent numpy restatement of the
definition - vectorised over (view, person, joint), every operation on float32 arrays, which round every result to float32;
the same code in float64 is the second judge - the constructed scenes with the entries each of them is about, the wrong
readings of the definition (mutants) the scenes must tell apart, seeded random scenes, and a runner that calls the entry
point on torch memory (CPU for the emulator, the card otherwise).  Outputs are compared bit for bit: no tolerance anywhere."""
import ctypes as C

import numpy as np
import torch

f32, f64 = np.float32, np.float64
NAN, INF = float("nan"), float("inf")
EINVAL, ELIMIT = 10001, 10002
MAX_JOINTS, MAX_VIEWS, MAX_PEOPLE, MAX_PRIMS, CAM_FLOATS = 32, 8, 32, 64, 24
FLT_MAX = float(np.finfo(f32).max)
MUTANTS = ("infinite_ray", "no_guard", "no_exclusion", "exclude_self", "skip_spheres", "no_t_clamp", "parallel_skipped",
           "lowest_slot_wins", "last_wins", "ignore_ids", "ignore_valid", "nan_evaluated", "guard_inclusive",
           "edge_exclusive", "depth_ge", "mean_over_all_views", "frame_set_ignored")


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _dev(a, device):
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a).copy())
    return t if str(device) == "cpu" else t.to(device)


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream(device):
    return C.c_void_p(torch.cuda.current_stream().cuda_stream) if str(device).startswith("cuda") else None


def _sync(device):
    if str(device).startswith("cuda"):
        torch.cuda.synchronize()


# ======================================================================================================================
# the definition
# ======================================================================================================================
def _dot(p, q):
    return (p[..., 0] * q[..., 0] + p[..., 1] * q[..., 1]) + p[..., 2] * q[..., 2]


def _clamp(x, lo, hi):
    return np.fmin(np.fmax(x, lo), hi)


def reference(case, dt=f32, mutant=None, detail=False):
    """(occluder [B,V,N,J] i32, vis_conf [B,N,J] f32 or None, vis_count [B,N,J] i32 or None) by the definition in
    include/fvp.h, in ``dt``.  ``detail``: also (margin [B,V,N,J] = min over the candidates of |dist - r|, hit_s [B,V,N,J,N] =
    the smallest s of each person's hits, inf without one)."""
    poses, cams, fset, ids, views = case["poses"], case["cams"], case["frame_set"], case.get("ids"), case.get("views")
    prims, radius, guard = case["prims"], case["radius"], dt(f32(case["guard"]))
    B, N, J = poses.shape[:3]
    V = cams.shape[1]
    occ = np.full((B, V, N, J), -2, np.int32)
    margin = np.full((B, V, N, J), np.inf, f64)
    hit_s = np.full((B, V, N, J, N), np.inf, f64)
    nn, jj = np.arange(N)[None, :, None], np.arange(J)[None, None, :]
    zero, one = dt(0), dt(1)
    with np.errstate(all="ignore"):
        for b in range(B):
            cset = 0 if mutant == "frame_set_ignored" else fset[b]
            Cc = cams[cset, :, 9:12].astype(dt)[:, None, None, :]                          # [V,1,1,3]
            X = poses[b, :, :, :3].astype(dt)                                              # [N,J,3]
            present = poses[b, :, 0, 3] >= 0 if mutant != "ignore_valid" else np.ones(N, bool)
            if ids is not None and mutant != "ignore_ids":
                present = present & (ids[b] >= 0)
            finite = (np.abs(X) <= dt(FLT_MAX)).all(-1)                                    # [N,J]; a NaN fails
            d1 = X[None] - Cc                                                              # [V,N,J,3]
            a = _dot(d1, d1)
            ln = np.sqrt(a)
            ev = present[None, :, None] & (ln >= guard if mutant == "guard_inclusive" else ln > guard)
            if mutant != "nan_evaluated":
                ev = ev & finite[None]
            smax = one - guard / ln
            if mutant == "no_guard":
                smax = np.ones_like(smax)
            if mutant == "infinite_ray":
                smax = np.full_like(smax, 4)
            S = np.full((V, N, J, N), np.inf, dt)                                          # per person: smallest s of a hit
            for m in range(N):
                if not present[m]:
                    continue
                for (i, k), r in zip(prims, radius):
                    if not (finite[m, i] and finite[m, k]) or (mutant == "skip_spheres" and i == k):
                        continue
                    own = (nn == m) & ((jj == i) | (jj == k))                               # the limbs that end in the joint
                    if mutant == "no_exclusion":
                        own = np.zeros_like(own)
                    if mutant == "exclude_self":
                        own = nn == m
                    A, Bq = X[m, i], X[m, k]
                    d2 = Bq - A
                    r0 = Cc - A                                                            # [V,1,1,3]
                    e, f = _dot(d2, d2), _dot(d2, r0)
                    c = _dot(d1, r0)
                    s_end = _clamp(-c / a, zero, smax)
                    if e == 0:
                        s, t = s_end, np.zeros_like(a)
                    else:
                        bb = _dot(d1, d2)
                        den = a * e - bb * bb
                        s = np.where(den > 0, _clamp((bb * f - c * e) / den, zero, smax), zero)
                        t = (bb * s + f) / e
                        if mutant != "no_t_clamp":
                            lo, hi = t < 0, t > 1
                            s = np.where(lo, s_end, np.where(hi, _clamp((bb - c) / a, zero, smax), s))
                            t = np.where(lo, zero, np.where(hi, one, t))
                        s, t = s.astype(dt), t.astype(dt)
                    w = (Cc + d1 * s[..., None]) - (A + d2 * t[..., None])
                    dist2 = _dot(w, w)
                    rr = dt(f32(r)) * dt(f32(r))
                    hit = (dist2 <= rr) & ~own & ev
                    if mutant == "parallel_skipped" and e != 0:
                        hit = hit & (den > 0)
                    S[..., m] = np.where(hit & (s < S[..., m]), s, S[..., m])
                    if detail:
                        cand = ev & ~own
                        margin[b] = np.where(cand, np.minimum(margin[b], np.abs(np.sqrt(dist2.astype(f64)) - f64(r))), margin[b])
            any_hit = np.isfinite(S).any(-1)
            first = np.argmin(S, axis=-1)                                                  # the lowest slot among equal s
            if mutant == "lowest_slot_wins":
                first = np.argmax(np.isfinite(S), axis=-1)
            if mutant == "last_wins":
                first = N - 1 - np.argmin(S[..., ::-1], axis=-1)
            occ[b] = np.where(ev, np.where(any_hit, first, -1), -2)
            hit_s[b] = S
    conf = count = None
    if views is not None:
        px, py, depth, sv = (views[..., q] for q in range(4))                              # [B,V,N,J] float32
        xmax, ymax = f32(case["Ws"] - 1), f32(case["Hs"] - 1)
        with np.errstate(all="ignore"):
            if mutant == "edge_exclusive":
                inside = (px > 0) & (px < xmax) & (py > 0) & (py < ymax)
            else:
                inside = (px >= 0) & (px <= xmax) & (py >= 0) & (py <= ymax)
            sees = (occ == -1) & (depth >= 0 if mutant == "depth_ge" else depth > 0) & inside
            total = np.zeros((B, N, J), f32)
            count = np.zeros((B, N, J), np.int32)
            for v in range(V):
                total = np.where(sees[:, v], total + sv[:, v], total).astype(f32)
                count = count + sees[:, v]
            div = f32(V) if mutant == "mean_over_all_views" else count.astype(f32)
            conf = np.where(count > 0, _clamp(total / div, f32(0), f32(1)), f32(0)).astype(f32)
        count = count.astype(np.int32)
    if detail:
        return occ, conf, count, margin, hit_s
    return occ, conf, count


# ======================================================================================================================
# constructed scenes: every named entry is what the scene is about; the rest of the scene is judged by the yardstick
# ======================================================================================================================
def camera_table(centres):
    """[nsets][V] camera centres -> [nsets,V,24] records; only T (floats 9..11) is read by the call."""
    c = np.asarray(centres, f32)
    cams = np.zeros(c.shape[:2] + (CAM_FLOATS,), f32)
    cams[..., 0] = cams[..., 4] = cams[..., 8] = 1.0
    cams[..., 9:12] = c
    cams[..., 12:14] = 1000.0
    return cams


def blank(B, N, J):
    """Valid persons whose joints are parked behind the cameras of the scenes, far from every ray that matters."""
    poses = np.zeros((B, N, J, 5), f32)
    for n in range(N):
        for j in range(J):
            poses[:, n, j, :3] = (-3000.0 - 500.0 * n, 3000.0 + 500.0 * j, 2000.0)
    poses[..., 3] = 0.5
    poses[..., 4] = 0.25
    return poses


def _case(poses, centres=(((0, 0, 0),),), prims=((0, 1), (1, 3), (2, 2)), radius=(50.0, 50.0, 100.0), guard=60.0, frame_set=None,
          ids=None, views=None, Hs=1, Ws=1, expect=None):
    B = poses.shape[0]
    return dict(poses=poses, cams=camera_table(centres), frame_set=np.zeros(B, np.int32) if frame_set is None
                else np.asarray(frame_set, np.int32), ids=None if ids is None else np.asarray(ids, np.int32), views=views,
                prims=[tuple(p) for p in prims], radius=[float(r) for r in radius], guard=float(guard), Hs=Hs, Ws=Ws,
                expect=expect or {})


def _between_and_behind():
    p = blank(1, 3, 4)
    p[0, 0, 0, :3] = (4000, 0, 0)                                   # the target, along +x
    p[0, 1, 0, :3], p[0, 1, 1, :3] = (2000, 0, -300), (2000, 0, 300)   # a limb exactly between camera and target
    p[0, 2, 0, :3], p[0, 2, 1, :3] = (6000, 0, -300), (6000, 0, 300)   # one behind it
    p[0, 0, 2, :3] = (0, 4000, 0)                                   # a second target along +y with a sphere behind it ...
    p[0, 2, 2, :3] = (0, 5000, 0)                                   # ... which is itself behind the first one's sphere
    return _case(p, expect={(0, 0, 0, 0): 1, (0, 0, 0, 2): -1, (0, 0, 2, 2): 0, (0, 0, 1, 0): -1})


def _guard_zone():
    p = blank(1, 2, 4)
    p[0, 0, 0, :3] = (4000, 0, 0)
    p[0, 1, 2, :3] = (3970, 0, 0)                                   # a 15 mm sphere 30 mm before the joint: inside the guard
    p[0, 0, 1, :3] = (0, 4000, 0)
    p[0, 1, 3, :3] = (0, 3900, 0)                                   # the same sphere 100 mm before a joint: outside
    return _case(p, prims=((2, 2), (3, 3)), radius=(15.0, 15.0), expect={(0, 0, 0, 0): -1, (0, 0, 0, 1): 1})


def _own_limbs():
    p = blank(1, 2, 4)
    p[0, 0, 2, :3], p[0, 0, 3, :3] = (1000, 0, 400), (2400, 0, 0)   # a forearm pointing at the camera: 16 degrees off the ray
    p[0, 1, 0, :3], p[0, 1, 1, :3] = (0, 2000, -300), (0, 2000, 300)   # a torso across the +y ray ...
    p[0, 1, 2, :3], p[0, 1, 3, :3] = (400, 2400, 300), (0, 2400, 0)    # ... and the same person's wrist behind it
    return _case(p, prims=((0, 1), (1, 2), (2, 3)), radius=(120.0, 40.0, 40.0),
                 expect={(0, 0, 0, 3): -1, (0, 0, 0, 2): -1, (0, 0, 1, 3): 1})


def _limb_ends():
    p = blank(1, 5, 4)
    p[0, 0, :, :3] = ((4000, 0, 0), (0, 4000, 0), (-4000, 0, 0), (0, -4000, 0))
    p[0, 1, 0, :3], p[0, 1, 1, :3] = (2000, 0, 80), (2000, 0, 500)       # t < 0, 80 mm off: misses (the line would hit)
    p[0, 2, 0, :3], p[0, 2, 1, :3] = (0, 2000, -500), (0, 2000, -80)     # t > 1, 80 mm off: misses
    p[0, 3, 0, :3], p[0, 3, 1, :3] = (-2000, 0, 40), (-2000, 0, 500)     # t < 0, 40 mm off: hits
    p[0, 4, 0, :3], p[0, 4, 1, :3] = (0, -2000, -500), (0, -2000, -40)   # t > 1, 40 mm off: hits
    return _case(p, prims=((0, 1),), radius=(50.0,),
                 expect={(0, 0, 0, 0): -1, (0, 0, 0, 1): -1, (0, 0, 0, 2): 3, (0, 0, 0, 3): 4})


def _parallel():
    p = blank(1, 2, 4)
    p[0, 0, 0, :3] = (4000, 0, 0)
    p[0, 1, 0, :3], p[0, 1, 1, :3] = (1000, 0, 30), (3000, 0, 30)   # parallel to the ray, 30 mm beside it: den == 0
    return _case(p, prims=((0, 1),), radius=(50.0,), expect={(0, 0, 0, 0): 1})


def _two_occluders():
    p = blank(1, 3, 4)
    p[0, 0, 0, :3] = (4000, 0, 0)
    p[0, 1, 0, :3], p[0, 1, 1, :3] = (2000, 0, -300), (2000, 0, 300)
    p[0, 2, 0, :3], p[0, 2, 1, :3] = (1000, 0, -300), (1000, 0, 300)   # the higher slot is nearer the camera: it wins
    p[0, 0, 1, :3] = (0, 4000, 0)
    p[0, 1, 2, :3] = p[0, 2, 2, :3] = (0, 2000, 0)                  # two spheres in the same place: an exact tie in s
    return _case(p, expect={(0, 0, 0, 0): 2, (0, 0, 0, 1): 1})


def _absent_people():
    p = blank(1, 3, 4)
    p[0, 0, 0, :3] = (4000, 0, 0)
    p[0, 1, 0, :3], p[0, 1, 1, :3] = (2000, 0, -300), (2000, 0, 300)   # ids < 0
    p[0, 2, 0, :3], p[0, 2, 1, :3] = (1000, 0, -300), (1000, 0, 300)   # an invalid slot
    p[0, 2, 0, 3] = -1.0
    exp = {(0, 0, 0, 0): -1}
    exp.update({(0, 0, n, j): -2 for n in (1, 2) for j in range(4)})
    return _case(p, ids=[[7, -1, 3]], expect=exp)


def _nan_joint():
    p = blank(1, 4, 4)
    p[0, 0, 0, :3] = (4000, 0, 0)
    p[0, 1, 0, :3], p[0, 1, 1, :3] = (2000, 0, -300), (2000, NAN, 300)   # a limb with a NaN end: no primitive
    p[0, 2, 0, :3], p[0, 2, 1, :3] = (1000, 0, -300), (INF, 0, 300)      # and one with an Inf end
    p[0, 0, 1, :3] = (0, 4000, NAN)                                 # a NaN target
    p[0, 0, 2, :3] = (0, -INF, 0)
    p[0, 3, 0, :3], p[0, 3, 1, :3] = (0, 2000, -300), (0, 2000, 300)
    return _case(p, expect={(0, 0, 0, 0): -1, (0, 0, 0, 1): -2, (0, 0, 0, 2): -2, (0, 0, 1, 1): -2, (0, 0, 1, 0): -1})


def _camera_close():
    p = blank(1, 2, 4)
    p[0, 0, 0, :3] = (4000, 0, 0)
    p[0, 1, 0, :3], p[0, 1, 1, :3] = (2000, 0, -300), (2000, 0, 300)
    centres = (((0, 0, 0), (3950, 0, 0), (3940, 0, 0), (3939, 0, 0)),)     # 4000, 50, 60 (== guard) and 61 mm away
    return _case(p, centres=centres, expect={(0, 0, 0, 0): 1, (0, 1, 0, 0): -2, (0, 2, 0, 0): -2, (0, 3, 0, 0): -1})


def _two_camera_sets():
    p = blank(2, 2, 4)
    p[:, 0, 0, :3] = (4000, 0, 0)
    p[:, 1, 0, :3], p[:, 1, 1, :3] = (2000, 0, -300), (2000, 0, 300)
    centres = (((0, 0, 0),), ((0, 3000, 0),))                      # set 1 looks past the limb
    return _case(p, centres=centres, frame_set=[1, 0], expect={(0, 0, 0, 0): -1, (1, 0, 0, 0): 1})


HS, WS = 48, 64


def _seeing_views():
    """No body at all (L = 0): what a view sees is decided by depth and the frame.  Joint 0: all three views; 1: one view
    (the others at depth 0 and behind the camera); 2: none (just past each edge); 3: on the edges; person 1: a NaN pixel, a
    NaN sample, a sum beyond 1 and one below 0."""
    p = blank(1, 2, 4)
    v = np.zeros((1, 3, 2, 4, 4), f32)
    v[..., 0], v[..., 1], v[..., 2] = 10.0, 10.0, 2000.0
    v[0, :, 0, 0, 3] = (0.3, 0.5, 0.9)
    v[0, :, 0, 1, 3] = (0.3, 0.5, 0.9)
    v[0, 0, 0, 1, 2], v[0, 2, 0, 1, 2] = 0.0, -1.0
    v[0, :, 0, 2, 3] = (0.3, 0.5, 0.9)
    v[0, 0, 0, 2, 0] = np.nextafter(f32(0), f32(-1))
    v[0, 1, 0, 2, 0] = np.nextafter(f32(WS - 1), f32(1e9))
    v[0, 2, 0, 2, 1] = np.nextafter(f32(HS - 1), f32(1e9))
    v[0, :, 0, 3, 3] = (0.125, 0.25, 0.75)
    v[0, 0, 0, 3, :2], v[0, 1, 0, 3, :2], v[0, 2, 0, 3, :2] = (0, 0), (WS - 1, 0), (0, HS - 1)
    v[0, :, 1, 0, 3] = (0.3, 0.5, 0.9)
    v[0, 1, 1, 0, 0] = NAN
    v[0, :, 1, 1, 3] = (0.3, NAN, 0.9)
    v[0, :, 1, 2, 3] = (1.5, 2.5, 0.9)
    v[0, :, 1, 3, 3] = (-1.5, 0.25, 0.5)
    centres = (((-9000, 0, 0), (0, -9000, 0), (0, 0, 9000)),)
    c = _case(p, centres=centres, prims=(), radius=(), views=v, Hs=HS, Ws=WS)
    return _with_counts(c, {(0, 0, 0): 3, (0, 0, 1): 1, (0, 0, 2): 0, (0, 0, 3): 3, (0, 1, 0): 2, (0, 1, 1): 3, (0, 1, 2): 3,
                            (0, 1, 3): 3})


def _with_counts(case, counts):
    case["expect_count"] = counts
    return case


def _hidden_views():
    """Occlusion and the frame together: the limb hides the joint in view 0 only; view 1 sees it, view 2 has it out of frame."""
    p = blank(1, 2, 4)
    p[0, 0, 0, :3] = (4000, 0, 0)
    p[0, 1, 0, :3], p[0, 1, 1, :3] = (2000, 0, -300), (2000, 0, 300)
    v = np.zeros((1, 3, 2, 4, 4), f32)
    v[..., 0], v[..., 1], v[..., 2], v[..., 3] = 10.0, 10.0, 2000.0, 0.5
    v[0, :, 0, 0, 3] = (0.9, 0.4, 0.8)
    v[0, 2, 0, 0, 0] = float(WS)
    centres = (((0, 0, 0), (0, 3000, 0), (0, -3000, 0)),)
    c = _case(p, centres=centres, views=v, Hs=HS, Ws=WS, expect={(0, 0, 0, 0): 1, (0, 1, 0, 0): -1, (0, 2, 0, 0): -1})
    return _with_counts(c, {(0, 0, 0): 1})


BUILDERS = {
    "between_and_behind": _between_and_behind, "guard_zone": _guard_zone, "own_limbs": _own_limbs, "limb_ends": _limb_ends,
    "parallel": _parallel, "two_occluders": _two_occluders, "absent_people": _absent_people, "nan_joint": _nan_joint,
    "camera_close": _camera_close, "two_camera_sets": _two_camera_sets, "seeing_views": _seeing_views,
    "hidden_views": _hidden_views,
}
# the first scene that tells each wrong reading of the definition from the definition
TELLS = {"infinite_ray": "between_and_behind", "skip_spheres": "between_and_behind", "no_guard": "guard_zone",
         "no_exclusion": "own_limbs", "exclude_self": "own_limbs", "no_t_clamp": "limb_ends", "parallel_skipped": "parallel",
         "lowest_slot_wins": "two_occluders", "last_wins": "two_occluders", "ignore_ids": "absent_people",
         "ignore_valid": "absent_people", "nan_evaluated": "nan_joint", "guard_inclusive": "camera_close",
         "frame_set_ignored": "two_camera_sets", "edge_exclusive": "seeing_views", "depth_ge": "seeing_views",
         "mean_over_all_views": "seeing_views"}


# ======================================================================================================================
# seeded random scenes
# ======================================================================================================================
LIMBS15 = [(0, 1), (0, 2), (0, 3), (3, 4), (4, 5), (0, 9), (9, 10), (10, 11), (2, 6), (2, 12), (6, 7), (7, 8), (12, 13), (13, 14)]


def body15():
    """14 limbs of 60 mm, a 110 mm head sphere and a 140 mm torso capsule."""
    return LIMBS15 + [(1, 1), (0, 2)], [60.0] * 14 + [110.0, 140.0]


def ring_cameras(V, nsets=1, radius=5000.0, height=2500.0):
    ang = 2 * np.pi * (np.arange(V)[None, :] + 0.37 * np.arange(nsets)[:, None]) / V
    return np.stack([radius * np.cos(ang), radius * np.sin(ang), np.full_like(ang, height)], axis=-1)


def random_scene(B, V, N, J, prims, radius, seed, guard=50.0, nsets=1, spoil=True, with_views=True):
    """People with roots uniform in +-1500 mm at z = 900 and joints root + clip(N(0,1), +-2) * (150, 150, 250); cameras on a
    5 m ring at 2.5 m.  ``spoil``: some invalid slots, negative ids, NaN / Inf joints and a camera on top of a joint."""
    rng = np.random.default_rng(seed)
    poses = np.zeros((B, N, J, 5), f32)
    root = np.concatenate([rng.uniform(-1500, 1500, (B, N, 1, 2)), np.full((B, N, 1, 1), 900.0)], axis=-1)
    poses[..., :3] = root + np.clip(rng.standard_normal((B, N, J, 3)), -2, 2) * (150.0, 150.0, 250.0)
    poses[..., 3] = rng.uniform(0, 1, (B, N, 1))
    poses[..., 4] = rng.uniform(0, 1, (B, N, J))
    centres = ring_cameras(V, nsets)
    ids = None
    if spoil:
        poses[..., 3] = np.where(rng.uniform(size=(B, N, 1)) < 0.15, -1.0, poses[..., 3])
        ids = np.where(rng.uniform(size=(B, N)) < 0.15, -1, rng.integers(0, 100, (B, N))).astype(np.int32)
        bad = rng.uniform(size=(B, N, J)) < 0.02
        poses[..., 0] = np.where(bad, rng.choice([NAN, INF, -INF], (B, N, J)), poses[..., 0])
        centres[-1, -1] = poses[B - 1, N - 1, J - 1, :3].astype(f64) + (20.0, 0.0, 0.0)     # closer than the guard
    views = None
    if with_views:
        views = np.zeros((B, V, N, J, 4), f32)
        views[..., 0] = rng.uniform(-40, WS + 40, (B, V, N, J))
        views[..., 1] = rng.uniform(-30, HS + 30, (B, V, N, J))
        views[..., 2] = rng.uniform(-500, 6000, (B, V, N, J))
        views[..., 3] = rng.uniform(-0.2, 1.2, (B, V, N, J))
    c = _case(poses, centres=centres, prims=prims, radius=radius, guard=guard, frame_set=rng.integers(0, nsets, B), ids=ids,
              views=views, Hs=HS, Ws=WS)
    return c


def _random_small():
    prims, radius = body15()
    return random_scene(2, 3, 4, 15, prims, radius, seed=11, nsets=2)


def _random_full():
    rng = np.random.default_rng(5)
    prims = [tuple(int(x) for x in rng.integers(0, 32, 2)) for _ in range(60)] + [(j, j) for j in (0, 7, 19, 31)]
    radius = [float(r) for r in rng.uniform(30, 120, 64)]
    return random_scene(1, 8, 32, 32, prims, radius, seed=12)


BUILDERS.update({"random_b2_v3_n4_j15": _random_small, "random_b1_v8_n32_j32_l64": _random_full})
CASES = list(BUILDERS)
_cache = {}


def get(name):
    """(case, (occluder, vis_conf, vis_count)) - computed once, shared, never modified."""
    if name not in _cache:
        case = BUILDERS[name]()
        _cache[name] = (case, reference(case))
    return _cache[name]


# ======================================================================================================================
# runners
# ======================================================================================================================
OCC_FILL, COUNT_FILL = -77, -78


def call(lib, device, case, outs=(True, True, True), **over):
    """fvp_joint_visibility on ``device``; returns (rc, [occluder, vis_conf, vis_count] as numpy or None).  The outputs start
    filled with sentinels.  ``over``: arguments that replace the case's (B, V, N, J, L, guard, Hs, Ws, prims, radius,
    null=<names of pointers passed as NULL>)."""
    poses, cams, fset = _dev(case["poses"], device), _dev(case["cams"], device), _dev(case["frame_set"], device)
    ids, views = _dev(case.get("ids"), device), _dev(case.get("views"), device)
    B, N, J = case["poses"].shape[:3]
    V = case["cams"].shape[1]
    has_views = views is not None and "views" not in over.get("null", ())
    want_vis = over.get("force_vis", has_views)
    o = [_dev(np.full((B, V, N, J), OCC_FILL, np.int32), device) if outs[0] else None,
         _dev(np.full((B, N, J), NAN, f32), device) if outs[1] and want_vis else None,
         _dev(np.full((B, N, J), COUNT_FILL, np.int32), device) if outs[2] and want_vis else None]
    prims, radius = over.get("prims", case["prims"]), over.get("radius", case["radius"])
    L = over.get("L", len(prims))
    cp = (C.c_int32 * max(2 * len(prims), 1))(*[int(x) for p in prims for x in p])
    cr = (C.c_float * max(len(radius), 1))(*[float(r) for r in radius])
    null = over.get("null", ())
    a = dict(poses=_ptr(poses), cams=_ptr(cams), frame_set=_ptr(fset), ids=_ptr(ids), views=_ptr(views), prims=cp, radius=cr)
    for k in null:
        a[k] = None
    rc = lib.fvp_joint_visibility(a["poses"], a["cams"], a["frame_set"], a["ids"], a["views"], over.get("B", B),
                                  over.get("V", V), over.get("N", N), over.get("J", J), a["prims"], a["radius"], L,
                                  over.get("guard", case["guard"]), over.get("Hs", case["Hs"]), over.get("Ws", case["Ws"]),
                                  _ptr(o[0]), _ptr(o[1]), _ptr(o[2]), _stream(device))
    _sync(device)
    return rc, [None if t is None else t.cpu().numpy() for t in o]


def assert_equal(got, want, what):
    occ, conf, count = got
    assert occ is None or np.array_equal(occ, want[0]), (what, np.argwhere(occ != want[0])[:8])
    if want[1] is not None:
        assert count is None or np.array_equal(count, want[2]), (what, np.argwhere(count != want[2])[:8])
        assert conf is None or np.array_equal(bits(conf), bits(want[1])), (what, np.argwhere(bits(conf) != bits(want[1]))[:8])


def check(lib, device, name):
    case, want = get(name)
    rc, got = call(lib, device, case)
    assert rc == 0, rc
    assert_equal(got, want, name)


def check_expectations(name):
    """The yardstick gives every named entry of a constructed scene the value the scene was built for."""
    case, (occ, conf, count) = get(name)
    assert case["expect"] or case.get("expect_count"), name
    for idx, want in case["expect"].items():
        assert occ[idx] == want, (name, idx, int(occ[idx]), want)
    for idx, want in case.get("expect_count", {}).items():
        assert count[idx] == want, (name, idx, int(count[idx]), want)


def check_null_outputs(lib, device):
    """Each output may be NULL, not all three; the others keep their bits.  Without views only occluder is written."""
    case, want = get("random_b2_v3_n4_j15")
    for outs in ((True, False, False), (False, True, False), (False, False, True), (False, True, True), (True, False, True)):
        rc, got = call(lib, device, case, outs=outs)
        assert rc == 0
        assert [g is not None for g in got] == list(outs)
        assert_equal(got, want, outs)
    assert call(lib, device, case, outs=(False, False, False))[0] == EINVAL
    rc, got = call(lib, device, case, null=("views",))
    assert rc == 0 and got[1] is None and np.array_equal(got[0], want[0])
    case, want = get("absent_people")
    rc, got = call(lib, device, case, null=("ids",))
    assert rc == 0
    assert_equal(got, reference(dict(case, ids=None)), "ids = NULL")
    assert not np.array_equal(got[0], want[0])


def _untouched(got):
    occ, conf, count = got
    return (occ is None or (occ == OCC_FILL).all()) and (conf is None or np.isnan(conf).all()) and (count is None or (count == COUNT_FILL).all())


def argument_errors(lib, device):
    case, _ = get("hidden_views")
    J = case["poses"].shape[2]
    bad = [dict(null=("poses",)), dict(null=("cams",)), dict(null=("frame_set",)), dict(null=("prims",)),
           dict(null=("radius",)), dict(null=("views",), force_vis=True), dict(B=-1), dict(V=0), dict(N=0), dict(J=0),
           dict(Hs=0), dict(Ws=0), dict(L=-1), dict(prims=[(0, 1), (1, J), (2, 2)]), dict(prims=[(0, 1), (-1, 3), (2, 2)]),
           dict(radius=[50.0, 0.0, 100.0]), dict(radius=[50.0, -1.0, 100.0]), dict(radius=[NAN, 50.0, 100.0]),
           dict(radius=[50.0, 50.0, INF]), dict(guard=-1.0), dict(guard=NAN), dict(guard=INF)]
    for over in bad:
        rc, got = call(lib, device, case, **over)
        assert rc == EINVAL, (over, rc)
        assert _untouched(got), over                                                      # nothing written
    for outs in ((False, True, False), (False, False, True)):                          # vis_* without views
        rc, got = call(lib, device, case, outs=outs, null=("views",), force_vis=True)
        assert rc == EINVAL and _untouched(got), outs
    many = [(0, 1)] * (MAX_PRIMS + 1)
    for over in (dict(N=MAX_PEOPLE + 1), dict(J=MAX_JOINTS + 1), dict(V=MAX_VIEWS + 1),
                 dict(prims=many, radius=[50.0] * len(many))):
        rc, got = call(lib, device, case, **over)
        assert rc == ELIMIT, (over, rc)
        assert _untouched(got), over
    rc, got = call(lib, device, case, B=0)                                              # no launch: nothing written
    assert rc == 0 and _untouched(got)
    rc, got = call(lib, device, case, prims=[], radius=[], null=("prims", "radius"))    # L == 0: no body, all visible
    assert rc == 0 and set(np.unique(got[0])) <= {-1, -2}


# ======================================================================================================================
# the second judge: the same definition in float64
# ======================================================================================================================
def fp64_scene():
    """The generator of the random scenes at 5 cameras, 10 people of 15 joints, guard 50: 4 500 joint-views."""
    prims, radius = body15()
    return random_scene(6, 5, 10, 15, prims, radius, seed=21, guard=50.0, spoil=False, with_views=False)


def fp64_compare(occ32, case, margin_mm=0.25, s_gap=1e-3):
    """occluder of the fp32 kernel against the fp64 definition.  Returns (joint-views evaluated, share left out, share
    occluded, disagreements on occluded / not, slots compared, slot disagreements).  Left out: some candidate primitive
    passes within ``margin_mm`` of its own surface in fp64.  The slot is compared only where the best hit of every other
    person is at least ``s_gap`` away in s."""
    occ64, _, _, margin, hit_s = reference(case, dt=f64, detail=True)
    ev = occ64 != -2
    assert np.array_equal(ev, occ32 != -2)
    keep = ev & (margin >= margin_mm)
    wrong = int(((occ32 >= 0) != (occ64 >= 0))[keep].sum())
    both = keep & (occ64 >= 0) & (occ32 >= 0)
    srt = np.sort(hit_s, axis=-1)
    with np.errstate(invalid="ignore"):                                                    # inf - inf where nobody hits
        clear = both & ((srt[..., 1] - srt[..., 0]) >= s_gap)
    slot_wrong = int((occ32 != occ64)[clear].sum())
    n = int(ev.sum())
    return n, 1.0 - keep.sum() / n, float((occ64 >= 0)[ev].mean()), wrong, int(clear.sum()), slot_wrong
