"""Shared by tests/test_limb_emu.py (CPU emulator) and tests/test_limb_gpu.py (the shipped library on the card): the yardstick
of fvp_limb_learn and fvp_limb_fit - an independent fp32 numpy restatement of the definitions in include/fvp.h (np.float32
scalars, np.sqrt, plain Python loops; no code shared with the product) - seeded scenarios, and the case bodies both files run.
Everything is compared bit for bit: target, limb_obs, limb_state, fitted, resid viewed as int32, and the five state arrays
after every call.  No tolerance appears anywhere; the property cases assert the bounds the definition was chosen for."""
import ctypes as C

import numpy as np
import torch

import track_cases as TC
from track_cases import EINVAL, ELIMIT, F32, _np, at, bits, chunks_of, pack, same

FLT_MAX = np.finfo(F32).max
DEFAULTS = dict(conf_min=0.0, min_frames=10, window=64, gate_sigma=3.0, gate_mm=20.0, relearn=15, stiffness=1.0, iters=4)
LEARNED, LEARNING, NOT_MEASURED, OUTLIER, RELEARNED, INVALID = 1, 2, 0, -1, -2, -3
# the tables of the three joint sets (COCO-17: cycles), restated here: the yardstick shares nothing with the product
LIMBS = {17: [(0, 1), (0, 2), (1, 2), (1, 3), (2, 4), (3, 5), (4, 6), (5, 7), (7, 9), (6, 8), (8, 10), (5, 11), (11, 13),
              (13, 15), (6, 12), (12, 14), (14, 16), (5, 6), (11, 12)],
         14: [(0, 1), (1, 2), (3, 4), (4, 5), (2, 3), (6, 7), (7, 8), (9, 10), (10, 11), (2, 8), (3, 9), (8, 12), (9, 12),
              (12, 13)],
         15: [(0, 1), (0, 2), (0, 3), (3, 4), (4, 5), (0, 9), (9, 10), (10, 11), (2, 6), (2, 12), (6, 7), (7, 8), (12, 13),
              (13, 14)]}


def random_limbs(seed, J, L):
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < L:
        i, k = (int(v) for v in rng.integers(0, J, size=2))
        if i != k:
            out.append((i, k))
    return out


# ---- the yardstick -----------------------------------------------------------------------------------------------
class Spec:
    def __init__(self, N, J, T, limbs, nseq=1, **kw):
        p = dict(DEFAULTS, **kw)
        self.N, self.J, self.T, self.nseq, self.limbs, self.L = N, J, T, nseq, list(limbs), len(limbs)
        self.conf_min, self.gate_sigma, self.gate_mm = F32(p["conf_min"]), F32(p["gate_sigma"]), F32(p["gate_mm"])
        self.min_frames, self.window, self.relearn = int(p["min_frames"]), int(p["window"]), int(p["relearn"])
        self.stiffness, self.iters = F32(p["stiffness"]), int(p["iters"])
        self.len = np.zeros((nseq, T, self.L), F32)
        self.var = np.zeros((nseq, T, self.L), F32)
        self.cnt = np.zeros((nseq, T, self.L), np.int32)
        self.out = np.zeros((nseq, T, self.L), np.int32)
        self.id = np.full((nseq, T), -1, np.int32)

    def supported(self, x, conf):
        return (conf is None or conf >= self.conf_min) and all(np.abs(x[c]) <= FLT_MAX for c in range(3))

    @staticmethod
    def dist(a, b):
        """delta = b - a, d and whether d is valid."""
        d0, d1, d2 = b[0] - a[0], b[1] - a[1], b[2] - a[2]
        d = np.sqrt((d0 * d0 + d1 * d1) + d2 * d2)
        assert d.dtype == F32
        return (d0, d1, d2), d, bool(d > 0 and d <= FLT_MAX)

    def limb(self, s, t, l, x, conf):
        """One limb of a slot whose id is settled: the statistics updated in place from the pose x [J,3]; (d, e, state)."""
        i, k = self.limbs[l]
        if not (self.supported(x[i], None if conf is None else conf[i]) and self.supported(x[k], None if conf is None else conf[k])):
            return F32(-1), F32(0), NOT_MEASURED
        _, d, ok = self.dist(x[i], x[k])
        if not ok:
            return F32(-1), F32(0), NOT_MEASURED
        e = d - self.len[s, t, l]
        passed = True
        if self.cnt[s, t, l] >= self.min_frames:
            tol = np.fmax(self.gate_sigma * np.sqrt(self.var[s, t, l]), self.gate_mm)
            passed = bool(np.abs(e) <= tol)
        if not passed:
            self.out[s, t, l] += 1
            if self.out[s, t, l] > self.relearn:
                self.len[s, t, l], self.var[s, t, l], self.cnt[s, t, l], self.out[s, t, l] = d, 0, 1, 0
                return d, e, RELEARNED
            return d, e, OUTLIER
        self.out[s, t, l] = 0
        c = min(int(self.cnt[s, t, l]) + 1, self.window)
        self.cnt[s, t, l] = c
        g = F32(1.0) / F32(c)
        ln = self.len[s, t, l] + g * e
        self.len[s, t, l] = ln
        v = self.var[s, t, l]
        self.var[s, t, l] = v + g * (e * (d - ln) - v)
        return d, e, (LEARNED if c >= self.min_frames else LEARNING)

    def update(self, poses, ids, slots, conf=None, frame_set=None):
        poses = np.asarray(poses, F32)
        B, N, T, L = poses.shape[0], self.N, self.T, self.L
        target = np.zeros((B, N, L), F32)
        obs = np.zeros((B, N, L, 2), F32)
        obs[..., 0] = -1
        state = np.full((B, N, L), INVALID, np.int32)
        with np.errstate(all="ignore"):
            for b in range(B):
                s = 0 if frame_set is None else int(frame_set[b])
                if not 0 <= s < self.nseq:
                    continue
                ok = [n for n in range(N) if ids[b, n] >= 0 and 0 <= slots[b, n] < T]
                for t in range(T):
                    here = [n for n in ok if slots[b, n] == t]
                    if not here:
                        continue
                    n = here[0]
                    if self.id[s, t] != ids[b, n]:
                        self.id[s, t] = ids[b, n]
                        self.len[s, t], self.var[s, t], self.cnt[s, t], self.out[s, t] = 0, 0, 0, 0
                    for l in range(L):
                        d, e, st = self.limb(s, t, l, poses[b, n, :, :3], None if conf is None else conf[b, n])
                        tg = self.len[s, t, l] if self.cnt[s, t, l] >= self.min_frames else F32(0)
                        for m in here:
                            target[b, m, l], obs[b, m, l], state[b, m, l] = tg, (d, e), st
        return target, obs, state

    def fit(self, poses, target, ids=None, conf=None):
        poses = np.asarray(poses, F32)
        B, N, L = poses.shape[0], self.N, self.L
        fitted = poses.copy()
        resid = np.zeros((B, N, L), F32)
        half, zero, one = F32(0.5), F32(0), F32(1)
        with np.errstate(all="ignore"):
            for b in range(B):
                for n in range(N):
                    if not (poses[b, n, 0, 3] >= 0 and (ids is None or ids[b, n] >= 0)):
                        continue
                    y = [[poses[b, n, j, c] for c in range(3)] for j in range(self.J)]
                    m = [self.supported(y[j], None if conf is None else conf[b, n, j]) for j in range(self.J)]
                    for _ in range(self.iters):
                        for l, (i, k) in enumerate(self.limbs):
                            tg = target[b, n, l]
                            if not tg > 0:
                                continue
                            dl, d, ok = self.dist(y[i], y[k])
                            if not ok:
                                continue
                            sc = (self.stiffness * (d - tg)) / d
                            wi, wk = (half, half) if m[i] == m[k] else ((zero, one) if m[i] else (one, zero))
                            for c in range(3):
                                y[i][c] = y[i][c] + (wi * sc) * dl[c]
                                y[k][c] = y[k][c] - (wk * sc) * dl[c]
                    for l, (i, k) in enumerate(self.limbs):
                        if target[b, n, l] > 0:
                            _, d, ok = self.dist(y[i], y[k])
                            if ok:
                                resid[b, n, l] = d - target[b, n, l]
                    fitted[b, n, :, :3] = np.asarray(y, F32)
        return fitted, resid

    def state(self):
        return dict(limb_len=self.len, limb_var=self.var, limb_cnt=self.cnt, limb_out=self.out, limb_id=self.id)


# ---- comparisons -----------------------------------------------------------------------------------------------------
NAMES = ("target", "limb_obs", "limb_state", "fitted", "resid")


def assert_outputs(got, want, what, names=NAMES):
    for name, g, w in zip(names, got, want):
        g, w = _np(g), _np(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.dtype, w.shape)
        bad = np.argwhere(bits(g) != bits(w))
        assert bad.size == 0, f"{what}: {name} differs at {len(bad)} elements, first {tuple(bad[0])}: " \
                              f"{g[tuple(bad[0])]!r} vs {w[tuple(bad[0])]!r}"


def assert_state(lm, spec, what):
    got = lm.state()
    for k, w in spec.state().items():
        g = _np(got[k])
        bad = np.argwhere(bits(g) != bits(w))
        assert g.shape == w.shape and g.dtype == w.dtype and bad.size == 0, \
            f"{what}: state {k} differs at {len(bad)} elements, first {tuple(bad[0])}: {g[tuple(bad[0])]!r} vs {w[tuple(bad[0])]!r}"


def _dev(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ---- runners ----------------------------------------------------------------------------------------------------------
def run(mk, poses, chunks, limbs, conf=None, frame_set=None, what="", nseq=1, T=None, max_age=15, **kw):
    """``poses`` [F,N,J,5] through a fresh PoseTracker and a LimbModel built from it (``mk(N, J, nseq, T, max_age, limbs,
    **kw)`` -> (tracker, limb model)) in calls of the given sizes: tracker -> learn -> fit of the same poses.  After EVERY
    call the five outputs and the whole state equal the yardstick's (fed the tracker's ids / slots).  Returns the
    concatenated outputs + ids, slots (numpy), the state after every call, and the pair."""
    F, N, J = poses.shape[:3]
    T = 2 * N if T is None else T
    assert sum(chunks) == F
    tracker, lm = mk(N, J, nseq, T, max_age, limbs, **kw)
    spec = Spec(N, J, T, limbs, nseq, **kw)
    dev = lm.device
    outs, states, f = [], [], 0
    for c in chunks:
        x = _dev(poses[f:f + c], dev)
        fs = None if frame_set is None else np.asarray(frame_set[f:f + c], np.int32)
        seqs = _dev(fs, dev)
        cf = None if conf is None else np.ascontiguousarray(conf[f:f + c])
        ids, slots, _ = tracker.update(x, sequences=seqs)
        got = lm.update(x, ids, slots, joint_conf=_dev(cf, dev), sequences=seqs)
        got = tuple(got) + tuple(lm.fit(x, got[0], ids, _dev(cf, dev)))
        want = spec.update(poses[f:f + c], _np(ids), _np(slots), cf, fs)
        want = want + spec.fit(poses[f:f + c], want[0], _np(ids), cf)
        assert_outputs(got, want, f"{what} frames {f}..{f + c - 1}")
        assert_state(lm, spec, f"{what} after frame {f + c - 1}")
        outs.append([_np(g).copy() for g in got] + [_np(ids).copy(), _np(slots).copy()])
        states.append({k: _np(v).copy() for k, v in lm.state().items()})
        f += c
    return [np.concatenate([o[k] for o in outs]) for k in range(7)], states, (tracker, lm)


def run_direct(mk_shape, poses, ids, slots, chunks, limbs, conf=None, what="", T=None, **kw):
    """As ``run`` with hand-made ids / slots and a limb model built from the shape (no tracker)."""
    F, N, J = poses.shape[:3]
    T = 2 * N if T is None else T
    lm = mk_shape(N, J, T, 1, limbs, **kw)
    spec = Spec(N, J, T, limbs, 1, **kw)
    dev = lm.device
    ids, slots = np.asarray(ids, np.int32), np.asarray(slots, np.int32)
    outs, states, f = [], [], 0
    for c in chunks:
        sl = slice(f, f + c)
        cf = None if conf is None else np.ascontiguousarray(conf[sl])
        x, i = _dev(poses[sl], dev), _dev(ids[sl], dev)
        got = lm.update(x, i, _dev(slots[sl], dev), joint_conf=_dev(cf, dev))
        got = tuple(got) + tuple(lm.fit(x, got[0], i, _dev(cf, dev)))
        want = spec.update(poses[sl], ids[sl], slots[sl], cf)
        want = want + spec.fit(poses[sl], want[0], ids[sl], cf)
        assert_outputs(got, want, f"{what} frames {f}..{f + c - 1}")
        assert_state(lm, spec, f"{what} after frame {f + c - 1}")
        outs.append([_np(g).copy() for g in got])
        states.append({k: _np(v).copy() for k, v in lm.state().items()})
        f += c
    return [np.concatenate([o[k] for o in outs]) for k in range(5)], states, lm


def fit_direct(mk_shape, poses, target, limbs, ids=None, conf=None, what="fit", **kw):
    """One fvp_limb_fit call through LimbModel.fit against the yardstick; (fitted, resid) as numpy."""
    B, N, J = poses.shape[:3]
    lm = mk_shape(N, J, N, 1, limbs, **kw)
    dev = lm.device
    got = lm.fit(_dev(poses, dev), _dev(target, dev), _dev(ids, dev), _dev(conf, dev))
    want = Spec(N, J, N, limbs, 1, **kw).fit(poses, target, ids, conf)
    assert_outputs(got, want, what, NAMES[3:])
    return _np(got[0]).copy(), _np(got[1]).copy()


# ---- scenarios ----------------------------------------------------------------------------------------------------------
N = 4


def rigid_walkers(seed, P, J, F, noise=5.0, step=20.0):
    """truth [F,P,J,3] float64: P rigid skeletons 1500 mm apart that walk (root step ~ N(0, step) mm per axis and frame) and
    turn about the vertical (~ N(0, 0.05) rad per frame) - every limb keeps its length; noisy [F,P,J,3] fp32: the truth
    with Gaussian jitter of ``noise`` mm per coordinate."""
    rng = np.random.default_rng(seed)
    roots = np.stack([np.array([1500.0 * (p % 4) - 2250.0, 1500.0 * (p // 4) - 1500.0, 900.0]) for p in range(P)])
    skel = np.stack([TC.skeleton(rng, J) for _ in range(P)]).astype(np.float64)
    heading = rng.uniform(-np.pi, np.pi, size=P)
    truth = np.empty((F, P, J, 3))
    for f in range(F):
        roots = roots + rng.normal(0.0, step, size=roots.shape)
        heading = heading + rng.normal(0.0, 0.05, size=P)
        c, s = np.cos(heading), np.sin(heading)
        rot = np.zeros((P, 3, 3))
        rot[:, 0, 0], rot[:, 0, 1], rot[:, 1, 0], rot[:, 1, 1], rot[:, 2, 2] = c, -s, s, c, 1.0
        truth[f] = roots[:, None, :] + np.einsum("pab,pjb->pja", rot, skel)
    noisy = (truth + rng.normal(0.0, noise, size=truth.shape)).astype(F32)
    return truth, noisy


def _scene(J, F=9, seed=71, P=3, present=None):
    _, people = rigid_walkers(seed, P, J, F)
    present = np.ones((F, P), bool) if present is None else present
    poses, slot_of = pack(seed + 1, people, present, N)
    conf = np.random.default_rng(seed + 2).uniform(0.0, 1.0, size=(F, N, J)).astype(F32)
    return people, poses, slot_of, conf


def _person(track, n=2, t=1, ident=0):
    """track [F,J,3] as one person in detection slot n / track slot t -> poses [F,N,J,5], ids, slots."""
    F, J = track.shape[:2]
    poses = np.zeros((F, N, J, 5), F32)
    poses[:, :, :, 3] = -1.0
    poses[:, n, :, :3], poses[:, n, :, 3], poses[:, n, :, 4] = track, 0.0, 0.5
    ids = np.full((F, N), -1, np.int32)
    slots = np.full((F, N), -1, np.int32)
    ids[:, n], slots[:, n] = ident, t
    return poses, ids, slots


def _stick(lengths):
    """J = 2, L = 1: joint 0 at the origin, joint 1 at (d, 0, 0) - the measured length is d exactly."""
    track = np.zeros((len(lengths), 2, 3), F32)
    track[:, 1, 0] = np.asarray(lengths, F32)
    return track


# ---- the cases (each takes the factories of its file) ----------------------------------------------------------------------
# J, T, B, limbs: four / three slots per wave, the Shelf table with a partial last wave, one slot per wave (L = 1, L = 64)
WALKERS = [(15, 4, 1, LIMBS[15]), (17, 8, 3, LIMBS[17]), (14, 5, 8, LIMBS[14]), (15, 5, 3, LIMBS[15]),
           (32, 4, 3, [(31, 7)]), (32, 8, 8, random_limbs(64, 32, 64))]


def case_walkers(mk, J, T, B, limbs):
    """Noisy rigid walkers through tracker -> learn -> fit, slots permuted per frame, a third of the joints below conf_min."""
    F = 12
    _, poses, slot_of, conf = _scene(J, F, seed=71 + J + B)
    (target, obs, state, fitted, resid, ids, slots), states, _ = run(mk, poses, chunks_of(F, B), limbs, conf, what="walkers",
                                                                     T=T, conf_min=0.33, min_frames=3)
    assert (slot_of[0] != slot_of[1]).any()
    for f in range(F):
        inv = ids[f] < 0
        assert inv.sum() == 1 and (state[f][inv] == INVALID).all() and (target[f][inv] == 0).all()
        assert same(fitted[f][inv], poses[f][inv]) and (resid[f][inv] == 0).all()
        assert same(fitted[f][..., 3:], poses[f][..., 3:]) and (state[f][~inv] != INVALID).all()
    assert (state == NOT_MEASURED).any() and (state == LEARNED).any() and (state[0][ids[0] >= 0] != LEARNED).all()
    assert (target[-1][ids[-1] >= 0] > 0).any() and np.isfinite(fitted).all() and (resid != 0).any()
    assert not same(fitted[-1], poses[-1])


def case_constant(mk, J, B):
    """A constant pose: var == 0, target == d from the min_frames-th frame on and 0 before it, and the fit leaves the bits of
    a pose that already has its target lengths (d - l == 0: y + (w * 0) * delta = y)."""
    F, mf, limbs = 8, 3, LIMBS[J]
    people = np.repeat(rigid_walkers(5, 3, J, 1)[1], F, axis=0)
    poses, slot_of = pack(6, people, np.ones((F, 3), bool), N)
    (target, obs, state, fitted, resid, ids, slots), states, (_, lm) = run(mk, poses, chunks_of(F, B), limbs, what="constant",
                                                                          T=8, min_frames=mf)
    st = states[-1]
    live = st["limb_id"][0] >= 0
    assert live.sum() == 3 and (st["limb_var"] == 0).all() and (st["limb_cnt"][0][live] == F).all()
    assert same(fitted, poses) and (resid == 0).all()
    for f in range(F):
        v = ids[f] >= 0
        assert (state[f][v] == (LEARNED if f >= mf - 1 else LEARNING)).all()
        assert same(target[f][v], obs[f][v][..., 0]) if f >= mf - 1 else (target[f] == 0).all()
        assert (obs[f][v][..., 1] == 0).all() if f else same(obs[f][v][..., 1], obs[f][v][..., 0])


def case_first_sample_and_edges(mk_shape):
    """The first sample gives len = d, var = 0; target is 0 until the min_frames-th sample and len from it on; cnt saturates
    at window (exponential forgetting from there)."""
    mf, win = 3, 5
    d = [100.0, 104.0, 99.0, 101.0, 103.0, 98.0, 102.0, 100.5]
    poses, ids, slots = _person(_stick(d))
    (target, obs, state, _, _), states, _ = run_direct(mk_shape, poses, ids, slots, [1] * len(d), [(0, 1)], what="edges",
                                                       min_frames=mf, window=win, gate_mm=50.0)
    s0 = states[0]
    assert s0["limb_len"][0, 1, 0] == F32(100.0) and s0["limb_var"][0, 1, 0] == 0 and s0["limb_cnt"][0, 1, 0] == 1
    assert s0["limb_id"][0].tolist() == [-1, 0, -1, -1, -1, -1, -1, -1] and (s0["limb_cnt"][0, [0, 2, 3]] == 0).all()
    assert obs[0, 2, 0].tolist() == [100.0, 100.0] and state[:, 2, 0].tolist() == [LEARNING] * (mf - 1) + [LEARNED] * (len(d) - mf + 1)
    assert (target[:mf - 1, 2, 0] == 0).all()
    for f in range(mf - 1, len(d)):
        assert target[f, 2, 0] == states[f]["limb_len"][0, 1, 0] and states[f]["limb_var"][0, 1, 0] > 0
    assert [int(s["limb_cnt"][0, 1, 0]) for s in states] == [1, 2, 3, 4, 5, 5, 5, 5]


def case_gate_edges(mk_shape):
    """|e| == tol is accepted, nextafter above it is an outlier; gate_mm governs when var == 0, gate_sigma * sqrt(var) when
    it is larger; gate_sigma == gate_mm == 0 rejects everything but an exact repeat."""
    up = lambda v: float(np.nextafter(F32(v), F32(np.inf)))                                     # noqa: E731

    def last_state(d, **kw):
        poses, ids, slots = _person(_stick(d))
        (target, obs, state, _, _), states, _ = run_direct(mk_shape, poses, ids, slots, [len(d)], [(0, 1)], what=f"gate {d}",
                                                           min_frames=2, **kw)
        return int(state[-1, 2, 0]), obs[-1, 2, 0], states[-1]
    # var == 0: tol = gate_mm = 20; 120 - 100 == 20 exactly
    st, ob, _ = last_state([100.0, 100.0, 120.0], gate_sigma=3.0, gate_mm=20.0)
    assert st == LEARNED and ob[1] == F32(20.0)
    st, ob, s = last_state([100.0, 100.0, up(120.0)], gate_sigma=3.0, gate_mm=20.0)
    assert st == OUTLIER and ob[1] > F32(20.0) and s["limb_out"][0, 1, 0] == 1 and s["limb_len"][0, 1, 0] == F32(100.0)
    # var > 0, gate_mm = 0: the largest accepted d by the yardstick's own arithmetic, and its successor
    _, _, s = last_state([100.0, 108.0], gate_sigma=2.0, gate_mm=0.0)
    ln, var = s["limb_len"][0, 1, 0], s["limb_var"][0, 1, 0]
    tol = F32(2.0) * np.sqrt(var)
    assert var > 0 and tol > 0
    d = F32(ln + tol)
    while np.abs(F32(d - ln)) <= tol:
        d = np.nextafter(d, F32(np.inf))
    while not np.abs(F32(d - ln)) <= tol:
        d = np.nextafter(d, F32(0))
    assert last_state([100.0, 108.0, float(d)], gate_sigma=2.0, gate_mm=0.0)[0] == LEARNED
    assert last_state([100.0, 108.0, up(d)], gate_sigma=2.0, gate_mm=0.0)[0] == OUTLIER
    assert last_state([100.0, 108.0, up(d)], gate_sigma=2.0, gate_mm=float(tol) + 1.0)[0] == LEARNED     # gate_mm governs
    # both 0: only the exact repeat passes
    assert last_state([100.0, 100.0, 100.0], gate_sigma=0.0, gate_mm=0.0)[0] == LEARNED
    assert last_state([100.0, 100.0, up(100.0)], gate_sigma=0.0, gate_mm=0.0)[0] == OUTLIER
    # below min_frames nothing is gated
    assert last_state([100.0, 900.0], gate_sigma=0.0, gate_mm=0.0)[0] == LEARNED


def case_outliers_and_relearn(mk_shape):
    """A burst of `relearn` outlier frames leaves the statistics bit-identical and `out` counts it; the next inlier clears the
    count.  relearn + 1 outliers start over: RELEARNED, cnt = 1, target = 0 until learned again."""
    relearn, mf = 3, 2
    d = [100.0, 101.0, 99.0] + [300.0] * relearn + [100.0] + [300.0, 301.0, 299.0, 300.5, 300.0]
    poses, ids, slots = _person(_stick(d))
    (target, obs, state, fitted, _), states, _ = run_direct(mk_shape, poses, ids, slots, [1] * len(d), [(0, 1)], what="burst",
                                                            min_frames=mf, relearn=relearn, gate_mm=10.0)
    for f in range(3, 3 + relearn):
        assert state[f, 2, 0] == OUTLIER and states[f]["limb_out"][0, 1, 0] == f - 2
        for k in ("limb_len", "limb_var", "limb_cnt"):
            assert same(states[f][k], states[2][k])
        assert target[f, 2, 0] == states[2]["limb_len"][0, 1, 0] and obs[f, 2, 0, 0] == F32(300.0)
        assert fitted[f, 2, 1, 0] - fitted[f, 2, 0, 0] < F32(110.0)                                             # the fit pulls the outlier back
    f = 3 + relearn
    assert state[f, 2, 0] == LEARNED and states[f]["limb_out"][0, 1, 0] == 0 and states[f]["limb_cnt"][0, 1, 0] == 4
    assert state[f + 1:f + 1 + relearn, 2, 0].tolist() == [OUTLIER] * relearn
    f += relearn + 1
    assert state[f, 2, 0] == RELEARNED and target[f, 2, 0] == 0 and obs[f, 2, 0, 0] == F32(300.5)
    s = states[f]
    assert (s["limb_len"][0, 1, 0], s["limb_var"][0, 1, 0], s["limb_cnt"][0, 1, 0], s["limb_out"][0, 1, 0]) == (F32(300.5), 0, 1, 0)
    assert state[f + 1, 2, 0] == LEARNED and target[f + 1, 2, 0] == states[f + 1]["limb_len"][0, 1, 0] > 300


def case_conf_edge(mk_shape, J):
    """conf == conf_min is supported, nextafter below it and NaN are not; joint_conf = None: every finite joint is."""
    cm = F32(0.4)
    below = np.nextafter(cm, F32(0))
    limbs = LIMBS[J]
    sk = TC.skeleton(np.random.default_rng(9), J)
    poses = np.stack([at({1: (100.0 * f, 50.0, 900.0)}, N, J, sk) for f in range(3)])
    ids = np.full((3, N), -1, np.int32)
    slots = np.full((3, N), -1, np.int32)
    ids[:, 1], slots[:, 1] = 7, 2
    conf = np.ones((3, N, J), F32)
    conf[:, 1, 0], conf[1:, 1, 1], conf[1:, 1, 2], conf[1:, 1, 3] = cm, below, np.nan, 0.0
    (_, _, state, fitted, _), _, _ = run_direct(mk_shape, poses, ids, slots, [1, 2], limbs, conf, what="conf edge",
                                                conf_min=float(cm), min_frames=1)
    touched = np.array([bool({i, k} & {1, 2, 3}) for i, k in limbs])
    assert touched.any() and not touched.all() and (state[0, 1] == LEARNED).all()
    for f in (1, 2):
        assert (state[f, 1][touched] == NOT_MEASURED).all() and (state[f, 1][~touched] == LEARNED).all()
    (_, _, state, _, _), _, _ = run_direct(mk_shape, poses, ids, slots, [3], limbs, None, what="no joint_conf",
                                           conf_min=float(cm), min_frames=1)
    assert (state[:, 1] == LEARNED).all()


def case_nonfinite(mk_shape, J):
    """NaN / Inf / overflowing joints and coincident ends: NOT_MEASURED in learn, skipped by the fit; every other joint stays
    finite and bit-equal to the yardstick."""
    limbs = LIMBS[J]
    sk = TC.skeleton(np.random.default_rng(10), J)
    poses = np.stack([at({0: (20.0 * f, 0.0, 900.0), 3: (3000.0, 10.0 * f, 900.0)}, N, J, sk) for f in range(5)])
    poses[:, :, :, :3] += np.random.default_rng(11).normal(0.0, 5.0, size=poses[:, :, :, :3].shape).astype(F32)
    i0, k0 = limbs[0]
    i1, k1 = limbs[-1]
    poses[2, 0, 3, 1] = np.nan
    poses[2, 0, 4, 2] = np.inf
    poses[3, 0, 5, 0] = F32(3.0e38)                                                            # finite, every distance overflows
    poses[3, 0, 6, 0] = F32(-3.0e38)
    poses[4, 0, k0, :3] = poses[4, 0, i0, :3]                                                  # d == 0
    poses[4, 3, k1, :3] = poses[4, 3, i1, :3]
    ids = np.full((5, N), -1, np.int32)
    slots = np.full((5, N), -1, np.int32)
    ids[:, 0], slots[:, 0], ids[:, 3], slots[:, 3] = 0, 1, 1, 0
    (target, obs, state, fitted, resid), states, _ = run_direct(mk_shape, poses, ids, slots, [2, 1, 2], limbs,
                                                                what="non-finite", min_frames=2, gate_mm=100.0)
    for f, joints in ((2, {3, 4}), (3, {5, 6})):
        hit = np.array([bool({i, k} & joints) for i, k in limbs])
        assert (state[f, 0][hit] == NOT_MEASURED).all() and (state[f, 0][~hit] == LEARNED).all()
        assert (obs[f, 0][hit] == np.array([-1, 0], F32)).all() and (target[f, 0] > 0).all()
        others = [j for j in range(J) if j not in joints]
        assert np.isfinite(fitted[f, 0, others, :3]).all() and same(fitted[f, 0, sorted(joints)], poses[f, 0, sorted(joints)])
        assert (resid[f, 0][hit] == 0).all()
    assert state[4, 0, 0] == NOT_MEASURED and state[4, 3, -1] == NOT_MEASURED and (state[4, 0, 1:] == LEARNED).all()
    assert np.isfinite(states[-1]["limb_len"]).all() and np.isfinite(fitted[4]).all() and np.isfinite(resid).all()


def case_id_changes(mk, J):
    """N = T = 4: a birth into a full table evicts a track and every limb of the slot starts over in that same frame."""
    def pt(k):
        return (3000.0 * k, 0.0, 0.0)
    limbs = LIMBS[J]
    frames = [{0: pt(0), 1: pt(1), 2: pt(2), 3: pt(3)}, {0: pt(0), 1: pt(1), 2: pt(4), 3: pt(5)},
              {0: pt(0), 1: pt(4), 2: pt(6), 3: pt(7)}, {0: pt(6), 1: pt(8)}, {0: pt(6), 1: pt(9), 2: pt(10)}]
    sk = TC.skeleton(np.random.default_rng(13), J)
    poses = np.stack([at(fr, N, J, sk) for fr in frames])
    (target, _, state, _, _, ids, slots), states, _ = run(mk, poses, [1] * 5, limbs, what="full table", T=4, min_frames=2)
    assert slots[2].tolist() == [0, 2, 1, 3] and ids[2].tolist() == [0, 4, 6, 7]               # (the tracker's own case)
    want_cnt = [[1, 1, 1, 1], [2, 2, 1, 1], [3, 1, 2, 1]]                                      # per track slot
    for f, w in enumerate(want_cnt):
        assert states[f]["limb_cnt"][0, :, 0].tolist() == w, (f, states[f]["limb_cnt"][0, :, 0].tolist())
        assert states[f]["limb_id"][0].tolist() == [ids[f][slots[f].tolist().index(t)] for t in range(4)]
    assert (state[1, 2] == LEARNING).all() and (target[1, 2] == 0).all() and (state[1, 0] == LEARNED).all()
    assert (state[3, 2:] == INVALID).all() and ids[3].tolist() == [6, 8, -1, -1] and slots[3].tolist() == [1, 0, -1, -1]
    for k in ("limb_len", "limb_var", "limb_cnt", "limb_id"):                                  # unseen slots: kept as they are
        assert same(states[3][k][0, 2:], states[2][k][0, 2:])
    assert (states[3]["limb_cnt"][0, 0] == 1).all() and (states[3]["limb_cnt"][0, 1] == 2).all()


def case_gaps(mk, J, B):
    """max_age = 3.  A is missing for 3 frames and comes back as itself: its lengths and counts carry on.  B is missing for 4:
    freed, and newcomer C takes the slot under a new id - every limb of the slot starts over in that frame."""
    F, max_age, limbs = 8, 3, LIMBS[J]
    present = np.ones((F, 4), bool)
    present[1:4, 0] = False
    present[1:5, 1] = False
    present[:4, 3] = False
    _, poses, slot_of, _ = _scene(J, F, seed=21 + J, P=4, present=present)
    (target, _, state, _, _, ids, slots), states, _ = run(mk, poses, chunks_of(F, B), limbs, what="gaps", T=8,
                                                          max_age=max_age, min_frames=2, gate_mm=100.0)
    ta, tb = slots[0, slot_of[0, 0]], slots[0, slot_of[0, 1]]
    nc = slot_of[4, 3]
    assert slots[4, slot_of[4, 0]] == ta and ids[4, slot_of[4, 0]] == ids[0, slot_of[0, 0]]
    assert slots[4, nc] == tb and ids[4, nc] != ids[0, slot_of[0, 1]]
    assert (state[4, slot_of[4, 0]] != LEARNING).all() and (state[4, nc] == LEARNING).all() and (target[4, nc] == 0).all()
    last = states[-1]
    assert (last["limb_cnt"][0, ta] == 5).all() and (last["limb_cnt"][0, tb] == 4).all() and last["limb_id"][0, tb] == ids[4, nc]
    if B == 1:                                                                                 # while A and B coast: untouched
        for f in (1, 2, 3):
            for k in ("limb_len", "limb_var", "limb_cnt", "limb_out", "limb_id"):
                assert same(states[f][k][0, [ta, tb]], states[0][k][0, [ta, tb]])


# the fit on its own -------------------------------------------------------------------------------------------------------
def case_fit_weights(mk_shape):
    """One case per (m_i, m_k): the unsupported end alone moves; with both ends supported, and with both unsupported, each
    moves half."""
    poses = np.zeros((1, N, 2, 5), F32)
    poses[0, :, 0, :3], poses[0, :, 1, :3] = (10.0, 20.0, 30.0), (310.0, 420.0, 30.0)          # d = 500
    poses[..., 4] = 0.5
    target = np.full((1, N, 1), 400.0, F32)
    conf = np.array([[[1, 1], [1, 0], [0, 1], [0, 0]]], F32)
    fitted, resid = fit_direct(mk_shape, poses, target, [(0, 1)], conf=conf, what="fit weights", conf_min=0.5, iters=1)
    moved = np.abs(fitted[0, :, :, :3] - poses[0, :, :, :3]).max(axis=-1) > 0
    assert moved.tolist() == [[True, True], [False, True], [True, False], [True, True]]
    assert same(fitted[0, 1, 0], poses[0, 1, 0]) and same(fitted[0, 2, 1], poses[0, 2, 1]) and same(fitted[0, 0], fitted[0, 3])
    step = np.linalg.norm(fitted[0, :, :, :3].astype(np.float64) - poses[0, :, :, :3], axis=-1)
    assert np.allclose(step, [[50, 50], [0, 100], [100, 0], [50, 50]], atol=1e-3) and (np.abs(resid) < 1e-3).all()


def case_fit_parameters(mk_shape, J):
    """stiffness = 0 returns the input bits; iters = 1 and 32; a target of 0 / negative / NaN leaves the limb unconstrained;
    B * N = 65 people: a second workgroup with one live lane."""
    limbs = LIMBS[J]
    L = len(limbs)
    rng = np.random.default_rng(17)
    B, N_ = 13, 5
    poses = np.zeros((B, N_, J, 5), F32)
    poses[..., :3] = (rng.uniform(-2000, 2000, size=(B, N_, 1, 3)) + rng.uniform(-300, 300, size=(B, N_, J, 3))).astype(F32)
    poses[..., 4] = rng.uniform(0, 1, size=(B, N_, J)).astype(F32)
    poses[rng.uniform(size=(B, N_)) < 0.2, :, 3] = -1.0
    poses[12, 4, :, 3] = 0.0                                                                   # person 65 is a live one
    target = rng.uniform(100.0, 500.0, size=(B, N_, L)).astype(F32)
    conf = rng.uniform(0, 1, size=(B, N_, J)).astype(F32)
    mk5 = lambda n, j, t, s, lb, **kw: mk_shape(n, j, max(t, n), s, lb, **kw)                   # noqa: E731
    fitted, _ = fit_direct(mk5, poses, target, limbs, conf=conf, what="stiffness 0", stiffness=0.0, conf_min=0.3)
    assert same(fitted, poses)
    res = {}
    for iters in (1, 32):
        fitted, resid = fit_direct(mk5, poses, target, limbs, conf=conf, what=f"iters {iters}", iters=iters, conf_min=0.3,
                                   stiffness=0.7)
        valid = poses[:, :, 0, 3] >= 0
        assert same(fitted[~valid], poses[~valid]) and (resid[~valid] == 0).all() and not same(fitted[12, 4], poses[12, 4])
        res[iters] = np.abs(resid[valid]).mean()
    if J != 17:
        assert res[32] < 0.1 * res[1]                                                          # on a tree more sweeps leave less
    t2 = target.copy()
    t2[:, :, 0], t2[:, :, 1], t2[:, :, 2] = 0.0, -250.0, np.nan
    fitted, resid = fit_direct(mk5, poses, t2, limbs, conf=conf, what="unconstrained limbs", conf_min=0.3)
    assert (resid[:, :, :3] == 0).all() and np.isfinite(fitted).all()
    t3 = np.zeros_like(target)
    t3[:, :, 3] = target[:, :, 3]
    fitted, _ = fit_direct(mk5, poses, t3, limbs, what="one limb")
    free = [j for j in range(J) if j not in limbs[3]]
    assert same(fitted[:, :, free], poses[:, :, free])


def case_fit_invalid_slots(mk_shape, J):
    """Invalid slots (flag < 0), ids NULL against given, negative ids: copied unchanged, resid 0."""
    limbs = LIMBS[J]
    _, poses, _, conf = _scene(J, 3, seed=33)
    target = np.full((3, N, len(limbs)), 250.0, F32)
    ids = np.array([[0, -1, 2, 3], [-1, -1, -1, -1], [5, 6, 7, -2]], np.int32)
    flag_ok = poses[:, :, 0, 3] >= 0
    f0, r0 = fit_direct(mk_shape, poses, target, limbs, what="ids NULL")
    f1, r1 = fit_direct(mk_shape, poses, target, limbs, ids=ids, what="ids given")
    assert same(f0[~flag_ok], poses[~flag_ok]) and (r0[~flag_ok] == 0).all() and (r0[flag_ok] != 0).any()
    ok = flag_ok & (ids >= 0)
    assert same(f1[~ok], poses[~ok]) and (r1[~ok] == 0).all() and same(f1[ok], f0[ok]) and same(r1[ok], r0[ok])
    assert ok.any() and (flag_ok & ~ok).any()


# chunking and sequences ----------------------------------------------------------------------------------------------------
def _mixed(J, F=8, seed=41):
    present = np.ones((F, 4), bool)
    present[2:4, 1] = False
    present[3, 2] = False
    present[:2, 3] = False
    return _scene(J, F, seed, P=4, present=present)


def case_chunk_invariance(mk, J):
    _, poses, _, conf = _mixed(J)
    runs = [run(mk, poses, ch, LIMBS[J], conf, what=f"chunks {ch}", T=8, max_age=1, conf_min=0.25, min_frames=2)
            for ch in ([8], [3, 5], [1] * 8)]
    for out, states, _ in runs[1:]:
        for x, y in zip(out, runs[0][0]):
            assert same(x, y)
        for k, v in states[-1].items():
            assert same(v, runs[0][1][-1][k])


def case_two_sequences(mk, J):
    (_, a, _, ca), (_, b, _, cb) = _mixed(J, 4, seed=51), _mixed(J, 4, seed=61)
    frame_set = [0, 1, 1, 0, 1, 0, 0, 1]
    fs = np.asarray(frame_set)
    poses, conf = np.empty((8,) + a.shape[1:], F32), np.empty((8,) + ca.shape[1:], F32)
    poses[fs == 0], poses[fs == 1], conf[fs == 0], conf[fs == 1] = a, b, ca, cb
    kw = dict(T=8, conf_min=0.25, min_frames=2)
    out, states, _ = run(mk, poses, [8], LIMBS[J], conf, frame_set, what="two sequences", nseq=2, **kw)
    for s, own, cown in ((0, a, ca), (1, b, cb)):
        out1, states1, _ = run(mk, own, [4], LIMBS[J], cown, what=f"sequence {s} alone", **kw)
        for x, y in zip(out, out1):
            assert same(x[fs == s], y)
        for k, v in states1[-1].items():
            assert same(states[-1][k][s], v[0])
    # a frame of no sequence (row 2 of two): written as invalid, fitted is the input; no state changes
    fs2 = list(frame_set)
    fs2[3] = 2
    (target, obs, state, fitted, resid, ids, _), _, _ = run(mk, poses, [8], LIMBS[J], conf, fs2, what="a frame of no sequence",
                                                            nseq=2, **kw)
    assert (ids[3] == -1).all() and (state[3] == INVALID).all() and (target[3] == 0).all() and (obs[3, ..., 0] == -1).all()
    assert same(fitted[3], poses[3]) and (resid[3] == 0).all() and (state[4] != INVALID).any()


# ---- the C entry points themselves ----------------------------------------------------------------------------------------------
LEARN_PRM = dict(conf_min=0.3, min_frames=2, window=8, gate_sigma=3.0, gate_mm=20.0, relearn=2)
FIT_PRM = dict(conf_min=0.3, stiffness=1.0, iters=4)


def _limb_array(limbs):
    return (C.c_int32 * (2 * len(limbs)))(*[j for ab in limbs for j in ab])


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream) if torch.device(dev).type == "cuda" else None


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def raw_learn(lib, dev, inputs, limbs, state, outs, B, N_, J, nseq, T, L=None, **kw):
    q = dict(LEARN_PRM, **kw)
    return lib.fvp_limb_learn(*[_p(t) for t in inputs], None if limbs is None else _limb_array(limbs),
                              len(limbs) if L is None else L, *[_p(t) for t in tuple(state) + tuple(outs)], B, N_, J, nseq, T,
                              q["conf_min"], q["min_frames"], q["window"], q["gate_sigma"], q["gate_mm"], q["relearn"],
                              _stream(dev))


def raw_fit(lib, dev, poses, ids, conf, target, limbs, fitted, resid, B, N_, J, L=None, **kw):
    q = dict(FIT_PRM, **kw)
    return lib.fvp_limb_fit(_p(poses), _p(ids), _p(conf), _p(target), None if limbs is None else _limb_array(limbs),
                            len(limbs) if L is None else L, _p(fitted), _p(resid), B, N_, J, q["conf_min"], q["stiffness"],
                            q["iters"], _stream(dev))


def _raw_setup(dev, J=15, T=8, B=3):
    limbs = LIMBS[J]
    L = len(limbs)
    _, poses, _, conf = _mixed(J)
    poses, conf = np.ascontiguousarray(poses[:B]), np.ascontiguousarray(conf[:B])
    ids = np.full((B, N), -1, np.int32)
    slots = np.full((B, N), -1, np.int32)
    for b in range(B):
        for k, n in enumerate(np.flatnonzero(poses[b, :, 0, 3] >= 0)):
            ids[b, n], slots[b, n] = 10 + k, (k + 1) % T
    inputs = [_dev(a, dev) for a in (poses, np.zeros((B,), np.int32), ids, slots, conf)]

    def buffers(T_=T, L_=L):
        state = (torch.full((1, T_, L_), 7.0, device=dev), torch.full((1, T_, L_), 2.0, device=dev),
                 torch.full((1, T_, L_), 1, dtype=torch.int32, device=dev), torch.full((1, T_, L_), 0, dtype=torch.int32, device=dev),
                 torch.full((1, T_), -1, dtype=torch.int32, device=dev))
        outs = (torch.full((B, N, L_), 77.0, device=dev), torch.full((B, N, L_, 2), 77.0, device=dev),
                torch.full((B, N, L_), 77, dtype=torch.int32, device=dev))
        return state, outs
    return inputs, buffers, limbs, B, J, T


def case_null_arguments(lib, dev):
    """frame_set and joint_conf may be NULL in learn, ids, joint_conf and resid in fit - what is written equals the yardstick's
    and the full call's; fitted may be poses itself; every other null pointer is an error with nothing written."""
    inputs, buffers, limbs, B, J, T = _raw_setup(dev)
    L = len(limbs)
    poses, ids, slots, conf = (_np(inputs[k]) for k in (0, 2, 3, 4))
    state, outs = buffers()
    assert raw_learn(lib, dev, [inputs[0], None, inputs[2], inputs[3], None], limbs, state, outs, B, N, J, 1, T) == 0
    spec = Spec(N, J, T, limbs, **LEARN_PRM)
    spec.len[:], spec.var[:], spec.cnt[:] = 7.0, 2.0, 1                                        # the buffers' initial content
    want = spec.update(poses, ids, slots)
    assert_outputs(outs, want, "frame_set, joint_conf NULL", NAMES[:3])
    assert all(same(state[k], v) for k, v in enumerate(spec.state().values()))
    target = outs[0]
    fitted, resid = torch.full((B, N, J, 5), 77.0, device=dev), torch.full((B, N, L), 77.0, device=dev)
    assert raw_fit(lib, dev, inputs[0], inputs[2], inputs[4], target, limbs, fitted, resid, B, N, J) == 0
    full = Spec(N, J, T, limbs, **FIT_PRM).fit(poses, want[0], ids, conf)
    assert_outputs((fitted, resid), full, "fit", NAMES[3:])
    f2 = torch.full((B, N, J, 5), 77.0, device=dev)
    assert raw_fit(lib, dev, inputs[0], inputs[2], inputs[4], target, limbs, f2, None, B, N, J) == 0 and same(f2, fitted)
    f3, r3 = torch.full((B, N, J, 5), 77.0, device=dev), torch.full((B, N, L), 77.0, device=dev)
    assert raw_fit(lib, dev, inputs[0], None, None, target, limbs, f3, r3, B, N, J) == 0
    assert_outputs((f3, r3), Spec(N, J, T, limbs, **FIT_PRM).fit(poses, want[0]), "fit, ids and joint_conf NULL", NAMES[3:])
    inplace = inputs[0].clone()
    assert raw_fit(lib, dev, inplace, inputs[2], inputs[4], target, limbs, inplace, resid, B, N, J) == 0 and same(inplace, fitted)
    # learn: 0 fused_poses, 2 ids, 3 slots, 5 limbs, 6..10 state, 11..13 outputs
    for null in (0, 2, 3, 5, 6, 7, 8, 9, 10, 11, 12, 13):
        state, outs = buffers()
        keep = [t.clone() for t in state + outs]
        args = list(inputs) + [limbs] + list(state) + list(outs)
        args[null] = None
        assert raw_learn(lib, dev, args[:5], args[5], args[6:11], args[11:], B, N, J, 1, T, L=L) == EINVAL, null
        assert all(same(a, b) for a, b in zip(state + outs, keep)), "an error return wrote something"
    for null in ("poses", "target", "limbs", "fitted"):
        a = dict(poses=inputs[0], target=target, limbs=limbs, fitted=torch.full((B, N, J, 5), 77.0, device=dev))
        out = a["fitted"]
        a[null] = None
        r = torch.full((B, N, L), 77.0, device=dev)
        assert raw_fit(lib, dev, a["poses"], inputs[2], inputs[4], a["target"], a["limbs"], a["fitted"], r, B, N, J, L=L) == EINVAL
        assert (_np(out) == 77).all() and (_np(r) == 77).all()


def case_argument_limits(lib, dev):
    """Every limit and every parameter error, NaN included, of both exports, with nothing written; then the edges that pass."""
    inputs, buffers, limbs, B, J, T = _raw_setup(dev)
    L = len(limbs)
    nan = float("nan")
    big = random_limbs(3, J, 65)
    cases = [(dict(T_=3, T=3), EINVAL), (dict(N_=0), EINVAL), (dict(J=0), EINVAL), (dict(nseq=0), EINVAL), (dict(L=0), EINVAL),
             (dict(T_=65, T=65), ELIMIT), (dict(T_=64, T=64, N_=33), ELIMIT), (dict(J=33), ELIMIT),
             (dict(limbs=big, L_=65), ELIMIT), (dict(limbs=[(0, J)] + limbs[1:]), EINVAL), (dict(limbs=limbs[:-1] + [(-1, 2)]), EINVAL),
             (dict(limbs=limbs[:3] + [(4, 4)] + limbs[4:]), EINVAL), (dict(J=14), EINVAL),
             (dict(min_frames=0), EINVAL), (dict(min_frames=9, window=8), EINVAL), (dict(window=0), EINVAL),
             (dict(relearn=-1), EINVAL), (dict(gate_sigma=-0.5), EINVAL), (dict(gate_sigma=nan), EINVAL),
             (dict(gate_mm=-1.0), EINVAL), (dict(gate_mm=nan), EINVAL)]
    for kw, want in cases:
        kw = dict(kw)
        state, outs = buffers(kw.pop("T_", T), kw.pop("L_", L))
        keep = [t.clone() for t in state + outs]
        a = dict(B=B, N_=N, J=J, nseq=1, T=T)
        lb = kw.pop("limbs", limbs)
        a.update(kw)
        assert raw_learn(lib, dev, inputs, lb, state, outs, **a) == want, kw
        assert all(same(x, y) for x, y in zip(state + outs, keep)), "an error return wrote something"
    target = torch.full((B, N, 65), 200.0, device=dev)
    fcases = [(dict(N_=0), EINVAL), (dict(J=0), EINVAL), (dict(L=0), EINVAL), (dict(N_=33), ELIMIT), (dict(J=33), ELIMIT),
              (dict(limbs=big), ELIMIT), (dict(limbs=[(0, J)] + limbs[1:]), EINVAL), (dict(limbs=[(3, 3)] + limbs[1:]), EINVAL),
              (dict(stiffness=-0.1), EINVAL), (dict(stiffness=1.5), EINVAL), (dict(stiffness=nan), EINVAL),
              (dict(iters=0), EINVAL), (dict(iters=33), EINVAL), (dict(B=-1), EINVAL)]
    for kw, want in fcases:
        kw = dict(kw)
        fitted, resid = torch.full((B, N, J, 5), 77.0, device=dev), torch.full((B, N, 65), 77.0, device=dev)
        a = dict(B=B, N_=N, J=J)
        lb = kw.pop("limbs", limbs)
        a.update(kw)
        assert raw_fit(lib, dev, inputs[0], inputs[2], inputs[4], target, lb, fitted, resid, **a) == want, kw
        assert (_np(fitted) == 77).all() and (_np(resid) == 77).all(), "an error return wrote something"
    # the edges that are fine: gate_sigma = gate_mm = 0, relearn = 0, window == min_frames, stiffness 0 and 1, iters 1 and
    # 32, the largest tables, B = 0 (no launch, nothing written)
    for kw in (dict(gate_sigma=0.0, gate_mm=0.0), dict(relearn=0), dict(min_frames=8, window=8), dict(min_frames=1, window=1)):
        state, outs = buffers()
        assert raw_learn(lib, dev, inputs, limbs, state, outs, B, N, J, 1, T, **kw) == 0
    state, outs = buffers(64, 64)
    lb64 = random_limbs(5, J, 64)
    assert raw_learn(lib, dev, inputs, lb64, state, outs, B, N, J, 1, 64) == 0 and all((_np(o) != 77).all() for o in outs)
    for kw in (dict(stiffness=0.0), dict(stiffness=1.0, iters=1), dict(iters=32)):
        fitted, resid = torch.full((B, N, J, 5), 77.0, device=dev), torch.full((B, N, 64), 77.0, device=dev)
        assert raw_fit(lib, dev, inputs[0], inputs[2], inputs[4], outs[0], lb64, fitted, resid, B, N, J, **kw) == 0
        assert (_np(fitted) != 77).all() and (_np(resid) != 77).all()
    state, outs = buffers()
    assert raw_learn(lib, dev, inputs, limbs, state, outs, 0, N, J, 1, T) == 0 and all((_np(o) == 77).all() for o in outs)
    assert (_np(state[0]) == 7).all()
    fitted = torch.full((B, N, J, 5), 77.0, device=dev)
    assert raw_fit(lib, dev, inputs[0], None, None, target, limbs, fitted, None, 0, N, J) == 0 and (_np(fitted) == 77).all()


# ---- properties: conditions on the definition, asserted on the library ---------------------------------------------------------
PROPERTY = [(15, 100), (15, 200), (15, 300), (17, 400), (17, 500), (17, 600)]                   # J, seed: 4 walkers each


def case_property_walkers(mk_shape, J, seed, B=8):
    """Rigid walkers with 5 mm Gaussian jitter per coordinate at the defaults, frames 40-119, four seeded walkers per case
    (twelve per joint set over the three cases): the mean joint error of fitted to the noiseless truth is at most 0.90 of
    the raw pose's, and the rms error of the fitted limb lengths at most 0.25 of the raw limb lengths'.  (A float64 model
    of the definition gave 0.82 / 0.12 at J = 15 and 0.79 / 0.13 with the cyclic COCO table.)"""
    F, limbs = 120, LIMBS[J]
    truth, noisy = rigid_walkers(seed, N, J, F)
    poses = np.zeros((F, N, J, 5), F32)
    poses[..., :3], poses[..., 4] = noisy, 0.5
    ids = np.tile(np.arange(N, dtype=np.int32), (F, 1))
    slots = np.tile(np.array([2, 0, 3, 1], np.int32), (F, 1))
    (target, _, state, fitted, _), _, _ = run_direct(mk_shape, poses, ids, slots, chunks_of(F, B), limbs, what="property", T=4)
    assert (state[40:] == LEARNED).mean() > 0.98 and (target[40:] > 0).all()
    fit64, raw64, tr = fitted[40:, ..., :3].astype(np.float64), noisy[40:].astype(np.float64), truth[40:]
    err_fit, err_raw = np.linalg.norm(fit64 - tr, axis=-1).mean(), np.linalg.norm(raw64 - tr, axis=-1).mean()

    def lengths(x):
        return np.stack([np.linalg.norm(x[..., k, :] - x[..., i, :], axis=-1) for i, k in limbs], axis=-1)
    rms_fit = np.sqrt(((lengths(fit64) - lengths(tr)) ** 2).mean())
    rms_raw = np.sqrt(((lengths(raw64) - lengths(tr)) ** 2).mean())
    print(f"J = {J} seed {seed}: joint error {err_fit:.3f} / {err_raw:.3f} mm = {err_fit / err_raw:.3f}; limb length rms "
          f"{rms_fit:.3f} / {rms_raw:.3f} mm = {rms_fit / rms_raw:.3f}")
    assert err_fit <= 0.90 * err_raw
    assert rms_fit <= 0.25 * rms_raw


def case_property_occluded_end(mk_shape, J):
    """A limb whose far joint is unsupported and displaced by 150 mm: |resid| below 1 mm after the fit; constrained by that
    limb alone, the supported end keeps its bits."""
    F, limbs = 60, LIMBS[J]
    leaf = [l for l, (i, k) in enumerate(limbs) if sum(k in ab for ab in limbs) == 1][0]
    i, k = limbs[leaf]
    truth, noisy = rigid_walkers(77, 1, J, F)
    noisy = noisy[:, 0].copy()
    noisy[-1, k] += np.array([90.0, -120.0, 0.0], F32)                                          # 150 mm
    poses, ids, slots = _person(noisy)
    conf = np.ones((F, N, J), F32)
    conf[-1, 2, k] = 0.1
    (target, _, state, fitted, resid), _, _ = run_direct(mk_shape, poses, ids, slots, chunks_of(F, 8), limbs, conf,
                                                         what="occluded end", conf_min=0.5)
    assert state[-1, 2, leaf] == NOT_MEASURED and target[-1, 2, leaf] > 0
    moved = np.linalg.norm(fitted[-1, 2, k, :3].astype(np.float64) - poses[-1, 2, k, :3])
    print(f"occluded end: resid {resid[-1, 2, leaf]:.2e} mm, the joint moved {moved:.1f} mm")
    assert abs(resid[-1, 2, leaf]) < 1.0 and moved > 50.0
    only = np.zeros_like(target[-1:])
    only[0, 2, leaf] = target[-1, 2, leaf]
    f1, r1 = fit_direct(mk_shape, poses[-1:], only, limbs, conf=conf[-1:], what="that limb alone", conf_min=0.5)
    others = [j for j in range(J) if j != k]
    assert same(f1[0, 2, others], poses[-1, 2, others]) and not same(f1[0, 2, k], poses[-1, 2, k]) and abs(r1[0, 2, leaf]) < 1.0


# ---- behind the forward ---------------------------------------------------------------------------------------------------
def case_behind_forward(model, lm, spec, heats, meta, cams, rt, smoother):
    """A model with tracker and evidence (and a smoother) set: update on fused_poses with joint_conf = last_evidence[1], fit
    on fused_poses or on last_smooth[0]; every output and the state against the yardstick after every forward.  The first two
    inputs are the same, so every limb seen has two samples after the second."""
    constrained = 0
    with torch.no_grad():
        for x in heats:
            out = model(meta=meta, input_heatmaps=x, cameras=cams, resize_transform=rt)
            ids, slots, _ = model.last_tracks
            conf = model.last_evidence[1]
            if smoother:
                poses = model.last_smooth[0]
                target, obs, state = lm.update(out[0], ids, slots, joint_conf=conf, meta=meta)
                fitted, resid = lm.fit(poses, target, ids, conf)
            else:
                poses = out[0]
                fitted, target, state, resid = lm(out[0], ids, slots, joint_conf=conf, meta=meta)
            fs = _np(model.tracker.frame_sets(meta["seq"]))
            want = spec.update(_np(out[0]), _np(ids), _np(slots), _np(conf), fs)
            wfit = spec.fit(_np(poses), want[0], _np(ids), _np(conf))
            if smoother:
                assert_outputs((target, obs, state, fitted, resid), want + wfit, "behind the forward")
            else:
                assert_outputs((target, state, fitted, resid), (want[0], want[2]) + wfit, "behind the forward",
                               ("target", "limb_state", "fitted", "resid"))
            assert_state(lm, spec, "behind the forward")
            valid = _np(ids) >= 0
            assert valid.any() and same(_np(fitted)[~valid], _np(poses)[~valid])
            constrained += int((_np(target) > 0).sum())
    assert constrained > 0 and (_np(lm.state()["limb_cnt"]) >= 2).any()
