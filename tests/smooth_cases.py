"""Shared by tests/test_smooth_emu.py (CPU emulator) and tests/test_smooth_gpu.py (the shipped library on the card): the
yardstick of fvp_track_smooth - an independent fp32 numpy restatement of the definition in include/fvp.h (np.float32
scalars, np.sqrt, plain Python loops; no code shared with the product) - seeded scenarios, and the case bodies both files
run.  Everything is compared bit for bit: smooth, track_poses, track_state viewed as int32, and the four state arrays after
every call.  No tolerance appears anywhere; the three property cases assert the bounds the definition was chosen for."""
import ctypes as C

import numpy as np
import torch

import track_cases as TC
from track_cases import EINVAL, ELIMIT, F32, _np, at, bits, chunks_of, pack, same, walks

FLT_MAX = np.finfo(F32).max
DEFAULTS = dict(rate_hz=30.0, min_cutoff=1.0, beta=0.005, d_cutoff=1.0, conf_min=0.0, damp=0.8)


# ---- the yardstick -----------------------------------------------------------------------------------------------
class Spec:
    def __init__(self, N, J, T, nseq=1, max_age=15, **kw):
        p = dict(DEFAULTS, **kw)
        self.N, self.J, self.T, self.nseq, self.max_age = N, J, T, nseq, int(max_age)
        self.rate, self.min_cutoff, self.beta = F32(p["rate_hz"]), F32(p["min_cutoff"]), F32(p["beta"])
        self.d_cutoff, self.conf_min, self.damp = F32(p["d_cutoff"]), F32(p["conf_min"]), F32(p["damp"])
        self.pose = np.zeros((nseq, T, J, 3), F32)
        self.vel = np.zeros((nseq, T, J, 3), F32)
        self.id = np.full((nseq, T), -1, np.int32)
        self.age = np.zeros((nseq, T), np.int32)

    def alpha(self, fc):
        r = (F32(6.2831855) * fc) / self.rate
        a = r / (r + F32(1.0))
        assert a.dtype == F32
        return a

    def predicted(self, x, v):
        dt = F32(1.0) / self.rate
        for c in range(3):
            v[c] = v[c] * self.damp
            x[c] = x[c] + v[c] * dt

    def joint(self, x, v, m, conf):
        """One joint of a slot that keeps its id: state x, v [3] updated in place from the measurement m [3]; the flag."""
        e = [m[c] - x[c] for c in range(3)]
        measured = (conf is None or conf >= self.conf_min) and all(np.abs(e[c]) <= FLT_MAX for c in range(3))
        if not measured:
            self.predicted(x, v)
            return F32(0.0)
        a_d = self.alpha(self.d_cutoff)
        for c in range(3):
            vc = e[c] * self.rate
            v[c] = v[c] + a_d * (vc - v[c])
        sp = np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
        a = self.alpha(self.min_cutoff + self.beta * sp)
        for c in range(3):
            x[c] = x[c] + a * e[c]
        return F32(1.0)

    def update(self, poses, ids, slots, conf=None, frame_set=None):
        poses = np.asarray(poses, F32)
        B, N, J, T = poses.shape[0], self.N, self.J, self.T
        smooth = poses.copy()
        track_poses = np.zeros((B, T, J, 4), F32)
        track_state = np.zeros((B, T, 2), np.int32)
        track_state[:, :, 0] = -1
        with np.errstate(all="ignore"):
            for b in range(B):
                s = 0 if frame_set is None else int(frame_set[b])
                if not 0 <= s < self.nseq:
                    continue
                ok = [n for n in range(N) if ids[b, n] >= 0 and 0 <= slots[b, n] < T]
                for t in range(T):
                    here = [n for n in ok if slots[b, n] == t]
                    flags = np.zeros((J,), F32)
                    x, v = self.pose[s, t], self.vel[s, t]
                    if here:
                        n = here[0]
                        self.age[s, t] = 0
                        if self.id[s, t] != ids[b, n]:
                            self.id[s, t] = ids[b, n]
                            x[:] = poses[b, n, :, :3]
                            v[:] = 0
                            flags[:] = 1
                        else:
                            for j in range(J):
                                flags[j] = self.joint(x[j], v[j], poses[b, n, j, :3], None if conf is None else conf[b, n, j])
                    elif self.id[s, t] >= 0:
                        self.age[s, t] += 1
                        if self.age[s, t] > self.max_age:
                            self.id[s, t], self.age[s, t] = -1, 0
                        else:
                            for j in range(J):
                                self.predicted(x[j], v[j])
                    if self.id[s, t] >= 0:
                        track_poses[b, t, :, :3] = x
                        track_poses[b, t, :, 3] = flags
                    track_state[b, t] = (self.id[s, t], self.age[s, t])
                    for n in here:
                        smooth[b, n, :, :3] = x
        return smooth, track_poses, track_state

    def state(self):
        return dict(flt_pose=self.pose, flt_vel=self.vel, flt_id=self.id, flt_age=self.age)


# ---- comparisons -----------------------------------------------------------------------------------------------------
NAMES = ("smooth", "track_poses", "track_state")


def assert_outputs(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        g, w = _np(g), _np(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape)
        bad = np.argwhere(bits(g) != bits(w))
        assert bad.size == 0, f"{what}: {name} differs at {len(bad)} elements, first {tuple(bad[0])}: " \
                              f"{g[tuple(bad[0])]!r} vs {w[tuple(bad[0])]!r}"


def assert_state(sm, spec, what):
    got = sm.state()
    for k, w in spec.state().items():
        g = _np(got[k])
        bad = np.argwhere(bits(g) != bits(w))
        assert g.shape == w.shape and bad.size == 0, f"{what}: state {k} differs at {len(bad)} elements, first " \
                                                     f"{tuple(bad[0])}: {g[tuple(bad[0])]!r} vs {w[tuple(bad[0])]!r}"


def assert_mirror(sm, tracker, what):
    """flt_id == trk_id everywhere; flt_age == trk_age in every live slot, 0 in a free one (include/fvp.h)."""
    fid, fage = _np(sm.state()["flt_id"]), _np(sm.state()["flt_age"])
    tid, tage = _np(tracker.state()["trk_id"]), _np(tracker.state()["trk_age"])
    assert np.array_equal(fid, tid), (what, fid.tolist(), tid.tolist())
    assert np.array_equal(fage[tid >= 0], tage[tid >= 0]) and (fage[tid < 0] == 0).all(), (what, fage.tolist(), tage.tolist())


# ---- runners ----------------------------------------------------------------------------------------------------------
def run(mk, poses, chunks, conf=None, frame_set=None, what="", nseq=1, T=None, max_age=15, **kw):
    """``poses`` [F,N,J,5] through a fresh PoseTracker and a PoseSmoother built from it (``mk(N, J, nseq, T, max_age, **kw)``
    -> (tracker, smoother)) in calls of the given sizes.  After EVERY call the three outputs and the whole state equal the
    yardstick's (fed the tracker's ids / slots) and the smoother's id / age mirror the tracker's.  Returns the concatenated
    outputs, ids, slots (numpy) and the pair."""
    F, N, J = poses.shape[:3]
    T = 2 * N if T is None else T
    assert sum(chunks) == F
    tracker, sm = mk(N, J, nseq, T, max_age, **kw)
    spec = Spec(N, J, T, nseq, max_age, **kw)
    dev = sm.device
    outs, f = [], 0
    for c in chunks:
        x = torch.from_numpy(np.ascontiguousarray(poses[f:f + c])).to(dev)
        fs = None if frame_set is None else np.asarray(frame_set[f:f + c], np.int32)
        seqs = None if fs is None else torch.from_numpy(fs).to(dev)
        cf = None if conf is None else np.ascontiguousarray(conf[f:f + c])
        ids, slots, _ = tracker.update(x, sequences=seqs)
        got = sm.update(x, ids, slots, joint_conf=None if cf is None else torch.from_numpy(cf).to(dev), sequences=seqs)
        want = spec.update(poses[f:f + c], _np(ids), _np(slots), cf, fs)
        assert_outputs(got, want, f"{what} frames {f}..{f + c - 1}")
        assert_state(sm, spec, f"{what} after frame {f + c - 1}")
        assert_mirror(sm, tracker, f"{what} after frame {f + c - 1}")
        outs.append([_np(g).copy() for g in got] + [_np(ids).copy(), _np(slots).copy()])
        f += c
    return [np.concatenate([o[k] for o in outs]) for k in range(5)], (tracker, sm)


def run_direct(mk_shape, poses, ids, slots, chunks, conf=None, what="", T=None, max_age=15, **kw):
    """As ``run`` with hand-made ids / slots and a smoother built from the shape (no tracker)."""
    F, N, J = poses.shape[:3]
    T = 2 * N if T is None else T
    sm = mk_shape(N, J, T, 1, max_age=max_age, **kw)
    spec = Spec(N, J, T, 1, max_age, **kw)
    dev = sm.device
    ids, slots = np.asarray(ids, np.int32), np.asarray(slots, np.int32)
    outs, f = [], 0
    for c in chunks:
        sl = slice(f, f + c)
        cf = None if conf is None else np.ascontiguousarray(conf[sl])
        got = sm.update(torch.from_numpy(np.ascontiguousarray(poses[sl])).to(dev),
                        torch.from_numpy(np.ascontiguousarray(ids[sl])).to(dev),
                        torch.from_numpy(np.ascontiguousarray(slots[sl])).to(dev),
                        joint_conf=None if cf is None else torch.from_numpy(cf).to(dev))
        want = spec.update(poses[sl], ids[sl], slots[sl], cf)
        assert_outputs(got, want, f"{what} frames {f}..{f + c - 1}")
        assert_state(sm, spec, f"{what} after frame {f + c - 1}")
        outs.append([_np(g).copy() for g in got])
        f += c
    return [np.concatenate([o[k] for o in outs]) for k in range(3)], sm


# ---- the cases (each takes the factories of its file) ----------------------------------------------------------------------
N = 4
WALKERS = [(15, 4, 1), (17, 8, 3), (15, 8, 8), (17, 4, 8)]                                      # J, T, B


def _scene(J, F=9, seed=71, P=3, present=None):
    people = walks(seed, P, J, F)
    present = np.ones((F, P), bool) if present is None else present
    poses, slot_of = pack(seed + 1, people, present, N)
    conf = np.random.default_rng(seed + 2).uniform(0.0, 1.0, size=(F, N, J)).astype(F32)
    return people, poses, slot_of, conf


def case_walkers(mk, J, T, B):
    """Noisy walkers, slots permuted per frame, a third of the joints below conf_min in every frame."""
    F = 9
    people, poses, slot_of, conf = _scene(J, F, seed=71 + J + B)
    (smooth, tp, ts, ids, slots), _ = run(mk, poses, chunks_of(F, B), conf, what="walkers", T=T, conf_min=0.33)
    assert (slot_of[0] != slot_of[1]).any()
    # a slot's first frame equals the detection, every joint flagged as measured
    for p in range(3):
        n = slot_of[0, p]
        assert same(smooth[0, n], poses[0, n]) and same(tp[0, slots[0, n], :, :3], poses[0, n, :, :3])
        assert (tp[0, slots[0, n], :, 3] == 1).all()
    # person-stable rows: a person's row of track_poses never moves, and smooth carries that row in the person's slot
    for f in range(F):
        for p in range(3):
            n = slot_of[f, p]
            assert slots[f, n] == slots[0, slot_of[0, p]]
            assert same(smooth[f, n, :, :3], tp[f, slots[f, n], :, :3]) and same(smooth[f, n, :, 3:], poses[f, n, :, 3:])
        inv = ids[f] < 0
        assert inv.sum() == 1 and same(smooth[f][inv], poses[f][inv])
        flags = tp[f, slots[f][~inv], :, 3]
        if f:
            assert same(flags, (conf[f][~inv] >= F32(0.33)).astype(F32)) and 0 < flags.mean() < 1
    assert (ts[:, :, 0] >= 0).sum() == 3 * F and (tp[ts[:, :, 0] < 0] == 0).all()


def case_constant(mk, J, B):
    """A constant pose comes back with the input's bits every frame (e = 0: the velocity stays 0, x + a * 0 = x)."""
    F = 8
    people = np.repeat(walks(5, 3, J, 1), F, axis=0)
    poses, slot_of = pack(6, people, np.ones((F, 3), bool), N)
    (smooth, tp, _, ids, slots), (_, sm) = run(mk, poses, chunks_of(F, B), what="constant", T=8)
    assert same(smooth, poses)
    assert (_np(sm.state()["flt_vel"]) == 0).all() and (tp[:, :, :, 3][tp[:, :, :, 3] != 0] == 1).all()
    for f in range(F):
        for p in range(3):
            assert same(tp[f, slots[f, slot_of[f, p]], :, :3], people[0, p])


def case_conf_edge(mk_shape, J):
    """conf == conf_min is measured, nextafter below it is predicted, NaN is predicted; joint_conf = None: all measured."""
    cm = F32(0.4)
    below = np.nextafter(cm, F32(0))
    assert below < cm
    rng = np.random.default_rng(9)
    poses = np.stack([at({1: (100.0 * f, 50.0, 900.0)}, N, J, TC.skeleton(rng, J)) for f in range(3)])
    ids = np.full((3, N), -1, np.int32)
    slots = np.full((3, N), -1, np.int32)
    ids[:, 1], slots[:, 1] = 7, 2
    conf = np.ones((3, N, J), F32)
    conf[1:, 1, 0], conf[1:, 1, 1], conf[1:, 1, 2], conf[1:, 1, 3] = cm, below, np.nan, 0.0
    (_, tp, _), _ = run_direct(mk_shape, poses, ids, slots, [1, 2], conf, what="conf edge", conf_min=float(cm))
    assert tp[0, 2, :, 3].tolist() == [1.0] * J                                                # the first frame: initialised
    for f in (1, 2):
        assert tp[f, 2, :4, 3].tolist() == [1.0, 0.0, 0.0, 0.0] and (tp[f, 2, 4:, 3] == 1).all()
    (_, tp, _), _ = run_direct(mk_shape, poses, ids, slots, [3], None, what="no joint_conf", conf_min=float(cm))
    assert (tp[:, 2, :, 3] == 1).all()


def case_nonfinite_joint(mk_shape, J):
    """Same id, one joint NaN, one Inf, one whose error overflows: each is predicted, stays finite, touches no other."""
    rng = np.random.default_rng(10)
    sk = TC.skeleton(rng, J)
    poses = np.stack([at({0: (20.0 * f, 0.0, 900.0), 3: (3000.0, 10.0 * f, 900.0)}, N, J, sk) for f in range(4)])
    poses[:, 0, 5, 0] = F32(3.0e38)
    poses[2, 0, 3, 1] = np.nan
    poses[2, 0, 4, 2] = np.inf
    poses[2, 0, 5, 0] = F32(-3.0e38)                                                           # e = -inf, the inputs finite
    ids = np.full((4, N), -1, np.int32)
    slots = np.full((4, N), -1, np.int32)
    ids[:, 0], slots[:, 0], ids[:, 3], slots[:, 3] = 0, 1, 1, 0
    (smooth, tp, _), sm = run_direct(mk_shape, poses, ids, slots, [2, 1, 1], what="NaN / Inf joint")
    assert tp[2, 1, 3:6, 3].tolist() == [0.0, 0.0, 0.0] and (np.delete(tp[2, 1, :, 3], [3, 4, 5]) == 1).all()
    assert np.isfinite(tp).all() and np.isfinite(smooth[..., :3]).all()
    assert (tp[3, :2, :, 3] == 1).all() and np.isfinite(_np(sm.state()["flt_vel"])).all()


def case_nan_born(mk, J):
    """The tracker's own NaN case: a detection with a NaN joint is born, never matched; the person's own track ages a frame
    and takes the person back in the next one.  The NaN-born track coasts as NaN in that one coordinate, poisons nothing."""
    F = 5
    people, poses, slot_of, _ = _scene(J, F, seed=91)
    n = slot_of[2, 1]
    poses[2, n, J // 2, 1] = np.nan
    (smooth, tp, ts, ids, slots), _ = run(mk, poses, [2, 3], what="NaN-born track", T=8)
    t = slots[2, n]
    own = slots[1, slot_of[1, 1]]
    assert ids[2, n] == 3 and t != own and ids[3, slot_of[3, 1]] == ids[1, slot_of[1, 1]] and slots[3, slot_of[3, 1]] == own
    assert ts[2, own, 1] == 1 and (tp[2, own, :, 3] == 0).all() and (tp[3, own, :, 3] == 1).all()
    for f in (2, 3, 4):
        nan = np.isnan(tp[f])
        assert nan.sum() == 1 and nan[t, J // 2, 1] and ts[f, t].tolist() == [3, f - 2]
    assert np.isnan(smooth).sum() == 1 and np.isnan(smooth[2, n, J // 2, 1])


def case_gaps(mk, J, B):
    """max_age = 3.  A is missing for 3 frames: it coasts (flag 0, velocity * damp per frame) and comes back as itself.  B is
    missing for 4: freed in the 4th, where newcomer C takes the slot at once with a reinitialised filter."""
    F, max_age = 8, 3
    present = np.ones((F, 4), bool)
    present[1:4, 0] = False                                                                    # A: frames 1-3
    present[1:5, 1] = False                                                                    # B: frames 1-4
    present[:4, 3] = False                                                                     # C: from frame 4
    people, poses, slot_of, _ = _scene(J, F, seed=21 + J, P=4, present=present)
    (smooth, tp, ts, ids, slots), _ = run(mk, poses, chunks_of(F, B), what="gaps", T=8, max_age=max_age)
    ta, tb = slots[0, slot_of[0, 0]], slots[0, slot_of[0, 1]]
    for f in (1, 2, 3):
        assert ts[f, ta].tolist() == [ids[0, slot_of[0, 0]], f] and (tp[f, ta, :, 3] == 0).all()
        assert ts[f, tb].tolist() == [ids[0, slot_of[0, 1]], f] and (tp[f, tb, :, 3] == 0).all()
        assert same(tp[f, ta, :, :3], tp[0, ta, :, :3])                                        # born with v = 0: coasting stands still
    assert ts[4, ta].tolist() == [ids[0, slot_of[0, 0]], 0] and (tp[4, ta, :, 3] == 1).all()   # A is back as itself
    nc = slot_of[4, 3]
    assert slots[4, nc] == tb and ts[4, tb].tolist() == [ids[4, nc], 0] and ids[4, nc] != ids[0, slot_of[0, 1]]
    assert same(tp[4, tb, :, :3], poses[4, nc, :, :3]) and (tp[4, tb, :, 3] == 1).all()        # reinitialised, same frame


def case_coasting_velocity(mk, J):
    """A moving person drops out for max_age frames and for max_age + 1: each coasting frame multiplies the velocity by damp
    and moves the pose by v * dt; one frame later the slot is free - (-1, 0), four zeros."""
    max_age, damp, rate = 2, F32(0.8), F32(30.0)
    for gap in (max_age, max_age + 1):
        F = 4 + gap + 1
        sk = TC.skeleton(np.random.default_rng(12), J)
        present = [f < 4 or f == F - 1 for f in range(F)]
        poses = np.stack([at({1: (40.0 * f, 10.0 * f, 900.0)} if present[f] else {}, N, J, sk) for f in range(F)])
        tr, sm = mk(N, J, 1, 4, max_age)
        spec = Spec(N, J, 4, 1, max_age)
        vel = None
        for f in range(F):
            x = torch.from_numpy(poses[f:f + 1].copy()).to(sm.device)
            ids, slots, _ = tr.update(x)
            got = sm.update(x, ids, slots)
            assert_outputs(got, spec.update(poses[f:f + 1], _np(ids), _np(slots)), f"coast {gap} frame {f}")
            assert_state(sm, spec, f"coast {gap} frame {f}")
            assert_mirror(sm, tr, f"coast {gap} frame {f}")
            tp, ts = _np(got[1])[0], _np(got[2])[0]
            v, p = _np(sm.state()["flt_vel"])[0, 0].copy(), _np(sm.state()["flt_pose"])[0, 0].copy()
            if 4 <= f < 4 + min(gap, max_age):
                assert same(v, vel * damp) and same(p, pose + v * (F32(1.0) / rate)) and (np.abs(v) > 0).any()
                assert (tp[0, :, 3] == 0).all() and same(tp[0, :, :3], p) and ts[0].tolist() == [0, f - 3]
            if gap > max_age and f == 4 + max_age:
                assert ts[0].tolist() == [-1, 0] and (tp[0] == 0).all()
            vel, pose = v, p
        last = _np(got[2])[0, 0].tolist()
        assert last == ([0, 0] if gap == max_age else [1, 0])                                  # itself / a new identity
        if gap > max_age:
            assert same(_np(got[1])[0, 0, :, :3], poses[-1, 1, :, :3]) and (v == 0).all()      # the filter starts over


def case_full_table(mk, J):
    """N = T = 4: a birth into a full table evicts a track; the slot's filter starts over from the detection."""
    def pt(k):
        return (3000.0 * k, 0.0, 0.0)
    frames = [{0: pt(0), 1: pt(1), 2: pt(2), 3: pt(3)}, {0: pt(0), 1: pt(1), 2: pt(4), 3: pt(5)},
              {0: pt(0), 1: pt(4), 2: pt(6), 3: pt(7)}, {0: pt(6), 1: pt(8)}, {0: pt(6), 1: pt(9), 2: pt(10)}]
    poses = np.stack([at(fr, N, J) for fr in frames])
    (smooth, tp, ts, ids, slots), _ = run(mk, poses, [2, 3], what="full table", T=4)
    assert slots[2].tolist() == [0, 2, 1, 3] and ids[2].tolist() == [0, 4, 6, 7]               # (the tracker's own case)
    assert ts[1, :, 0].tolist() == [0, 1, 4, 5] and ts[2, :, 0].tolist() == [0, 6, 4, 7]
    for f, n in ((1, 2), (1, 3), (2, 2), (2, 3), (3, 1), (4, 1), (4, 2)):                      # the evictions
        assert same(tp[f, slots[f, n], :, :3], poses[f, n, :, :3]) and (tp[f, slots[f, n], :, 3] == 1).all()
    assert same(smooth, poses)                                                                 # nobody moves in this scenario


def _mixed(J, F=8, seed=41):
    present = np.ones((F, 4), bool)
    present[2:4, 1] = False
    present[3, 2] = False
    present[:2, 3] = False
    return _scene(J, F, seed, P=4, present=present)


def case_chunk_invariance(mk, J):
    _, poses, _, conf = _mixed(J)
    runs = [run(mk, poses, ch, conf, what=f"chunks {ch}", T=8, max_age=1, conf_min=0.25) for ch in ([8], [3, 5], [1] * 8)]
    for out, (_, sm) in runs[1:]:
        for x, y in zip(out, runs[0][0]):
            assert same(x, y)
        for k, v in sm.state().items():
            assert same(v, runs[0][1][1].state()[k])


def case_two_sequences(mk, J):
    (_, a, _, ca), (_, b, _, cb) = _mixed(J, 4, seed=51), _mixed(J, 4, seed=61)
    frame_set = [0, 1, 1, 0, 1, 0, 0, 1]
    fs = np.asarray(frame_set)
    poses, conf = np.empty((8,) + a.shape[1:], F32), np.empty((8,) + ca.shape[1:], F32)
    poses[fs == 0], poses[fs == 1], conf[fs == 0], conf[fs == 1] = a, b, ca, cb
    out, (_, sm) = run(mk, poses, [8], conf, frame_set, what="two sequences", nseq=2, T=8, conf_min=0.25)
    for s, own, cown in ((0, a, ca), (1, b, cb)):
        out1, (_, sm1) = run(mk, own, [4], cown, what=f"sequence {s} alone", T=8, conf_min=0.25)
        for x, y in zip(out, out1):
            assert same(x[fs == s], y)
        for k, v in sm1.state().items():
            assert same(_np(sm.state()[k])[s], _np(v)[0])
    # a frame of no sequence (row 2 of two): written as invalid - smooth is the input, track rows are free - no state changes
    fs2 = list(frame_set)
    fs2[3] = 2
    (smooth, tp, ts, ids, _), _ = run(mk, poses, [8], conf, fs2, what="a frame of no sequence", nseq=2, T=8, conf_min=0.25)
    assert (ids[3] == -1).all() and same(smooth[3], poses[3]) and (tp[3] == 0).all()
    assert (ts[3, :, 0] == -1).all() and (ts[3, :, 1] == 0).all() and (ts[4, :, 0] >= 0).any()


# ---- the C entry point itself -----------------------------------------------------------------------------------------------
PARAMS = (30.0, 1.0, 0.005, 1.0, 0.0, 0.8)


def raw_call(lib, dev, inputs, state, outs, B, N_, J, nseq, T, params=PARAMS, max_age=15):
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream) if torch.device(dev).type == "cuda" else None
    p = [None if t is None else C.c_void_p(t.data_ptr()) for t in tuple(inputs) + tuple(state) + tuple(outs)]
    return lib.fvp_track_smooth(*p, B, N_, J, nseq, T, *params, max_age, stream)


def _raw_setup(dev, J=15, T=8, B=3):
    _, poses, _, conf = _mixed(J)
    poses, conf = np.ascontiguousarray(poses[:B]), np.ascontiguousarray(conf[:B])
    ids = np.full((B, N), -1, np.int32)
    slots = np.full((B, N), -1, np.int32)
    for b in range(B):
        for k, n in enumerate(np.flatnonzero(poses[b, :, 0, 3] >= 0)):
            ids[b, n], slots[b, n] = 10 + k, (k + 1) % T
    inputs = [torch.from_numpy(a).to(dev) for a in (poses, np.zeros((B,), np.int32), ids, slots, conf)]

    def buffers(T_=T):
        state = (torch.full((1, T_, J, 3), 7.0, device=dev), torch.full((1, T_, J, 3), 2.0, device=dev),
                 torch.full((1, T_), -1, dtype=torch.int32, device=dev), torch.full((1, T_), 0, dtype=torch.int32, device=dev))
        outs = (torch.full((B, N, J, 5), 77.0, device=dev), torch.full((B, T_, J, 4), 77.0, device=dev),
                torch.full((B, T_, 2), 77, dtype=torch.int32, device=dev))
        return state, outs
    return inputs, buffers, B, J, T


def case_null_outputs(lib, dev):
    """Every NULL-output combination: what is written equals the full call's, the state moves the same way; all three NULL
    is an error; frame_set and joint_conf may be NULL."""
    inputs, buffers, B, J, T = _raw_setup(dev)
    state0, full = buffers()
    assert raw_call(lib, dev, inputs, state0, full, B, N, J, 1, T) == 0
    assert all((_np(o) != 77).all() for o in full)
    for mask in range(8):
        state, outs = buffers()
        outs = tuple(o if mask >> k & 1 else None for k, o in enumerate(outs))
        rc = raw_call(lib, dev, inputs, state, outs, B, N, J, 1, T)
        if mask == 0:
            assert rc == EINVAL and all(same(a, b) for a, b in zip(state, buffers()[0]))
            continue
        assert rc == 0, mask
        for o, w in zip(outs, full):
            assert o is None or same(o, w), mask
        assert all(same(a, b) for a, b in zip(state, state0)), mask
    state, outs = buffers()
    assert raw_call(lib, dev, [inputs[0], None, inputs[2], inputs[3], None], state, outs, B, N, J, 1, T) == 0
    spec = Spec(N, J, T)
    spec.pose[:], spec.vel[:] = 7.0, 2.0
    assert_outputs(outs, spec.update(_np(inputs[0]), _np(inputs[2]), _np(inputs[3])), "frame_set, joint_conf NULL")


def case_argument_limits(lib, dev):
    inputs, buffers, B, J, T = _raw_setup(dev)
    nan = float("nan")

    def with_param(k, v):
        p = list(PARAMS)
        p[k] = v
        return dict(params=tuple(p))
    cases = [(dict(T_=3, T=3), EINVAL), (dict(N_=0), EINVAL), (dict(J=0), EINVAL), (dict(nseq=0), EINVAL),
             (dict(max_age=-1), EINVAL), (dict(T_=65, T=65), ELIMIT), (dict(T_=64, T=64, N_=33), ELIMIT), (dict(J=33), ELIMIT)]
    # rate_hz, min_cutoff, d_cutoff not > 0; beta not >= 0; damp outside [0, 1]; NaN anywhere
    for k, bad in ((0, (0.0, -30.0, nan)), (1, (0.0, -1.0, nan)), (3, (0.0, -1.0, nan)), (2, (-0.001, nan)),
                   (5, (-0.1, 1.5, nan))):
        cases += [(with_param(k, v), EINVAL) for v in bad]
    for null in (0, 2, 3, 5, 6, 7, 8):                                                          # a null required pointer
        cases.append((dict(null=null), EINVAL))
    for kw, want in cases:
        kw = dict(kw)
        state, outs = buffers(kw.pop("T_", T))
        keep = [t.clone() for t in state + outs]
        args = list(inputs) + list(state)
        null = kw.pop("null", None)
        if null is not None:
            args[null] = None
        a = dict(B=B, N_=N, J=J, nseq=1, T=T)
        a.update(kw)
        assert raw_call(lib, dev, args[:5], args[5:], outs, **a) == want, (kw, null)
        for t, k2 in zip(state + outs, keep):
            assert same(t, k2), "an error return wrote something"
    # the edges that are fine: beta = 0, damp = 0 and 1, the largest table, B = 0 (no launch, nothing written)
    for kw in (with_param(2, 0.0), with_param(5, 0.0), with_param(5, 1.0)):
        state, outs = buffers()
        assert raw_call(lib, dev, inputs, state, outs, B, N, J, 1, T, **kw) == 0
    state, outs = buffers(64)
    assert raw_call(lib, dev, inputs, state, outs, B, N, J, 1, 64) == 0 and all((_np(o) != 77).all() for o in outs)
    state, outs = buffers()
    assert raw_call(lib, dev, inputs, state, outs, 0, N, J, 1, T) == 0 and all((_np(o) == 77).all() for o in outs)


# ---- properties: conditions on the definition, asserted on the library ---------------------------------------------------------
def _single(mk_shape, track, B=8):
    """track [F,J,3] as one person in detection slot 2 / track slot 1 at the defaults -> the filtered [F,J,3]."""
    F, J = track.shape[:2]
    poses = np.zeros((F, N, J, 5), F32)
    poses[:, :, :, 3] = -1.0
    poses[:, 2, :, :3], poses[:, 2, :, 3] = track, 0.0
    ids = np.full((F, N), -1, np.int32)
    slots = np.full((F, N), -1, np.int32)
    ids[:, 2], slots[:, 2] = 0, 1
    (smooth, tp, _), _ = run_direct(mk_shape, poses, ids, slots, chunks_of(F, B), what="property")
    assert same(smooth[:, 2, :, :3], tp[:, 1, :, :3])
    return smooth[:, 2, :, :3].astype(np.float64)


def case_property_jitter(mk_shape):
    """A stationary joint with 5 mm Gaussian noise at 30 Hz: after 50 frames the frame-to-frame RMS of the output is at most
    a quarter of the input's (the numpy restatement gave 0.16-0.17 over five seeds).  15 joints = 15 independent samples."""
    rng = np.random.default_rng(3)
    track = (np.array([500.0, -200.0, 900.0]) + rng.normal(0.0, 5.0, size=(120, 15, 3))).astype(F32)
    out = _single(mk_shape, track)
    rms_in = np.sqrt((np.diff(track[50:].astype(np.float64), axis=0) ** 2).mean())
    rms_out = np.sqrt((np.diff(out[50:], axis=0) ** 2).mean())
    print(f"jitter: input {rms_in:.3f} mm, output {rms_out:.3f} mm, ratio {rms_out / rms_in:.3f}")
    assert rms_out <= 0.25 * rms_in


def case_property_lag(mk_shape):
    """A joint moving at 1000 mm/s: the settled lag is at most 25 mm (the numpy restatement gave 18.2 mm)."""
    F = 120
    track = np.zeros((F, 15, 3), F32)
    track[:, :, 0] = (np.arange(F, dtype=np.float64) * (1000.0 / 30.0))[:, None]
    track[:, :, 2] = 900.0
    out = _single(mk_shape, track)
    lag = np.abs(out[60:, :, 0] - track[60:, :, 0].astype(np.float64)).max()
    print(f"lag at 1000 mm/s: {lag:.2f} mm")
    assert lag <= 25.0


def case_property_step(mk_shape):
    """A 300 mm step: within 5 mm three frames after the step, and from then on.  The definition gives 105.6, 33.7, 11.3 and
    4.1 mm in the step's frame and the three after it (the same figures in float64 by hand)."""
    F, k = 40, 24
    track = np.zeros((F, 15, 3), F32)
    track[:, :, 2] = 900.0
    track[k:, :, 1] = 300.0
    out = _single(mk_shape, track)
    err = np.abs(out[k:k + 4, 0, 1] - 300.0)
    print(f"300 mm step: error after 1..4 frames {err.round(2).tolist()} mm")
    assert err[3] <= 5.0 and (np.abs(out[k + 3:, :, 1] - 300.0) <= 5.0).all()
