"""Shared by tests/test_track_emu.py (CPU emulator) and tests/test_track_gpu.py (the shipped library on the card): the
yardstick of fvp_track_update - an independent fp32 numpy restatement of the definition in include/fvp.h (np.float32
scalars, np.sqrt, plain Python loops; no code shared with the product) - seeded scenarios, and the case bodies both files
run.  Everything is compared bit for bit: ids, slots, costs viewed as int32, and the four state arrays after every call."""
import ctypes as C

import numpy as np
import torch

F32 = np.float32
EINVAL, ELIMIT = 10001, 10002


# ---- the yardstick -----------------------------------------------------------------------------------------------
class Spec:
    def __init__(self, N, J, nseq=1, T=None, gate_mm=500.0, max_age=15):
        self.N, self.J, self.nseq, self.T = N, J, nseq, 2 * N if T is None else T
        self.gate, self.max_age = F32(gate_mm), int(max_age)
        self.pose = np.zeros((nseq, self.T, J, 3), F32)
        self.id = np.full((nseq, self.T), -1, np.int32)
        self.age = np.zeros((nseq, self.T), np.int32)
        self.next = np.zeros((nseq,), np.int32)

    def cost(self, det, trk):
        total = None
        for j in range(self.J):
            dx, dy, dz = det[j, 0] - trk[j, 0], det[j, 1] - trk[j, 1], det[j, 2] - trk[j, 2]
            d = np.sqrt(dx * dx + dy * dy + dz * dz)
            total = d if total is None else total + d
        c = total / F32(self.J)
        assert c.dtype == F32
        return c

    def update(self, poses, frame_set=None):
        poses = np.asarray(poses, F32)
        B = poses.shape[0]
        ids = np.full((B, self.N), -1, np.int32)
        slots = np.full((B, self.N), -1, np.int32)
        costs = np.full((B, self.N), -1, F32)
        with np.errstate(all="ignore"):
            for b in range(B):
                s = 0 if frame_set is None else int(frame_set[b])
                if 0 <= s < self.nseq:
                    self.frame(poses[b], s, ids[b], slots[b], costs[b])
        return ids, slots, costs

    def frame(self, p, s, ids, slots, costs):
        N, T = self.N, self.T
        pose, tid, age = self.pose[s], self.id[s], self.age[s]
        dets = [n for n in range(N) if p[n, 0, 3] >= 0]
        live = [t for t in range(T) if tid[t] >= 0]
        pairs = []
        for n in dets:
            for t in live:
                c = self.cost(p[n, :, :3], pose[t])
                if c <= self.gate:                   # False for NaN
                    pairs.append((c, n, t))
        pairs.sort()                                 # (cost, n, t) lexicographic: taking them in this order IS the greedy rule
        det_done, trk_done = set(), set()
        for c, n, t in pairs:
            if n in det_done or t in trk_done:
                continue
            det_done.add(n)
            trk_done.add(t)
            pose[t] = p[n, :, :3]
            age[t] = 0
            ids[n], slots[n], costs[n] = tid[t], t, c
        for t in live:
            if t not in trk_done:
                age[t] += 1
                if age[t] > self.max_age:
                    tid[t] = -1
        for n in dets:
            if n in det_done:
                continue
            free = [t for t in range(T) if tid[t] < 0]
            if free:
                t = free[0]
            else:
                oldest = max(int(age[u]) for u in range(T))
                t = [u for u in range(T) if age[u] == oldest][0]
                assert oldest >= 1
            tid[t] = self.next[s]
            self.next[s] += 1
            age[t] = 0
            pose[t] = p[n, :, :3]
            ids[n], slots[n], costs[n] = tid[t], t, F32(-1)

    def state(self):
        return dict(trk_pose=self.pose, trk_id=self.id, trk_age=self.age, next_id=self.next)


# ---- comparisons -----------------------------------------------------------------------------------------------------
def _np(a):
    return a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


def bits(a):
    a = _np(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def same(a, b):
    a, b = _np(a), _np(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def assert_outputs(got, want, what):
    for name, g, w in zip(("ids", "slots", "costs"), got, want):
        g, w = _np(g), _np(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape)
        bad = np.argwhere(bits(g) != bits(w))
        assert bad.size == 0, f"{what}: {name} differs at {len(bad)} (b,n), first {tuple(bad[0])}: {g[tuple(bad[0])]!r} " \
                              f"vs {w[tuple(bad[0])]!r}\n got {g.tolist()}\nwant {w.tolist()}"


def assert_state(tracker, spec, what):
    got = tracker.state()
    for k, w in spec.state().items():
        assert same(got[k], w), f"{what}: state {k} differs\n got {_np(got[k]).tolist() if k != 'trk_pose' else ''}\n" \
                                f"want {w.tolist() if k != 'trk_pose' else ''}"


# ---- scenarios ------------------------------------------------------------------------------------------------------
def skeleton(rng, J, integer=False):
    off = rng.uniform(-300.0, 300.0, size=(J, 3))
    return (np.round(off) if integer else off).astype(F32)


def walks(seed, P, J, frames, step=20.0):
    """[frames, P, J, 3]: P people 1500 mm apart on seeded random walks (root step ~ N(0, step) mm per axis and frame, every
    joint jittered by a further 5 mm): three times the default gate between any two of them for the whole scenario."""
    rng = np.random.default_rng(seed)
    roots = np.stack([np.array([1500.0 * (p % 4) - 2250.0, 1500.0 * (p // 4) - 1500.0, 900.0]) for p in range(P)])
    skel = np.stack([skeleton(rng, J) for _ in range(P)])
    out = np.empty((frames, P, J, 3), F32)
    for f in range(frames):
        roots = roots + rng.normal(0.0, step, size=roots.shape)
        out[f] = (roots[:, None, :] + skel + rng.normal(0.0, 5.0, size=skel.shape)).astype(F32)
    return out


def pack(seed, people, present, N):
    """people [F,P,J,3], present [F,P] bool -> fused_poses [F,N,J,5] with the slot order permuted every frame, and
    slot_of [F,P] (-1 = absent).  Slots without a person are invalid (flag -1) and carry a copy of some person's joints, so a
    kernel that read an invalid slot would show it."""
    rng = np.random.default_rng(seed)
    F, P, J = people.shape[:3]
    poses = np.empty((F, N, J, 5), F32)
    slot_of = np.full((F, P), -1, np.int64)
    for f in range(F):
        poses[f, :, :, :3] = people[f, rng.integers(0, P, size=N)]
        poses[f, :, :, 3] = -1.0
        poses[f, :, :, 4] = 0.5
        order = rng.permutation(N)
        k = 0
        for p in range(P):
            if present[f, p]:
                n = order[k]
                k += 1
                poses[f, n, :, :3] = people[f, p]
                poses[f, n, :, 3] = 0.0
                slot_of[f, p] = n
    return poses, slot_of


def at(points, N, J, skel=None):
    """One frame [N,J,5] from {slot: (x, y, z)}: every joint of the person at the point plus the shared skeleton offsets."""
    fr = np.zeros((N, J, 5), F32)
    fr[:, :, 3] = -1.0
    fr[:, :, 4] = 0.5
    for n, xyz in points.items():
        fr[n, :, :3] = np.asarray(xyz, F32) + (0 if skel is None else skel)
        fr[n, :, 3] = 0.0
    return fr


# ---- runner -----------------------------------------------------------------------------------------------------------
def run(mk, poses, chunks, frame_set=None, what="", **kw):
    """Feed ``poses`` [F,N,J,5] to a fresh tracker ``mk(N, J, **kw)`` in calls of the given sizes; after EVERY call the
    outputs and the whole state equal the yardstick's.  Returns the concatenated outputs (numpy) and the tracker."""
    F, N, J = poses.shape[:3]
    assert sum(chunks) == F
    tracker = mk(N, J, **kw)
    spec = Spec(N, J, kw.get("nseq", 1), kw.get("max_tracks"), kw.get("gate_mm", 500.0), kw.get("max_age", 15))
    dev = tracker.device
    outs, f = [], 0
    for c in chunks:
        x = torch.from_numpy(np.ascontiguousarray(poses[f:f + c])).to(dev)
        fs = None if frame_set is None else np.asarray(frame_set[f:f + c], np.int32)
        got = tracker.update(x, sequences=None if fs is None else torch.from_numpy(fs).to(dev))
        want = spec.update(poses[f:f + c], fs)
        assert_outputs(got, want, f"{what} frames {f}..{f + c - 1}")
        assert_state(tracker, spec, f"{what} after frame {f + c - 1}")
        outs.append([_np(g).copy() for g in got])
        f += c
    return [np.concatenate([o[k] for o in outs]) for k in range(3)], tracker


def chunks_of(F, B):
    return [B] * (F // B) + ([F % B] if F % B else [])


# ---- the cases (each takes the tracker factory of its file) ----------------------------------------------------------------
CONTINUITY = [(15, 10, 16, 3), (17, 10, 16, 1), (15, 10, 16, 8), (17, 4, 4, 3)]      # J, N, T, B


def case_continuity(mk, J, N, T, B):
    P, F = (6, 12) if N == 10 else (3, 9)
    people = walks(11 + J + B, P, J, F)
    poses, slot_of = pack(5 + B, people, np.ones((F, P), bool), N)
    (ids, slots, costs), _ = run(mk, poses, chunks_of(F, B), what="continuity", max_tracks=T)
    # the scenario's own ground truth: person p keeps the id it was born with, whatever slot it sits in
    assert (slot_of[0] != slot_of[1]).any()
    first = ids[0, slot_of[0]]
    assert sorted(first.tolist()) == list(range(P))
    for f in range(F):
        assert (ids[f, slot_of[f]] == first).all(), (f, ids[f].tolist(), slot_of[f].tolist())
        assert (ids[f] >= 0).sum() == P
    assert (costs[1:][ids[1:] >= 0] > 0).all() and (costs[1:][ids[1:] >= 0] <= 500).all()
    assert (costs[0] == -1).all()


def case_ties(mk, J):
    """Exact ties, integer coordinates: one detection 100 mm from two tracks, two detections 100 mm from one track."""
    N, T = 10, 16
    skel = skeleton(np.random.default_rng(3), J, integer=True)
    f0 = at({1: (0, 0, 0), 3: (200, 0, 0), 4: (5000, 0, 0)}, N, J, skel)                       # tracks 0, 1, 2
    f1 = at({0: (100, 0, 0), 2: (5000, 100, 0), 6: (5000, -100, 0)}, N, J, skel)
    (ids, slots, costs), tr = run(mk, np.stack([f0, f1]), [1, 1], what="ties")
    assert ids[0].tolist() == [-1, 0, -1, 1, 2, -1, -1, -1, -1, -1]
    # n = 0 ties between tracks 0 and 1: the lower t; n = 2 and n = 6 tie on track 2: the lower n, the other is born
    assert ids[1].tolist() == [0, -1, 2, -1, -1, -1, 3, -1, -1, -1]
    assert slots[1].tolist() == [0, -1, 2, -1, -1, -1, 3, -1, -1, -1]
    assert costs[1, 0] == costs[1, 2] == F32(100) and costs[1, 6] == -1
    assert _np(tr.state()["trk_age"])[0, :4].tolist() == [0, 1, 0, 0]
    # the same frame with the tied detections in the other slot order: again the lower n
    f1b = at({0: (100, 0, 0), 2: (5000, -100, 0), 6: (5000, 100, 0)}, N, J, skel)
    (ids, slots, costs), _ = run(mk, np.stack([f0, f1b]), [2], what="ties, swapped")
    assert ids[1].tolist() == [0, -1, 2, -1, -1, -1, 3, -1, -1, -1]


def case_gate_edge(mk, J):
    N, T = 10, 16
    skel = skeleton(np.random.default_rng(4), J, integer=True)
    f0 = at({2: (1000, 1000, 0)}, N, J, skel)
    f1 = at({5: (1300, 1400, 0)}, N, J, skel)                                                  # 3-4-5: exactly 500 mm
    below = float(np.nextafter(F32(500), F32(0)))
    assert F32(below) < F32(500)
    (ids, _, costs), _ = run(mk, np.stack([f0, f1]), [2], what="gate == cost", gate_mm=500.0)
    assert ids[1, 5] == 0 and costs[1, 5] == F32(500)
    (ids, slots, costs), _ = run(mk, np.stack([f0, f1]), [2], what="gate just below the cost", gate_mm=below)
    assert ids[1, 5] == 1 and slots[1, 5] == 1 and costs[1, 5] == -1


def case_gaps(mk, J, B):
    """max_age = 3.  A is missing for 3 frames and keeps its id; B is missing for 4, its slot is freed in the 4th - where a
    newcomer C takes it at once - and B comes back under a new id.  D never leaves."""
    N, T, F, max_age = 10, 16, 8, 3
    people = walks(21 + J, 4, J, F, step=10.0)                                                   # A, B, D, C
    present = np.ones((F, 4), bool)
    present[1:4, 0] = False                                                                    # A: frames 1-3
    present[1:5, 1] = False                                                                    # B: frames 1-4
    present[:4, 3] = False                                                                     # C: from frame 4
    poses, slot_of = pack(8, people, present, N)
    (ids, slots, _), _ = run(mk, poses, chunks_of(F, B), what="gaps", max_tracks=T, max_age=max_age)

    def of(f, p, a):
        return int(a[f, slot_of[f, p]])
    born = [of(0, p, ids) for p in range(3)]
    assert sorted(born) == [0, 1, 2]
    assert of(4, 0, ids) == born[0] and of(7, 0, ids) == born[0]                               # A is back as itself
    assert of(4, 3, ids) == 3 and of(4, 3, slots) == of(0, 1, slots)                           # C: new id, B's slot, same frame
    assert of(5, 1, ids) == 4 and of(7, 1, ids) == 4                                           # B: a new identity
    assert all(of(f, 2, ids) == born[2] for f in range(F))


def case_full_table(mk, J):
    """N = T = 4, people 3 m apart coming and going: births into a full table evict the oldest track, lowest slot on a tie."""
    N = 4

    def pt(k):
        return (3000.0 * k, 0.0, 0.0)
    a, b, c, d, e, f_, g, h, i, j, k = range(11)
    frames = [
        {0: pt(a), 1: pt(b), 2: pt(c), 3: pt(d)},          # slots 0-3 = a b c d
        {0: pt(a), 1: pt(b), 2: pt(e), 3: pt(f_)},         # c, d aged 1: e evicts slot 2 (tie: lowest), f slot 3
        {0: pt(a), 1: pt(e), 2: pt(g), 3: pt(h)},          # b (slot 1), f (slot 3) aged 1: g -> 1, h -> 3
        {0: pt(g), 1: pt(i)},                              # a, e, h aged 1: i -> slot 0
        {0: pt(g), 1: pt(j), 2: pt(k)},                    # i aged 1, e and h aged 2: j -> slot 2 (oldest), k -> slot 3
    ]
    poses = np.stack([at(fr, N, J) for fr in frames])
    (ids, slots, _), tr = run(mk, poses, [2, 3], what="full table", max_tracks=4)
    assert slots[1].tolist() == [0, 1, 2, 3] and ids[1].tolist() == [0, 1, 4, 5]
    assert slots[2].tolist() == [0, 2, 1, 3] and ids[2].tolist() == [0, 4, 6, 7]
    assert slots[3].tolist() == [1, 0, -1, -1] and ids[3].tolist() == [6, 8, -1, -1]
    assert slots[4].tolist() == [1, 2, 3, -1] and ids[4].tolist() == [6, 9, 10, -1]
    st = tr.state()
    assert _np(st["trk_id"])[0].tolist() == [8, 6, 9, 10] and _np(st["trk_age"])[0].tolist() == [1, 0, 0, 0]


def case_empty_and_first(mk, J, B):
    N, T = 10, 16
    people = walks(31, 5, J, 4)
    present = np.ones((4, 5), bool)
    present[1:3] = False                                                                       # two empty frames
    poses, slot_of = pack(2, people, present, N)
    poses = np.concatenate([at({}, N, J)[None], poses])                                        # and an empty FIRST frame
    (ids, slots, costs), tr = run(mk, poses, chunks_of(5, B), what="empty frames")
    assert (ids[0] == -1).all() and (slots[0] == -1).all() and (costs[0] == -1).all()
    valid = poses[1, :, 0, 3] >= 0
    assert ids[1][valid].tolist() == [0, 1, 2, 3, 4] and slots[1][valid].tolist() == [0, 1, 2, 3, 4]     # in slot order
    assert (ids[2:4] == -1).all() and (costs[2:4] == -1).all()
    assert sorted(ids[4][ids[4] >= 0].tolist()) == [0, 1, 2, 3, 4]                             # aged 2, back as themselves
    assert (ids[4, slot_of[3]] == ids[1, slot_of[0]]).all()


def _mixed(J, N=10, F=8, seed=41):
    people = walks(seed, 6, J, F)
    present = np.ones((F, 6), bool)
    present[2:4, 1] = False
    present[3, 4] = False
    present[:2, 5] = False
    return pack(seed + 1, people, present, N)[0]


def case_chunk_invariance(mk, J):
    poses = _mixed(J)
    runs = [run(mk, poses, ch, what=f"chunks {ch}", max_age=1) for ch in ([8], [3, 5], [1] * 8)]
    for out, tr in runs[1:]:
        for x, y in zip(out, runs[0][0]):
            assert same(x, y)
        for k2, v in tr.state().items():
            assert same(v, runs[0][1].state()[k2])


def case_two_sequences(mk, J):
    N, T = 10, 16
    a, b = _mixed(J, seed=51)[:4], _mixed(J, seed=61)[:4]
    frame_set = [0, 1, 1, 0, 1, 0, 0, 1]
    poses = np.empty((8,) + a.shape[1:], F32)
    ia = ib = 0
    for f, s in enumerate(frame_set):
        if s == 0:
            poses[f] = a[ia]
            ia += 1
        else:
            poses[f] = b[ib]
            ib += 1
    (ids, slots, costs), tr = run(mk, poses, [8], frame_set, what="two sequences", nseq=2, max_tracks=T)
    fs = np.asarray(frame_set)
    for s, own in ((0, a), (1, b)):
        out1, tr1 = run(mk, own, [4], what=f"sequence {s} alone", max_tracks=T)
        for x, y in zip((ids, slots, costs), out1):
            assert same(x[fs == s], y)
        for k2, v in tr1.state().items():
            assert same(_np(tr.state()[k2])[s], _np(v)[0])
        assert ids[fs == s][0].max() == (own[0, :, 0, 3] >= 0).sum() - 1                       # ids restart at 0
    # a frame of no sequence (row 2 of a two-sequence tracker): all -1, nothing changes; every output element is written
    fs2 = list(frame_set)
    fs2[3] = 2
    (ids2, _, _), _ = run(mk, poses, [8], fs2, what="a frame outside the tracker", nseq=2, max_tracks=T)
    assert (ids2[3] == -1).all()


def case_nan(mk, J):
    poses = _mixed(J)
    f, n = 4, int(np.argmax(poses[4, :, 0, 3] >= 0))
    bad = poses.copy()
    bad[f, n, J // 2, 1] = np.nan
    (ids, slots, costs), tr = run(mk, bad, [8], what="NaN detection")
    without = poses.copy()
    without[f, n, :, 3] = -1.0
    (ids0, slots0, costs0), _ = run(mk, without, [8], what="that slot invalid")
    assert costs[f, n] == -1 and ids[f, n] == ids[:f + 1].max() and ids[f, n] > ids[:f].max()      # a birth
    others = np.arange(poses.shape[1]) != n
    for x, y in ((ids, ids0), (slots, slots0), (costs, costs0)):
        assert same(x[f][others], y[f][others]) and same(x[:f], y[:f])
    st = _np(tr.state()["trk_pose"])[0, slots[f, n]]
    assert np.isnan(st).sum() == 1


def raw_call(lib, dev, poses, state, outs, nseq, T, gate=500.0, max_age=15, N=None, J=None):
    B = poses.shape[0]
    N = poses.shape[1] if N is None else N
    J = poses.shape[2] if J is None else J
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream) if torch.device(dev).type == "cuda" else None
    p = [C.c_void_p(t.data_ptr()) for t in (poses,) + tuple(state) + tuple(outs)]
    return lib.fvp_track_update(p[0], None, *p[1:], B, N, J, nseq, T, gate, max_age, stream)


def case_argument_limits(lib, dev):
    N, J = 10, 15
    poses = torch.from_numpy(_mixed(J)[:2].copy()).to(dev)

    def buffers(T):
        state = (torch.full((1, T, J, 3), 7.0, device=dev), torch.full((1, T), -1, dtype=torch.int32, device=dev),
                 torch.full((1, T), 5, dtype=torch.int32, device=dev), torch.full((1,), 3, dtype=torch.int32, device=dev))
        outs = (torch.full((2, N), 77, dtype=torch.int32, device=dev), torch.full((2, N), 77, dtype=torch.int32, device=dev),
                torch.full((2, N), 77.0, device=dev))
        return state, outs
    for T, kw, want in ((9, {}, EINVAL), (65, {}, ELIMIT), (64, dict(N=33), ELIMIT), (64, dict(J=33), ELIMIT),
                        (16, dict(max_age=-1), EINVAL)):
        state, outs = buffers(T)
        keep = [t.clone() for t in state + outs]
        assert raw_call(lib, dev, poses, state, outs, 1, T, **kw) == want, (T, kw)
        for t, k2 in zip(state + outs, keep):
            assert same(t, k2), "an error return wrote something"
    state, outs = buffers(64)                                                                  # the largest table is fine
    assert raw_call(lib, dev, poses, state, outs, 1, 64) == 0
    assert (_np(outs[0]) != 77).all() and (_np(outs[2]) != 77).all()
