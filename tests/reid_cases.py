"""Cases and the yardsticks of fvp_person_signature and fvp_track_reid (include/fvp.h, ABI 20), shared by
tests/test_reid_emu.py (CPU emulator) and tests/test_reid_gpu.py (the shipped library on the card): an independent numpy
restatement of both definitions - the sample positions in numpy float32 (every operation rounds to float32), the histograms and
the intersection in Python ints, the quotient in Python floats (fp64) with one rounding to float32 - seeded frames inside a guard
band of sentinel bytes, hand-made id / slot / signature streams for the state machine, and runners that call the entry points on
torch memory (CPU for the emulator, the card otherwise).  Everything is compared bit for bit: no tolerance anywhere."""
import ctypes as C

import numpy as np
import torch

f32 = np.float32
NAN, INF = float("nan"), float("inf")
EINVAL, ELIMIT = 10001, 10002
BINS, MAX_PARTS, MAX_GALLERY, MAX_WINDOW = 64, 4, 64, 1024
GUARD = 4096                                             # sentinel bytes in front of and behind the frames
LIMBS17 = [[0, 1], [0, 2], [1, 2], [1, 3], [2, 4], [3, 5], [4, 6], [5, 7], [7, 9], [6, 8], [8, 10], [5, 11], [11, 13],
           [13, 15], [6, 12], [12, 14], [14, 16], [5, 6], [11, 12]]
LIMBS15 = [[0, 1], [0, 2], [0, 3], [3, 4], [4, 5], [0, 9], [9, 10], [10, 11], [2, 6], [2, 12], [6, 7], [7, 8], [12, 13],
           [13, 14]]
LIMBS = {15: LIMBS15, 17: LIMBS17}


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _dev(a, device):
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a).copy())
    return t if str(device) == "cpu" else t.to(device)


def _ptr(t, off=0):
    return None if t is None else C.c_void_p(t.data_ptr() + off)


def _stream(device):
    return C.c_void_p(torch.cuda.current_stream().cuda_stream) if str(device).startswith("cuda") else None


def _sync(device):
    if str(device).startswith("cuda"):
        torch.cuda.synchronize()


def _ia(v):
    v = [int(x) for x in v]
    return (C.c_int32 * max(len(v), 1))(*v)


# ======================================================================================================================
# fvp_person_signature
# ======================================================================================================================
def usable(c, b, v, n, j):
    """The header's usable joint-view, on float32 scalars (a NaN fails every compare)."""
    px, py, depth = (f32(x) for x in c["views"][b, v, n, j, :3])
    ok = bool(depth > f32(0)) and bool(np.abs(px) <= f32(32768)) and bool(np.abs(py) <= f32(32768))
    if ok and c["conf"] is not None:
        ok = bool(f32(c["conf"][b, n, j]) >= f32(c["conf_min"]))
    if ok and c["occ"] is not None:
        ok = int(c["occ"][b, v, n, j]) == -1
    return ok


def sig_reference(c):
    """-> (sig [B,N,P,64] int32, sig_count [B,N,P] int32, the number of counting samples)."""
    B, V, N, J = c["views"].shape[:4]
    Hs, Ws = c["frames"].shape[2:4]
    P, K = c["P"], c["K"]
    sig = [[[[0] * BINS for _ in range(P)] for _ in range(N)] for _ in range(B)]
    taken = 0
    m = np.arange(K).astype(f32)
    t = (m + f32(0.5)) / f32(K)                                               # float32 array ops: one rounding each
    for b in range(B):
        for n in range(N):
            if c["ids"] is not None and c["ids"][b, n] < 0:
                continue
            for v in range(V):
                for (i, k), part in zip(c["limbs"], c["parts"]):
                    if not (usable(c, b, v, n, i) and usable(c, b, v, n, k)):
                        continue
                    a, e = c["views"][b, v, n, i, :2].astype(f32), c["views"][b, v, n, k, :2].astype(f32)
                    x = a[0] + t * (e[0] - a[0])
                    y = a[1] + t * (e[1] - a[1])
                    assert x.dtype == f32 and y.dtype == f32
                    xi, yi = np.rint(x).astype(np.int64), np.rint(y).astype(np.int64)        # round-half-even
                    for s in range(K):
                        if 0 <= xi[s] < Ws and 0 <= yi[s] < Hs:
                            c0, c1, c2 = (int(q) for q in c["frames"][b, v, yi[s], xi[s]])
                            sig[b][n][part][(c0 >> 6) * 16 + (c1 >> 6) * 4 + (c2 >> 6)] += 1
                            taken += 1
    sig = np.array(sig, np.int64).reshape(B, N, P, BINS)
    return sig.astype(np.int32), sig.sum(axis=3).astype(np.int32), taken


def _sig(B, V, N, J, hs, ws, K, P, seed, limbs=None, parts=None, conf=False, conf_min=0.0, ids=False, occ=False):
    rng = np.random.default_rng(seed)
    views = np.empty((B, V, N, J, 4), f32)
    views[..., 0] = rng.uniform(-6, ws + 6, (B, V, N, J))
    views[..., 1] = rng.uniform(-6, hs + 6, (B, V, N, J))
    views[..., 2] = rng.uniform(500, 5000, (B, V, N, J))
    views[..., 3] = rng.uniform(0, 1, (B, V, N, J))
    limbs = LIMBS[J] if limbs is None else limbs
    return dict(frames=rng.integers(0, 256, (B, V, hs, ws, 3), dtype=np.uint8), views=views,
                ids=rng.integers(0, 50, (B, N)).astype(np.int32) if ids else None,
                conf=rng.uniform(0, 1, (B, N, J)).astype(f32) if conf else None, conf_min=conf_min,
                occ=np.full((B, V, N, J), -1, np.int32) if occ else None, limbs=[list(l) for l in limbs],
                parts=[l % P for l in range(len(limbs))] if parts is None else parts, P=P, K=K)


def _sig_edges(ws_hs):
    """Self-limbs (both ends on one joint: the K samples land on that joint's pixel) on and around the frame's border; the
    ties of rintf at .5 go to the even neighbour, i.e. both ways."""
    hs, ws = ws_hs
    c = _sig(1, 1, 4, 15, hs, ws, 8, 2, 11, limbs=[(j, j) for j in range(15)], parts=[j % 2 for j in range(15)])
    v = c["views"]
    xs = [0.0, -0.5, -0.50001, 0.5, 1.5, 2.5, ws - 1.0, ws - 0.5, ws - 0.50001, ws - 1.5, ws, 3.49999, -0.0, ws - 0.75, 7.0]
    ys = [0.0, -0.5, -0.50001, 0.5, 1.5, 2.5, hs - 1.0, hs - 0.5, hs - 0.50001, hs - 1.5, hs, 3.49999, -0.0, hs - 0.75, 7.0]
    for j in range(15):
        v[0, 0, 0, j, :2] = (xs[j], 5.0)                                      # person 0: x on the edges
        v[0, 0, 1, j, :2] = (5.0, ys[j])                                      # person 1: y on the edges
        v[0, 0, 2, j, :2] = (xs[j], ys[j])                                    # person 2: the corners
        v[0, 0, 3, j, :2] = (xs[14 - j], ys[j])
    return c


def _sig_behind_camera():
    c = _sig(3, 3, 4, 17, 50, 67, 8, 2, 12)
    c["views"][0, 0, 0, 5, 2] = -100.0                                        # one end of four limbs behind the camera
    c["views"][1, 2, 3, 0, 2] = 0.0
    c["views"][2, 1, 1, 11, 2] = -0.0
    return c


def _sig_nan_pixel():
    c = _sig(3, 3, 4, 15, 50, 67, 8, 4, 13)
    c["views"][0, 1, 1, 0, 0] = NAN
    c["views"][0, 1, 2, 3, 1] = NAN
    c["views"][1, 0, 0, 2, 0] = INF
    c["views"][1, 0, 1, 6, 1] = -INF
    c["views"][2, 2, 3, 9, 0] = 32768.0                                       # usable, far outside the frame
    c["views"][2, 2, 3, 10, 0] = 32769.0                                      # not usable
    c["views"][2, 0, 0, 0, 2] = NAN
    return c


def _sig_conf(on):
    c = _sig(3, 3, 4, 17, 50, 67, 8, 2, 14, conf=True, conf_min=0.5)
    c["conf"][0, 0, 5] = 0.5                                                  # exactly at the limit: usable
    c["conf"][0, 1, 5] = np.nextafter(f32(0.5), f32(0))
    c["conf"][1, 2, 0] = NAN
    if not on:
        c["conf"] = None
    return c


def _sig_occluder():
    c = _sig(3, 3, 4, 17, 50, 67, 8, 2, 15, occ=True)
    c["occ"][:, 1, 0, :] = 2                                                  # view 1 does not see person 0 ...
    c["occ"][1, 0, 2, 5] = -2                                                 # ... and one joint is not evaluated
    c["occ"][2, 2, 3, 6] = 3                                                  # a self-occluded joint
    return c


def _sig_ids():
    c = _sig(3, 3, 4, 15, 50, 67, 8, 2, 16, ids=True)
    c["ids"][0, 1] = c["ids"][1, 0] = c["ids"][2, 3] = -1
    return c


def _sig_coincide():
    c = _sig(1, 3, 4, 15, 50, 67, 32, 2, 17)
    for n in range(4):
        c["views"][0, :, n, 4, :2] = c["views"][0, :, n, 3, :2]               # limb (3, 4) has no length
    c["views"][0, :, 0, 3, :2] = (20.25, 30.75)
    c["views"][0, :, 0, 4, :2] = (20.25, 30.75)
    return c


def _sig_all_invalid():
    c = _sig(3, 3, 4, 17, 50, 67, 8, 2, 18)
    c["views"][:] = 0.0                                                       # what fvp_joint_evidence writes for them
    return c


SIG_BUILDERS = {
    "rand_b1_v1_k1_p1_j15_odd": lambda: _sig(1, 1, 4, 15, 50, 67, 1, 1, 1),
    "rand_b3_v3_k8_p2_j17": lambda: _sig(3, 3, 4, 17, 96, 128, 8, 2, 2),
    "rand_b8_v5_k32_p4_n10_j15_odd": lambda: _sig(8, 5, 10, 15, 50, 67, 32, 4, 3, ids=True),
    "rand_b1_v5_k8_p4_j17": lambda: _sig(1, 5, 4, 17, 96, 128, 8, 4, 4, conf=True, conf_min=0.2, occ=True),
    "edges_128x96": lambda: _sig_edges((96, 128)),
    "edges_67x50": lambda: _sig_edges((50, 67)),
    "behind_camera": _sig_behind_camera,
    "nan_pixel": _sig_nan_pixel,
    "conf_on": lambda: _sig_conf(True),
    "conf_off": lambda: _sig_conf(False),
    "occluder_one_view": _sig_occluder,
    "ids_minus1": _sig_ids,
    "limb_ends_coincide_k32": _sig_coincide,
    "all_invalid": _sig_all_invalid,
}
SIG_CASES = list(SIG_BUILDERS)
_sig_cache = {}


def sig_case(name):
    if name not in _sig_cache:
        c = SIG_BUILDERS[name]()
        _sig_cache[name] = (c, sig_reference(c))
    return _sig_cache[name]


def sig_call(lib, device, c, outs=(True, True), fence=None, **over):
    """fvp_person_signature on ``device`` with the frames inside a guard band of 0xFF bytes and poisoned outputs: (rc, sig or
    None, sig_count or None[, fenced reads]).  ``fence``: "guard" or "frames" (emulator only).  ``over`` replaces arguments."""
    a = dict(c)
    a.update(over)
    B, V, N, J = c["views"].shape[:4]
    Hs, Ws = c["frames"].shape[2:4]
    raw = np.full(GUARD + c["frames"].size + GUARD, 0xFF, np.uint8)
    raw[GUARD:GUARD + c["frames"].size] = c["frames"].reshape(-1)
    buf = _dev(raw, device)
    views, ids, conf, occ = (_dev(c[k], device) for k in ("views", "ids", "conf", "occ"))
    sig = _dev(np.full((B, N, c["P"], BINS), -7, np.int32), device) if outs[0] else None
    cnt = _dev(np.full((B, N, c["P"]), -7, np.int32), device) if outs[1] else None
    if fence is not None:
        lib.hipemu_fence.argtypes = [C.c_void_p, C.c_size_t]
        lib.hipemu_fenced_reads.restype = C.c_long
        lib.hipemu_fences_clear()
        if fence == "guard":        # a fence counts a read whose four bytes from its address on meet the range
            lib.hipemu_fence(C.c_void_p(buf.data_ptr()), GUARD - 3)
            lib.hipemu_fence(C.c_void_p(buf.data_ptr() + GUARD + c["frames"].size + 1), GUARD - 1)
        else:
            lib.hipemu_fence(C.c_void_p(buf.data_ptr() + GUARD), c["frames"].size)
    limbs = [j for l in a["limbs"] for j in l]
    rc = lib.fvp_person_signature(None if a.get("null_frames") else _ptr(buf, GUARD), a.get("B", B), a.get("V", V),
                                  a.get("Hs", Hs), a.get("Ws", Ws), None if a.get("null_views") else _ptr(views), _ptr(ids),
                                  _ptr(conf), _ptr(occ), a.get("N", N), a.get("J", J),
                                  None if a.get("null_limbs") else _ia(limbs), None if a.get("null_parts") else _ia(a["parts"]),
                                  a.get("L", len(a["limbs"])), a["P"], a["K"], a["conf_min"], _ptr(sig), _ptr(cnt),
                                  _stream(device))
    _sync(device)
    res = (rc, None if sig is None else sig.cpu().numpy(), None if cnt is None else cnt.cpu().numpy())
    if fence is not None:
        res += (int(lib.hipemu_fenced_reads()),)
        lib.hipemu_fences_clear()
    return res


def sig_check(lib, device, name):
    c, (want_sig, want_cnt, _) = sig_case(name)
    rc, sig, cnt = sig_call(lib, device, c)
    assert rc == 0, rc
    assert np.array_equal(sig, want_sig), name
    assert np.array_equal(cnt, want_cnt), name


def sig_check_null_outputs(lib, device):
    c, (want_sig, want_cnt, _) = sig_case("rand_b3_v3_k8_p2_j17")
    rc, sig, _ = sig_call(lib, device, c, outs=(True, False))
    assert rc == 0 and np.array_equal(sig, want_sig)
    rc, _, cnt = sig_call(lib, device, c, outs=(False, True))
    assert rc == 0 and np.array_equal(cnt, want_cnt)


def sig_argument_errors(lib, device):
    """Every refusal of the header, and that a refused call writes nothing."""
    c, _ = sig_case("rand_b1_v1_k1_p1_j15_odd")
    L = len(c["limbs"])

    def refused(want, outs=(True, True), **over):
        rc, sig, cnt = sig_call(lib, device, c, outs=outs, **over)
        assert rc == want, (over, rc)
        assert (sig is None or (sig == -7).all()) and (cnt is None or (cnt == -7).all()), over

    for over in (dict(null_frames=True), dict(null_views=True), dict(null_limbs=True), dict(null_parts=True), dict(B=-1),
                 dict(V=-1), dict(N=0), dict(J=0), dict(Hs=0), dict(Ws=0), dict(L=0), dict(P=0), dict(K=0), dict(K=33),
                 dict(conf_min=NAN), dict(limbs=[[0, 15]] + c["limbs"][1:]), dict(limbs=[[-1, 0]] + c["limbs"][1:]),
                 dict(parts=[1] + c["parts"][1:]), dict(parts=[-1] + c["parts"][1:])):
        refused(EINVAL, **over)
    refused(EINVAL, outs=(False, False))
    for over in (dict(N=33), dict(J=33), dict(V=9), dict(L=65, limbs=[[0, 1]] * 65, parts=[0] * 65), dict(P=5), dict(Hs=16385),
                 dict(Ws=16385)):
        refused(ELIMIT, **over)
    for over in (dict(B=0), dict(V=0)):                                       # nothing to do: no launch, nothing written
        refused(0, **over)


# ======================================================================================================================
# fvp_track_reid
# ======================================================================================================================
STATE = ("slot_sig", "slot_tid", "slot_pid", "slot_frames", "slot_age", "slot_sim", "gal_sig", "gal_pid", "gal_age")
PRM = dict(max_age=3, min_samples=4, min_frames=2, window=8, sim_min=0.6, margin=0.1, gallery_max_age=0)


def reid_init(nseq, T, G, P):
    return dict(slot_sig=np.zeros((nseq, T, P, BINS), np.int32), slot_tid=np.full((nseq, T), -1, np.int32),
                slot_pid=np.full((nseq, T), -1, np.int32), slot_frames=np.zeros((nseq, T), np.int32),
                slot_age=np.zeros((nseq, T), np.int32), slot_sim=np.full((nseq, T), -1, f32),
                gal_sig=np.zeros((nseq, G, P, BINS), np.int32), gal_pid=np.full((nseq, G), -1, np.int32),
                gal_age=np.zeros((nseq, G), np.int32))


def similarity(a, g):
    """sim of a slot signature and a gallery signature [P][64] (Python ints): ints for the intersection, fp64 for the quotient,
    one rounding to float32."""
    acc, parts = 0.0, 0
    for ap, gp in zip(a, g):
        ca, cg = sum(ap), sum(gp)
        if ca > 0 and cg > 0:
            inter = sum(min(x * cg, y * ca) for x, y in zip(ap, gp))
            acc = acc + float(inter) / (float(ca) * float(cg))
            parts += 1
    return f32(acc / float(parts)) if parts else f32(0)


def reid_reference(st, ids, slots, sig, cnt, frame_set, prm):
    """One call of the header's state machine on the numpy state ``st`` (rewritten in place) -> (pids, reid_state, reid_sim)."""
    B, N = ids.shape
    nseq, T = st["slot_tid"].shape
    G = st["gal_pid"].shape[1]
    pids, rstate, rsim = np.full((B, N), -1, np.int32), np.full((B, N), -1, np.int32), np.full((B, N), -1, f32)

    def clear_slot(s, t):
        st["slot_sig"][s, t] = 0
        st["slot_tid"][s, t] = st["slot_pid"][s, t] = -1
        st["slot_frames"][s, t] = st["slot_age"][s, t] = 0
        st["slot_sim"][s, t] = -1

    def free_entry(s, g):
        st["gal_sig"][s, g] = 0
        st["gal_pid"][s, g] = -1
        st["gal_age"][s, g] = 0

    for b in range(B):
        s = 0 if frame_set is None else int(frame_set[b])
        if not 0 <= s < nseq:
            continue
        for g in range(G):                                                    # 1. gallery ageing
            if st["gal_pid"][s, g] >= 0:
                st["gal_age"][s, g] += 1
                if prm["gallery_max_age"] > 0 and st["gal_age"][s, g] > prm["gallery_max_age"]:
                    free_entry(s, g)
        for t in range(T):                                                    # 2. the slots in ascending order
            ns = [n for n in range(N) if ids[b, n] >= 0 and slots[b, n] == t]
            n = ns[0] if ns else None
            tid = int(st["slot_tid"][s, t])
            if tid >= 0 and ((n is not None and ids[b, n] != tid) or (n is None and st["slot_age"][s, t] + 1 > prm["max_age"])):
                if st["slot_frames"][s, t] >= prm["min_frames"]:
                    free = [g for g in range(G) if st["gal_pid"][s, g] < 0]
                    g = free[0] if free else int(np.argmax(st["gal_age"][s]))          # argmax: the first of the largest
                    st["gal_sig"][s, g] = st["slot_sig"][s, t]
                    st["gal_pid"][s, g] = st["slot_pid"][s, t] if st["slot_pid"][s, t] >= 0 else tid
                    st["gal_age"][s, g] = 0
                clear_slot(s, t)
            if n is None and st["slot_tid"][s, t] >= 0:
                st["slot_age"][s, t] += 1
            if n is not None:
                if st["slot_tid"][s, t] != ids[b, n]:
                    clear_slot(s, t)
                    st["slot_tid"][s, t] = ids[b, n]
                st["slot_age"][s, t] = 0
                if int(cnt[b, n].astype(np.int64).sum()) >= prm["min_samples"]:
                    if st["slot_frames"][s, t] == prm["window"]:
                        st["slot_sig"][s, t] >>= 1
                        st["slot_frames"][s, t] = prm["window"] >> 1
                    st["slot_sig"][s, t] += sig[b, n]
                    st["slot_frames"][s, t] += 1
            if st["slot_tid"][s, t] >= 0 and st["slot_pid"][s, t] == -1 and st["slot_frames"][s, t] >= prm["min_frames"]:
                a = [[int(x) for x in part] for part in st["slot_sig"][s, t]]
                occupied = [g for g in range(G) if st["gal_pid"][s, g] >= 0]
                sims = {g: similarity(a, [[int(x) for x in part] for part in st["gal_sig"][s, g]]) for g in occupied}
                best = None
                for g in occupied:
                    if best is None or sims[g] > sims[best]:
                        best = g
                second = max([sims[g] for g in occupied if g != best], default=f32(0))
                if best is not None and sims[best] >= f32(prm["sim_min"]) and f32(sims[best] - second) >= f32(prm["margin"]):
                    st["slot_pid"][s, t] = st["gal_pid"][s, best]
                    free_entry(s, best)
                else:
                    st["slot_pid"][s, t] = st["slot_tid"][s, t]
                st["slot_sim"][s, t] = sims[best] if best is not None else f32(-1)
        for n in range(N):                                                    # 3. outputs
            t = int(slots[b, n])
            if ids[b, n] >= 0 and 0 <= t < T:
                tid, pid = int(st["slot_tid"][s, t]), int(st["slot_pid"][s, t])
                pids[b, n] = pid if pid >= 0 else tid
                rstate[b, n] = 0 if pid < 0 else (1 if pid == tid else 2)
                rsim[b, n] = st["slot_sim"][s, t]
    return pids, rstate, rsim


def reid_call(lib, device, st, ids, slots, sig, cnt, frame_set, prm, **over):
    """fvp_track_reid on ``device``: (rc, new state, pids, reid_state, reid_sim); ``st`` is not changed.  Outputs start poisoned."""
    B, N = ids.shape
    nseq, T = st["slot_tid"].shape
    G, P = st["gal_pid"].shape[1], st["slot_sig"].shape[2]
    a = dict(prm, B=B, N=N, nseq=nseq, T=T, G=G, P=P)
    a.update(over)
    d = {k: _dev(st[k], device) for k in STATE}
    ins = [_dev(x, device) for x in (ids, slots, sig, cnt, frame_set)]
    outs = [_dev(np.full((B, N), -7, np.int32), device), _dev(np.full((B, N), -7, np.int32), device),
            _dev(np.full((B, N), -7, f32), device)]
    args = [_ptr(x) for x in ins] + [_ptr(d[k]) for k in STATE] + [_ptr(o) for o in outs]
    for i in a.get("null", ()):
        args[i] = None
    rc = lib.fvp_track_reid(*args, a["B"], a["N"], a["nseq"], a["T"], a["G"], a["P"], a["max_age"], a["min_samples"],
                            a["min_frames"], a["window"], a["sim_min"], a["margin"], a["gallery_max_age"], _stream(device))
    _sync(device)
    return (rc, {k: d[k].cpu().numpy() for k in STATE}) + tuple(o.cpu().numpy() for o in outs)


def same_state(a, b):
    return all(a[k].dtype == b[k].dtype and np.array_equal(a[k].view(np.int32), b[k].view(np.int32)) for k in STATE)


def check_invariants(st):
    """A person id is held by at most one live slot or gallery entry of a sequence; a free slot / entry is cleared."""
    for s in range(st["slot_tid"].shape[0]):
        live = st["slot_tid"][s] >= 0
        held = [int(p if p >= 0 else t) for p, t in zip(st["slot_pid"][s][live], st["slot_tid"][s][live])]
        held += [int(p) for p in st["gal_pid"][s] if p >= 0]
        assert len(held) == len(set(held)), held
        assert not st["slot_sig"][s][~live].any() and (st["slot_pid"][s][~live] == -1).all()
        assert not st["slot_frames"][s][~live].any() and not st["slot_age"][s][~live].any()
        assert (st["slot_sim"][s][~live] == -1).all()
        free = st["gal_pid"][s] < 0
        assert not st["gal_sig"][s][free].any() and not st["gal_age"][s][free].any()


def hist(P, *parts):
    """[P][64] int32 from one {bin: count} dict per part."""
    h = np.zeros((P, BINS), np.int32)
    for p, d in enumerate(parts):
        for k, v in d.items():
            h[p, k] = v
    return h


def stream(B, N, P, dets, frame_set=None):
    """ids, slots, sig, sig_count, frame_set of B frames from ``dets``: {b: [(n, track id, slot, hist [P][64]), ...]}."""
    ids, slots = np.full((B, N), -1, np.int32), np.full((B, N), -1, np.int32)
    sig, cnt = np.zeros((B, N, P, BINS), np.int32), np.zeros((B, N, P), np.int32)
    for b, lst in dets.items():
        for n, tid, slot, h in lst:
            ids[b, n], slots[b, n], sig[b, n] = tid, slot, h
            cnt[b, n] = h.sum(axis=1)
    return ids, slots, sig, cnt, None if frame_set is None else np.asarray(frame_set, np.int32)


def run_script(lib, device, shape, prm, calls):
    """The calls one after the other through the library and through the restatement, compared after every call: outputs,
    every state array and the invariants.  -> (list of (pids, reid_state, reid_sim) per call, list of states after each)."""
    nseq, T, G, P = shape
    st = reid_init(nseq, T, G, P)
    outs, states = [], []
    for k, call in enumerate(calls):
        rc, got_st, pids, rstate, rsim = reid_call(lib, device, st, *call, prm)
        want = reid_reference(st, *call, prm)                                 # advances st
        assert rc == 0, (k, rc)
        assert np.array_equal(pids, want[0]), (k, pids, want[0])
        assert np.array_equal(rstate, want[1]), (k, rstate, want[1])
        assert np.array_equal(bits(rsim), bits(want[2])), (k, rsim, want[2])
        for key in STATE:
            assert np.array_equal(got_st[key].view(np.int32), st[key].view(np.int32)), (k, key)
        check_invariants(st)
        outs.append(want)
        states.append({key: st[key].copy() for key in STATE})
    return outs, states


def random_stream(seed, B, N, T, P, people=6, nseq=1):
    """A tracker-like stream: persons with a fixed colour come and go, every appearance under a fresh track id in some free
    slot; the signatures are noisy copies of the person's histogram, sometimes with too few samples."""
    rng = np.random.default_rng(seed)
    base = [np.stack([rng.multinomial(40, rng.dirichlet(np.full(BINS, 0.05))) for _ in range(P)]).astype(np.int32)
            for _ in range(people)]
    fs = rng.integers(0, nseq, B) if nseq > 1 else np.zeros(B, np.int64)
    if nseq > 1:
        fs[rng.integers(0, B)] = nseq + 3                                     # a frame of no sequence
    next_id = [0] * nseq
    present = [dict() for _ in range(nseq)]                                   # person -> (track id, slot)
    dets = {}
    for b in range(B):
        s = int(fs[b])
        if not 0 <= s < nseq:
            dets[b] = [(0, 5, 0, base[0])]
            continue
        cur = present[s]
        for person in list(cur):
            if rng.random() < 0.15:
                del cur[person]
        for person in range(people):
            if person not in cur and len(cur) < N and rng.random() < 0.3:
                used = {sl for _, sl in cur.values()}
                slot = int(rng.choice([t for t in range(T) if t not in used]))
                cur[person] = (next_id[s], slot)
                next_id[s] += 1
        lst, order = [], rng.permutation(N)
        for k, (person, (tid, slot)) in enumerate(cur.items()):
            if rng.random() < 0.2:
                continue                                                      # missed in this frame: the slot coasts
            h = base[person] + rng.integers(0, 2, (P, BINS)).astype(np.int32)
            if rng.random() < 0.15:
                h = (h > 40).astype(np.int32)                                 # too few samples
            if P > 1 and rng.random() < 0.2:
                h[rng.integers(0, P)] = 0                                     # a part without samples
            lst.append((int(order[k]), tid, slot, h))
        dets[b] = lst
    return stream(B, N, P, dets, fs if nseq > 1 else None)


def chunks(call, cuts):
    """The stream split at ``cuts`` into consecutive calls."""
    edges = [0] + list(cuts) + [len(call[0])]
    return [tuple(None if x is None else x[a:e] for x in call) for a, e in zip(edges[:-1], edges[1:])]


def reid_argument_errors(lib, device):
    """Every refusal of the header, and that a refused call writes nothing: outputs and state."""
    N, T, G, P = 4, 8, 2, 2
    st = reid_init(1, T, G, P)
    h = hist(P, {1: 6}, {2: 6})
    call = stream(2, N, P, {0: [(0, 0, 0, h)], 1: [(0, 0, 0, h)]})

    def refused(want, **over):
        rc, got, pids, rstate, rsim = reid_call(lib, device, st, *call, PRM, **over)
        assert rc == want, (over, rc)
        assert same_state(got, st) and (pids == -7).all() and (rstate == -7).all() and (rsim == -7).all(), over

    for i in [0, 1, 2, 3] + list(range(5, 17)):                               # every pointer but frame_set
        refused(EINVAL, null=(i,))
    for over in (dict(B=-1), dict(N=0), dict(nseq=0), dict(G=0), dict(P=0), dict(T=N - 1), dict(max_age=-1),
                 dict(min_samples=-1), dict(gallery_max_age=-1), dict(min_frames=0), dict(window=1), dict(sim_min=NAN),
                 dict(margin=NAN)):
        refused(EINVAL, **over)
    for over in (dict(N=33, T=40), dict(T=65), dict(G=65), dict(P=5), dict(window=MAX_WINDOW + 1)):
        refused(ELIMIT, **over)
    refused(0, B=0)
    rc, got, pids, _, _ = reid_call(lib, device, st, *call, PRM, window=MAX_WINDOW)
    assert rc == 0 and (pids[:, 0] == 0).all() and not same_state(got, st)


# ======================================================================================================================
# closed loop: painted people, the evidence kernel's pixels, the tracker's ids
# ======================================================================================================================
# COCO-17 offsets (mm) from the point on the floor under a standing person: x lateral, z up
_BODY17 = np.array([[0, 0, 1650], [30, 0, 1680], [-30, 0, 1680], [70, 0, 1650], [-70, 0, 1650], [200, 0, 1400], [-200, 0, 1400],
                    [250, 0, 1100], [-250, 0, 1100], [270, 0, 850], [-270, 0, 850], [120, 0, 900], [-120, 0, 900],
                    [130, 0, 500], [-130, 0, 500], [130, 0, 100], [-130, 0, 100]], np.float64)
LOOP_MAX_AGE, LOOP_MIN_FRAMES, LOOP_SIM_MIN, LOOP_MARGIN = 3, 3, 0.7, 0.1
# colours far apart in the 2-bit bins: bins 48, 12, 3
LOOP_PALETTE = [(250, 10, 10), (10, 250, 10), (10, 10, 250)]


def closed_loop(lib, device, variant):
    """Three people painted into grey-noise frames of the Campus rig (3 views, 360 x 288, 17 joints); pixels from
    fvp_joint_evidence, ids from PoseTracker, identities from PersonReId.  ``variant`` "return": person 0 leaves for max_age +
    5 frames and returns 1.5 m from where they vanished; "twins": persons 0 and 1 wear the same colour, both leave, person 0
    returns.  ``lib``: the emulated library, or None for the shipped one.  -> a list per frame of {person: (track id, person id,
    reid_state, reid_sim)} and the frame at which person 0 returns."""
    import fvp_synthetic as S
    from faster_voxelpose_amd.core.reid import PersonReId
    from faster_voxelpose_amd.core.tracking import PoseTracker
    from faster_voxelpose_amd.engine import HotPath
    from faster_voxelpose_amd.utils.overlay import PoseOverlay
    cfg = S.make_cfg("campus", device=str(device), min_score=-1.0)
    cams, seq = S.load_cameras("campus")
    rt = S.resize_transform(cfg).to(device)
    N, J, V = cfg.CAPTURE_SPEC.MAX_PEOPLE, cfg.DATASET.NUM_JOINTS, cfg.DATASET.CAMERA_NUM
    ws, hs = cfg.DATASET.ORI_IMAGE_SIZE
    engine = HotPath(cfg, _lib=lib)
    tracker = PoseTracker(cfg, max_age=LOOP_MAX_AGE, _lib=lib)
    reid = PersonReId(cfg, gallery=4, max_age=LOOP_MAX_AGE, min_samples=32, min_frames=LOOP_MIN_FRAMES, window=16,
                      sim_min=LOOP_SIM_MIN, margin=LOOP_MARGIN, _lib=lib)
    colours = [0, 0, 2] if variant == "twins" else [0, 1, 2]
    overlay = PoseOverlay(cfg, palette=LOOP_PALETTE, alpha=1.0, limb_width=8.0, joint_radius=4.0, _lib=lib)
    away = LOOP_MAX_AGE + 5
    t_leave, t_back = 5, 5 + away
    frames_total = t_back + LOOP_MIN_FRAMES + 2
    home = np.array([[2200.0, 3800.0], [3600.0, 5200.0], [4300.0, 3600.0]])
    rng = np.random.default_rng(5)
    history = []
    for first in range(0, frames_total, 4):                                   # four frames per call, the last call fewer
        B = min(4, frames_total - first)
        fused = np.zeros((B, N, J, 5), f32)
        fused[..., 3] = -1.0
        person_of = np.full((B, N), -1, np.int64)
        for k in range(B):
            f = first + k
            order = rng.permutation(N)                                        # the NMS rank changes from frame to frame
            for person in range(3):
                gone = t_leave <= f < t_back if person == 0 else (variant == "twins" and person == 1 and f >= t_leave)
                if gone:
                    continue
                pos = home[person] + 20.0 * f
                if person == 0 and f >= t_back:
                    pos = pos + np.array([1500.0, 0.0])                       # further than gate_mm from where they vanished
                fused[k, order[person], :, :3] = _BODY17 + np.array([pos[0], pos[1], 0.0])
                fused[k, order[person], :, 3] = 0.0
                person_of[k, order[person]] = person
        fused_t = torch.from_numpy(fused).to(device)
        meta = {"seq": [seq] * B}
        heat = torch.zeros((B, V, J, cfg.DATASET.HEATMAP_SIZE[1], cfg.DATASET.HEATMAP_SIZE[0]), device=device)
        views = engine.joint_evidence(fused_t, heat, meta, cams, rt)[0]
        ids, slots, _ = tracker.update(fused_t, meta=meta)
        grey = rng.integers(96, 160, (B, V, hs, ws, 1), dtype=np.uint8).repeat(3, axis=4)
        frames = torch.from_numpy(grey).to(device)
        keys = np.where(person_of >= 0, np.array(colours + [0])[person_of], -1).astype(np.int32)
        overlay.draw(frames, views, ids=torch.from_numpy(keys).to(device))
        pids, rstate, rsim = reid(frames, views, ids, slots, meta=meta)
        assert torch.equal(reid.slot_tid, tracker.trk_id)                     # the stated consequence, after every call
        ids, pids, rstate, rsim = (x.cpu().numpy() for x in (ids, pids, rstate, rsim))
        for k in range(B):
            history.append({int(person_of[k, n]): (int(ids[k, n]), int(pids[k, n]), int(rstate[k, n]), float(rsim[k, n]))
                            for n in range(N) if person_of[k, n] >= 0})
            assert all(ids[k, n] < 0 and pids[k, n] == -1 and rstate[k, n] == -1 for n in range(N) if person_of[k, n] < 0)
    return history, t_back, reid


def closed_loop_check(lib, device, variant):
    """What the scenario must show, with the decision far from sim_min and margin on both sides (restated from the state)."""
    history, t_back, reid = closed_loop(lib, device, variant)
    decided = t_back + LOOP_MIN_FRAMES - 1
    first_tid, first_pid = history[0][0][:2]
    assert first_tid == first_pid and history[LOOP_MIN_FRAMES - 1][0][2] == 1         # a new person at min_frames
    for f in range(t_back, len(history)):
        tid, pid, state, sim = history[f][0]
        assert tid != first_tid                                                       # the tracker gave a new id
        if f < decided:
            assert (pid, state, sim) == (tid, 0, -1.0)                                # pending
        elif variant == "return":
            assert (pid, state) == (first_pid, 2) and sim >= LOOP_SIM_MIN + 0.2       # the old identity, sim - second = sim
        else:
            assert (pid, state) == (tid, 1) and sim >= LOOP_SIM_MIN + 0.2             # refused by the margin rule alone
        for other in (1, 2):                                                          # nobody else is disturbed
            if other in history[f]:
                assert history[f][other][1] == history[0][other][1] and history[f][other][2] == 1
    st = {k: v.cpu().numpy() for k, v in reid.state().items()}
    check_invariants(st)
    if variant == "twins":                                                            # both twins still wait in the gallery
        t = int(np.flatnonzero(st["slot_tid"][0] == history[-1][0][0])[0])
        entries = np.flatnonzero(st["gal_pid"][0] >= 0)
        assert len(entries) == 2
        sims = [float(similarity(st["slot_sig"][0, t].tolist(), st["gal_sig"][0, g].tolist())) for g in entries]
        assert min(sims) >= LOOP_SIM_MIN + 0.2 and abs(sims[0] - sims[1]) <= LOOP_MARGIN / 2, sims
    else:
        assert not (st["gal_pid"][0] >= 0).any()                                      # the adopted entry is gone
    return history


# ======================================================================================================================
# fvp_track_reid: every edge of the state machine on hand-made streams (SCENARIOS: name -> check(lib, device))
# ======================================================================================================================
N, T, G, P = 4, 8, 2, 2
RED, GREEN, BLUE = hist(P, {48: 8}, {48: 8}), hist(P, {12: 8}, {12: 8}), hist(P, {3: 8}, {3: 8})
WHITE = hist(P, {63: 8}, {63: 8})


def _run(lib, device, dets, B, prm=None, shape=None, frame_set=None, cuts=(), p=P):
    call = stream(B, N, p, dets, frame_set)
    return run_script(lib, device, shape or (1, T, G, p), dict(PRM, **(prm or {})), chunks(call, cuts))


def cat(outs, k):
    return np.concatenate([o[k] for o in outs])


def sc_birth_and_decision_exactly_at_min_frames(lib, device):
    outs, states = _run(lib, device, {b: [(1, 7, 2, RED)] for b in range(5)}, 5, prm=dict(min_frames=3))
    assert cat(outs, 1)[:, 1].tolist() == [0, 0, 1, 1, 1] and (cat(outs, 0)[:, 1] == 7).all()
    assert (cat(outs, 2) == -1).all()                                                 # an empty gallery: sim stays -1
    st = states[-1]
    assert st["slot_tid"][0, 2] == 7 and st["slot_pid"][0, 2] == 7 and st["slot_frames"][0, 2] == 5
    assert np.array_equal(st["slot_sig"][0, 2], 5 * RED)


def sc_min_samples_one_below_and_at_the_limit(lib, device):
    below, at = hist(P, {48: 5}, {48: 4}), hist(P, {48: 5}, {48: 5})
    dets = {0: [(0, 0, 0, below)], 1: [(0, 0, 0, at)], 2: [(0, 0, 0, below)], 3: [(0, 0, 0, at)]}
    outs, states = _run(lib, device, dets, 4, prm=dict(min_samples=10, min_frames=2))
    assert cat(outs, 1)[:, 0].tolist() == [0, 0, 0, 1] and states[-1]["slot_frames"][0, 0] == 2


def sc_retire_by_age_exactly_at_max_age_and_one_beyond(lib, device):
    dets = {0: [(0, 0, 0, RED)], 1: [(0, 0, 0, RED)]}
    for absent, kept in ((3, True), (4, False)):                                      # max_age = 3
        _, states = _run(lib, device, dets, 2 + absent, cuts=(2,))
        st = states[-1]
        assert (st["slot_tid"][0, 0] == 0) == kept and (st["gal_pid"][0, 0] == 0) == (not kept)
        if kept:
            assert st["slot_age"][0, 0] == 3
        else:
            assert np.array_equal(st["gal_sig"][0, 0], 2 * RED) and st["gal_age"][0, 0] == 0


def sc_retire_by_slot_reuse_and_a_short_track_is_forgotten(lib, device):
    dets = {0: [(0, 0, 0, RED)], 1: [(0, 0, 0, RED)], 2: [(2, 5, 0, GREEN)], 3: [(2, 6, 0, BLUE)]}
    _, states = _run(lib, device, dets, 4)
    st = states[-1]
    assert st["gal_pid"][0].tolist() == [0, -1]                                       # track 5 had one frame: forgotten
    assert st["slot_tid"][0, 0] == 6 and st["slot_frames"][0, 0] == 1 and np.array_equal(st["slot_sig"][0, 0], BLUE)


def sc_full_gallery_evicts_the_oldest_lowest_index_on_a_tie(lib, device):
    two, next_two = [(0, 0, 0, RED), (1, 1, 1, GREEN)], [(0, 2, 0, BLUE), (1, 3, 1, WHITE)]
    dets = {0: two, 1: two, 2: next_two, 3: next_two, 4: [(0, 4, 0, RED)]}           # frame 2: both retire at once, a tie
    _, states = _run(lib, device, dets, 5, prm=dict(sim_min=2.0), cuts=(3,))
    assert states[0]["gal_pid"][0].tolist() == [0, 1] and states[0]["gal_age"][0].tolist() == [0, 0]
    st = states[-1]
    assert st["gal_pid"][0].tolist() == [2, 1] and st["gal_age"][0].tolist() == [0, 2]        # entry 0 went, not entry 1
    _, states = _run(lib, device, {**dets, 5: [(0, 4, 0, RED)], 6: [(0, 9, 0, RED)]}, 7, prm=dict(sim_min=2.0))
    assert states[-1]["gal_pid"][0].tolist() == [2, 4]                                # now entry 1 was the oldest


def sc_gallery_max_age_edge(lib, device):
    dets = {0: [(0, 0, 0, RED)], 1: [(0, 0, 0, RED)], 2: [(0, 1, 0, GREEN)]}          # the entry is stored in frame 2, age 0
    for extra, kept in ((3, True), (4, False)):
        _, states = _run(lib, device, {**dets, **{3 + k: [(0, 1, 0, GREEN)] for k in range(extra)}}, 3 + extra,
                         prm=dict(gallery_max_age=3))
        st = states[-1]
        assert (st["gal_pid"][0, 0] == 0) == kept and st["gal_age"][0, 0] == (3 if kept else 0)
        assert bool(st["gal_sig"][0, 0].any()) == kept


def sc_sim_exactly_at_sim_min_and_margin_exactly_met(lib, device):
    """Slot (2,2,0,0) against the entries (2,0,2,0) and (1,0,0,3) of one part: the sims are exactly 0.5 and 0.25."""
    def p1(*v):
        return hist(1, {k: x for k, x in enumerate(v) if x})

    def up(x):
        return float(np.nextafter(f32(x), f32(1)))

    dets = {0: [(0, 0, 0, p1(2, 0, 2, 0)), (1, 1, 1, p1(1, 0, 0, 3))], 1: [], 2: [(0, 2, 0, p1(2, 2, 0, 0))]}
    for sim_min, margin, adopted in ((0.5, 0.25, True), (up(0.5), 0.25, False), (0.5, up(0.25), False), (0.25, 0.0, True)):
        prm = dict(max_age=0, min_samples=1, min_frames=1, window=4, sim_min=sim_min, margin=margin)
        outs, states = _run(lib, device, dets, 3, prm=prm, shape=(1, T, G, 1), p=1)
        pid, state, sim = int(cat(outs, 0)[2, 0]), int(cat(outs, 1)[2, 0]), float(cat(outs, 2)[2, 0])
        assert sim == 0.5 and (pid, state) == ((0, 2) if adopted else (2, 1)), (sim_min, margin)
        assert states[-1]["gal_pid"][0].tolist() == ([-1, 1] if adopted else [0, 1])


def sc_two_pending_tracks_one_entry_the_lower_slot_wins(lib, device):
    back = [(0, 1, 3, RED), (1, 2, 1, RED)]
    dets = {0: [(0, 0, 5, RED)], 1: [(0, 0, 5, RED)], 2: [], 3: [], 4: [], 5: [], 6: back, 7: back}
    outs, _ = _run(lib, device, dets, 8)
    assert cat(outs, 0)[7].tolist()[:2] == [1, 0] and cat(outs, 1)[7].tolist()[:2] == [1, 2]      # slot 1 (n = 1) took it
    assert cat(outs, 2)[7].tolist()[:2] == [-1.0, 1.0]                                # slot 3 found the gallery empty


def sc_a_part_missing_on_one_side_does_not_count(lib, device):
    legs_only, mixed = hist(P, {}, {48: 8}), hist(P, {12: 8}, {48: 8})
    dets = {0: [(0, 0, 0, RED)], 1: [(0, 0, 0, RED)], 2: [(0, 1, 0, legs_only)], 3: [(0, 1, 0, legs_only)]}
    outs, _ = _run(lib, device, dets, 4, prm=dict(max_age=0))
    assert cat(outs, 1)[3, 0] == 2 and cat(outs, 2)[3, 0] == 1.0                      # part 1 alone: a perfect match
    outs, _ = _run(lib, device, {**dets, 2: [(0, 1, 0, mixed)], 3: [(0, 1, 0, mixed)]}, 4, prm=dict(max_age=0))
    assert cat(outs, 1)[3, 0] == 1 and cat(outs, 2)[3, 0] == 0.5                      # both parts count: (0 + 1) / 2


def sc_halving_at_window(lib, device):
    h = hist(P, {48: 5}, {12: 3})
    _, states = _run(lib, device, {b: [(0, 0, 0, h)] for b in range(7)}, 7, prm=dict(window=4), cuts=range(1, 7))
    assert [int(s["slot_frames"][0, 0]) for s in states] == [1, 2, 3, 4, 3, 4, 3]
    assert [int(s["slot_sig"][0, 0, 0, 48]) for s in states] == [5, 10, 15, 20, 15, 20, 15]
    assert [int(s["slot_sig"][0, 0, 1, 12]) for s in states] == [3, 6, 9, 12, 9, 12, 9]


def sc_two_interleaved_sequences_and_a_frame_of_no_sequence(lib, device):
    dets = {b: [(0, 0, 0, RED if b % 2 == 0 else GREEN)] for b in range(8)}
    dets[4] = [(0, 9, 0, BLUE)]                                                       # frame 4 belongs to no sequence
    outs, states = _run(lib, device, dets, 8, shape=(2, T, G, P), frame_set=[0, 1, 0, 1, 7, 1, 0, -1])
    assert cat(outs, 1)[:, 0].tolist() == [0, 0, 1, 1, -1, 1, 1, -1] and cat(outs, 0)[4, 0] == -1
    st = states[-1]
    assert np.array_equal(st["slot_sig"][0, 0], 3 * RED) and np.array_equal(st["slot_sig"][1, 0], 3 * GREEN)


SCENARIOS = {k[3:]: v for k, v in sorted(globals().items()) if k.startswith("sc_")}
RANDOM_STREAMS = [(0, 4, 4, 1, 1, 1), (1, 4, 8, 2, 2, 1), (2, 4, 8, 4, 4, 2), (3, 10, 20, 4, 2, 1), (4, 4, 4, 2, 4, 2)]


def random_stream_check(lib, device, seed, n, t, g, p, nseq):
    """A tracker-like stream of 40 frames in calls of B = 1, 3, 8 and others: outputs, state and invariants after every call;
    then B = 8 in one call against 3 + 5, and the whole stream in one call against the chunks."""
    def ibits(a):
        return np.ascontiguousarray(a).view(np.int32)

    shape = (nseq, t, g, p)
    call = random_stream(seed, 40, n, t, p, nseq=nseq)
    outs, states = run_script(lib, device, shape, PRM, chunks(call, [1, 4, 12, 15, 20, 28, 36]))
    assert {1, 2} <= set(cat(outs, 1).reshape(-1).tolist())                           # new people and returning ones
    head = tuple(None if x is None else x[:8] for x in call)
    whole, st_whole = run_script(lib, device, shape, PRM, [head])
    split, st_split = run_script(lib, device, shape, PRM, chunks(head, [3]))
    assert same_state(st_whole[-1], st_split[-1])
    once, st_once = run_script(lib, device, shape, PRM, [call])
    assert same_state(st_once[-1], states[-1])
    for k in range(3):
        assert np.array_equal(ibits(whole[0][k]), ibits(cat(split, k)))
        assert np.array_equal(ibits(once[0][k]), ibits(cat(outs, k)))
