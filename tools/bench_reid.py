#!/usr/bin/env python
"""Person re-identification (fvp_person_signature + fvp_track_reid): the two launches, HIP-event timed, next to
the route a user has without them - the pixels, ids and slots through ``.cpu()``, the sample positions in numpy, the sampled
frame bytes gathered on the device and copied to the host, histograms and the gallery in numpy / Python, the person ids back
to the device - alternating window by window in the same job.  Input sets rotate (people on seeded random walks in the image,
two of the slots of every frame invalid, one person replaced by a new track every few frames), so both routes do real work in
every call.

The host route is the definition of include/fvp.h written the way a user would write it (the state machine is the numpy
restatement the tests use).  It is checked against the kernels' signatures and person ids on the first rotation before anything
is timed."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import reid_cases as RC  # noqa: E402
from faster_voxelpose_amd.core.reid import PersonReId  # noqa: E402

f32 = np.float32


def make_inputs(sets, B, V, N, J, hs, ws, seed=1):
    """``sets`` consecutive batches of one scene: N - 2 people on random walks in the image, a skeleton of J joints around each
    root, slot order permuted per frame; every 5th frame the oldest track is replaced by a new one in its slot."""
    rng = np.random.default_rng(seed)
    P = N - 2
    roots = rng.uniform([0.2 * ws, 0.2 * hs], [0.8 * ws, 0.8 * hs], size=(V, P, 2))
    skel = rng.uniform(-0.12 * hs, 0.12 * hs, size=(V, P, J, 2))
    tid = list(range(P))
    next_id, frame = P, 0
    out = []
    for _ in range(sets):
        views = np.zeros((B, V, N, J, 4), f32)
        ids, slots = np.full((B, N), -1, np.int32), np.full((B, N), -1, np.int32)
        for b in range(B):
            frame += 1
            if frame % 5 == 0:
                tid[(frame // 5) % P] = next_id
                next_id += 1
            roots = roots + rng.normal(0.0, 2.0, size=roots.shape)
            order = rng.permutation(N)[:P]
            views[b][:, order, :, :2] = (roots[:, :, None, :] + skel).astype(f32)
            views[b][:, order, :, 2] = 3000.0
            views[b][:, order, :, 3] = 0.5
            ids[b, order], slots[b, order] = tid, np.arange(P)
        out.append((views, ids, slots))
    return out


class HostRoute:
    """What a user writes without the two calls."""

    def __init__(self, reid, hs, ws):
        self.r, self.hs, self.ws = reid, hs, ws
        self.limbs = np.array(reid.limbs)
        self.part = np.array(reid.limb_part)
        self.t = ((np.arange(reid.K).astype(f32) + f32(0.5)) / f32(reid.K))[None, None, None, None, :]
        self.st = RC.reid_init(reid.nseq, reid.T, reid.G, reid.P)
        self.prm = dict(max_age=reid.max_age, min_samples=reid.min_samples, min_frames=reid.min_frames, window=reid.window,
                        sim_min=reid.sim_min, margin=reid.margin, gallery_max_age=reid.gallery_max_age)

    def __call__(self, frames, views_dev, ids_dev, slots_dev):
        views, ids, slots = views_dev.cpu().numpy(), ids_dev.cpu().numpy(), slots_dev.cpu().numpy()       # synchronising copies
        B, V, N, J = views.shape[:4]
        P, L = self.r.P, len(self.limbs)
        ok = (views[..., 2] > 0) & (np.abs(views[..., 0]) <= 32768) & (np.abs(views[..., 1]) <= 32768)
        a, e = views[:, :, :, self.limbs[:, 0]], views[:, :, :, self.limbs[:, 1]]                         # [B,V,N,L,4]
        both = ok[:, :, :, self.limbs[:, 0]] & ok[:, :, :, self.limbs[:, 1]] & (ids >= 0)[:, None, :, None]
        x = a[..., 0:1] + self.t * (e[..., 0:1] - a[..., 0:1])
        y = a[..., 1:2] + self.t * (e[..., 1:2] - a[..., 1:2])
        xi, yi = np.rint(x).astype(np.int64), np.rint(y).astype(np.int64)                                 # [B,V,N,L,K]
        take = both[..., None] & (xi >= 0) & (xi < self.ws) & (yi >= 0) & (yi < self.hs)
        f = (np.arange(B)[:, None] * V + np.arange(V)[None, :])[:, :, None, None, None]
        flat = ((f * self.hs + yi) * self.ws + xi)[take]
        px = frames.view(-1, 3)[torch.from_numpy(flat).to(frames.device)].cpu().numpy()                  # the sampled bytes
        bins = (px[:, 0] >> 6).astype(np.int64) * 16 + (px[:, 1] >> 6) * 4 + (px[:, 2] >> 6)
        bb = np.broadcast_to(np.arange(B)[:, None, None, None, None], take.shape)[take]
        nn = np.broadcast_to(np.arange(N)[None, None, :, None, None], take.shape)[take]
        pp = np.broadcast_to(self.part[None, None, None, :, None], take.shape)[take]
        sig = np.bincount(((bb * N + nn) * P + pp) * RC.BINS + bins, minlength=B * N * P * RC.BINS)
        sig = sig.reshape(B, N, P, RC.BINS).astype(np.int32)
        cnt = sig.sum(axis=3).astype(np.int32)
        return sig, RC.reid_reference(self.st, ids, slots, sig, cnt, None, self.prm)


def window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(iters):
        fn(i)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters * 1e3           # us per call


def main(args):
    dev = "cuda:0"
    B, V, N, J, hs, ws = args.batch, args.views, args.people, args.joints, args.height, args.width
    sets = [tuple(torch.from_numpy(x).to(dev) for x in s) for s in make_inputs(args.inputs, B, V, N, J, hs, ws)]
    gen = torch.Generator(device=dev).manual_seed(3)
    frames = [torch.randint(0, 256, (B, V, hs, ws, 3), generator=gen, dtype=torch.uint8, device=dev) for _ in range(2)]
    reid = PersonReId((N, J), max_tracks=args.tracks, samples=args.samples, device=dev)
    host = HostRoute(reid, hs, ws)
    for i in range(args.inputs):                     # the same signatures and person ids by both routes before anything is timed
        views, ids, slots = sets[i]
        sig, cnt = reid.signature(frames[i % 2], views, ids=ids)
        pids = reid.update(ids, slots, sig, cnt)[0]
        want_sig, want = host(frames[i % 2], views, ids, slots)
        assert np.array_equal(sig.cpu().numpy(), want_sig), f"the host route and the signature kernel disagree in rotation {i}"
        assert np.array_equal(pids.cpu().numpy(), want[0]), f"the host route and the re-ID kernel disagree in rotation {i}"
    held = {}
    pids_dev = torch.empty((B, N), dtype=torch.int32, device=dev)

    def k_sig(i):
        views, ids, _ = sets[i % args.inputs]
        held["sig"] = reid.signature(frames[i % 2], views, ids=ids)

    def k_reid(i):
        _, ids, slots = sets[i % args.inputs]
        reid.update(ids, slots, *held["sig"])

    def k_both(i):
        views, ids, slots = sets[i % args.inputs]
        reid(frames[i % 2], views, ids, slots)

    def h(i):
        views, ids, slots = sets[i % args.inputs]
        pids_dev.copy_(torch.from_numpy(host(frames[i % 2], views, ids, slots)[1][0]), non_blocking=True)

    for i in range(args.warmup):
        k_sig(i)
        k_reid(i)
        k_both(i)
        h(i)
    torch.cuda.synchronize()
    res = {"sig": [], "reid": [], "both": [], "host": []}
    for _ in range(args.repeats):                    # alternating windows: every route sees the same clocks
        res["sig"].append(window(k_sig, args.iters))
        res["reid"].append(window(k_reid, args.iters))
        res["both"].append(window(k_both, args.iters))
        res["host"].append(window(h, args.host_iters))
    print(torch.cuda.get_device_name(0))
    print(f"== B = {B} frames x V = {V} views x N = {N} slots ({N - 2} people) x J = {J} joints, {len(reid.limbs)} limbs x K = "
          f"{reid.K} samples = {B * V * (N - 2) * len(reid.limbs) * reid.K} samples per call at most, frames {ws} x {hs}; T = "
          f"{reid.T} track slots, G = {reid.G} gallery entries, P = {reid.P} parts; {args.inputs} input sets in rotation; "
          f"{args.warmup} warm-up calls, median / min / max over {args.repeats} windows of {args.iters} calls "
          f"({args.host_iters} for the host route)")
    for key, label in (("sig", "fvp_person_signature (k_person_signature, one launch, no host sync)"),
                       ("reid", "fvp_track_reid (k_track_reid, one launch, no host sync)"),
                       ("both", "PersonReId.__call__: both launches"),
                       ("host", "views / ids / slots .cpu() + numpy sampling + device gather .cpu() + host gallery + pids back")):
        v = res[key]
        print(f"{label:100s} {statistics.median(v):9.1f} us  (min {min(v):.1f}, max {max(v):.1f})")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--views", type=int, default=5)
    ap.add_argument("--people", type=int, default=10)
    ap.add_argument("--tracks", type=int, default=20)
    ap.add_argument("--joints", type=int, default=15)
    ap.add_argument("--samples", type=int, default=8)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--inputs", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--host-iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=10)
    main(ap.parse_args())
