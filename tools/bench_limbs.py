#!/usr/bin/env python
"""Limb model (fvp_limb_learn + fvp_limb_fit): the two launches alone, HIP-event timed, next to the route a
user had before - ``fused_poses.cpu()`` (with ids, slots and joint_conf), the same running lengths and the same Gauss-Seidel
fit on the host in numpy, the fitted poses copied back to the device - alternating window by window in the same job.  Pose
sets rotate (people on seeded random walks, two of the slots of every frame invalid, slot order permuted); the ids / slots of
every set come from a ``PoseTracker`` run over the rotation before anything is timed, and a fifth of the joints lies below
``conf_min`` so every branch of both kernels runs.

The host route is the definition of include/fvp.h written the way a user would write it: the learner one person at a time,
vectorised over the limbs; the fit one limb at a time, vectorised over the people.  It equals the definition bit for bit
(tests/test_limb_emu.py checks it on the CPU) and is checked against the kernels' output on the first rotation."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402

F32 = np.float32


class HostLimbs:
    """The host loops a user writes today: numpy, fp32."""

    def __init__(self, lm):
        self.T, self.J, self.L = lm.T, lm.J, lm.L
        self.i = np.array([a for a, _ in lm.limbs])
        self.k = np.array([b for _, b in lm.limbs])
        self.conf_min, self.gate_sigma, self.gate_mm = F32(lm.conf_min), F32(lm.gate_sigma), F32(lm.gate_mm)
        self.min_frames, self.window, self.relearn = lm.min_frames, lm.window, lm.relearn
        self.stiffness, self.iters = F32(lm.stiffness), lm.iters
        self.len = np.zeros((lm.T, lm.L), F32)
        self.var = np.zeros((lm.T, lm.L), F32)
        self.cnt = np.zeros((lm.T, lm.L), np.int32)
        self.out = np.zeros((lm.T, lm.L), np.int32)
        self.id = np.full(lm.T, -1, np.int32)
        self.big = np.finfo(F32).max

    def supported(self, xyz, conf):
        return (conf >= self.conf_min) & (np.abs(xyz) <= self.big).all(axis=-1)

    @staticmethod
    def norm(d):
        return np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])

    def learn(self, poses, ids, slots, conf):
        B, N = ids.shape
        target = np.zeros((B, N, self.L), F32)
        with np.errstate(all="ignore"):
            for b in range(B):
                for n in np.flatnonzero(ids[b] >= 0):
                    t = int(slots[b, n])
                    if self.id[t] != ids[b, n]:
                        self.id[t] = ids[b, n]
                        self.len[t], self.var[t], self.cnt[t], self.out[t] = 0, 0, 0, 0
                    x = poses[b, n, :, :3]
                    m = self.supported(x, conf[b, n])
                    d = self.norm(x[self.k] - x[self.i])
                    ln, var, cnt, out = self.len[t], self.var[t], self.cnt[t], self.out[t]
                    meas = m[self.i] & m[self.k] & (d > 0) & (d <= self.big)
                    e = d - ln
                    tol = np.fmax(self.gate_sigma * np.sqrt(var), self.gate_mm)
                    ok = meas & ((cnt < self.min_frames) | (np.abs(e) <= tol))
                    bad = meas & ~ok
                    redo = bad & (out + 1 > self.relearn)
                    c = np.minimum(cnt + 1, self.window)
                    g = F32(1.0) / c.astype(F32)
                    ln2 = ln + g * e
                    var2 = var + g * (e * (d - ln2) - var)
                    self.len[t] = np.where(ok, ln2, np.where(redo, d, ln))
                    self.var[t] = np.where(ok, var2, np.where(redo, F32(0), var))
                    self.cnt[t] = np.where(ok, c, np.where(redo, 1, cnt))
                    self.out[t] = np.where(ok | redo, 0, np.where(bad, out + 1, out))
                    target[b, n] = np.where(self.cnt[t] >= self.min_frames, self.len[t], F32(0))
        return target

    def fit(self, poses, target, ids, conf):
        fitted = poses.copy()
        valid = (poses[:, :, 0, 3] >= 0) & (ids >= 0)
        y = poses[valid][:, :, :3].copy()                         # [P,J,3]
        m = self.supported(y, conf[valid])                        # [P,J]
        tg = target[valid]
        half, zero, one = F32(0.5), F32(0), F32(1)
        with np.errstate(all="ignore"):
            for _ in range(self.iters):
                for l in range(self.L):
                    i, k = self.i[l], self.k[l]
                    dl = y[:, k] - y[:, i]
                    d = self.norm(dl)
                    act = (tg[:, l] > 0) & (d > 0) & (d <= self.big)
                    sc = (self.stiffness * (d - tg[:, l])) / d
                    wi = np.where(m[:, i] == m[:, k], half, np.where(m[:, i], zero, one))
                    wk = np.where(m[:, i] == m[:, k], half, np.where(m[:, i], one, zero))
                    yi = y[:, i] + (wi * sc)[:, None] * dl
                    yk = y[:, k] - (wk * sc)[:, None] * dl
                    y[:, i] = np.where(act[:, None], yi, y[:, i])
                    y[:, k] = np.where(act[:, None], yk, y[:, k])
        out = fitted[valid]
        out[:, :, :3] = y
        fitted[valid] = out
        return fitted

    def __call__(self, poses, ids, slots, conf):
        return self.fit(poses, self.learn(poses, ids, slots, conf), ids, conf)


def kernel_bench(args):
    import torch

    from bench_track import make_poses, window
    from faster_voxelpose_amd.core.skeleton import LimbModel
    from faster_voxelpose_amd.core.tracking import PoseTracker
    dev = "cuda:0"
    B, N, J, T = args.batch, args.people, args.joints, args.tracks
    sets = make_poses(args.inputs, B, N, J)
    rng = np.random.default_rng(2)
    for x in sets:                                   # 5 mm jitter: the lengths breathe, the gate and the fit have work
        x[..., :3] += rng.normal(0.0, 5.0, size=x[..., :3].shape).astype(F32)
    poses = [torch.from_numpy(x).to(dev) for x in sets]
    conf = [torch.from_numpy(rng.uniform(0.0, 1.0, size=(B, N, J)).astype(F32)).to(dev) for _ in sets]
    trk = PoseTracker((N, J), max_tracks=T, device=dev)
    lm = LimbModel(trk, conf_min=0.2)
    host = HostLimbs(lm)
    tracks = []
    for i in range(args.inputs):                     # same fitted poses by both routes before anything is timed
        ids, slots, _ = trk.update(poses[i])
        tracks.append((ids, slots))
        got = lm(poses[i], ids, slots, joint_conf=conf[i])[0].cpu().numpy()
        want = host(sets[i], ids.cpu().numpy(), slots.cpu().numpy(), conf[i].cpu().numpy())
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), f"the host route and the kernels disagree in rotation {i}"
    out_dev = torch.empty((B, N, J, 5), device=dev)

    def k(i):
        r = i % args.inputs
        lm(poses[r], tracks[r][0], tracks[r][1], joint_conf=conf[r])

    def h(i):
        r = i % args.inputs
        x = poses[r].cpu().numpy()                   # the synchronising copies
        out_dev.copy_(torch.from_numpy(host(x, tracks[r][0].cpu().numpy(), tracks[r][1].cpu().numpy(), conf[r].cpu().numpy())),
                      non_blocking=True)

    for i in range(args.warmup):
        k(i)
        h(i)
    torch.cuda.synchronize()
    ks, hs = [], []
    for _ in range(args.repeats):                    # alternating windows: both routes see the same clocks
        ks.append(window(k, args.iters))
        hs.append(window(h, args.host_iters))
    print(torch.cuda.get_device_name(0))
    print(f"== B = {B} frames x N = {N} slots x T = {T} track slots x J = {J} joints, L = {lm.L} limbs: {T * lm.L} learners "
          f"walking {B} frames, {B * N} fits of {lm.iters} sweeps; {args.inputs} pose sets in rotation ({N - 2} people on random "
          f"walks with 5 mm jitter, 2 invalid slots per frame, a fifth of the joints below conf_min); {args.warmup} warm-up calls, "
          f"median / min / max over {args.repeats} windows of {args.iters} calls ({args.host_iters} for the host route)")
    print(f"fvp_limb_learn + fvp_limb_fit (two launches, no host sync)                             {statistics.median(ks):9.1f} us  "
          f"(min {min(ks):.1f}, max {max(ks):.1f})")
    print(f"poses / ids / slots / conf .cpu() + numpy lengths and fit + fitted poses to the device {statistics.median(hs):9.1f} us  "
          f"(min {min(hs):.1f}, max {max(hs):.1f})")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--people", type=int, default=10)
    ap.add_argument("--tracks", type=int, default=20)
    ap.add_argument("--joints", type=int, default=15)
    ap.add_argument("--inputs", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--host-iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=20)
    kernel_bench(ap.parse_args())
