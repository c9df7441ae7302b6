#!/usr/bin/env python
"""Track smoother (fvp_track_smooth): the launch alone, HIP-event timed, next to the route a user had
before - ``fused_poses.cpu()`` (with ids and slots), the same One-Euro filter on the host in numpy, the result copied back
to the device - alternating window by window in the same job.  Pose sets rotate (people on seeded random walks, two of the
slots of every frame invalid, slot order permuted); the ids / slots of every set come from a ``PoseTracker`` run over the
rotation before anything is timed, and a fifth of the joints lies below ``conf_min`` so both branches of the filter run.

The host route is the definition of include/fvp.h written the way a user would write it: one track slot at a time,
vectorised over its joints.  It is checked against the kernel's output, bit for bit, on the first rotation.

--headline [bench.py arguments]: run bench.py's own measurement with a ``PoseTracker`` and a ``PoseSmoother`` attached
(bench.py itself is not changed: FV.get and PipelinedForward are wrapped for this process).  A model that runs plain or
graphed forwards carries them as ``model.tracker`` / ``model.smoother``; a model handed to a pipeline gives them up, and the
pipeline calls ``tracker.update`` and ``smoother.update`` on a consumer stream of its own, in submit order, behind each
batch's event - the usage INTEGRATION.md documents."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_track import make_poses, window  # noqa: E402
from faster_voxelpose_amd.core.smoothing import PoseSmoother  # noqa: E402
from faster_voxelpose_amd.core.tracking import PoseTracker  # noqa: E402
from faster_voxelpose_amd.models import faster_voxelpose as FV  # noqa: E402

F32 = np.float32


class HostSmoother:
    """The host loop a user writes today: numpy, fp32, one frame and one track slot after the other."""

    def __init__(self, sm):
        self.T, self.J, self.max_age = sm.T, sm.J, sm.max_age
        self.rate, self.min_cutoff, self.beta = F32(sm.rate_hz), F32(sm.min_cutoff), F32(sm.beta)
        self.d_cutoff, self.conf_min, self.damp = F32(sm.d_cutoff), F32(sm.conf_min), F32(sm.damp)
        self.x = np.zeros((sm.T, sm.J, 3), F32)
        self.v = np.zeros((sm.T, sm.J, 3), F32)
        self.id = np.full(sm.T, -1, np.int32)
        self.age = np.zeros(sm.T, np.int32)
        self.big = np.finfo(F32).max

    def alpha(self, fc):
        r = (F32(6.2831855) * fc) / self.rate
        return r / (r + F32(1.0))

    def update(self, poses, ids, slots, conf):
        B = poses.shape[0]
        smooth = poses.copy()
        dt, a_d = F32(1.0) / self.rate, self.alpha(self.d_cutoff)
        with np.errstate(all="ignore"):
            for b in range(B):
                seen = np.zeros(self.T, bool)
                for n in np.flatnonzero(ids[b] >= 0):
                    t = int(slots[b, n])
                    seen[t] = True
                    m, x, v = poses[b, n, :, :3], self.x[t], self.v[t]
                    self.age[t] = 0
                    if self.id[t] != ids[b, n]:
                        self.id[t] = ids[b, n]
                        x[:] = m
                        v[:] = 0
                    else:
                        e = m - x
                        meas = (conf[b, n] >= self.conf_min) & (np.abs(e) <= self.big).all(axis=1)
                        vm = v + a_d * (e * self.rate - v)
                        sp = np.sqrt((vm[:, 0] * vm[:, 0] + vm[:, 1] * vm[:, 1]) + vm[:, 2] * vm[:, 2])
                        a = self.alpha(self.min_cutoff + self.beta * sp)
                        vp = v * self.damp
                        xp = x + vp * dt
                        xm = x + a[:, None] * e
                        v[:] = np.where(meas[:, None], vm, vp)
                        x[:] = np.where(meas[:, None], xm, xp)
                    smooth[b, n, :, :3] = x
                for t in np.flatnonzero(~seen & (self.id >= 0)):
                    self.age[t] += 1
                    if self.age[t] > self.max_age:
                        self.id[t], self.age[t] = -1, 0
                    else:
                        self.v[t] = self.v[t] * self.damp
                        self.x[t] = self.x[t] + self.v[t] * dt
        return smooth


def kernel_bench(args):
    dev = "cuda:0"
    B, N, J, T = args.batch, args.people, args.joints, args.tracks
    sets = make_poses(args.inputs, B, N, J)
    rng = np.random.default_rng(2)
    poses = [torch.from_numpy(x).to(dev) for x in sets]
    conf = [torch.from_numpy(rng.uniform(0.0, 1.0, size=(B, N, J)).astype(F32)).to(dev) for _ in sets]
    trk = PoseTracker((N, J), max_tracks=T, device=dev)
    sm = PoseSmoother(trk, conf_min=0.2)
    host = HostSmoother(sm)
    tracks = []
    for i in range(args.inputs):                     # same filtered poses by both routes before anything is timed
        ids, slots, _ = trk.update(poses[i])
        tracks.append((ids, slots))
        got = sm.update(poses[i], ids, slots, joint_conf=conf[i])[0].cpu().numpy()
        want = host.update(sets[i], ids.cpu().numpy(), slots.cpu().numpy(), conf[i].cpu().numpy())
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), f"the host route and the kernel disagree in rotation {i}"
    out_dev = torch.empty((B, N, J, 5), device=dev)

    def k(i):
        r = i % args.inputs
        sm.update(poses[r], tracks[r][0], tracks[r][1], joint_conf=conf[r])

    def h(i):
        r = i % args.inputs
        x = poses[r].cpu().numpy()                   # the synchronising copies
        out_dev.copy_(torch.from_numpy(host.update(x, tracks[r][0].cpu().numpy(), tracks[r][1].cpu().numpy(),
                                                   conf[r].cpu().numpy())), non_blocking=True)

    for i in range(args.warmup):
        k(i)
        h(i)
    torch.cuda.synchronize()
    ks, hs = [], []
    for _ in range(args.repeats):                    # alternating windows: both routes see the same clocks
        ks.append(window(k, args.iters))
        hs.append(window(h, args.host_iters))
    print(torch.cuda.get_device_name(0))
    print(f"== B = {B} frames x N = {N} slots x T = {T} track slots x J = {J} joints = {T * J} filters walking {B} frames, "
          f"{args.inputs} pose sets in rotation ({N - 2} people on random walks, 2 invalid slots per frame, a fifth of the joints "
          f"below conf_min); {args.warmup} warm-up calls, median / min / max over {args.repeats} windows of {args.iters} calls "
          f"({args.host_iters} for the host route)")
    print(f"fvp_track_smooth (k_track_smooth, one launch, no host sync)                  {statistics.median(ks):9.1f} us  "
          f"(min {min(ks):.1f}, max {max(ks):.1f})")
    print(f"poses / ids / slots / conf .cpu() + numpy One-Euro filter + poses to the device {statistics.median(hs):9.1f} us  "
          f"(min {min(hs):.1f}, max {max(hs):.1f})")


def headline(rest):
    import bench
    orig_get, orig_init, orig_submit = FV.get, FV.PipelinedForward.__init__, FV.PipelinedForward.submit

    def get(cfg):
        m = orig_get(cfg)
        m.tracker = PoseTracker(cfg)
        m.smoother = PoseSmoother(m.tracker)
        return m

    def pipe_init(self, model, *a, **kw):
        # batches on several streams: tracker and smoother move from the model to a consumer stream beside the pipeline
        self._tracker, model.tracker = model.tracker, None
        self._smoother, model.smoother = model.smoother, None
        self._consumer = torch.cuda.Stream(device=model.device)
        orig_init(self, model, *a, **kw)

    def submit(self, **kw):
        out, ev = orig_submit(self, **kw)
        if self._tracker is not None:
            with torch.cuda.stream(self._consumer):  # submit order, after the batch's event: INTEGRATION.md
                ev.wait()
                self.consume(out)
                ids, slots, _ = self._tracker.update(out[0], kw["meta"])
                self._smoother.update(out[0], ids, slots, meta=kw["meta"])
        return out, ev
    FV.get = get
    FV.PipelinedForward.__init__ = pipe_init
    FV.PipelinedForward.submit = submit
    sys.argv = ["bench.py"] + rest
    bench.main()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--headline", action="store_true")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--people", type=int, default=10)
    ap.add_argument("--tracks", type=int, default=20)
    ap.add_argument("--joints", type=int, default=15)
    ap.add_argument("--inputs", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--host-iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=20)
    a, rest = ap.parse_known_args()
    headline(rest) if a.headline else kernel_bench(a)
