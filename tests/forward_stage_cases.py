"""One forward with every optional stage set, on the tiny configuration through the CPU emulation of the kernels: the
scenario shared by tests/test_forward_stages.py and tests/golden/make_forward_stage_launches.py (which records the
kernel-name sequence of a warm forward into tests/golden/forward_stage_launches.json)."""
import ctypes as C
import os

import torch

import fvp_synthetic as FS
import overlay_nv12_cases as NC
from faster_voxelpose_amd.core.smoothing import PoseSmoother
from faster_voxelpose_amd.core.tracking import PoseTracker
from faster_voxelpose_amd.models import faster_voxelpose as FV
from faster_voxelpose_amd.utils.crops import PersonCrops
from faster_voxelpose_amd.utils.overlay import PoseOverlay
from faster_voxelpose_amd.utils.recalibrate import CameraRefiner
from faster_voxelpose_amd.utils.triangulate import JointTriangulator
from faster_voxelpose_amd.utils.visibility import JointVisibility

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "forward_stage_launches.json")
KINDS = ("rgb", "nv12")                                  # the entries of the golden file, in this order
TINY_LIMBS = [(0, 1), (1, 2), (2, 3), (3, 4)]            # the tiny configuration has 5 joints: no default skeleton
B = 2


def launches(lib, fn):
    lib.hipemu_launch_log.restype = C.c_char_p
    lib.hipemu_launch_log_reset()
    out = fn()
    return out, lib.hipemu_launch_log().decode().split()


def stages(cfg, lib, nv12):
    """Fresh stage objects with the scenario's parameters, by model attribute name."""
    tracker = PoseTracker(cfg, _lib=lib)
    return dict(visibility=JointVisibility(cfg, prims=TINY_LIMBS, radius=80.0, spheres={0: 120.0}, _lib=lib),
                triangulator=JointTriangulator(cfg, radius=8, min_peak=0.0, _lib=lib),
                recalibrator=CameraRefiner(cfg, huber_px=4.0, _lib=lib),
                tracker=tracker, smoother=PoseSmoother(tracker, conf_min=0.3),
                crops=PersonCrops(cfg, size=(8, 6), min_joints=1, _lib=lib),
                overlay=PoseOverlay(cfg, limbs=TINY_LIMBS, alpha=0.5, nv12=nv12, _lib=lib))


class Scenario:
    """The model with all stages set, a stub torch backbone and B = 2 camera frames: uint8 RGB, or an NV12 surface."""

    def __init__(self, lib, kind):
        self.lib, self.nv12 = lib, kind == "nv12"
        self.cfg = cfg = FS.make_cfg("tiny", device="cpu", min_score=-1.0)
        self.cams, seq = FS.load_cameras("tiny")
        self.rt = FS.resize_transform(cfg)
        self.meta = {"seq": [seq] * B}
        ws, hs = cfg.DATASET.ORI_IMAGE_SIZE
        J, V = cfg.DATASET.NUM_JOINTS, cfg.DATASET.CAMERA_NUM
        if self.nv12:
            self.surface = NC.Surface(B, V, hs, ws, standard=1, seed=70)
            self.pristine = [torch.from_numpy(b.copy()) for b in self.surface.bufs]
        else:
            self.pristine = [torch.randint(0, 256, (B, V, hs, ws, 3), dtype=torch.uint8,
                                           generator=torch.Generator().manual_seed(5))]
        self.bufs = [t.clone() for t in self.pristine]
        self.frames = self.as_frames(self.bufs)

        class Stub(torch.nn.Module):
            def forward(self, x):
                pooled = torch.nn.functional.avg_pool2d(x, 4).mean(dim=1, keepdim=True)
                return pooled.expand(-1, J, -1, -1).contiguous()

        self.model = model = FV.FasterVoxelPoseNet(cfg, _lib=lib)
        model.load_state_dict(FS.fill_state_dict(model.state_dict(), seed=7))
        model.evidence = True
        for name, stage in stages(cfg, lib, self.nv12).items():
            setattr(model, name, stage)
        self.kw = dict(backbone=Stub(), meta=self.meta, cameras=self.cams, resize_transform=self.rt)

    def as_frames(self, bufs):
        return NC.nv12_frames(self.surface, bufs) if self.nv12 else bufs[0]

    def restore(self):
        """Clean frames and fresh state, so that the next forward is the first one its stateful stages see."""
        for t, b in zip(self.bufs, self.pristine):
            t.copy_(b)
        self.model.tracker.reset()
        self.model.smoother.reset()
        self.model.recalibrator.reset()

    def forward(self):
        with torch.no_grad():
            return self.model(views=self.frames, **self.kw)

    def warm_launches(self):
        """The kernel names of one warm forward (the first packs the weights and fills the caches)."""
        self.forward()
        self.restore()
        return launches(self.lib, self.forward)
