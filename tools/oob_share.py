#!/usr/bin/env python
"""Share of back-projection samples that cannot contribute: (voxel, view) pairs whose four bilinear taps all lie outside
the view's heat map (floor(ix) + 1 < 0, floor(ix) > W - 1, or the same in y).  The fused projection kernels skip them
(fvp_project_lds.h, tap_contributes); this counts how many there are.  CPU only: the committed camera fixtures and the
oracle's own sampling grid (build_sample_grids), no library.

    python tools/oob_share.py [--config panoptic shelf campus] [--stride 4 4 2]
        the whole fine grid of the joint stage (every window is a box of it), subsampled by --stride
    python tools/oob_share.py --config panoptic --dump DIR [--window-stride 2 2 2]
        additionally the person windows of a `bench.py --config panoptic --dump-outputs DIR` run: proposal_centers.npy
        through the oracle's person_boxes; the share over the in-window samples of all valid proposals, and per view

A property of the rig (no camera sees the whole capture space) and of where the people stand, not of the heat maps."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)
import fvp_oracle as O  # noqa: E402
import fvp_synthetic as S  # noqa: E402


def no_tap_inside(grid, W, H):
    """grid [..., 2] -> bool [...]: pixel coordinates as oracle.bilinear_mean forms them."""
    ix = (grid[..., 0] + 1) * ((W - 1) / 2)
    iy = (grid[..., 1] + 1) * ((H - 1) / 2)
    x0, y0 = torch.floor(ix), torch.floor(iy)
    return (x0 + 1 < 0) | (x0 > W - 1) | (y0 + 1 < 0) | (y0 > H - 1)


def axis_points(spec, lo, hi, stride):
    ax = [spec.fine_axes[a][int(lo[a]):int(hi[a]):stride[a]] for a in range(3)]
    mx, my, mz = torch.meshgrid(*ax, indexing="ij")
    return torch.stack([mx.reshape(-1), my.reshape(-1), mz.reshape(-1)], dim=1)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", nargs="+", default=["panoptic", "shelf", "campus"])
    ap.add_argument("--stride", nargs=3, type=int, default=[4, 4, 2], help="subsampling of the whole fine grid")
    ap.add_argument("--dump", default=None, help="directory written by bench.py --dump-outputs (one config)")
    ap.add_argument("--window-stride", nargs=3, type=int, default=[2, 2, 2], help="subsampling inside the person windows")
    args = ap.parse_args()
    assert args.dump is None or len(args.config) == 1, "--dump belongs to one config"
    for name in args.config:
        cfg = S.make_cfg(name)
        cams_all, seq = S.load_cameras(name)
        cams = [cams_all[seq][i] for i in range(cfg.DATASET.CAMERA_NUM)]
        rt = S.resize_transform(cfg)
        W, H = cfg.DATASET.HEATMAP_SIZE
        spec = O.IndividualSpec(cfg)
        fine = [int(v) for v in spec.fine]
        out = no_tap_inside(O.build_sample_grids(axis_points(spec, [0, 0, 0], fine, args.stride), cams, cfg, rt), W, H)
        per_view = out.float().mean(dim=1)
        print("%-12s fine grid %s, stride %s: no tap inside %.1f %% of (voxel, view) samples; per view %s" % (
            name, fine, args.stride, 100 * float(out.float().mean()), " ".join("%.1f" % (100 * float(v)) for v in per_view)))
        if args.dump is None:
            continue
        cen = torch.as_tensor(np.load(os.path.join(args.dump, "proposal_centers.npy"))).reshape(-1, 7)
        cen = cen[cen[:, 3] >= 0]
        tl, _, start, end = O.person_boxes(spec, cen)
        n_out, n_all = torch.zeros(len(cams)), 0
        live = 0
        for i in range(cen.shape[0]):
            if bool((start[i] >= end[i]).any()):
                continue
            live += 1
            o = no_tap_inside(O.build_sample_grids(axis_points(spec, start[i], end[i], args.window_stride), cams, cfg, rt), W, H)
            n_out += o.float().sum(dim=1)
            n_all += o.shape[1]
        cube = int(spec.cube[0]) ** 3
        vox = sum(int((end[i] - start[i]).clamp(min=0).prod()) for i in range(cen.shape[0]))
        print("%-12s %d valid proposals (%d with a window), window stride %s: no tap inside %.1f %% of the in-window samples; per view %s"
              % (name, cen.shape[0], live, args.window_stride, 100 * float(n_out.sum()) / max(n_all * len(cams), 1),
                 " ".join("%.1f" % (100 * float(v) / max(n_all, 1)) for v in n_out)))
        print("%-12s voxels outside the windows (also skipped): %.1f %% of the %d cube voxels of these proposals"
              % (name, 100 * (1 - vox / (cube * max(cen.shape[0], 1))), cube * cen.shape[0]))


if __name__ == "__main__":
    main()
