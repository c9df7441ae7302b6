#!/usr/bin/env python
"""Share of the 7x7 front conv's matrix work that multiplies the zero margin of P2PNet's planes, from the proposals of a
`bench.py --config NAME --dump-outputs DIR` run (proposal_centers.npy through the oracle's person_boxes).  CPU only: no
library.

    python tools/live_rows_share.py --config panoptic --dump DIR [--rows-per-tile 4]

A person's cube is masked by the predicted box (project_individual.py:113-121): in the x-y and x-z planes the rows (x) outside
[s0 - tl0, e0 - tl0), in the y-z plane the rows (y) outside [s1 - tl1, e1 - tl1) are zero.  k_conv7 (csrc/fvp_conv7.h) works in
tiles of R output rows + 6 halo rows; a (input row, output row) pair is 7 MFMAs per channel group and column block.  Printed:
the margins, the share of pairs whose input row is dead (outside the range, or outside the image: the kernel skips both), the
share that is outside the image alone (skipped without the promise too), and the share of tiles without any live row."""
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


def tile_pairs(H, R, r0, r1):
    """(pairs executed without skipping, pairs with a live input row, pairs inside the image, tiles, dead tiles) of one
    plane whose live rows are [r0, r1)."""
    r0, r1 = min(max(r0, 0), H), min(max(r1, 0), H)
    allp = live = inside = tiles = dead = 0
    for y0 in range(0, H, R):
        tiles += 1
        any_live = False
        for r in range(R + 6):
            y = y0 - 3 + r
            n = sum(1 for j in range(R) if 0 <= r - j < 7)
            allp += n
            inside += n if 0 <= y < H else 0
            if r0 <= y < r1:
                live += n
                any_live = True
        dead += not any_live
    return allp, live, inside, tiles, dead


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", default="panoptic")
    ap.add_argument("--dump", required=True, help="directory written by bench.py --dump-outputs")
    ap.add_argument("--rows-per-tile", type=int, default=4)
    args = ap.parse_args()
    cfg = S.make_cfg(args.config)
    spec = O.IndividualSpec(cfg)
    Cn = int(spec.cube[0])
    cen = torch.as_tensor(np.load(os.path.join(args.dump, "proposal_centers.npy"))).reshape(-1, 7)
    cen = cen[cen[:, 3] >= 0]
    tl, _, start, end = O.person_boxes(spec, cen)
    tl, start, end = (np.asarray(v).astype(np.int64) for v in (tl, start, end))
    tot = np.zeros(5, np.int64)
    per_axis = {0: np.zeros(5, np.int64), 1: np.zeros(5, np.int64)}
    width = {0: [], 1: []}
    margins = {0: [], 1: []}
    for i in range(cen.shape[0]):
        empty = bool((start[i] >= end[i]).any())
        for plane, a in ((0, 0), (1, 0), (2, 1)):
            r0, r1 = (0, 0) if empty else (start[i, a] - tl[i, a], end[i, a] - tl[i, a])
            t = np.array(tile_pairs(Cn, args.rows_per_tile, int(r0), int(r1)), np.int64)
            tot += t
            per_axis[a] += t
            if plane != 1:
                width[a].append(int(r1 - r0))
                margins[a] += [int(r0), int(Cn - r1)]
    print("%-12s %d valid proposals, cube %d, tiles of %d rows" % (args.config, cen.shape[0], Cn, args.rows_per_tile))
    for a, name in ((0, "x"), (1, "y")):
        m, w = np.array(margins[a]), np.array(width[a])
        print("  %s: margin rows min / median / max %d / %d / %d, window rows min / median / max %d / %d / %d"
              % (name, m.min(), np.median(m), m.max(), w.min(), np.median(w), w.max()))
    z = (end[:, 2] - start[:, 2])
    print("  z: window min / median / max %d / %d / %d" % (z.min(), np.median(z), z.max()))

    def line(label, t):
        allp, live, inside, tiles, dead = (int(v) for v in t)
        print("  %-22s dead (input row, output row) pairs %.1f %% (outside the image alone %.1f %%), dead tiles %.1f %% of %d"
              % (label, 100 * (1 - live / allp), 100 * (1 - inside / allp), 100 * dead / tiles, tiles))
    line("rows = x (two planes):", per_axis[0])
    line("rows = y (y-z plane):", per_axis[1])
    line("all three planes:", tot)


if __name__ == "__main__":
    main()
