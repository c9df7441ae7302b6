#!/usr/bin/env python
"""Writes tests/golden/triangulate_floor.json: how far the DEFINITION of fvp_triangulate_joints (include/fvp.h) lies from the
truth, measured with the numpy yardstick of tests/triangulate_cases.py alone - no library, no reference checkout, CPU only.
Scene: points with known 3-D positions in the field of view of the five Panoptic-fixture cameras, every heat-map peak an exact
paraboloid at the true projection (so the sub-cell refinement is exact), the fused input the truth plus 20 mm; a second scene
with Gaussian peaks of sigma 3 reports the parabola's bias.  Per scene: (a) the float64 yardstick's largest distance from the
truth, (b) the float32 yardstick's largest distance from the float64 one, (c) the share of joint-views whose state differs
between the two.  tests/test_triangulate_*.py hold the kernel to 2 x ((a) + (b)) on the scene of another seed."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import triangulate_cases as TC  # noqa: E402

GEN_SEEDS, TEST_SEED = (101, 102, 103), 104


def main():
    out = dict(gen_seeds=list(GEN_SEEDS), test_seed=TEST_SEED, radius=3, offset_mm=20.0)
    for kind in ("paraboloid", "gaussian"):
        figs = [TC.floor_figures(TC.floor_scene(s, shape=kind)) for s in GEN_SEEDS]
        for f in figs:
            f.pop("kernel_to_truth_mm")
            assert f["state_mismatch_share"] <= 0.05 and f["triangulated_share"] >= 0.90, f
        out[kind] = {k: max(f[k] for f in figs) for k in ("fp64_to_truth_mm", "fp32_to_fp64_mm", "state_mismatch_share",
                                                          "not_enclosed_share")}
        out[kind]["triangulated_share"] = min(f["triangulated_share"] for f in figs)
        out[kind]["joints_compared"] = sum(f["joints_compared"] for f in figs)
        print(kind, out[kind])
    with open(TC.FLOOR_JSON, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
