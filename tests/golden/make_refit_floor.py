"""Writes tests/golden/refit_floor.json: how close three rounds of the camera re-fit DEFINITION (the numpy yardstick of
tests/recalibrate_cases.py alone, no kernel) bring a bumped camera back to the truth - a rig of 4 cameras with lens terms,
150 seeded points, camera 0 bumped by 1.5 degrees and 30 mm, observations noise-free and rounded to float32; every figure is
the largest over three seeds.  The tests hold the kernels, on a fourth seed, to 2 x these figures.

    python tests/golden/make_refit_floor.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import recalibrate_cases as RC  # noqa: E402

SEEDS, TEST_SEED = (201, 202, 203), 204

if __name__ == "__main__":
    per_seed = {}
    for seed in SEEDS:
        case = RC.floor_scene(seed)
        rounds = []
        for n in range(1, RC.FLOOR_ROUNDS + 1):
            res = RC.ref_refine(case, n)
            rounds.append(dict(RC.floor_figures(case, res), state=res["cal_state"].reshape(-1).tolist()))
        per_seed[str(seed)] = rounds
    last = [r[-1] for r in per_seed.values()]
    out = dict(seeds=list(SEEDS), test_seed=TEST_SEED, rounds=RC.FLOOR_ROUNDS, bump=dict(deg=1.5, mm=30.0),
               figures={k: max(r[k] for r in last) for k in last[0] if k != "state"}, per_seed=per_seed)
    with open(RC.FLOOR_JSON, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out["figures"], indent=1))
