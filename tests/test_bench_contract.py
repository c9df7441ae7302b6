"""bench.py pieces that can be checked without a GPU: the PMC-traffic gate (a traffic figure
from another workload or another kernel variant must not reach the bench line), the argument surface, and the plain run
with --dump-outputs on the CPU stand-in step."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_traffic_is_taken_only_from_a_file_collected_on_the_same_workload(tmp_path, monkeypatch):
    prof = tmp_path / "profiles"
    prof.mkdir()
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    # no file at all
    v, why = bench.load_pmc_traffic("k_conv_wino", 8, "panoptic")
    assert v is None and "no profiles" in why
    # a pre-round-3 file (no workload tag, flat keys): refused
    (prof / "r02_pmc_traffic.json").write_text(json.dumps({"conv_wino_bytes_per_launch": 1.3e8}))
    v, why = bench.load_pmc_traffic("k_conv_wino", 8, "panoptic")
    assert v is None and "refused" in why
    # a tagged file: accepted for its own workload and class, refused for another batch / config / class
    good = {"workload": {"config": "panoptic", "frames_per_step": 8}, "collected": "2026-09-27", "commit": "abc",
            "classes": {"k_conv_wino": {"bytes_per_launch": 1.9e8, "launches": 64,
                                        "variants": {"fvp::k_conv_wino<2, 4, 8, true, false>": {"bytes_per_launch": 2.0e8}}},
                        "k_project_triplane": {"bytes_per_launch": 4.6e8, "launches": 4, "variants": {}}}}
    (prof / "r03_pmc_traffic.json").write_text(json.dumps(good))
    v, src = bench.load_pmc_traffic("k_conv_wino", 8, "panoptic")
    assert v == 1.9e8 and "r03_pmc_traffic.json" in src and "k_conv_wino<2, 4, 8, true, false>" in src
    assert bench.load_pmc_traffic("k_conv_wino", 1, "panoptic")[0] is None
    assert bench.load_pmc_traffic("k_conv_wino", 8, "shelf")[0] is None
    assert bench.load_pmc_traffic("k_conv_dma", 8, "panoptic")[0] is None            # class absent
    assert bench.load_pmc_traffic("k_project_triplane", 8, "panoptic")[0] is None    # no variants listed


def test_committed_traffic_file_matches_the_headline_workload():
    v, src = bench.load_pmc_traffic("k_conv_wino", 8, "panoptic")
    assert v and v > 1e8, src


def test_argument_surface():
    a = bench.parse_args([])
    assert (a.gpus, a.batch, a.config, a.streams) == (1, 8, "panoptic", 4) and a.steps > 0 and a.warmup >= 0
    a = bench.parse_args(["--gpus", "8", "--config", "panoptic128", "--batch", "1", "--steps", "5", "--warmup", "2"])
    assert (a.gpus, a.config, a.batch, a.steps, a.warmup) == (8, "panoptic128", 1, 5, 2)
    assert bench.parse_args(["--backbone"]).backbone
    assert not a.full and a.dump_outputs is None
    a = bench.parse_args(["--full", "--dump-outputs", "out"])
    assert a.full and a.dump_outputs == "out"


def test_plain_run_times_the_steps_and_dumps_the_last_one(tmp_path):
    """A plain run (no --full) on the CPU stand-in step (FVP_BENCH_STUB=1): exactly --steps timed steps behind
    ms_per_step, none of the secondary measurements, and --dump-outputs writes the last step's result, the same
    bits from run to run."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env["FVP_BENCH_STUB"] = "1"
    dumped = []
    for run in ("a", "b"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "5", "--warmup", "2", "--batch", "3",
                            "--dump-outputs", str(tmp_path / run)], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        d = json.loads(r.stdout.strip().splitlines()[-1])
        assert d["steps"] == 5 and d["warmup"] == 2 and d["full"] is False and d["ms_per_step"] > 0
        assert abs(d["value"] - 3 * 5 / (d["ms_per_step"] * 5e-3)) < 1e-6 * d["value"]
        assert d["unit"] == "frames/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
        assert d["cpu_baseline"] is None and d["mpjpe_vs_ref_mm"] is None and d["kernels"] == {}
        assert d["value_long"] is None and d["other_configs"] is None
        assert sorted(os.listdir(tmp_path / run)) == ["fused_poses.npy"]
        dumped.append(np.load(tmp_path / run / "fused_poses.npy"))
    assert dumped[0].dtype == np.float32 and dumped[0].shape == (3, 10, 15, 5)
    assert np.array_equal(dumped[0], dumped[1])
    assert np.array_equal(dumped[0][:, 0, 0, 0], np.arange(3, dtype=np.float32))     # the stand-in step's frame ids
