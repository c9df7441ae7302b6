"""The back-projection kernels on the CPU emulator against the float64 reference of tests/projection_cases.py (see there
for the rig, the reference, its bounds and the cases), and the self-tests of that fixture, which need no kernel: coverage
of every tap / clamp class, both clamps of the view mean, the vacuity cap and the discrimination of mutated references."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest

import projection_cases as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fixture_covers_every_tap_and_clamp_class():
    frac = P.coverage()
    print(frac)


def test_both_clamps_of_the_view_mean_occur():
    """Each clamp in >= 1 % of the (voxel, joint) values of at least one whole-space case (the high one needs V <= 2)."""
    low, high = {}, {}
    for name, grid, B, V, J, (W, H) in P.WHOLE_CASES:
        g, ax3, pts, heat, cams, _ = P.whole_inputs(name)
        raw = P.reference(cams[0], g, pts, heat[0])["raw"]
        low[name], high[name] = float((raw < 0).mean()), float((raw > 1).mean())
    print(low, high)
    assert max(low.values()) >= 0.01 and max(high.values()) >= 0.01, (low, high)
    assert max(low[c[0]] for c in P.WHOLE_CASES if c[3] >= 4) >= 0.01, low


def test_mutated_references_leave_the_bounds():
    frac = P.discrimination()
    print(frac)
    assert frac["vacuous"] <= 0.02, frac
    for m in P.MUTANTS_C + P.MUTANTS_B:
        assert frac[m] >= 0.10, (m, frac)


@pytest.mark.parametrize("name", [c[0] for c in P.WHOLE_CASES])
def test_emulated_whole_space(emu_lib, name):
    fig = P.check_whole(P.Ctx(emu_lib, "cpu"), name)
    print(name, fig)


def test_emulated_lane_per_voxel_form(emu_lib, tmp_path):
    """k_project_whole, reached through FVP_WHOLE_NO_QUAD only: a fresh process (the switch is read once)."""
    out = tmp_path / "lane.json"
    env = dict(os.environ, FVP_WHOLE_NO_QUAD="1")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "projection_child.py"), str(out), P.LANE_CASE], env=env,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    res = json.load(open(out))
    assert "error" not in res, res["error"]
    assert "k_project_wholeI" in res["log"] and "k_project_whole_q" not in res["log"], res["log"]
    print(res["figures"])


@pytest.mark.parametrize("J,W,H", P.STAGING)
def test_emulated_staging(emu_lib, J, W, H):
    P.check_staging(P.Ctx(emu_lib, "cpu"), J, W, H)


def test_emulated_staging_refuses_a_side_of_one(emu_lib):
    P.check_staging_refusal(P.Ctx(emu_lib, "cpu"))


@pytest.mark.parametrize("shape", P.PERSON_EMU, ids=lambda s: "C%d_J%d_V%d" % s)
def test_emulated_per_person(emu_lib, monkeypatch, shape):
    """Materialised cubes against the reference, fvp_triplane_max, the fused planes in the form the shape rule picks (the
    launch log names it) and in the block form."""
    emu_lib.hipemu_launch_log.restype = C.c_char_p
    fx = P.person(P.Ctx(emu_lib, "cpu"), shape, "emu")
    form = P.expected_form(shape[0], fx.g.JP)
    emu_lib.hipemu_launch_log_reset()
    signs = fx.check_fused("shape rule")
    log = emu_lib.hipemu_launch_log().decode()
    other = {"own": "blk", "blk": "own"}[form]
    assert "k_project_triplane_" + form in log and "k_project_triplane_" + other not in log, (form, log)
    monkeypatch.setenv("FVP_TRI_OWNED", "0")
    emu_lib.hipemu_launch_log_reset()
    signs = max(signs, fx.check_fused("block form"))
    log = emu_lib.hipemu_launch_log().decode()
    assert "k_project_triplane_blk" in log and "k_project_triplane_own" not in log, log
    print(shape, form, fx.figures, "zero-sign differences:", signs)


def test_emulated_person_boxes(emu_lib):
    P.check_person_boxes(P.Ctx(emu_lib, "cpu"), 16)
    P.check_person_boxes(P.Ctx(emu_lib, "cpu"), 4)


def test_emulated_proposal_glue(emu_lib):
    P.check_proposal_glue(P.Ctx(emu_lib, "cpu"))
