"""The back-projection kernels on the MI355X against the float64 reference of tests/projection_cases.py (see there for the
rig, the reference, its bounds and the cases): every whole-space and per-person case, through the shipped library
(_capi.load()) and, where a switch selects the form, the diagnostics build.

Which fused form a per-person case takes follows the shape rule of fvp_project_individual_triplane (the owned form where
tri_owned_lds(C, JP) fits 36 KB, else the block form; the emulator suite reads it from the launch log):
  owned: every C <= 16 case, C 64 JP 20, C 128 JP 8 (23 KB: the rule is on the bytes, not on C)     block: C 64 JP 28 and JP 32
and every case also runs the block form on the diagnostics build (FVP_TRI_OWNED=0).  Whole-space cases take the quad-lane
form k_project_whole_q; the lane-per-voxel form k_project_whole runs in a child process under FVP_WHOLE_NO_QUAD.

Measured on the MI355X, largest error / bound per case (the emulator gives the same figures; K = V + 7 roundings in (b)):
  whole space          (a)   (b)   (c)        per person (C, J, V)   form   (a)   (b)   (c)
  5x7x20  B3  V4 J5    0.40  0.20  0.07       4, 1, 1                owned  0.30  0.18  0.02
  3x3x1   B1  V1 J1    0.17  0.04  0.01       4, 17, 2               owned  0.31  0.23  0.03
  2x3x256 B1  V2 J4    0.30  0.28  0.06       8, 5, 8                owned  0.72  0.15  0.04
  4x5x3   B8  V6 J17   0.57  0.23  0.05       8, 29, 2               owned  0.35  0.26  0.04
  3x2x200 B3  V8 J21   0.73  0.20  0.07       16, 9, 2               owned  0.39  0.29  0.04
   (lane form: the same)                      16, 21, 1              owned  0.39  0.35  0.07
  2x2x129 B1  V8 J32   0.71  0.20  0.05       16, 13, 8              owned  0.75  0.24  0.05
  5x7x20  B16 V2 J16   0.36  0.29  0.11       16, 25, 8              owned  0.75  0.21  0.06
  4x5x3   B3  V1 J32   0.26  0.21  0.10       64, 25, 2              block  0.40  0.34  0.05
  3x3x1   B8  V8 J21   0.41  0.13  0.02       64, 17, 8              owned  0.75  0.26  0.08
  5x7x20  B1  V6 J4    0.67  0.16  0.04       64, 32, 1              block  0.40  0.31  0.09
  4x5x3   B3  V4 J16 (heat map 2 x 3)         128, 5, 2              owned  0.44  0.26  0.04
                       0.48  0.17  0.10
  2x2x129 B3  V2 J17   0.35  0.26  0.12
No end-to-end bound above 1e-3 in any case; no zero of a fused plane differed in sign from the materialised one."""
import json
import os
import subprocess
import sys

import pytest
import torch

import projection_cases as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _shipped():
    from faster_voxelpose_amd import _capi as capi
    return P.Ctx(capi.load(), "cuda:0")


@pytest.mark.parametrize("name", [c[0] for c in P.WHOLE_CASES])
def test_gpu_whole_space(name):
    fig = P.check_whole(_shipped(), name)
    print(name, fig)


def test_gpu_lane_per_voxel_form(diag_lib, tmp_path):
    """k_project_whole, reached through FVP_WHOLE_NO_QUAD only: a fresh process (the switch is read once)."""
    out = tmp_path / "lane.json"
    env = dict(os.environ, FVP_WHOLE_NO_QUAD="1")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "projection_child.py"), str(out), P.LANE_CASE, "--gpu"], env=env,
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    res = json.load(open(out))
    assert "error" not in res, res["error"]
    print(res["figures"])


@pytest.mark.parametrize("J,W,H", P.STAGING)
def test_gpu_staging(J, W, H):
    P.check_staging(_shipped(), J, W, H)


def test_gpu_staging_refuses_a_side_of_one():
    P.check_staging_refusal(_shipped())


@pytest.mark.parametrize("shape", P.PERSON_CASES, ids=lambda s: "C%d_J%d_V%d" % s)
def test_gpu_per_person(diag_lib, monkeypatch, shape):
    """Diagnostics build: materialised cubes against the reference, fvp_triplane_max, the fused planes in the form the shape
    rule picks and in the block form.  Shipped library: the same cubes bit for bit, and its own fused planes."""
    fx = P.Person(P.Ctx(diag_lib, "cuda:0"), shape)
    signs = fx.check_fused("diagnostics build, shape rule (%s)" % P.expected_form(shape[0], fx.g.JP))
    monkeypatch.setenv("FVP_TRI_OWNED", "0")
    signs = max(signs, fx.check_fused("diagnostics build, block form"))
    monkeypatch.delenv("FVP_TRI_OWNED")
    sh = P.Person(_shipped(), shape, check=False)
    assert torch.equal(sh.want.view(torch.int32), fx.want.view(torch.int32)), "the shipped library's materialised planes differ"
    signs = max(signs, sh.check_fused("shipped library"))
    print(shape, P.expected_form(shape[0], fx.g.JP), fx.figures, "zero-sign differences:", signs)


def test_gpu_person_boxes():
    P.check_person_boxes(_shipped(), 16)
    P.check_person_boxes(_shipped(), 4)


def test_gpu_proposal_glue():
    P.check_proposal_glue(_shipped())
