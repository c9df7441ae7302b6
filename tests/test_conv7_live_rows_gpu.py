"""The live-row promise of fvp_conv_stack_run_rows on the MI355X: the case table of tests/conv7_live_rows_cases.py through the
shipped k_conv7 (same bits with and without the array, fp64 bound without it), the pixel-pair fallback form in the diagnostics
build (a child process under FVP_CONV_NO_K7=1), fvp_plane_live_rows against its numpy restatement, and the whole forward on the
conditioned Panoptic and Shelf fixtures with engine.conv_live_rows on and off, fused and materialised projection.

Measured worst error / bound of the run without the array against fp64 (bound (cinp * 49 + 3) * eps32): 0.0027, the
emulator's figure (tests/test_conv7_live_rows_emu.py)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import conv7_live_rows_cases as LR
import conv_form_cases as T
from cases import make_inputs, make_weights

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import torch  # noqa: F401,F811  (its HIP runtime first)
    from faster_voxelpose_amd import _capi as capi
    return capi.load()


@pytest.mark.parametrize("case", LR.CASES, ids=LR.case_id)
def test_conv7_with_live_rows_keeps_the_bits(lib, case):
    ratio = LR.check_case(lib, "cuda", case, LR.CASES.index(case))
    print(f"{LR.case_id(case)}: error / bound {ratio:.3g}")


def test_fallback_form_ignores_live_rows(diag_lib, tmp_path):
    out = tmp_path / "fallback.pt"
    env = T.child_env("no_k7", os.environ)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "conv7_live_rows_cases.py"), str(out), "--gpu"], env=env,
                       stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    res = torch.load(out)
    assert sorted(res) == sorted(LR.case_id(c) for c in LR.FALLBACK_CASES)
    for name, v in res.items():
        assert v["equal"] and v["finite"], (name, v)


def _live_rows_numpy(boxes, Cn):
    """The restatement: planes 0 and 1 {s0 - tl0, e0 - tl0}, plane 2 {s1 - tl1, e1 - tl1}, clamped to [0, C]; an empty window in
    any axis gives {0, 0} for all three planes."""
    b = boxes.astype(np.int64)
    tl, s, e = b[:, 0:3], b[:, 3:6], b[:, 6:9]
    empty = (s >= e).any(axis=1)
    lo = np.clip(s - tl, 0, Cn)
    hi = np.clip(e - tl, 0, Cn)
    out = np.zeros((b.shape[0], 3, 2), np.int32)
    for plane, a in ((0, 0), (1, 0), (2, 1)):
        out[:, plane, 0] = np.where(empty, 0, lo[:, a])
        out[:, plane, 1] = np.where(empty, 0, hi[:, a])
    return out.reshape(-1, 2)


def test_plane_live_rows_against_numpy(lib):
    from faster_voxelpose_amd import _capi as capi
    rng = np.random.default_rng(5)
    Cn, fine = 64, np.array([300, 300, 80])
    n = 203                                              # more than three workgroups of 64, not a multiple
    tl = rng.integers(-70, 320, size=(n, 3))
    m = rng.integers(0, 40, size=(n, 3))                 # margins up to past the middle: empty windows among them
    m[:, 2] = 0
    s = np.maximum(tl + m, 0)                            # clipped at the grid like fvp_person_boxes (:119-121)
    e = np.minimum(tl + Cn - m, fine)
    boxes = np.concatenate([tl, s, e], axis=1).astype(np.int32)
    boxes[0] = [5, 5, 5, 10, 20, 5, 9, 30, 60]           # empty in x only
    boxes[1] = [5, 5, 5, 10, 20, 70, 40, 30, 60]         # empty in z only
    boxes[2] = [0, 0, 0, -9, -9, 0, 99, 99, 64]          # not from fvp_person_boxes: clamped to [0, C]
    want = _live_rows_numpy(boxes, Cn)
    assert (want[:, 0] >= want[:, 1]).any() and (want[:, 1] - want[:, 0] > 0).any()
    bd = torch.from_numpy(boxes).to(DEV)
    got = torch.full((n * 3, 2), -77, dtype=torch.int32, device=DEV)
    capi.check(lib, lib.fvp_plane_live_rows(C.c_void_p(bd.data_ptr()), n, Cn, C.c_void_p(got.data_ptr()), None),
               "fvp_plane_live_rows")
    torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy(), want)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "materialised"])
@pytest.mark.parametrize("case", ["panoptic_c_b2_thr", "shelf_c_b1_thr"])
def test_forward_with_live_rows_keeps_the_bits(case, fused):
    from faster_voxelpose_amd.models import faster_voxelpose as FV
    cfg, cams, seq, rt, heat, meta, wseed = make_inputs(case, device=DEV)
    model = FV.get(cfg).to(DEV)
    model.load_state_dict(make_weights(case, model.state_dict()))
    model.joint_net.fused_projection = fused
    heat, rt = heat.to(DEV), rt.to(DEV)
    got = {}
    for on in (True, False):
        model.engine.conv_live_rows = on
        with torch.no_grad():
            fused_poses, plane_poses, centers, _, _ = model(meta=meta, input_heatmaps=heat, cameras=cams, resize_transform=rt)
        torch.cuda.synchronize()
        got[on] = dict(fused_poses=fused_poses.cpu().numpy(), plane_poses=plane_poses.cpu().numpy(),
                       feat=model.engine.last_jln["feat"].cpu().numpy(), valid=model.engine.last_jln["valid"].cpu().numpy())
    assert int(got[True]["valid"].sum()) >= 3
    spec = model.engine.specs["conv_net"]         # the fixture's front conv takes k_conv7: the switch is not idle
    assert model.engine.lib.fvp_conv_stack_reads_live_rows(spec.op_array, len(spec.ops), 3 * got[True]["valid"].size) == 1
    # the promise itself, on the planes P2PNet read: every row outside a valid person's range is +0.0 (bit pattern 0)
    eng = model.engine
    rows = eng.plane_live_rows(eng.last_jln["boxes"]).cpu().numpy().reshape(-1, 3, 2)
    planes = eng.last_jln["planes"].cpu().numpy().view(np.int32)                 # [nP, 3, J, C, C]
    for p in np.nonzero(got[True]["valid"])[0]:
        for k in range(3):
            r0, r1 = rows[p, k]
            assert not planes[p, k, :, :r0].any() and not planes[p, k, :, r1:].any(), (p, k, r0, r1)
            assert r1 - r0 < eng.C, "the fixture's boxes leave no margin: the test would not see a skipped row"
    for k in ("fused_poses", "plane_poses", "feat"):
        # (slots of invalid proposals are never written by P2PNet: compare what the forward defines)
        a, b = got[True][k], got[False][k]
        if k == "feat":
            v = np.repeat(got[True]["valid"].astype(bool), 3)
            a, b = a[v], b[v]
        assert np.array_equal(a.view(np.int32), b.view(np.int32)), k
