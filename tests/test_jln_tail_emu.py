"""The JLN tail (fvp_softargmax_weightnet, fvp_fuse_poses, fvp_pack_weightnet) without a GPU: first the sensitivity of the
float64 bounds of tests/jln_tail_cases.py (pure numpy / torch), then the kernels on the CPU emulation (tests/hipemu) on the
case list the GPU test runs.  The emulated library is a diagnostics build: FVP_SOFTARGMAX_GENERIC acts, and its launch log
shows which kernel a call took."""
import ctypes

import numpy as np
import pytest
import torch

import fvp_oracle as O
import fvp_synthetic as S
import jln_tail_cases as T

WORST = {}


# ---- 1. the bounds accept the clean references and reject subtly wrong ones (no kernel) ------------------------------------
MUTATION_SHAPES = [(2, 1, 1), (6, 7, 9), (16, 32, 64), (18, 31, 63), (64, 32, 64)]
SOFTARGMAX_MUTANTS = ["plane 1 with the grid of plane 0", "last cell left out", "last row left out", "pmax of the neighbouring joint"]
WEIGHTNET_MUTANTS = ["edge-replicate padding", "pooling windows shifted by one cell", "max-pool before BN", "average divided by C^2",
                     "feature F-1 dropped", "fc1 with row stride Hd", "b2 omitted"]
FUSE_MUTANTS = ["xz / yz weights swapped in z", "oy for the xz plane", "confidence averaged over J"]


def _mutation_cases():
    return [T.case_data(f"mutation {c} {f} {hd}", grid_kind=k) for c, f, hd in MUTATION_SHAPES for k in ("uniform", "engine")]


def test_bound_rejects_mutated_references():
    """The float64 reference rounded to fp32 and the oracle's float64 soft-argmax stay within the bounds on every case; each
    mutation a subtly wrong kernel could make leaves them on at least one."""
    cases = _mutation_cases()
    assert len(SOFTARGMAX_MUTANTS) + len(WEIGHTNET_MUTANTS) + len(FUSE_MUTANTS) == 14
    for c in cases:
        Cn, F, Hd, J, nP = c["dims"]
        ref = c["ref"]
        assert (c["blob"][10 * F:11 * F] < 0).any() or F == 1, "BN scales of both signs"
        for key, b in (("pose", "bound_pose"), ("pmax", "bound_pmax"), ("wgt", "bound_wgt")):
            assert T.ratio(ref[key].astype(np.float32), ref[key], ref[b]) <= 1.0, (c["name"], key)
        x = torch.from_numpy(np.array(c["feat"])).permute(1, 0, 2, 3, 4).contiguous()
        pose, conf = O.soft_argmax(x, torch.from_numpy(np.array(c["grid"])).view(3, Cn, Cn, 2), c["beta"], accumulate=torch.float64)
        assert T.ratio(pose.permute(1, 0, 2, 3).float().numpy(), ref["pose"], ref["bound_pose"]) <= 1.0, c["name"]
        assert T.ratio(conf.float().numpy(), ref["pmax"].mean((1, 2)), ref["bound_pmax"].mean((1, 2))) <= 1.0, c["name"]
    feats = [c["feat"].reshape(c["dims"][4], 3, c["dims"][3], -1) for c in cases]
    for mut in SOFTARGMAX_MUTANTS:
        worst = 0.0
        for c, f in zip(cases, feats):
            m = T.ref_softargmax(f, c["grid"], c["beta"], mut=mut)
            worst = max(worst, T.ratio(m["pose"].astype(np.float32), c["ref"]["pose"], c["ref"]["bound_pose"]),
                        T.ratio(m["pmax"].astype(np.float32), c["ref"]["pmax"], c["ref"]["bound_pmax"]))
        assert worst > 1.0, f"the bound accepts: {mut} (worst error / bound {worst:.3g})"
    for mut in WEIGHTNET_MUTANTS:
        worst = 0.0
        for c in cases[::2]:                                        # WeightNet does not read the grid: one grid kind
            Cn, F, Hd, J, nP = c["dims"]
            w, _ = T.ref_weightnet(c["feat"], c["blob"], F, Hd, mut=mut)
            worst = max(worst, T.ratio(w.astype(np.float32), c["ref"]["wgt"], c["ref"]["bound_wgt"]))
        assert worst > 1.0, f"the bound accepts: {mut} (worst error / bound {worst:.3g})"
    rejected = dict.fromkeys(FUSE_MUTANTS, False)
    for nP, J in T.FUSE_CASES:
        inp = T.fuse_inputs(nP, J)
        args = (inp["pose2d"], inp["pmax"], inp["wgt"], inp["offset"], None, inp["centers"])
        ref = T.ref_fuse(*args)
        assert T.ratio(ref["fused"].astype(np.float32), ref["fused"], ref["bound"]) <= 1.0
        for mut in FUSE_MUTANTS:
            m = T.ref_fuse(*args, mut=mut)
            if T.ratio(m["fused"].astype(np.float32), ref["fused"], ref["bound"]) > 1.0:
                rejected[mut] = True
    assert all(rejected.values()), f"the bound accepts: {[m for m, r in rejected.items() if not r]}"


def test_engine_grid_restates_the_engines_center_grid(emu_lib):
    from faster_voxelpose_amd.engine import HotPath
    cfg = S.make_cfg("tiny", device="cpu", min_score=-1.0)
    e = HotPath(cfg, _lib=emu_lib)
    mine = T.engine_grid(e.C, tuple(float(v) for v in cfg.INDIVIDUAL_SPEC.SPACE_SIZE), tuple(float(v) for v in cfg.CAPTURE_SPEC.SPACE_CENTER))
    assert np.array_equal(mine, e.center_grid.numpy())


# ---- 2. the kernels, emulated ------------------------------------------------------------------------------------------------
def _log(lib):
    lib.hipemu_launch_log.restype = ctypes.c_char_p
    text = lib.hipemu_launch_log().decode()
    lib.hipemu_launch_log_reset()
    return text


@pytest.mark.parametrize("name", list(T.KERNEL_CASES))
def test_kernel_case_within_the_fp64_bound(name, emu_lib, monkeypatch):
    monkeypatch.delenv("FVP_SOFTARGMAX_GENERIC", raising=False)
    emu_lib.hipemu_launch_log_reset()
    T.run_and_check_case(emu_lib, "cpu", name, worst=WORST.setdefault("emu", {}))
    log = _log(emu_lib)
    Cn, F = T.KERNEL_CASES[name][:2]
    assert ("k_softargmax_wn_fast" in log) == (Cn == 64 and F == 32), log       # only the shipped shape takes the fast instance
    assert ("k_softargmax_weightnet" in log) != (Cn == 64 and F == 32), log


def test_forced_generic_kernel_at_the_shipped_shape(emu_lib, monkeypatch):
    monkeypatch.setenv("FVP_SOFTARGMAX_GENERIC", "1")
    emu_lib.hipemu_launch_log_reset()
    generic, _ = T.run_and_check_case(emu_lib, "cpu", "fast_instance", masks=False, worst=WORST.setdefault("emu", {}))
    log = _log(emu_lib)
    assert "k_softargmax_weightnet" in log and "k_softargmax_wn_fast" not in log, log
    monkeypatch.delenv("FVP_SOFTARGMAX_GENERIC")
    fast = T.run_softargmax(emu_lib, "cpu", T.case_data("fast_instance"))
    for a, b in zip(fast, generic):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))


@pytest.mark.parametrize("order", [T.ORDER_325_FIRST, T.ORDER_128_FIRST], ids=["325_first", "128_first"])
def test_large_lds_orderings(order, emu_lib):
    """The two sides of the 64 KB opt-in in both orders (the emulated hipFuncSetAttribute accepts everything: the order
    matters on the GPU, where the same lists run in fresh processes)."""
    for name in order:
        T.run_and_check_case(emu_lib, "cpu", name, masks=False)


@pytest.mark.parametrize("name", T.ALONE_CASES)
def test_a_person_alone_equals_the_person_in_the_batch(name, emu_lib):
    T.check_person_alone(emu_lib, "cpu", name)


@pytest.mark.parametrize("key", list(T.BETA_CASES))
def test_other_betas(key, emu_lib):
    name, beta = T.BETA_CASES[key]
    got, _ = T.run_and_check_case(emu_lib, "cpu", name, beta=beta, worst=WORST.setdefault("emu", {}))
    if beta == 1000.0:
        T.check_one_hot_gives_the_grid_point(got, T.case_data(name, beta))


@pytest.mark.parametrize("nP,J", T.FUSE_CASES)
def test_fuse_poses(nP, J, emu_lib):
    T.check_fuse(emu_lib, "cpu", nP, J, WORST.setdefault("emu", {}))


@pytest.mark.parametrize("F,Hd", T.PACK_CASES)
def test_pack_weightnet(F, Hd, emu_lib):
    T.check_pack(emu_lib, "cpu", F, Hd)


def test_argument_errors(emu_lib):
    T.check_argument_errors(emu_lib, "cpu")


def test_report_worst_ratios():
    """Prints (pytest -s) the worst error / bound of the emulated kernels over this module and of the fp32 oracle on the same
    inputs; the figures are recorded in the docstring of tests/jln_tail_cases.py."""
    if "emu" in WORST:
        T.report("the CPU emulation", WORST["emu"])
    worst = {}
    for name in T.KERNEL_CASES:
        for k, v in T.oracle_ratios(T.case_data(name)).items():
            worst[k] = max(worst.get(k, 0.0), v)
    T.report("the fp32 oracle", worst)
