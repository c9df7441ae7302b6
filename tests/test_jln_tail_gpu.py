"""The JLN tail (fvp_softargmax_weightnet, fvp_fuse_poses, fvp_pack_weightnet) of the shipped library on the MI355X against
the float64 restatement and bounds of tests/jln_tail_cases.py: the case list of tests/test_jln_tail_emu.py.  The diagnostics
build is used only where the generic kernel has to be forced at the shipped shape (C = 64, F = 32)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import jln_tail_cases as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WORST = {}


@pytest.fixture(scope="module")
def lib():
    from faster_voxelpose_amd import _capi as capi
    return capi.load()


@pytest.mark.parametrize("name", list(T.KERNEL_CASES))
def test_kernel_case_within_the_fp64_bound(name, lib):
    T.run_and_check_case(lib, DEV, name, worst=WORST)


def test_forced_generic_kernel_at_the_shipped_shape(diag_lib, lib, monkeypatch):
    monkeypatch.setenv("FVP_SOFTARGMAX_GENERIC", "1")
    generic, _ = T.run_and_check_case(diag_lib, DEV, "fast_instance", masks=False, worst=WORST)
    monkeypatch.delenv("FVP_SOFTARGMAX_GENERIC")
    fast = T.run_softargmax(lib, DEV, T.case_data("fast_instance"))
    for a, b in zip(fast, generic):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))


@pytest.mark.parametrize("order", [T.ORDER_325_FIRST, T.ORDER_128_FIRST], ids=["325_first", "128_first"])
def test_large_lds_orderings(order):
    """The two sides of the 64 KB opt-in in both orders, each in a process that has launched nothing before: the opt-in is
    remembered per process and device."""
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "jln_tail_child.py")
    r = subprocess.run([sys.executable, child] + order, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok: " in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


@pytest.mark.parametrize("name", T.ALONE_CASES)
def test_a_person_alone_equals_the_person_in_the_batch(name, lib):
    T.check_person_alone(lib, DEV, name)


@pytest.mark.parametrize("key", list(T.BETA_CASES))
def test_other_betas(key, lib):
    name, beta = T.BETA_CASES[key]
    got, _ = T.run_and_check_case(lib, DEV, name, beta=beta, worst=WORST)
    if beta == 1000.0:
        T.check_one_hot_gives_the_grid_point(got, T.case_data(name, beta))


@pytest.mark.parametrize("nP,J", T.FUSE_CASES)
def test_fuse_poses(nP, J, lib):
    T.check_fuse(lib, DEV, nP, J, WORST)


@pytest.mark.parametrize("F,Hd", T.PACK_CASES)
def test_pack_weightnet(F, Hd, lib):
    T.check_pack(lib, DEV, F, Hd)


def test_argument_errors(lib):
    T.check_argument_errors(lib, DEV)


def test_report_worst_ratios():
    """Prints (pytest -s) the worst error / bound over this module; recorded in the docstring of tests/jln_tail_cases.py."""
    if WORST:
        T.report("the MI355X", WORST)
