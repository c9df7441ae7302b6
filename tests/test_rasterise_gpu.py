"""fvp_rasterise_heatmaps on the MI355X through the shipped library: the checks of tests/test_rasterise_emu.py again (shared
cases, runner and float64 yardstick: tests/rasterise_cases.py).  Window placement is exact; values are within 1 ulp of float32
of the oracle (the device exp(double) may differ from the host's in its last float64 bit); counts, limits, argument checks,
the channels-last copy, determinism and batching are exact."""
import pytest

import rasterise_cases as RC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def lib():
    from faster_voxelpose_amd import _capi as capi
    return capi.load()


@pytest.mark.parametrize("name", list(RC.CASES))
def test_within_one_ulp_of_the_float64_oracle(lib, name):
    RC.check_case(lib, DEV, name, exact=False)


@pytest.mark.parametrize("form", RC.OUTPUT_FORMS)
@pytest.mark.parametrize("name", ["rb4_ragged", "rb2_ragged"])
def test_output_forms(lib, name, form):
    RC.check_output_forms(lib, DEV, name, form)


def test_counts_are_clamped(lib):
    RC.check_counts(lib, DEV, exact=False)


def test_limits(lib):
    RC.check_limits(lib, DEV)


def test_arguments(lib):
    RC.check_arguments(lib, DEV)


def test_determinism_and_batching(lib):
    RC.check_determinism_and_batching(lib, DEV)


def test_non_finite_joints_stamp_nothing(lib):
    """include/fvp.h: a joint with a non-finite coordinate stamps nothing and is left out of the person's extent.  Without the
    kernel's finiteness test the hardware double -> int32 conversion turns a NaN x into column 0 and the joint's Gaussian
    lands on the image border."""
    RC.check_nonfinite(lib, DEV, exact=False)
