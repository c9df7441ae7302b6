"""The split-K 3x3 conv with two and four pixel blocks per workgroup on the MI355X: the table of tests/ksplit_rows_cases.py on
the diagnostics build (FVP_CONV_KS_PB is read per call there).  Per case, for FVP_CONV_KS_PB = 2 and 4: the same bits as the
one-block form, the fp64 bound of tests/common.py for split K, person masks and the poison guards; the planner's own choice
(no switch) at 9 and 2 planes of a 64 x 4 map against the forced one-block form.  The device libraries keep no launch log:
which instantiation a switch value and the planner reach is asserted on the emulator (tests/test_ksplit_rows_emu.py), the same
host code.

Measured worst error / bound on the MI355X: 0.0316 for PB = 1, 2 and 4 (bound: (cinp * 9 + 6) * eps32; profiles/ksplit_rows.txt)."""
import pytest

import ksplit_rows_cases as K

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("k", range(len(K.CASES)), ids=[c.name for c in K.CASES])
def test_forced_blocks_equal_the_one_block_form(diag_lib, k):
    K.run_case(diag_lib, "cuda", K.CASES[k], k)


def test_masked_plane_groups_stay_untouched(diag_lib):
    K.run_mask_case(diag_lib, "cuda")


def test_planner_choice_equals_the_one_block_form(diag_lib):
    K.run_natural(diag_lib, "cuda")
