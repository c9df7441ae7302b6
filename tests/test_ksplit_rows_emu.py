"""The split-K 3x3 conv with two and four pixel blocks per workgroup on the CPU emulation (tests/hipemu): the table of
tests/ksplit_rows_cases.py.  Per case, for FVP_CONV_KS_PB = 2 and 4: the same bits as the one-block form, the fp64 bound of
tests/common.py for split K, the instantiation in the launch log, and person masks; the planner's own choice (no switch) at 9
and at 2 planes of a 64 x 4 map.

Measured worst error / bound on the emulator: 0.0316 (bound: (cinp * 9 + 6) * eps32), the same for PB = 1, 2 and 4 (the same
bits).  Mutation check (profiles/ksplit_rows.txt, section 7): with the row count of the last tile off by one in conv_epilogue
(y <= H for y < H) 25 of the 32 cases fail - all but those on the 64 x 4 map, whose tiles divide it."""
import pytest

import ksplit_rows_cases as K


@pytest.mark.parametrize("k", range(len(K.CASES)), ids=[c.name for c in K.CASES])
def test_forced_blocks_equal_the_one_block_form(emu_lib, k):
    K.run_case(K.T.load_lib(), "cpu", K.CASES[k], k)


def test_masked_plane_groups_stay_untouched(emu_lib):
    K.run_mask_case(K.T.load_lib(), "cpu")


def test_planner_takes_two_blocks_above_512_one_row_workgroups(emu_lib):
    insts9, insts2 = K.run_natural(K.T.load_lib(), "cpu")
    assert insts9 == [K.ks(2)], insts9
    assert insts2 == [K.ks(1)], insts2
