"""The live-row promise of fvp_conv_stack_run_rows on the CPU emulation (tests/hipemu): k_conv7 with the array computes the
bits it computes without it, in every branch of the row test (tests/conv7_live_rows_cases.py: the ranges, the checks), and
the pixel-pair fallback form ignores the array (a child process under FVP_CONV_NO_K7=1: the switch is read once when the
library loads).

Measured worst error / bound of the run without the array against fp64 (bound (cinp * 49 + 3) * eps32): 0.0027 (inputs in
[0, 1]: no cancellation)."""
import os
import subprocess
import sys

import pytest
import torch

import conv7_live_rows_cases as LR
import conv_form_cases as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("case", LR.CASES, ids=LR.case_id)
def test_conv7_with_live_rows_keeps_the_bits(emu_lib, case):
    emu_lib.hipemu_launch_log.restype = __import__("ctypes").c_char_p
    emu_lib.hipemu_launch_log_reset()
    ratio = LR.check_case(emu_lib, "cpu", case, LR.CASES.index(case))
    print(f"{LR.case_id(case)}: error / bound {ratio:.3g}")
    insts = T.instantiations(emu_lib.hipemu_launch_log().decode())
    assert insts == [f"k_conv7<64,{4 if case[0] <= 16 else 5},4>"] * 3, insts


def test_fallback_form_ignores_live_rows(tmp_path):
    out = tmp_path / "fallback.pt"
    env = dict(T.child_env("no_k7", os.environ), OMP_NUM_THREADS="1", MKL_NUM_THREADS="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "conv7_live_rows_cases.py"), str(out)], env=env,
                       stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    res = torch.load(out)
    assert sorted(res) == sorted(LR.case_id(c) for c in LR.FALLBACK_CASES)
    for name, v in res.items():
        assert v["equal"] and v["finite"], (name, v)
        assert v["insts"] and all(i.startswith("k_conv_dma<7,7,") for i in v["insts"]), (name, v["insts"])


def test_query_says_where_the_array_is_read(emu_lib):
    """fvp_conv_stack_reads_live_rows follows the routing: 1 where the first op takes k_conv7, 0 on a miniature map (the
    pixel-pair form), for a stack that starts with another op, and for no planes."""
    import common as CM
    k7, _ = LR.layer(15, 64, 0)
    small, _, _ = CM.conv_layer("conv", 15, 16, (16, 16), k=7, bn=True)
    other, _, _ = CM.conv_layer("conv", 15, 16, (64, 64), k=3)
    q = emu_lib.fvp_conv_stack_reads_live_rows
    assert q(k7.op_array, len(k7.ops), 7) == 1 and q(k7.op_array, len(k7.ops), 0) == 0
    assert q(small.op_array, len(small.ops), 7) == 0 and q(other.op_array, len(other.ops), 7) == 0
