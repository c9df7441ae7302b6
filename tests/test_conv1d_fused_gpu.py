"""fvp_conv_stack_run_fused_1d of the shipped library on the MI355X, op by op: the cases and checks of
tests/conv1d_fused_cases.py (the list of tests/test_conv1d_fused_emu.py).

Measured on the MI355X: op cases, worst error / bound 0.063; whole C2CNet, worst |fused - fp64| / tolerance 0.36 (printed
per case with -s)."""
import pytest
import torch

import common as CM
import conv1d_fused_cases as T

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def lib():
    from faster_voxelpose_amd import _capi as capi
    return capi.load()


# (op, as the last op?): a stack that ends in a pool is refused (test_fused_1d_last_pool_is_refused), so the pool is a middle op only
OP_CASES = [(i, last) for i in range(len(T.OPS)) for last in (True, False) if not (T.OPS[i][1] == "pool" and last)]


@pytest.mark.parametrize("op,last", OP_CASES, ids=[f"{T.OPS[i][0]}-{'last' if last else 'middle'}" for i, last in OP_CASES])
def test_fused_1d_op_within_fp64_bound_and_equal_to_generic(lib, op, last):
    o = T.OPS[op]
    worst = T.sweep_op(lib, DEV, o, last)
    ends = (o[5][4] if len(o[5]) > 4 else o[5][0], o[5][-1])
    worst = max(worst, T.sweep_op(lib, DEV, o, last, plane_counts=(1, 80), lengths=ends))
    print(f"{o[0]}: worst error / bound {worst:.4f}")


@pytest.mark.parametrize("Z", T.C2C_Z)
@pytest.mark.parametrize("cin", T.C2C_CIN)
def test_fused_1d_c2cnet_layers_within_bound_and_fused_equal_to_generic(lib, cin, Z):
    worst = T.check_c2cnet(lib, DEV, cin, Z)
    print(f"c2cnet({cin}, {Z}): worst |fused - fp64| / tolerance {worst:.3f}")


@pytest.mark.parametrize("case", range(6), ids=["Z28", "coutp160", "nops33", "last_op_pool", "odd_pool_L5", "odd_pool_L7"])
def test_fused_1d_refusals_leave_the_output_untouched(lib, case):
    T.check_refusal(lib, DEV, T.refusal_stacks()[case])


@pytest.mark.parametrize("op", ["up_128_64", "up_64_32"])
def test_fused_1d_last_transposed_conv_keeps_its_residual(lib, op):
    o = [v for v in T.OPS if v[0] == op][0]
    spec, w, ids = T.op_stack(o, 10, last=True, seed=1)
    x = T.stack_input(spec, 5, 11)
    rc, out, blob, check = T.run_fused(lib, DEV, spec, w, x)
    assert rc == 0
    check()
    val, err = CM.conv_chain_reference(spec, w, blob, x, split=True)
    assert CM.conv_ratio(out.cpu(), val[ids["out"]], err[ids["out"]]) <= 1.0
    without = val[ids["out"]] - x.double()
    assert float((out.cpu().double() - without).abs().max()) > 1.0


def test_fused_1d_last_pool_is_refused(lib):
    spec, w, _ = T.op_stack(T.OPS[-1], 8, last=True)
    rc, out, _, check = T.run_fused(lib, DEV, spec, w, T.stack_input(spec, 3, 1))
    assert rc == T.EINVAL
    check(untouched=True)
