"""fvp_conv_stack_run_fused_1d on the CPU emulation (tests/hipemu), op by op: the cases and checks of
tests/conv1d_fused_cases.py.  Two defects these cases exposed are pinned by name below: a transposed conv as the LAST op
lost its residual (the host placer gave the last op's dst no live range, so it was laid over the residual buffer, which the
slot-clearing step of a transposed conv then wiped), and a max-pool as the last op left `out` unwritten while returning 0."""
import os

import pytest
import torch

import common as CM
import conv1d_fused_cases as T


@pytest.fixture(scope="module")
def emu(emu_lib):
    """The emulated library; three emulator threads for this module (its launches are 1 .. 80 small workgroups, and every
    emulator thread sets up 1024 fibers per launch: more threads cost more than they save)."""
    old = os.environ.get("HIPEMU_THREADS")
    os.environ["HIPEMU_THREADS"] = "3"
    yield emu_lib
    if old is None:
        del os.environ["HIPEMU_THREADS"]
    else:
        os.environ["HIPEMU_THREADS"] = old


# (op, as the last op?): a stack that ends in a pool is refused (test_fused_1d_last_pool_is_refused), so the pool is a middle op only
OP_CASES = [(i, last) for i in range(len(T.OPS)) for last in (True, False) if not (T.OPS[i][1] == "pool" and last)]


@pytest.mark.parametrize("op,last", OP_CASES, ids=[f"{T.OPS[i][0]}-{'last' if last else 'middle'}" for i, last in OP_CASES])
def test_fused_1d_op_within_fp64_bound_and_equal_to_generic(emu, op, last):
    """Every length the op allows at 5 planes, and 1 and 80 planes at an odd and the longest length."""
    o = T.OPS[op]
    worst = T.sweep_op(emu, "cpu", o, last)
    ends = (o[5][4] if len(o[5]) > 4 else o[5][0], o[5][-1])
    worst = max(worst, T.sweep_op(emu, "cpu", o, last, plane_counts=(1, 80), lengths=ends))
    print(f"{o[0]}: worst error / bound {worst:.4f}")


@pytest.mark.parametrize("Z", T.C2C_Z)
@pytest.mark.parametrize("cin", T.C2C_CIN)
def test_fused_1d_c2cnet_layers_within_bound_and_fused_equal_to_generic(emu, cin, Z):
    worst = T.check_c2cnet(emu, "cpu", cin, Z)
    print(f"c2cnet({cin}, {Z}): worst |fused - fp64| / tolerance {worst:.3f}")


@pytest.mark.parametrize("case", range(6), ids=["Z28", "coutp160", "nops33", "last_op_pool", "odd_pool_L5", "odd_pool_L7"])
def test_fused_1d_refusals_leave_the_output_untouched(emu, case):
    T.check_refusal(emu, "cpu", T.refusal_stacks()[case])


@pytest.mark.parametrize("op", ["up_128_64", "up_64_32"])
def test_fused_1d_last_transposed_conv_keeps_its_residual(emu, op):
    """relu(convT(x) + b) + skip as the last op: the skip (|r| up to several units) must be in the output."""
    o = [v for v in T.OPS if v[0] == op][0]
    spec, w, ids = T.op_stack(o, 10, last=True, seed=1)
    x = T.stack_input(spec, 5, 11)
    rc, out, blob, check = T.run_fused(emu, "cpu", spec, w, x)
    assert rc == 0
    check()
    val, err = CM.conv_chain_reference(spec, w, blob, x, split=True)
    assert CM.conv_ratio(out, val[ids["out"]], err[ids["out"]]) <= 1.0
    without = val[ids["out"]] - x.double()                      # what the defect produced: the output without its skip
    assert float((out.double() - without).abs().max()) > 1.0


def test_fused_1d_last_pool_is_refused(emu):
    spec, w, _ = T.op_stack(T.OPS[-1], 8, last=True)
    rc, out, _, check = T.run_fused(emu, "cpu", spec, w, T.stack_input(spec, 3, 1))
    assert rc == T.EINVAL
    check(untouched=True)


@pytest.mark.parametrize("L", [5, 7])
def test_fused_1d_refuses_odd_pools_like_the_generic_interpreter(emu, L):
    spec, w, _ = T.op_stack(T.OPS[-1], L, last=False)
    x = T.stack_input(spec, 2, 1)
    rc, out, _, check = T.run_fused(emu, "cpu", spec, w, x)
    assert rc == T.EINVAL
    check(untouched=True)
    info = {}
    CM.run_custom_conv_stack(emu, "cpu", spec, w, x, info=info, allow_rc=(T.EINVAL,))
    assert info["rc"] == T.EINVAL


def test_fused_1d_product_stack_keeps_its_lds_footprint(emu):
    """The live-range placer must not grow the product's stack: c2cnet_spec(15, 20) takes 10 560 floats of activations, two
    12 288-float weight buffers and two 512-float epilogue slots = 144 640 bytes of dynamic LDS (the figure before every dst
    got a live range of its own)."""
    import ctypes as C

    from faster_voxelpose_amd import netspec
    spec = netspec.c2cnet_spec(15, 20)
    rc, _, _, check = T.run_fused(emu, "cpu", spec, T.random_weights(spec, 1), T.stack_input(spec, 1, 1).abs())
    assert rc == 0
    check()
    emu.hipemu_last_shmem.restype = C.c_size_t
    assert emu.hipemu_last_shmem() == 144640


def test_fused_1d_dead_middle_transposed_conv_leaves_its_neighbours_alone(emu):
    """A transposed conv whose result nobody reads still clears the LDS slots of its dst: they must not lie on a live buffer
    (every dst is live while its op runs).  The stack's result is that of the stack without the dead op."""
    from faster_voxelpose_amd import netspec

    def build(dead):
        s = netspec.StackSpec(1, 64, (1, 12))
        g = torch.Generator().manual_seed(4)
        w = {}
        for key, ci, co, k, tr in (("a", 64, 64, 3, False), ("u", 64, 32, 2, True), ("b", 64, 8, 1, False)):
            s._conv_entries(key, ci, co, k, transposed=tr)
            w[key + ".weight"] = torch.randn(((ci, co) if tr else (co, ci)) + (k,), generator=g) / (ci * (1 if tr else k)) ** 0.5
            w[key + ".bias"] = torch.randn(co, generator=g) * 0.1
        s._conv_entries("k", 64, 32, 1)
        w["k.weight"] = torch.randn(32, 64, 1, generator=g) / 8
        w["k.bias"] = torch.randn(32, generator=g) * 0.1
        h = s.conv("a", None, 0, 64, 3, relu=True)
        p = s.pool(h)
        skip = s.conv("k", None, 0, 32, 1, relu=False)
        if dead:
            s.up("u", None, p, 32, skip)               # result never read
        s.outputs["out"] = s.conv("b", None, h, 8, 1, relu=False, res=None)
        return s.finalize(), w
    x = torch.randn(3, 64, 1, 12, generator=torch.Generator().manual_seed(6))
    outs = []
    for dead in (True, False):
        spec, w = build(dead)
        rc, out, _, check = T.run_fused(emu, "cpu", spec, w, x)
        assert rc == 0
        check()
        outs.append(out.clone())
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
