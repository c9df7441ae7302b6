"""fvp_conv_stack_run_fused_1d (csrc/fvp_conv1d_fused.hip: a whole 1-D conv stack in one kernel, activations in LDS) op by op:
cases, runner, float64 reference.  Shared by tests/test_conv1d_fused_emu.py (CPU emulation) and tests/test_conv1d_fused_gpu.py
(MI355X).  Not a test module.

Short hand-made 1-D stacks in which every op kind is once the LAST op (its epilogue stores to `out`) and once a middle op
observed through a following 1x1 conv; only `in` and `out` exist, so the reference is the float64 chain with the propagated
bound of tests/common.py (conv_chain_reference, split=True: the kernel adds four K slices, three roundings more per op).  The
same stack through the generic interpreter agrees "to rounding": within the sum of the two chain bounds.  Then the whole
C2CNet (netspec.c2cnet_spec) for several joint counts and lengths (see NET_RTOL below), the LDS footprint of the product's
stack, and the refusals with their codes and an untouched output.

Measured: op cases, worst error / bound 0.063 (MI355X and emulator); whole C2CNet, worst |fused - fp64| over the 3e-6
tolerance 0.41 (emulator), 0.36 (MI355X)."""
import ctypes as C

import torch

import common as CM

EINVAL, ELIMIT = 10001, 10002
LENGTHS = (1, 2, 3, 4, 5, 7, 10, 12, 20, 24)

# (name, conv_layer kind, cin, cout, options, lengths the op allows)
OPS = [
    ("c7_15", "conv", 15, 16, dict(k=7, bn=True), LENGTHS),
    ("c7_17", "conv", 17, 16, dict(k=7, bn=True), LENGTHS),
    ("c7_1", "conv", 1, 16, dict(k=7), LENGTHS),
    ("c3_32_64", "conv", 32, 64, dict(k=3, bn=True, res=True), LENGTHS),          # residual: a 1x1 projection earlier in the stack
    ("c3_64_64", "conv", 64, 64, dict(k=3, bn=True, res=True), LENGTHS),          # residual: the input
    ("c3_128_128", "conv", 128, 128, dict(k=3, bn=True, res=True), LENGTHS),
    ("c1_32_1", "conv", 32, 1, dict(k=1, relu=False), LENGTHS),
    ("up_128_64", "up", 128, 64, dict(bn=True), tuple(v for v in LENGTHS if v <= 12)),   # output length 2 L <= 24
    ("up_64_32", "up", 64, 32, dict(bn=True), tuple(v for v in LENGTHS if v <= 12)),
    ("pool", "pool", 20, 20, dict(), tuple(v for v in LENGTHS if v % 2 == 0)),
]
TAIL = 8           # couts of the 1x1 conv behind a middle op


def op_stack(op, L, last, seed=0):
    """The finalized spec of one case: the op as the last op, or followed by a 1x1 conv."""
    name, kind, cin, cout, opts, _ = op
    opts = dict(opts)
    if not last:
        opts["head" if kind == "up" else "tail"] = TAIL
    return CM.conv_layer(kind, cin, cout, (1, L), dim=1, seed=seed, **opts)


def random_weights(spec, seed=0):
    """Random parameters for every entry of a spec built from the reference blocks (netspec.c2cnet_spec): conv weights
    ~ N(0, 1 / fan-in), BN scales of both signs."""
    g = torch.Generator().manual_seed(seed)
    w = {}
    for key, (shape, _) in spec.entries.items():
        if key.endswith("num_batches_tracked"):
            continue
        if key.endswith("running_var"):
            w[key] = 0.5 + torch.rand(shape, generator=g)
        elif key.endswith("running_mean"):
            w[key] = torch.randn(shape, generator=g) * 0.1
        elif len(shape) > 1:
            transposed = any(k == key[:-len(".weight")] and tr for k, _, tr, _ in spec.param_keys)
            fan = (shape[0] if transposed else shape[1] * int(torch.tensor(shape[2:]).prod()))
            w[key] = torch.randn(shape, generator=g) / fan ** 0.5
        elif key.endswith(".weight"):            # BN scale
            w[key] = (0.5 + torch.rand(shape, generator=g)) * torch.where(torch.rand(shape, generator=g) < 0.3, -1.0, 1.0)
        else:
            w[key] = torch.randn(shape, generator=g) * 0.1
    return w


def run_fused(lib, device, spec, weights, x, blob=None):
    """fvp_conv_stack_run_fused_1d on x [planes, cin, 1, L] with poisoned, guarded (on the emulator: fenced) `in` and `out`.
    Returns (rc, out [planes, cout, 1, L'], blob, check); check(untouched=False) asserts intact guards, no fenced read and a
    finite output - or, with untouched=True, an output that still holds its poison."""
    if blob is None:
        blob = CM.pack_custom_conv_stack(lib, device, spec, weights, torch.zeros(max(spec.nparams, 4), device=device))
    planes = x.shape[0]
    G = CM.POISON_GUARD
    oshape = (planes,) + tuple(spec.bufs[spec.op_array[len(spec.ops) - 1].dst])
    flats = []
    for shape in (tuple(x.shape), oshape):
        n = 1
        for v in shape:
            n *= v
        flats.append(torch.full((n + 2 * G,), CM.POISON_BITS, dtype=torch.int32, device=device).view(torch.float32))
    xin = flats[0][G:G + x.numel()].view(x.shape)
    xin.copy_(x.to(device))
    out = flats[1][G:flats[1].numel() - G].view(oshape)
    fence = device == "cpu" and hasattr(lib, "hipemu_fence")
    if fence:
        lib.hipemu_fence.argtypes = [C.c_void_p, C.c_size_t]
        lib.hipemu_fenced_reads.restype = C.c_long
        lib.hipemu_fences_clear()
        for f in flats:
            lib.hipemu_fence(C.c_void_p(f.data_ptr()), 4 * G)
            lib.hipemu_fence(C.c_void_p(f.data_ptr() + 4 * (f.numel() - G)), 4 * G)
    rc = lib.fvp_conv_stack_run_fused_1d(spec.op_array, len(spec.ops), C.c_void_p(blob.data_ptr()), C.c_void_p(xin.data_ptr()),
                                         C.c_void_p(out.data_ptr()), planes, None)
    reads = 0
    if fence:
        reads = int(lib.hipemu_fenced_reads())
        lib.hipemu_fences_clear()

    def check(untouched=False):
        assert reads == 0, f"{reads} reads of guard words"
        for i, f in enumerate(flats):
            bits = f.view(torch.int32)
            bad = int((bits[:G] != CM.POISON_BITS).sum()) + int((bits[bits.numel() - G:] != CM.POISON_BITS).sum())
            assert bad == 0, f"{'in' if i == 0 else 'out'}: {bad} guard words changed (out-of-bounds write)"
        obits = out.contiguous().view(torch.int32)
        if untouched:
            assert bool((obits == CM.POISON_BITS).all()), "the output was written"
        else:
            nf = int((~torch.isfinite(out)).sum())
            assert nf == 0, f"out: {nf} non-finite elements (unwritten, or computed from unmasked memory)"
    return rc, out, blob, check


# Whole nets.  The propagated worst-case bound of conv_chain_reference multiplies the magnitudes of |w| layer after layer: sharp
# for two or three ops, vacuous through the 26 ops of C2CNet (1e11).  There the generic interpreter, which stores every
# layer, is held to the per-op bound layer by layer (common.conv_stack_ratio: each op against the float64 evaluation of its
# own stored inputs), and the fused kernel - which differs from it only by the order in which an op's products are added -
# is held to the generic result, and both to the float64 chain, at the tolerance the suite's whole-net comparison already
# uses (tests/test_emu_kernels.py::test_fused_c2c_equals_generic_interpreter).
NET_RTOL = NET_ATOL = 3e-6


def check_stack(lib, device, spec, weights, x, what, also_planes=()):
    """One stack: fused within the fp64 bound, guards and finiteness, and fused = generic to rounding; for every count in
    ``also_planes`` the first planes alone give the same bits (one workgroup per plane).  Returns the worst error / bound of
    the fused run (whole nets: the worst |fused - fp64| / (NET_ATOL + NET_RTOL |fp64|))."""
    rc, out, blob, check = run_fused(lib, device, spec, weights, x)
    assert rc == 0, f"{what}: fvp_conv_stack_run_fused_1d returned {rc}"
    check()
    CM.conv_check_packed_epi(spec, weights, blob)
    last = spec.op_array[len(spec.ops) - 1].dst
    gbufs = CM._run_packed_conv_stack(lib, device, spec, blob, x, None, None, 1, False, None, ())
    generic = gbufs[last].cpu()
    got = out.cpu()
    if len(spec.ops) > 6:
        layers = CM.conv_stack_ratio(spec, weights, blob, gbufs)
        assert layers <= 1.0, f"{what}: generic interpreter, worst layer error / bound {layers:.3g}"
        y64 = CM.conv_chain_reference(spec, weights, blob, x)[0][last]
        tol = NET_ATOL + NET_RTOL * y64.abs()
        ratio = CM.conv_ratio(got, y64, tol)
        assert ratio <= 1.0, f"{what}: |fused - fp64| / tolerance {ratio:.3g}"
        rg = CM.conv_ratio(generic, y64, tol)
        assert rg <= 1.0, f"{what}: |generic - fp64| / tolerance {rg:.3g}"
        both = CM.conv_ratio(got, generic.double(), NET_ATOL + NET_RTOL * generic.double().abs())
        assert both <= 1.0, f"{what}: |fused - generic| / tolerance {both:.3g}"
    else:
        val, err = CM.conv_chain_reference(spec, weights, blob, x, split=True)
        y64, b_f = val[last], err[last]
        b_g = CM.conv_chain_reference(spec, weights, blob, x, split=False)[1][last]
        ratio = CM.conv_ratio(got, y64, b_f)
        assert ratio <= 1.0, f"{what}: fused error / bound {ratio:.3g}"
        both = CM.conv_ratio(got, generic.double(), b_f + b_g)
        assert both <= 1.0, f"{what}: |fused - generic| / (sum of their bounds) {both:.3g}"
        rg = CM.conv_ratio(generic, y64, b_g)
        assert rg <= 1.0, f"{what}: generic interpreter error / bound {rg:.3g}"
    for n in also_planes:
        rc, few, _, check = run_fused(lib, device, spec, weights, x[:n], blob=blob)
        assert rc == 0
        check()
        assert torch.equal(few.cpu().view(torch.int32), out[:n].cpu().contiguous().view(torch.int32)), f"{what}: {n} planes alone differ"
    return ratio


def stack_input(spec, planes, seed):
    return torch.randn((planes,) + tuple(spec.bufs[0]), generator=torch.Generator().manual_seed(seed))


def refusal_stacks():
    """(name, spec, weights, error code): stacks the fused entry refuses; the output must stay untouched."""
    from faster_voxelpose_amd import netspec
    out = []
    s = netspec.c2cnet_spec(15, 28)
    out.append(("Z28", s, random_weights(s, 1), ELIMIT))
    spec, w, _ = CM.conv_layer("conv", 8, 130, (1, 8), dim=1, k=1)
    out.append(("coutp160", spec, w, ELIMIT))
    s = netspec.StackSpec(1, 4, (1, 8))
    w = {}
    g = torch.Generator().manual_seed(2)
    b = 0
    for i in range(33):
        s._conv_entries(f"c{i}", 4, 4, 1)
        w[f"c{i}.weight"] = torch.randn(4, 4, 1, generator=g) * 0.5
        w[f"c{i}.bias"] = torch.randn(4, generator=g) * 0.1
        b = s.conv(f"c{i}", None, b, 4, 1, relu=True)
    out.append(("nops33", s.finalize(), w, ELIMIT))
    spec, w, _ = op_stack(OPS[-1], 8, last=True)
    out.append(("last_op_pool", spec, w, EINVAL))
    for L in (5, 7):
        spec, w, _ = op_stack(OPS[-1], L, last=False)
        out.append((f"odd_pool_L{L}", spec, w, EINVAL))
    return out


# ---- the checks, shared by the emulator and the GPU module ---------------------------------------------------------------
def sweep_op(lib, device, op, last, plane_counts=(5,), lengths=None):
    """Every allowed length of one op case (as the last op, or as a middle op); returns the worst error / bound."""
    worst = 0.0
    for planes in plane_counts:
        for L in (op[5] if lengths is None else [v for v in lengths if v in op[5]]):
            spec, w, _ = op_stack(op, L, last, seed=L)
            x = stack_input(spec, planes, 100 * L + planes)
            worst = max(worst, check_stack(lib, device, spec, w, x, f"{op[0]} {'last' if last else 'middle'} L={L} planes={planes}"))
    return worst


C2C_CIN = (1, 15, 17, 32)
C2C_Z = (4, 8, 12, 16, 20, 24)


def check_c2cnet(lib, device, cin, Z, plane_counts=(1, 5)):
    from faster_voxelpose_amd import netspec
    spec = netspec.c2cnet_spec(cin, Z)
    w = random_weights(spec, seed=cin * 100 + Z)
    x = stack_input(spec, max(plane_counts), cin + Z).abs()           # heatmap columns: non-negative
    return check_stack(lib, device, spec, w, x, f"c2cnet({cin}, {Z})", also_planes=[n for n in plane_counts if n != max(plane_counts)])


def check_refusal(lib, device, case):
    name, spec, w, code = case
    x = stack_input(spec, 3, 5)
    rc, out, _, check = run_fused(lib, device, spec, w, x)
    assert rc == code, f"{name}: returned {rc}, expected {code}"
    check(untouched=True)
