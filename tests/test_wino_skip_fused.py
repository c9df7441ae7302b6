"""The res-block's 1x1 skip conv computed in the epilogue of the block's second 3x3 Winograd conv (csrc/fvp_conv.hip:
fused_skip(); csrc/fvp_conv_wino_body.h: SKIP; kernels k_conv_wino_skip / k_conv_wsc_skip) on the MI355X, shipped library.

  (1) bit equality against the unfused path of the same library: the stack  conv3x3 -> (conv1x1 skip) -> conv3x3 + res
      [-> pool]  fuses; the same stack with one more 1x1 conv that also reads s has a second reader of s, so the planner
      launches the skip on its own.  The res conv's output and the pooled output must be the same words.
  (2) the fused cases against a float64 evaluation, inside the a-priori interval of tests/common.py (WINO_K) - 0 elements
      outside.  There the residual is the device's own buffer; here s exists in no buffer, so the reference takes the
      float64 s and the interval grows by the skip's own a-priori error: a chain of cin fmas plus bias add, BN fma (and one
      for the rounding of the float64 s itself), (cin + 3) eps32 (|scale| (conv(|x|, |w|) + |b|) + |shift|).
  (3) the planner: launches counted by the per-launch profiler (level 2).

The 64 -> 128 block at 16x16 is part of (1) and (2) as the issue lists it, but the planner does NOT fuse it (the cin <= 32
shape rule of fused_skip(): 32 KB of skip weights do not fit beside that conv's LDS ring); (3) asserts that, so for this
case (1) compares two unfused runs."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import common as CM

pytestmark = pytest.mark.gpu

# (name, cin, cout, (h, w), pool, planes, plane_valid)
CASES = [
    ("own_patch_16_32_64x64", 16, 32, (64, 64), True, 5, None),
    ("shared_w32_32_64_32x32", 32, 64, (32, 32), True, 5, None),
    ("shared_w16_64_128_16x16", 64, 128, (16, 16), False, 5, None),
    ("masked_16_32_80x80", 16, 32, (80, 80), False, 1, None),
    ("masked_32_64_40x40", 32, 64, (40, 40), False, 1, None),
    ("person_mask_16_32_64x64", 16, 32, (64, 64), True, 3, (1, 0, 1)),
    # The cases above run quarter-size units (few planes).  The same two blocks at the plane counts from which the planner
    # takes half-size (4-wave workgroups) and full-size units (>= 256 units: the 8-wave forms every large batch runs)
    ("own_patch_half_16_32_64x64", 16, 32, (64, 64), True, 17, None),
    ("own_patch_full_16_32_64x64", 16, 32, (64, 64), True, 33, None),
    ("shared_w32_half_32_64_32x32", 32, 64, (32, 32), True, 20, None),
    ("shared_w32_full_32_64_32x32", 32, 64, (32, 32), True, 65, None),
]
FUSES = {name: cin <= 32 for name, cin, *_ in CASES}


def skip_stack(cin, cout, hw, *, pool=False, second_reader=False, skip_relu=False, seed=0):
    """conv3x3 cin -> cout (BN, ReLU); skip = BN(conv1x1(x)); conv3x3 cout -> cout + skip (BN, ReLU) [; pool]
    [; one more 1x1 conv on the skip].  Returns (spec, weights, ids)."""
    from faster_voxelpose_amd import netspec
    spec = netspec.StackSpec(2, cin, hw)
    for key, ci, k in (("a", cin, 3), ("p", cin, 1), ("c", cout, 3)):
        spec._conv_entries(key, ci, cout, k)
        spec._bn_entries(key + "n", cout)
    h = spec.conv("a", "an", 0, cout, 3, relu=True)
    s = spec.conv("p", "pn", 0, cout, 1, relu=skip_relu)
    o = spec.conv("c", "cn", h, cout, 3, relu=True, res=s)
    ids = dict(h=h, s=s, out=o, op=len(spec.ops) - 1, skip_op=len(spec.ops) - 2, pool=spec.pool(o) if pool else None)
    if second_reader:
        spec._conv_entries("q", cout, cout, 1)
        ids["q"] = spec.conv("q", None, s, cout, 1, relu=False)
    spec.outputs["out"] = o
    spec.finalize()
    g = torch.Generator().manual_seed(seed)
    wt = {}
    for key, ci, k in (("a", cin, 3), ("p", cin, 1), ("c", cout, 3)) + ((("q", cout, 1),) if second_reader else ()):
        wt[key + ".weight"] = torch.randn(cout, ci, k, k, generator=g) / (ci * k * k) ** 0.5
        wt[key + ".bias"] = torch.randn(cout, generator=g) * 0.1
        if key != "q":
            wt[key + "n.weight"] = (0.5 + torch.rand(cout, generator=g)) * torch.where(torch.rand(cout, generator=g) < 0.3, -1.0, 1.0)
            wt[key + "n.bias"] = torch.randn(cout, generator=g) * 0.2
            wt[key + "n.running_mean"] = torch.randn(cout, generator=g) * 0.1
            wt[key + "n.running_var"] = 0.5 + torch.rand(cout, generator=g)
    return spec, wt, ids


@pytest.fixture(scope="module")
def lib():
    from faster_voxelpose_amd import _capi as capi
    return capi.load()


def _launches(lib, run):
    """Launches of every profiler class made by ``run()`` (fvp_prof_enable(2): one entry per launch)."""
    from faster_voxelpose_amd import _capi as capi
    lib.fvp_prof_reset()
    lib.fvp_prof_enable(2)
    try:
        run()
        torch.cuda.synchronize()
        total = 0
        for cls in range(capi.K_COUNT):
            ms, n, fl = C.c_double(), C.c_int64(), C.c_double()
            lib.fvp_prof_read(cls, C.byref(ms), C.byref(n), C.byref(fl))
            total += int(n.value)
    finally:
        lib.fvp_prof_enable(0)
        lib.fvp_prof_reset()
    return total


@pytest.fixture(scope="module")
def runs(lib):
    """Every case once: the fusing stack and the second-reader stack on the same weights and input."""
    out = {}
    for i, (name, cin, cout, hw, pool, planes, pv) in enumerate(CASES):
        x = torch.randn((planes, cin) + hw, generator=torch.Generator().manual_seed(100 + i))
        pvt = None if pv is None else torch.tensor(pv, dtype=torch.uint8)
        r = dict(x=x, valid=torch.ones(planes, dtype=torch.bool) if pv is None else pvt.bool())
        for kind, second in (("fused", False), ("second_reader", True)):
            spec, w, ids = skip_stack(cin, cout, hw, pool=pool, second_reader=second, seed=i)
            info = {}
            box = {}

            def go():
                box["bufs"], box["check"] = CM.run_custom_conv_stack(lib, "cuda", spec, w, x, plane_valid=pvt, valid_div=1,
                                                                    poison=True, info=info)
            n = _launches(lib, go)
            r[kind] = dict(spec=spec, w=w, ids=ids, bufs=box["bufs"], check=box["check"], blob=info["blob"], launches=n)
        out[name] = r
    return out


@pytest.mark.parametrize("case", [c[0] for c in CASES])
def test_fused_skip_same_words_as_launched_skip(runs, case):
    r = runs[case]
    f, u = r["fused"], r["second_reader"]
    v = r["valid"]
    # the second-reader stack has one op more (the extra 1x1 conv); the fusing one saves the skip's launch
    assert u["launches"] - f["launches"] == (2 if FUSES[case] else 1), (f["launches"], u["launches"])
    assert torch.equal(f["bufs"][f["ids"]["out"]].cpu()[v].view(torch.int32), u["bufs"][u["ids"]["out"]].cpu()[v].view(torch.int32))
    if f["ids"]["pool"] is not None:
        assert torch.equal(f["bufs"][f["ids"]["pool"]].cpu()[v].view(torch.int32),
                           u["bufs"][u["ids"]["pool"]].cpu()[v].view(torch.int32))
    # out-of-bounds writes and unwritten outputs; the fused stack never writes s, so only the other buffers are looked at
    u["check"]()
    for b in (f["ids"]["h"], f["ids"]["out"], f["ids"]["pool"]):
        if b is not None:
            assert bool(torch.isfinite(f["bufs"][b][v.to("cuda")]).all())


@pytest.mark.parametrize("case", [c[0] for c in CASES])
def test_fused_skip_vs_fp64(runs, case):
    r = runs[case]
    f = r["fused"]
    spec, w, ids, v = f["spec"], f["w"], f["ids"], r["valid"]
    x = r["x"][v]
    sc, sh = CM.wino_packed_bn(spec, f["blob"], ids["op"])
    ssc, ssh = CM.wino_packed_bn(spec, f["blob"], ids["skip_op"])
    ssc, ssh = ssc.double().view(1, -1, 1, 1), ssh.double().view(1, -1, 1, 1)
    pw, pb = w["p.weight"].double(), w["p.bias"].double().view(1, -1, 1, 1)
    s64 = (F.conv2d(x.double(), pw) + pb) * ssc + ssh
    smag = ssc.abs() * (F.conv2d(x.double().abs(), pw.abs()) + pb.abs()) + ssh.abs()
    cin = x.shape[1]
    h = f["bufs"][ids["h"]].cpu()[v]
    pool = ids["pool"] is not None
    ref = CM.wino_reference(w, h, s64, sc, sh, relu=True, pool=pool)
    bound = CM.WINO_K * CM.EPS32 * ref["mag"] + (cin + 3) * CM.EPS32 * smag
    y = f["bufs"][ids["out"]].cpu()[v].double()
    err = (y - ref["y"]).abs()
    assert bool(torch.isfinite(err).all())
    print(f"{case}: worst error / bound {float((err / bound).max()):.4f}")
    assert int((err > bound).sum()) == 0
    if pool:
        p = f["bufs"][ids["pool"]].cpu()[v].double()
        perr = (p - ref["p"]).abs()
        assert bool(torch.isfinite(perr).all())
        assert int((perr > F.max_pool2d(bound, 2)).sum()) == 0


def test_planner_launches_what_it_cannot_fuse(lib):
    """One launch fewer for the fusable stack is asserted per case above.  Here: a skip with a ReLU, a skip whose reader is not
    a Winograd conv (20x20: the direct kernel), a skip with 15 channels and the 64 -> 128 skip (the cin <= 32 shape rule) keep
    their launch: three convs, three launches."""
    def count(cin, cout, hw, **kw):
        spec, w, ids = skip_stack(cin, cout, hw, **kw)
        x = torch.randn((2, cin) + hw, generator=torch.Generator().manual_seed(7))
        return _launches(lib, lambda: CM.run_custom_conv_stack(lib, "cuda", spec, w, x))

    assert count(16, 32, (32, 32)) == 2                       # fuses
    assert count(16, 32, (32, 32), skip_relu=True) == 3
    assert count(16, 32, (20, 20)) == 3
    assert count(15, 32, (32, 32)) == 3
    assert count(64, 128, (16, 16)) == 3
