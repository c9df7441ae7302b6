"""The fused res-block skip (tests/test_wino_skip_fused.py) on the CPU emulation of the kernels (tests/hipemu): the stack
conv3x3 -> (conv1x1 skip) -> conv3x3 + res [-> pool], which fuses, against the same stack with a second reader of the skip,
which launches it - the same words - and against the float64 evaluation with the interval of the GPU test.  Emulator-sized
maps: the own-patch form (W = 64, a row band per unit), both shared-column forms (W = 32, W = 16: several planes, the last
plane group partial where planes share a unit), masked tiles (W = 40), and a person mask."""
import pytest
import torch
import torch.nn.functional as F

import common as CM
from test_wino_skip_fused import skip_stack

# (name, cin, cout, (h, w), pool, planes, plane_valid)
CASES = [
    ("own_patch_16_32_8x64", 16, 32, (8, 64), True, 2, None),
    ("shared_w32_32_64_8x32", 32, 64, (8, 32), True, 3, None),
    ("shared_w16_16_32_16x16", 16, 32, (16, 16), False, 5, None),
    ("masked_16_32_4x40", 16, 32, (4, 40), False, 1, None),
    ("person_mask_32_64_16x16", 32, 64, (16, 16), True, 3, (1, 0, 1)),
]


@pytest.mark.parametrize("case", range(len(CASES)), ids=[c[0] for c in CASES])
def test_emulated_fused_skip_same_words_and_inside_the_fp64_interval(emu_lib, case):
    name, cin, cout, hw, pool, planes, pv = CASES[case]
    x = torch.randn((planes, cin) + hw, generator=torch.Generator().manual_seed(200 + case))
    pvt = None if pv is None else torch.tensor(pv, dtype=torch.uint8)
    v = torch.ones(planes, dtype=torch.bool) if pv is None else pvt.bool()
    res = {}
    for kind, second in (("fused", False), ("second_reader", True)):
        spec, w, ids = skip_stack(cin, cout, hw, pool=pool, second_reader=second, seed=case)
        info = {}
        bufs, check = CM.run_custom_conv_stack(emu_lib, "cpu", spec, w, x, plane_valid=pvt, valid_div=1, poison=True, info=info)
        res[kind] = dict(spec=spec, w=w, ids=ids, bufs=bufs, check=check, blob=info["blob"])
    f, u = res["fused"], res["second_reader"]
    u["check"]()
    # the fused stack must not have written s: its buffer still holds the poison
    s_bits = f["bufs"][f["ids"]["s"]].view(torch.int32)
    assert bool((s_bits == CM.POISON_BITS).all()), "the skip was launched: nothing fused"
    assert torch.equal(f["bufs"][f["ids"]["out"]][v].view(torch.int32), u["bufs"][u["ids"]["out"]][v].view(torch.int32))
    if pool:
        assert torch.equal(f["bufs"][f["ids"]["pool"]][v].view(torch.int32), u["bufs"][u["ids"]["pool"]][v].view(torch.int32))
    # float64: the interval of tests/test_wino_skip_fused.py (WINO_K for the conv, (cin + 3) eps32 for the skip's own chain)
    spec, w, ids = f["spec"], f["w"], f["ids"]
    sc, sh = CM.wino_packed_bn(spec, f["blob"], ids["op"])
    ssc, ssh = CM.wino_packed_bn(spec, f["blob"], ids["skip_op"])
    ssc, ssh = ssc.double().view(1, -1, 1, 1), ssh.double().view(1, -1, 1, 1)
    pw, pb = w["p.weight"].double(), w["p.bias"].double().view(1, -1, 1, 1)
    xv = x[v].double()
    s64 = (F.conv2d(xv, pw) + pb) * ssc + ssh
    smag = ssc.abs() * (F.conv2d(xv.abs(), pw.abs()) + pb.abs()) + ssh.abs()
    ref = CM.wino_reference(w, f["bufs"][ids["h"]][v], s64, sc, sh, relu=True, pool=pool)
    bound = CM.WINO_K * CM.EPS32 * ref["mag"] + (cin + 3) * CM.EPS32 * smag
    err = (f["bufs"][ids["out"]][v].double() - ref["y"]).abs()
    assert bool(torch.isfinite(err).all()) and int((err > bound).sum()) == 0
    if pool:
        perr = (f["bufs"][ids["pool"]][v].double() - ref["p"]).abs()
        assert bool(torch.isfinite(perr).all()) and int((perr > F.max_pool2d(bound, 2)).sum()) == 0
