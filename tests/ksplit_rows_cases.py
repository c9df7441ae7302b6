"""Case table and runner of the split-K 3x3 conv with several pixel blocks per workgroup (k_conv_dma<3,3,1,PB,0,0,1>, PB = 2 / 4:
ksplit_blocks() in csrc/fvp_conv.hip), shared by tests/test_ksplit_rows_emu.py (CPU emulation) and
tests/test_ksplit_rows_gpu.py (MI355X, diagnostics build).  Not a test module.

One conv op per case (a 1x1 projection in front of it where the residual needs other channels, as conv_form_cases builds
it), driven through fvp_conv_stack_run with every op's wino_off = 0, so that maps the Winograd kernel would take (18 x 32,
and every width on the emulated session, which runs with FVP_WINO_GENERIC=1) reach the split-K form.  FVP_CONV_KS_PB is read
per call by the diagnostics build (and the emulated library, which is one): a case runs the same inputs with 1, 2 and 4.

run_case() asserts, for PB = 2 and 4:
  (1) array_equal (bit for bit) with the one-block form on the same inputs - csrc/fvp_conv.hip: "the bits do not depend on
      the choice";
  (2) the fp64 bound of tests/common.py for split K (conv_stack_ratio(split=True): (cinp * 9 + 3 + 3) * eps32), the rule and
      helper of the KSplit rows of tests/conv_form_cases.py;
  (3) where the library keeps a launch log (the emulator), that it names k_conv_dma<3,3,1,PB,0,0,1>;
and under a person mask (plane_valid, valid_div = 3): valid planes keep their bits, masked planes keep their poison.

Tile shapes (TH rows of the map per workgroup = 32 * PB // w):
    20 x 20   PB 2: 3 rows (60 of 64 lanes), 7 tiles, the last of 2 rows;  PB 4: 6 rows, 4 tiles, the last of 2 rows
    21 x 24   PB 2: 2 rows (48 of 64 lanes), 11 tiles, the last of 1 row;  PB 4: 5 rows, 5 tiles, the last of 1 row
    18 x 32   PB 2: 2 rows, PB 4: 4 rows, every lane used;  the last tile of PB 4 has 2 rows
    23 x 12   PB 2: 5 rows, the last tile 3;  PB 4: 10 rows, the last tile 3
    64 x 4    PB 2: 16 rows,  PB 4: 32 rows
Channels: 64 -> 32, 128 -> 128 (four cout blocks), 72 -> 17 (a ragged cout block; cinp = 72 is not a multiple of 16: chunks
of 8 or 24 channels).  Every map runs with every channel set and with 1 and 3 planes; the epilogues (residual before the ReLU
with a BN, residual after the ReLU, no ReLU, plain) rotate over the table so that every map and every channel set meets each."""
import collections
import os

import torch

import common as CM
import conv_form_cases as T

Case = collections.namedtuple("Case", "name cin cout hw planes opts")

MAPS = ((20, 20), (21, 24), (18, 32), (23, 12), (64, 4))
CHANNELS = ((64, 32), (128, 128), (72, 17))
EPILOGUES = (dict(res=True, bn=True), dict(res=True, res_after=True), dict(relu=False), dict())
_EPI_NAMES = ("res_bn", "res_after", "norelu", "plain")


def _cases():
    out = []
    for mi, hw in enumerate(MAPS):
        for ci, (cin, cout) in enumerate(CHANNELS):
            e = (mi + ci) % 4
            # planes: 1 and 3 alternate over the table; the second epilogue of the pair runs with the other count
            for planes, ee in ((1 + 2 * ((mi + ci) % 2), e), (3 - 2 * ((mi + ci) % 2), (e + 2) % 4)):
                out.append(Case(f"{hw[0]}x{hw[1]}_{cin}_{cout}_p{planes}_{_EPI_NAMES[ee]}", cin, cout, hw, planes, EPILOGUES[ee]))
    return out


CASES = _cases()

# the natural rule (no switch): 64 rows x 9 planes x 1 cout block = 576 > 512 workgroups at one row each -> two blocks
# (4 tiles x 9 planes = 36 workgroups fit); 2 planes: 128 -> one block
NATURAL = Case("natural_64x4_64_32", 64, 32, (64, 4), 9, dict())
NATURAL_FEW_PLANES = 2


def ks(pb):
    return T.dma(3, 3, 1, pb, ks=1)


def _bits(t):
    return t.contiguous().view(torch.int32)


def build(case, seed):
    """(spec, weights, ids, x) of a case; every op's Winograd copy dropped (wino_off = 0)."""
    spec, w, ids = CM.conv_layer("conv", case.cin, case.cout, case.hw, k=3, seed=seed, **case.opts)
    for i in range(len(spec.ops)):
        spec.op_array[i].wino_off = 0
    x = torch.randn((case.planes,) + spec.bufs[0], generator=torch.Generator().manual_seed(500 + seed))
    return spec, w, ids, x


def run_once(lib, device, spec, w, x, pb, pv=None, vd=1):
    """One run under FVP_CONV_KS_PB = pb (None: no switch).  Returns (buffers, blob, launched instantiations or None)."""
    emu = device == "cpu"
    old = os.environ.get("FVP_CONV_KS_PB")
    if pb is None:
        os.environ.pop("FVP_CONV_KS_PB", None)
    else:
        os.environ["FVP_CONV_KS_PB"] = str(pb)
    try:
        info = {}
        if emu:
            lib.hipemu_launch_log_reset()
        bufs, check = CM.run_custom_conv_stack(lib, device, spec, w, x.to(device), plane_valid=pv, valid_div=vd, poison=True, info=info)
        insts = T.instantiations(lib.hipemu_launch_log().decode()) if emu else None
        check()
    finally:
        if old is None:
            os.environ.pop("FVP_CONV_KS_PB", None)
        else:
            os.environ["FVP_CONV_KS_PB"] = old
    return [b.cpu() for b in bufs], info["blob"], insts


def run_case(lib, device, case, index):
    """Assertions (1) - (3) and the mask check of one forced case; returns the worst error / bound over PB = 1, 2, 4."""
    spec, w, ids, x = build(case, index)
    out = ids["out"]
    one, blob, insts = run_once(lib, device, spec, w, x, 1)
    if insts is not None:
        assert insts[-1] == ks(1), f"{case.name}: FVP_CONV_KS_PB=1 launched {insts}"
    worst = CM.conv_stack_ratio(spec, w, blob, one, split=True)
    print(f"{case.name}: PB 1 worst error / bound {worst:.4f}")
    assert worst <= 1.0, f"{case.name}: PB 1: error / bound {worst:.3g}"
    # person mask: groups of three planes, the first group masked where there is a second one
    vd = 3
    ng = -(-case.planes // vd)
    pv = torch.ones(ng, dtype=torch.uint8)
    if case.planes == 1:
        pv[0] = 0                                        # the only plane is masked: nothing may be written
    valid = pv.bool()[torch.arange(case.planes) // vd]
    for pb in (2, 4):
        got, blob_pb, insts = run_once(lib, device, spec, w, x, pb)
        ratio = CM.conv_stack_ratio(spec, w, blob_pb, got, split=True)                         # (2)
        print(f"{case.name}: PB {pb} worst error / bound {ratio:.4f}")
        assert ratio <= 1.0, f"{case.name}: PB {pb}: error / bound {ratio:.3g}"
        worst = max(worst, ratio)
        assert torch.equal(_bits(got[out]), _bits(one[out])), f"{case.name}: PB {pb} differs from the one-block form"   # (1)
        if insts is not None:
            assert insts[-1] == ks(pb), f"{case.name}: FVP_CONV_KS_PB={pb} launched {insts}"  # (3)
        masked, _, _ = run_once(lib, device, spec, w, x, pb, pv, vd)
        assert torch.equal(_bits(masked[out][valid]), _bits(one[out][valid])), f"{case.name}: PB {pb}: valid planes differ under the mask"
        assert bool((_bits(masked[out][~valid]) == CM.POISON_BITS).all()), f"{case.name}: PB {pb}: masked planes were written"
    return worst


def run_mask_case(lib, device, index=100):
    """Seven planes of 20 x 20, valid_div = 3, groups valid / masked / valid: planes 3 - 5 keep their poison under PB = 2 and 4,
    the others the bits of the unmasked one-block run."""
    case = Case("mask_20x20_64_32_p7", 64, 32, (20, 20), 7, dict(res=True, bn=True))
    spec, w, ids, x = build(case, index)
    out = ids["out"]
    one, _, _ = run_once(lib, device, spec, w, x, 1)
    pv = torch.tensor([1, 0, 1], dtype=torch.uint8)
    valid = pv.bool()[torch.arange(7) // 3]
    for pb in (2, 4):
        masked, _, _ = run_once(lib, device, spec, w, x, pb, pv, 3)
        assert torch.equal(_bits(masked[out][valid]), _bits(one[out][valid])), f"PB {pb}: valid planes differ under the mask"
        assert bool((_bits(masked[out][~valid]) == CM.POISON_BITS).all()), f"PB {pb}: masked planes were written"


def run_natural(lib, device, index=200):
    """No switch: 9 planes take the two-block instance, 2 planes the one-block one; same bits as the forced one-block form, and
    the fp64 bound.  Returns the launched instantiations of (9 planes, 2 planes), None without a launch log."""
    spec, w, ids, x = build(NATURAL, index)
    out = ids["out"]
    one, _, _ = run_once(lib, device, spec, w, x, 1)
    nat, blob, insts9 = run_once(lib, device, spec, w, x, None)
    ratio = CM.conv_stack_ratio(spec, w, blob, nat, split=True)
    print(f"{NATURAL.name}: worst error / bound {ratio:.4f}")
    assert ratio <= 1.0, f"{NATURAL.name}: error / bound {ratio:.3g}"
    assert torch.equal(_bits(nat[out]), _bits(one[out])), "the planner's choice at 9 planes differs from the one-block form"
    few, _, insts2 = run_once(lib, device, spec, w, x[:NATURAL_FEW_PLANES], None)
    assert torch.equal(_bits(few[out]), _bits(one[out][:NATURAL_FEW_PLANES])), "2 planes differ from the first 2 of 9"
    return insts9, insts2
