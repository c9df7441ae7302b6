"""k_conv_wino (Winograd F(2x2,3x3), csrc/fvp_conv_wino.hip) layer by layer without a GPU: the sensitivity of the fp64 error
bound of tests/common.py (pure torch), then the kernel on the CPU emulation (tests/hipemu) at its edge shapes, with poisoned
buffers and the bound, under the kernel-form switches (child processes), and the closure of its instantiations: every
k_conv_wino<...> of the shipped library is launched by some emulated case or listed as unreachable."""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

import common as CM
import wino_emu_child as WE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "faster-voxelpose_amd", "libfvp_hip.so")


# ---- 1. the bound rejects subtly wrong results (pure torch) ------------------------------------------------------------
def _ref_padded(w, b, xp, r, s, t, relu=True, res_after=False, relu_first=False):
    """float64 layer on an explicitly padded input xp [P, cin, H+2, W+2] (the halo as a kernel would stage it)."""
    z = F.conv2d(xp, w, None) + b.view(1, -1, 1, 1)
    y = z * s.view(1, -1, 1, 1) + t.view(1, -1, 1, 1)
    if r is not None and not res_after and not relu_first:
        y = y + r
    if relu:
        y = torch.relu(y)
    if r is not None and (res_after or relu_first):
        y = y + r
    return y


@pytest.mark.parametrize("cin,cout,hw", [(8, 64, (8, 8)), (32, 64, (16, 16)), (128, 128, (16, 16)), (12, 96, (10, 40))])
def test_wino_bound_rejects_mutated_references(cin, cout, hw):
    """Each mutation a subtly wrong kernel could make, applied to the float64 reference, must break the bound of
    tests/common.py (WINO_K) somewhere; the clean reference rounded to fp32 must stay within it."""
    g = torch.Generator().manual_seed(cin * 7 + cout)
    P, (H, W) = 3, hw
    spec, wt, ids = CM.wino_layer(cin, cout, hw, res=True, bn=True, seed=cin)
    w, b = wt["c.weight"].double(), wt["c.bias"].double()
    s = (wt["n.weight"] / torch.sqrt(wt["n.running_var"] + 1e-5)).double()
    t = wt["n.bias"].double() - wt["n.running_mean"].double() * s
    x = torch.randn(P, cin, H, W, generator=g, dtype=torch.float64).relu()      # post-ReLU activations, as in the product
    r = torch.randn(P, cout, H, W, generator=g, dtype=torch.float64)
    xp = F.pad(x, (1, 1, 1, 1))
    y64 = _ref_padded(w, b, xp, r, s, t)
    mag = s.abs().view(1, -1, 1, 1) * (F.conv2d(x.abs(), w.abs(), None, padding=1) + b.abs().view(1, -1, 1, 1)) \
        + t.abs().view(1, -1, 1, 1) + r.abs()
    assert CM.wino_ratio(y64.float(), y64, mag) <= 1.0
    # the same through wino_reference (the function the kernel tests use)
    ref = CM.wino_reference(wt, x.float(), r.float(), s.float(), t.float())
    assert CM.wino_ratio(y64.float(), ref["y"], ref["mag"]) <= 1.0
    co, ci = cout - 3, cin // 2
    mutants = {}
    w1 = w.clone()
    w1[co, ci] = 0.0
    mutants["input channel dropped for one cout"] = _ref_padded(w1, b, xp, r, s, t)
    w2 = w.clone()
    w2[co, ci, 2, 0] = 0.0
    mutants["one 3x3 tap zeroed"] = _ref_padded(w2, b, xp, r, s, t)
    xt = xp.clone()
    xt[1:, :, 0, 1:-1] = x[:-1, :, -1, :]                   # top halo row = the last row of the previous plane
    mutants["top halo row from the neighbouring plane"] = _ref_padded(w, b, xt, r, s, t)
    xb = xp.clone()
    xb[:-1, :, -1, 1:-1] = x[1:, :, 0, :]                   # bottom halo row = the first row of the next plane
    mutants["bottom halo row from the neighbouring plane"] = _ref_padded(w, b, xb, r, s, t)
    xr = xp.clone()
    xr[:, :, 1:-2, -1] = x[:, :, 1:, 0]                     # right halo column = column 0 of the next row
    mutants["right halo column wrapped from the next row"] = _ref_padded(w, b, xr, r, s, t)
    mutants["residual of the neighbouring plane"] = _ref_padded(w, b, xp, r.roll(1, dims=0), s, t)
    s2, t2 = s.clone(), t.clone()
    s2[32:64], t2[32:64] = s[0:32], t[0:32]
    mutants["BN of 32-cout block 0 applied to block 1"] = _ref_padded(w, b, xp, r, s2, t2)
    mutants["ReLU before the residual"] = _ref_padded(w, b, xp, r, s, t, relu_first=True)
    for name, ym in mutants.items():
        ratio = CM.wino_ratio(ym.float(), y64, mag)
        assert ratio > 1.0, f"{name}: error / bound {ratio:.3g} - the bound would not catch it"


# ---- 2. emulated layers -----------------------------------------------------------------------------------------------
# (cin, cout, (h, w), planes, layer options).  Channel counts: one chunk (4), CC = 8 vs CC = 4 (8 / 12 / 20), odd chunk counts,
# stacks of 1-2 chunks whose DMA ring (two chunks ahead) crosses units; cout 64 / 128: several 32-cout blocks (ysplit > 1).
# Maps: 8x8 / 16x16 (several planes per unit, ragged last plane group), 20x64 / 64x8 (ragged last row band, tall and thin),
# 40x40 / 48x48 / 80x80 (rows that do not divide the workgroup tile: masked lanes), h = 2.  Plane counts that leave the last
# workgroup of the persistent grid (3 emulated CUs) short.
EMU_CASES = [
    (4, 32, (8, 8), 1, dict()),
    (8, 32, (8, 8), 17, dict(res=True)),
    (12, 64, (16, 16), 3, dict(bn=True)),
    (16, 128, (16, 16), 5, dict(bn=True, res=True)),
    (20, 32, (20, 64), 2, dict(bn=True, res=True)),
    (32, 64, (64, 8), 3, dict(bn=True, pool=True)),
    (64, 64, (40, 40), 2, dict(bn=True, res=True, pool=True)),
    (32, 32, (48, 48), 1, dict(res=True)),
    (8, 32, (80, 80), 1, dict(bn=True, pool=True)),
    (12, 64, (2, 16), 7, dict(relu=False)),
    (4, 64, (2, 8), 4, dict(res=True, res_after=True)),
    (8, 128, (8, 8), 10, dict(res=True, res_after=True, relu=False)),
    (64, 128, (16, 16), 4, dict(bn=True, res=True)),
    (32, 32, (16, 16), 1, dict(bn=True, pool=True)),
    (12, 32, (20, 64), 1, dict(pool=True, res=True)),
    (20, 64, (48, 48), 1, dict(bn=True, relu=False)),
]


@pytest.fixture(scope="module")
def emu(emu_lib):
    return WE.load_emu()


@pytest.mark.parametrize("case", range(len(EMU_CASES)))
def test_wino_emulated_layer_within_fp64_bound(emu, case):
    cin, cout, hw, planes, opts = EMU_CASES[case]
    r = WE.run_layer(emu, cin, cout, hw, planes, opts, seed=case)
    assert r["insts"], "the layer did not run on k_conv_wino"
    assert r["ratio"] <= 1.0, f"error / bound {r['ratio']:.3g}"
    print(f"k_conv_wino{r['insts'][0]} worst error / bound {r['ratio']:.4f}")


@pytest.mark.parametrize("cin,cout,hw", [(16, 64, (16, 16)), (8, 32, (8, 8)), (8, 32, (40, 40))])
def test_wino_emulated_masked_planes_keep_valid_bits(emu, cin, cout, hw):
    """plane_valid with valid_div = 3 (the product's person masks: three planes per person): the valid planes are bit-identical
    to the unmasked run, finite, and within the bound; guards intact (poison check inside run_layer)."""
    planes = 12
    full = WE.run_layer(emu, cin, cout, hw, planes, dict(bn=True, res=True), seed=5)
    for pattern in ([0, 1, 1, 1], [1, 0, 1, 0], [0, 0, 0, 1], [0, 0, 0, 0]):
        pv = torch.tensor(pattern, dtype=torch.uint8)
        m = WE.run_layer(emu, cin, cout, hw, planes, dict(bn=True, res=True), seed=5, plane_valid=pv, valid_div=3, x=full["x"])
        valid = pv.bool()[torch.arange(planes) // 3]
        assert torch.equal(m["out"][valid], full["out"][valid]), pattern
        assert m["ratio"] <= 1.0, pattern


@pytest.fixture(scope="module")
def form_runs(emu_lib, tmp_path_factory):
    """FORM_CASES under each switch set, one child process per set (the emulated library reads the switches once)."""
    sets = {"default": {}, "wgs256": {"FVP_WINO_WGS": "256"}, "half1": {"FVP_WINO_HALF": "1"}, "half2": {"FVP_WINO_HALF": "2"},
            "quarter2": {"FVP_WINO_QUARTER": "2"}, "w16": {"FVP_WINO_W16": "1", "FVP_WINO_HALF": "2"},
            "wc1": {"FVP_WINO_WC1": "1"}, "no_resw": {"FVP_WINO_NO_RESW": "1"}}
    tmp = tmp_path_factory.mktemp("wino_forms")
    runs = {}
    for name, env in sets.items():
        e = dict(os.environ)
        for k in ("FVP_WINO_WGS", "FVP_WINO_HALF", "FVP_WINO_QUARTER", "FVP_WINO_W16", "FVP_WINO_WC1", "FVP_WINO_NO_RESW"):
            e.pop(k, None)
        e.update(env)
        out = tmp / f"{name}.pt"
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "wino_emu_child.py"), str(out)], env=e,
                           capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, f"{name}: {p.stderr[-2000:]}"
        runs[name] = torch.load(out)
    return runs


def test_wino_emulated_forms_within_bound_and_bit_identical(form_runs):
    """Full / half / quarter units, the 256-CU choice of forms, resident vs streamed weights, 32-cout blocks for every layer
    (WC1) and the 16-wave form: fvp_conv_wino.hip and DESIGN.md claim the same accumulation chain per (cout, tile), i.e. the
    same bits.  Each form within the fp64 bound; every form bit-identical to the default choice."""
    base = form_runs["default"]
    forms = {}
    for name, res in form_runs.items():
        for i, r in enumerate(res):
            cin, cout, hw, planes, opts = WE.FORM_CASES[i]
            assert r["insts"], f"{name} case {i}: not on k_conv_wino"
            forms.setdefault(i, set()).update(r["insts"])
            assert r["ratio"] <= 1.0, f"{name} case {i}: error / bound {r['ratio']:.3g}"
            assert torch.equal(r["out"], base[i]["out"]), \
                f"{name} case {i} {r['insts']} vs default {base[i]['insts']}: max |d| {(r['out'] - base[i]['out']).abs().max():.3g}"
            if r["pool"] is not None:
                assert torch.equal(r["pool"], base[i]["pool"]), f"{name} case {i}: pooled output differs"
    # the switches did move the forms: quarter (CW = 1, 4 waves), half (CW = 2, 4 waves), full 8-wave, resident weights, 16-wave
    seen = set().union(*forms.values())
    assert any(k[1] == 4 and k[6] == 1 for k in seen) and any(k[1] == 4 and k[6] == 2 for k in seen)
    assert any(k[0] * k[1] == 8 and k[6] == 2 for k in seen) and any(k[5] for k in seen)
    assert any(k[0] * k[1] == 16 for k in seen), "the 16-wave form (FVP_WINO_W16) did not run"


# ---- 3. instantiation closure ----------------------------------------------------------------------------------------
# (cin, cout, (h, w), planes): the cheapest emulated shape per reachable instantiation (3 CUs, every row width), each run
# with and without a residual.
COVER_CASES = [
    (4, 32, (4, 36), 1), (4, 32, (4, 36), 2), (4, 32, (4, 12), 1), (4, 64, (4, 12), 1), (4, 32, (2, 12), 1), (4, 64, (2, 12), 1),
    (4, 32, (2, 8), 1), (4, 64, (2, 8), 1), (8, 32, (4, 36), 1), (8, 32, (4, 36), 2), (8, 32, (4, 24), 1), (8, 32, (4, 12), 1),
    (4, 32, (6, 44), 3), (4, 32, (2, 132), 1), (4, 32, (2, 252), 1), (4, 32, (2, 8), 65), (40, 32, (6, 44), 3),
    (8, 32, (6, 44), 3), (40, 32, (2, 132), 1), (8, 32, (2, 132), 1), (32, 32, (2, 188), 1), (8, 32, (2, 188), 1),
    (4, 64, (2, 68), 3), (4, 64, (2, 8), 33), (8, 64, (4, 36), 3), (8, 64, (2, 68), 3),
]


def _unreachable(k):
    """Why instantiation k = (WC, WT, CC, NI, HAS_RES, RESW, CW) of the shipped library can never be launched (None: it can)."""
    wc, wt, cc, ni, _, resw, cw = k
    if wc * wt == 4 and cc == 8 and ni == 1:
        return ("a 4-wave unit covers more than 32 of its 64 tiles (wino_tiling), i.e. more than 8 x 32 = 256 input quads "
                "of 8 channels: never one DMA round")
    if wc * wt == 8 and wt == 8 and cc == 8 and ni == 1:
        return "an 8-wave unit covers more than 64 tiles: more than 512 quads of 8 channels, never one DMA round"
    if (wc, wt, cw) == (1, 4, 2) and cc == 8 and ni >= 3:
        return ("three ring slots of NI x 4 KB of input + 16 KB of weights exceed the 78 KB of a half-size (two per CU) "
                "workgroup from NI = 3: the planner falls back to CC = 4")
    if (wc, wt) == (2, 4) and cc == 8 and ni >= 3:
        return "three ring slots of NI x 8 KB of input + 32 KB of weights exceed the 152 KB budget from NI = 3: CC = 4"
    if (wc, wt) == (2, 4) and cc == 4 and ni >= 3:
        return ("a 64-tile unit stages at most 4 x 3/4 x 256 + 1 = 769 quads of 4 channels (3 input columns per 2 output "
                "columns, 2 halo rows per 2 output rows): at most 2 DMA rounds of 512 threads")
    return None


def test_wino_every_shipped_instantiation_is_launched_or_unreachable(emu):
    launched = set()
    for i, (cin, cout, hw, planes) in enumerate(COVER_CASES):
        for res in (False, True):
            r = WE.run_layer(emu, cin, cout, hw, planes, dict(res=res), seed=i)
            assert r["insts"] and r["ratio"] <= 1.0, (cin, cout, hw, planes, res, r["insts"], r["ratio"])
            launched.update(r["insts"])
    for k in launched:
        assert _unreachable(k) is None, f"k_conv_wino{k} launched but listed as unreachable"
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as KR
    if not os.path.isfile(LIB) or not os.path.isfile(os.path.join(KR.LLVM, "llvm-objdump")):
        pytest.skip("the shipped library or llvm-objdump is absent: closure against its instantiations not checked")
    rows = KR.scan_library(LIB)
    shipped = set()
    for d in KR.demangle([r["name"] for r in rows]):
        if "k_conv_wino<" in d:
            a = d.split("k_conv_wino<")[1].split(">")[0].split(",")
            shipped.add(tuple(int(v) if v.strip() not in ("true", "false") else int(v.strip() == "true") for v in a))
    assert len(shipped) == 72
    missing = sorted(k for k in shipped - launched if _unreachable(k) is None)
    assert not missing, f"shipped k_conv_wino instantiations no emulated case launches: {missing}"
    dead = sorted(k for k in shipped if _unreachable(k))
    assert len(dead) == 20, dead
    print(f"{len(shipped & launched)} shipped instantiations launched, {len(dead)} unreachable")
