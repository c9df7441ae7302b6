"""Shared-column input transform of the Winograd kernel (csrc/fvp_conv_wino.hip: k_conv_wsc, SH = 1 for W = 32, SH = 2 for
W = 16): the tiles of a row take the outer columns of the transform's first pass from their neighbours through DPP instead of
reading and transforming them themselves.  The claim is "the same bits", so the condition is equality of the output WORDS
(int32 view) between the form the planner picks and the own-patch form selected by FVP_WINO_SHARED_COLS=0 - on the CPU
emulation (tests/hipemu, two-plane cases) and on the MI355X (diagnostics build, two and three planes), at every unit size
the planner can pick (full / half / quarter, forced by FVP_WINO_HALF / FVP_WINO_QUARTER / FVP_WINO_WGS).  The library reads
its switches once when it loads: one child process per switch set (this file is its own child: `python
tests/test_wino_shared_columns.py emu|gpu OUT.pt`).

Inputs have no zeros (a wrong or wrapped neighbour cannot hide behind one), large values in the border rows and columns, and
one sparse case: a single non-zero pixel per corner and on both sides of every junction of two tile rows (the places where a
neighbour value that is not the zero margin would come from).

Also here: the code objects of the shipped k_conv_wsc instances (the neighbour values are DPP operands of the subtractions,
no moves, no packed f32, no more registers than the own-patch instance) and, on the emulation, which shapes take which form."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import common as CM  # noqa: E402

LIB = os.path.join(ROOT, "faster-voxelpose_amd", "libfvp_hip.so")
EMU_LIB = os.path.join(ROOT, "tests", "hipemu", "libfvp_emu.so")
DIAG_LIB = os.path.join(ROOT, "tests", "diag", "libfvp_hip_diag.so")

# (name, cin, cout, (h, w), layer options, input kind, masked)
#   32 x 32: 8 -> 64 (one chunk of 8) and 64 -> 64 (the product's layer); 16 x 16: 64 -> 128 and 128 -> 128; with and without
#   a residual; the fused 2x2 max-pool; a person mask that skips a unit (plane); the sparse input on both widths.
#   64 x 64 (the neighbouring tile lives in another wave) and 80 x 80 (masked rows) must not take the new form.
CASES = [
    ("w32_8_64", 8, 64, (32, 32), dict(bn=True), "dense", False),
    ("w32_8_64_res", 8, 64, (32, 32), dict(bn=True, res=True), "dense", False),
    ("w32_64_64_res", 64, 64, (32, 32), dict(bn=True, res=True), "dense", False),
    ("w32_64_64", 64, 64, (32, 32), dict(bn=True), "dense", False),
    ("w32_8_64_pool", 8, 64, (32, 32), dict(bn=True, pool=True), "dense", False),
    ("w32_8_64_sparse", 8, 64, (32, 32), dict(bn=True), "sparse", False),
    ("w16_64_128", 64, 128, (16, 16), dict(bn=True), "dense", False),
    ("w16_64_128_res", 64, 128, (16, 16), dict(bn=True, res=True), "dense", False),
    ("w16_128_128_res", 128, 128, (16, 16), dict(bn=True, res=True), "dense", False),
    ("w16_128_128", 128, 128, (16, 16), dict(bn=True), "dense", False),
    ("w16_64_128_sparse", 64, 128, (16, 16), dict(bn=True), "sparse", False),
    ("w16_64_128_masked", 64, 128, (16, 16), dict(bn=True, res=True), "dense", True),
    ("w32_8_64_masked", 8, 64, (32, 32), dict(bn=True), "dense", True),
    ("w64_32_32", 32, 32, (64, 64), dict(bn=True, res=True), "dense", False),
    ("w80_8_32", 8, 32, (80, 80), dict(bn=True), "dense", False),
]
SHARED_FORM = {32: 1, 16: 2}           # row width -> SH of the shapes that take the new form
UNIT_SETS = {                          # the unit sizes the planner can pick for these shapes
    "full": {"FVP_WINO_HALF": "2"},
    "half": {"FVP_WINO_HALF": "1", "FVP_WINO_QUARTER": "0"},
    "quarter": {"FVP_WINO_HALF": "1", "FVP_WINO_QUARTER": "2", "FVP_WINO_WGS": "256"},
}
_INST = re.compile(r"k_conv_winoILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELb([01])ELb([01])ELi(\d+)EE")
_FORM = re.compile(r"wino_shared_columns_formILi(\d)EE")


def make_input(cin, hw, planes, kind, seed):
    h, w = hw
    g = torch.Generator().manual_seed(seed)
    if kind == "sparse":
        x = torch.zeros(planes, cin, h, w)
        pix = [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)]
        for t in range(h // 2 - 1):    # the junction of tile rows t and t + 1: end of row t, start of row t + 1, both image rows
            pix += [(2 * t, w - 1), (2 * t + 1, w - 1), (2 * t + 2, 0), (2 * t + 3, 0)]
        for i, (y, xx) in enumerate(pix):
            x[:, :, y, xx] = (1.0 + 0.37 * i) * (0.5 + torch.rand(planes, cin, generator=g))
        return x
    x = torch.randn(planes, cin, h, w, generator=g)
    x = torch.where(x.abs() < 1e-3, torch.full_like(x, 1e-3), x)             # no zeros
    for sl in ((..., 0, slice(None)), (..., h - 1, slice(None)), (..., slice(None), 0), (..., slice(None), w - 1)):
        x[sl] *= 1000.0                                                     # large values on the four borders
    assert (x != 0).all()
    return x


def run_cases(lib, device, plane_counts, log=None):
    """Every case at every plane count: {(name, planes): dict(out, pool, valid, insts, forms)} (int32 words, on the CPU)."""
    res = {}
    for ci, (name, cin, cout, hw, opts, kind, masked) in enumerate(CASES):
        spec, w, ids = CM.wino_layer(cin, cout, hw, seed=ci, **opts)
        for planes in plane_counts:
            x = make_input(cin, hw, planes, kind, 100 * ci + planes)
            pv = torch.tensor([1, 0, 1][:planes], dtype=torch.uint8) if masked else None
            if log is not None:
                lib.hipemu_launch_log_reset()
            bufs, check = CM.run_custom_conv_stack(lib, device, spec, w, x, plane_valid=pv, valid_div=1, poison=True)
            text = log().decode() if log is not None else ""
            check()
            valid = torch.ones(planes, dtype=torch.bool) if pv is None else pv.bool()
            out = bufs[ids["out"]].cpu()[valid].contiguous().view(torch.int32).clone()
            pool = None
            if ids["pool"] is not None:
                pool = bufs[ids["pool"]].cpu()[valid].contiguous().view(torch.int32).clone()
            res[(name, planes)] = dict(out=out, pool=pool, insts=[tuple(int(v) for v in m) for m in _INST.findall(text)],
                                       forms=[int(v) for v in _FORM.findall(text)])
    return res


def _child(kind, path):
    from faster_voxelpose_amd import _capi as capi
    if kind == "emu":
        from faster_voxelpose_amd import netspec
        netspec.WINO_GENERIC = os.environ.get("FVP_WINO_GENERIC") == "1"       # (as tests/wino_emu_child.py)
        lib = capi.bind(C.CDLL(EMU_LIB))
        lib.hipemu_launch_log.restype = C.c_char_p
        lib.hipemu_launch_log.argtypes = []
        lib.hipemu_launch_log_reset.argtypes = []
        res = run_cases(lib, "cpu", (2,), log=lib.hipemu_launch_log)
    else:
        lib = capi.bind(C.CDLL(DIAG_LIB))
        assert lib.fvp_diag_build() == 1
        res = run_cases(lib, "cuda", (2, 3))
        torch.cuda.synchronize()
    torch.save(res, path)


_SWITCHES = ("FVP_WINO_WGS", "FVP_WINO_HALF", "FVP_WINO_QUARTER", "FVP_WINO_W16", "FVP_WINO_WC1", "FVP_WINO_NO_RESW",
             "FVP_WINO_SHARED_COLS")


def _runs(kind, sets, tmp):
    runs = {}
    for name, env in sets.items():
        e = dict(os.environ)
        for k in list(e):
            if k in _SWITCHES or (kind == "gpu" and k.startswith("FVP_")):
                e.pop(k)
        e.update(env)
        out = tmp / f"{kind}_{name}.pt"
        p = subprocess.run([sys.executable, os.path.abspath(__file__), kind, str(out)], env=e, capture_output=True, text=True,
                           timeout=600)
        assert p.returncode == 0, f"{name}: {p.stderr[-3000:]}"
        runs[name] = torch.load(out)
    return runs


def _switch_sets(separate):
    sets = {}
    for unit, env in UNIT_SETS.items():
        sets[f"{unit}_new"] = dict(env)
        sets[f"{unit}_old"] = dict(env, FVP_WINO_SHARED_COLS="0")
    if separate:                        # the two widths separately (full-size units)
        sets["full_w32_only"] = dict(UNIT_SETS["full"], FVP_WINO_SHARED_COLS="1")
        sets["full_w16_only"] = dict(UNIT_SETS["full"], FVP_WINO_SHARED_COLS="2")
    return sets


def _assert_same_words(runs, a, b):
    for key, ra in runs[a].items():
        rb = runs[b][key]
        assert torch.equal(ra["out"], rb["out"]), f"{key}: {a} vs {b}: {int((ra['out'] != rb['out']).sum())} output words differ"
        assert (ra["pool"] is None) == (rb["pool"] is None)
        if ra["pool"] is not None:
            assert torch.equal(ra["pool"], rb["pool"]), f"{key}: {a} vs {b}: pooled output words differ"


# ---- emulated half -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu_runs(emu_lib, tmp_path_factory):
    return _runs("emu", _switch_sets(separate=True), tmp_path_factory.mktemp("wino_shared_emu"))


@pytest.mark.parametrize("unit", sorted(UNIT_SETS))
def test_emulated_shared_columns_same_words_as_own_patch(emu_runs, unit):
    _assert_same_words(emu_runs, f"{unit}_new", f"{unit}_old")
    _assert_same_words(emu_runs, f"{unit}_new", "full_old")      # and across the unit sizes


def test_emulated_widths_switch_separately(emu_runs):
    _assert_same_words(emu_runs, "full_w32_only", "full_old")
    _assert_same_words(emu_runs, "full_w16_only", "full_old")


def test_emulated_forms_follow_the_shape_rule(emu_runs):
    """Which launches took the shared-column form (the emulation's launch log names it): W = 32 and W = 16 in full- and
    half-size units (two-block waves), never the quarter-size units, 64 x 64 or 80 x 80, and nothing under the switch."""
    for (name, planes), r in emu_runs["full_new"].items():
        assert r["insts"], name
    for unit in UNIT_SETS:
        for (name, planes), r in emu_runs[f"{unit}_new"].items():
            w = next(c[3][1] for c in CASES if c[0] == name)
            cw = {k[6] for k in r["insts"]}
            want = [SHARED_FORM[w]] if w in SHARED_FORM and cw == {2} else []
            assert r["forms"] == want, (unit, name, r["insts"], r["forms"])
        assert all(r["forms"] == [] for r in emu_runs[f"{unit}_old"].values()), unit
    # the switches did move the unit sizes: 8-wave, 4-wave two-block, 4-wave one-block instances
    seen = {u: set().union(*[set(r["insts"]) for r in emu_runs[f"{u}_new"].values()]) for u in UNIT_SETS}
    assert any(k[0] * k[1] == 8 for k in seen["full"]) and all(k[6] == 2 for k in seen["full"])
    assert any(k[0] * k[1] == 4 and k[6] == 2 for k in seen["half"])
    assert any(k[0] * k[1] == 4 and k[6] == 1 for k in seen["quarter"])
    for only, width in (("full_w32_only", 32), ("full_w16_only", 16)):
        for (name, planes), r in emu_runs[only].items():
            w = next(c[3][1] for c in CASES if c[0] == name)
            assert r["forms"] == ([SHARED_FORM[w]] if w == width else []), (only, name, r["forms"])


# ---- the shipped code objects --------------------------------------------------------------------------------------------
def test_shared_column_instances_fold_the_dpp_operand():
    """k_conv_wsc<WC, WT, CC, NI, RES, RESW, SH> of the shipped library: per step of 4 channels the 8 outer subtractions of the
    column pass carry the neighbour as their DPP operand (row_shr / row_shl by SH lanes, zero fill) - two chunk bodies x CC/4
    steps x 8 = 4 CC of them - and nothing else uses DPP (no standalone v_mov_b32_dpp); no packed-f32 VALU; no spills; no more
    registers than the own-patch instance k_conv_wino<..., 2> of the same parameters; the MFMA count of a straight-line body."""
    import kernel_resources as KR
    if not os.path.isfile(LIB):
        pytest.fail("libfvp_hip.so is not built (run __graft_entry__.build())")
    objdump = os.path.join(KR.LLVM, "llvm-objdump")
    if not os.path.isfile(objdump):
        pytest.skip("no llvm-objdump in this image")
    rows = KR.scan_library(LIB)
    for r, d in zip(rows, KR.demangle([r["name"] for r in rows])):
        r["demangled"] = d.split("(")[0]
    own = {}
    for r in rows:
        if "k_conv_wino<" in r["demangled"]:
            own[tuple(a.strip() for a in r["demangled"].split("k_conv_wino<")[1].split(">")[0].split(","))] = r
    wsc = {r["name"]: r for r in rows if "k_conv_wsc<" in r["demangled"]}
    assert len(wsc) == 24                             # 6 (workgroup, chunk, rounds) x residual or not x 2 widths
    import tempfile
    dpp = {}
    with tempfile.TemporaryDirectory() as tmp:
        for co in KR._code_objects(LIB, tmp):
            text = subprocess.run([objdump, "-d", "--no-show-raw-insn", co], capture_output=True, text=True, check=True).stdout
            name = None
            for line in text.splitlines():
                m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
                if m:
                    name = m.group(1)
                elif name in wsc and ("_dpp" in line or "v_pk_" in line):
                    dpp.setdefault(name, []).append(line.split("//")[0].strip())
    for name, r in wsc.items():
        a = [v.strip() for v in r["demangled"].split("k_conv_wsc<")[1].split(">")[0].split(",")]
        cc, sh = int(a[2]), int(a[6])
        ins = dpp.get(name, [])
        subs = [i for i in ins if re.match(r"v_sub(rev)?_f32_dpp ", i)]
        assert len(ins) == len(subs) == 4 * cc, (r["demangled"], ins)
        assert sum(f"row_shr:{sh} " in i for i in subs) == 2 * cc and sum(f"row_shl:{sh} " in i for i in subs) == 2 * cc, subs
        assert all("row_mask:0xf bank_mask:0xf bound_ctrl:1" in i for i in subs), subs
        assert r["sgpr_spill"] == 0 and r["vgpr_spill"] == 0 and r["scratch"] == 0, r
        assert r["packed_f32_between_mfma"] == 0 and r["mfma"] == 16 * cc, r
        base = own[tuple(a[:6] + ["2"])]
        assert r["vgpr"] + r["agpr"] <= base["vgpr"] + base["agpr"], (r, base)


# ---- MI355X half ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu_runs(diag_lib, tmp_path_factory):
    return _runs("gpu", _switch_sets(separate=False), tmp_path_factory.mktemp("wino_shared_gpu"))


@pytest.mark.gpu
@pytest.mark.parametrize("unit", sorted(UNIT_SETS))
def test_gpu_shared_columns_same_words_as_own_patch(gpu_runs, unit):
    _assert_same_words(gpu_runs, f"{unit}_new", f"{unit}_old")
    _assert_same_words(gpu_runs, f"{unit}_new", "full_old")


if __name__ == "__main__":
    _child(sys.argv[1], sys.argv[2])
