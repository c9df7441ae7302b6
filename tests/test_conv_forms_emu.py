"""The non-Winograd forms of the conv interpreter on the CPU emulation (tests/hipemu), one op per case: the table of
tests/conv_form_cases.py under the default routing and under every conv switch of csrc/fvp_conv.hip, each in a child
process (tests/conv_form_child.py: the switches are read once when the library loads), and the sharpness of the fp64
bound of tests/common.py (pure torch).

Per row: the bound, plane-count independence, person masks, poison guards and read fences (checked in the child, reported
here), the instantiation the row names in the launch log, and - over all rows - the closure: every instantiation of the
non-Winograd kernels is launched by some row (k_conv_dma<7,7,4,1> only under FVP_CONV_LDS_KB=128).  Between children: the
bit-equalities the source claims (conv_form_cases.py lists them).

Measured worst error / bound per form on the emulator (bound: (cinp * taps + 3) * eps32, + 3 with split K):
    Direct (k_conv_dma and k_conv) 0.30 (1x1, 4 channels)   KSplit 0.026   K7 0.015   Pair7 0.16   TPair 0.10   Reg 0.087
    k_pool2 exact
(MI355X: tests/test_conv_forms_gpu.py)."""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

import common as CM
import conv_form_cases as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the bound rejects subtly wrong results (pure torch) -------------------------------------------------------------
def _padded(w, b, xp, r, s, t, relu_first=False):
    y = (F.conv2d(xp, w, None) + b.view(1, -1, 1, 1)) * s.view(1, -1, 1, 1) + t.view(1, -1, 1, 1)
    if not relu_first:
        y = y + r
    y = torch.relu(y)
    return y + r if relu_first else y


@pytest.mark.parametrize("k,cin,cout,hw", [(1, 4, 64, (8, 8)), (1, 64, 128, (8, 8)), (3, 6, 64, (12, 12)), (3, 128, 128, (10, 12)),
                                           (7, 15, 64, (12, 16)), (7, 2, 64, (10, 10))])
def test_conv_bound_rejects_mutated_references(k, cin, cout, hw):
    """Each mistake a subtly wrong kernel could make, applied to the float64 reference, breaks the bound of tests/common.py
    (conv_gamma) somewhere; the clean reference rounded to fp32 stays within it."""
    spec, wt, ids = CM.conv_layer("conv", cin, cout, hw, k=k, res=True, bn=True, seed=cin)
    op = spec.op_array[ids["op"]]
    gamma = CM.conv_gamma(op)
    g = torch.Generator().manual_seed(k * 100 + cin)
    P, (H, W), pad = 3, hw, k // 2
    w, b = wt["c.weight"].double(), wt["c.bias"].double()
    s = (wt["n.weight"] / torch.sqrt(wt["n.running_var"] + 1e-5)).double()
    t = wt["n.bias"].double() - wt["n.running_mean"].double() * s
    x = torch.randn(P, cin, H, W, generator=g, dtype=torch.float64)
    r = torch.randn(P, cout, H, W, generator=g, dtype=torch.float64)
    xp = F.pad(x, (pad,) * 4)
    y64 = _padded(w, b, xp, r, s, t)
    mag = s.abs().view(1, -1, 1, 1) * (F.conv2d(x.abs(), w.abs(), None, padding=pad) + b.abs().view(1, -1, 1, 1)) \
        + t.abs().view(1, -1, 1, 1) + r.abs()
    assert CM.conv_ratio(y64.float(), y64, gamma * mag) <= 1.0
    co, ci = cout - 3, cin // 2
    mutants = {}
    w1 = w.clone()
    w1[co, ci] = 0.0
    mutants["input channel dropped for one cout"] = _padded(w1, b, xp, r, s, t)
    w2 = w.clone()
    w2[co, ci, k - 1, 0] = 0.0
    mutants["one tap zeroed"] = _padded(w2, b, xp, r, s, t)
    if k > 1:
        xt = xp.clone()
        xt[1:, :, pad - 1, pad:-pad] = x[:-1, :, -1, :]          # the halo row above = the last row of the previous plane
        mutants["top halo row from the neighbouring plane"] = _padded(w, b, xt, r, s, t)
        xr = xp.clone()
        xr[:, :, pad:-pad - 1, -pad] = x[:, :, 1:, 0]            # the first right halo column = column 0 of the next row
        mutants["right halo column wrapped from the next row"] = _padded(w, b, xr, r, s, t)
    else:
        mutants["pixels shifted by one"] = _padded(w, b, xp.roll(1, dims=3), r, s, t)
    mutants["residual of the neighbouring plane"] = _padded(w, b, xp, r.roll(1, dims=0), s, t)
    s2, t2 = s.clone(), t.clone()
    s2[32:64], t2[32:64] = s[0:32], t[0:32]
    mutants["BN of 32-cout block 0 applied to block 1"] = _padded(w, b, xp, r, s2, t2)
    mutants["ReLU before the residual"] = _padded(w, b, xp, r, s, t, relu_first=True)
    for name, ym in mutants.items():
        ratio = CM.conv_ratio(ym.float(), y64, gamma * mag)
        assert ratio > 1.0, f"{name}: error / bound {ratio:.3g} - the bound would not catch it"


@pytest.mark.parametrize("cin,cout,hw", [(128, 64, (4, 4)), (16, 32, (3, 5))])
def test_transposed_conv_bound_rejects_mutated_references(cin, cout, hw):
    """The same for ConvTranspose(k2,s2) + skip: swapped taps, a dropped channel, the skip before the ReLU."""
    spec, wt, ids = CM.conv_layer("up", cin, cout, hw, bn=True, seed=cout)
    i = ids["op"]
    op = spec.op_array[i]
    g = torch.Generator().manual_seed(cin)
    x = torch.randn((3, cin) + hw, generator=g)
    r = torch.randn((3, cout, 2 * hw[0], 2 * hw[1]), generator=g)
    s = wt["n.weight"] / torch.sqrt(wt["n.running_var"] + 1e-5)
    blob = torch.zeros(spec.nparams)
    blob[op.e_off:op.e_off + cout] = wt["u.bias"]
    blob[op.e_off + op.coutp:op.e_off + op.coutp + cout] = s
    blob[op.e_off + 2 * op.coutp:op.e_off + 2 * op.coutp + cout] = wt["n.bias"] - wt["n.running_mean"] * s
    y64, mag, _ = CM.conv_op_reference(spec, wt, blob, i, x, r)
    bound = CM.conv_gamma(op) * mag
    assert CM.conv_ratio(y64.float(), y64, bound) <= 1.0

    def variant(weight=None, res_first=False):
        w2 = dict(wt)
        if weight is not None:
            w2["u.weight"] = weight
        if not res_first:
            return CM.conv_op_reference(spec, w2, blob, i, x, r)[0]
        b, sc, sh = (v.view(1, -1, 1, 1) for v in CM.conv_packed_epi(spec, blob, i))
        return torch.relu((F.conv_transpose2d(x.double(), wt["u.weight"].double(), None, stride=2) + b) * sc + sh + r.double())

    mutants = {"column taps swapped": variant(wt["u.weight"].flip(3)), "row taps swapped": variant(wt["u.weight"].flip(2)),
               "skip added before the ReLU": variant(res_first=True)}
    w1 = wt["u.weight"].clone()
    w1[cin // 2, cout - 3] = 0.0
    mutants["input channel dropped for one cout"] = variant(w1)
    for name, ym in mutants.items():
        ratio = CM.conv_ratio(ym.float(), y64, bound)
        assert ratio > 1.0, f"{name}: error / bound {ratio:.3g} - the bound would not catch it"


# ---- 2. the table, one child process per switch set ------------------------------------------------------------------------
DEFAULT_PARTS = 3


@pytest.fixture(scope="module")
def runs(emu_lib, tmp_path_factory):
    """Every switch set in a child process; the children run side by side (CPU only) with small thread pools of their own,
    the default set in DEFAULT_PARTS of them."""
    tmp = tmp_path_factory.mktemp("conv_forms")
    child = os.path.join(ROOT, "tests", "conv_form_child.py")
    procs = []
    for name in T.SWITCH_SETS:
        for part in range(DEFAULT_PARTS if name == "default" else 1):
            out = tmp / f"{name}.{part}.pt"
            args = [sys.executable, child, str(out), name] + (["--part", f"{part}/{DEFAULT_PARTS}"] if name == "default" else [])
            env = dict(T.child_env(name, os.environ), OMP_NUM_THREADS="1", MKL_NUM_THREADS="1", HIPEMU_THREADS="2")
            procs.append((name, out, subprocess.Popen(args, env=env, stdout=subprocess.DEVNULL,
                                                      stderr=subprocess.PIPE, text=True)))
    res = {}
    try:
        for name, out, p in procs:
            _, err = p.communicate(timeout=900)
            assert p.returncode == 0, f"{name}: {err[-2000:]}"
            res.setdefault(name, {}).update(torch.load(out))
    finally:
        for _, _, p in procs:
            if p.poll() is None:
                p.kill()
    return res


def _failures(res):
    return {k: v["error"] for k, v in res.items() if "error" in v}


def test_default_routing_rows_hold_every_check(runs):
    """(a) - (d) for every row (asserted in the child) and (e): the launch log holds the instantiation the row names; a Reg
    row runs on k_conv_dma here (the register-direct kernel starts at 1024 / 200 tiles)."""
    res = runs["default"]
    assert not _failures(res), _failures(res)
    worst = {}
    for i, row in T.rows_of("default"):
        r = res[row.name]
        if row.form == "Reg":
            assert not any(k.startswith("k_conv_reg") for k in r["insts"]), (row.name, r["insts"])
        else:
            assert row.expect in r["insts"], f"{row.name}: expected {row.expect}, launched {r['insts']}"
        if row.form != "Reg" and row.kind == "conv" and not row.opts.get("res") and not row.opts.get("pool"):
            assert r["insts"] == [row.expect], f"{row.name}: {r['insts']}"       # a single op: exactly one launch
        worst[row.form] = max(worst.get(row.form, 0.0), r["ratio"])
    print("worst error / bound per form:", {k: round(v, 4) for k, v in worst.items()})


def test_refusals_return_their_codes_and_write_nothing(runs):
    res = runs["default"]
    for case in T.REFUSALS:
        r = res["refusal:" + case[0]]
        assert "error" not in r, f"{case[0]}: {r}"
        assert r["rc"] == case[-1]


def test_register_direct_rows_and_their_bit_equality_with_the_staged_kernel(runs):
    """The seven FVP_REG_INSTANCES (FVP_CONV_REG_MIN_TILES=1); csrc/fvp_conv.hip: 'k_conv_reg and k_conv_dma produce the same
    bits' - the rows of both children are compared bit for bit.  A residual with cout % 8 != 0 falls back to k_conv_dma."""
    res = runs["reg"]
    assert not _failures(res), _failures(res)
    for i, row in T.rows_of("reg"):
        r = res[row.name]
        assert row.expect in r["insts"], f"{row.name}: expected {row.expect}, launched {r['insts']}"
        if row.name == "reg_not_res_c20":
            assert not any(k.startswith("k_conv_reg") for k in r["insts"][-1:]), r["insts"]
        if "default" in row.sets:
            assert torch.equal(r["out"].view(torch.int32), runs["default"][row.name]["out"].view(torch.int32)), \
                f"{row.name}: k_conv_reg and k_conv_dma differ"


_PROPERTY = {
    "no_dma": lambda k: not k.startswith("k_conv_dma") or k.endswith(",0,1,0>"),        # (the paired transposed form stages by DMA whatever the switch says)
    "no_pair": lambda k: not (k.startswith("k_conv_dma") and (k.endswith(",1,0,0>") or k.endswith(",0,1,0>"))),
    "no_k7": lambda k: not k.startswith("k_conv7"),
    "no_ksplit": lambda k: not k.endswith(",0,0,1>"),
    "no_reg": lambda k: not k.startswith("k_conv_reg"),
    "no_wino": lambda k: not k.startswith("k_conv_wino"),
}


@pytest.mark.parametrize("name", [n for n in T.SWITCH_SETS if n not in ("default", "reg")])
def test_switch_set_rows_hold_the_bound_and_take_the_switched_form(runs, name):
    """(a) and (d) under each conv switch, and (e): the switch did move the forms."""
    res = runs[name]
    assert not _failures(res), _failures(res)
    rows = T.rows_of(name)
    assert rows and all(row.name in res for _, row in rows)
    launched = [k for _, row in rows for k in res[row.name]["insts"]]
    if name in _PROPERTY:
        bad = [k for k in launched if not _PROPERTY[name](k)]
        assert not bad, f"{name}: launched {sorted(set(bad))}"
    base = runs["default"]
    by_name = {row.name: row for _, row in rows}
    if name == "no_dma":
        assert res["dma3_12x12"]["insts"] == [T.stg(1, 1, 1, 1), T.stg(3, 3, 1, 1)] and T.stg(3, 3, 1, 1) in res["ks_64x4"]["insts"]
    if name == "no_pair":
        assert T.dma(7, 7, 1, 1) in res["p7_20x20"]["insts"] and T.dma(1, 1, 1, 1) in res["tp_128_64_8x8"]["insts"]
    if name == "no_k7":
        assert T.dma(7, 7, 1, 1, pair=1) in res["k7_c15_h6"]["insts"]
    if name == "no_ksplit":
        assert T.dma(3, 3, 1, 1) in res["ks_64x4"]["insts"]
    if name == "no_reg":
        assert T.dma(1, 1, 4, 1, tpair=1) in res["reg_128_4_1"]["insts"] and T.dma(1, 1, 1, 1) in res["reg_64_4_0"]["insts"]
    if name == "no_wino":
        assert res["nowino_16x16"]["insts"][-1] == T.dma(3, 3, 1, 1) and res["nowino_pool_8x32"]["insts"][-1] == "k_pool2"
    if name == "no_fuse":          # the head as a launch of its own behind both transposed forms
        assert res["tp_head15"]["insts"][-2:] == ["k_conv_reg<64,2,1,1>", "k_conv_reg<32,1,0,0>"]
        assert res["reg_64_2_2"]["insts"][-2:] == ["k_conv_reg<64,2,1,1>", "k_conv_reg<32,1,0,0>"]
        # the fused MFMA head of k_conv_reg against k_conv_reg's separate launch: the same bits
        assert torch.equal(res["reg_64_2_2"]["out"].view(torch.int32), runs["reg"]["reg_64_2_2"]["out"].view(torch.int32))
    if name == "no_head_fuse":     # ONLY the head switch: the claims of conv_epilogue_tpair (FUSE2) and above reg_takes()
        assert res["tp_head15"]["insts"][-2:] == [T.dma(1, 1, 2, 2, tpair=1), T.dma(1, 1, 1, 1)]
        assert torch.equal(res["tp_head15"]["out"].view(torch.int32), base["tp_head15"]["out"].view(torch.int32)), \
            "k_conv_dma: the head fused into the paired transposed conv and the separate launch differ"
        assert res["reg_64_2_2"]["insts"][-2:] == [T.dma(1, 1, 2, 2, tpair=1), T.dma(1, 1, 1, 1)]
        assert torch.equal(res["reg_64_2_2"]["out"].view(torch.int32), runs["reg"]["reg_64_2_2"]["out"].view(torch.int32)), \
            "k_conv_reg's fused head and k_conv_dma's two launches differ"
    if name == "lds128":
        assert res["dma7_cb4_lds128"]["insts"] == [T.dma(7, 7, 4, 1)]
    if name == "lds16":            # smaller chunks, ragged last chunk: the same kernels, and the bound
        for n, row in by_name.items():
            assert res[n]["insts"] == base[n]["insts"], n
    if name.startswith("pb"):
        pb = name[2:]
        for n, row in by_name.items():
            for k in res[n]["insts"]:
                if (k.startswith("k_conv<") or k.startswith("k_conv_dma<")) and not k.endswith(",0,1,0>") and not k.endswith(",0,0,1>"):
                    assert k.split("<")[1].split(",")[3].rstrip(">") == pb, f"{n}: {k}"


def test_every_instantiation_is_launched_or_listed_unreachable(runs):
    """The union of the launch logs holds every instantiation of the non-Winograd conv kernels (written out in
    conv_form_cases.ALL_INSTANTIATIONS: dispatch_tile() x dispatch_conv() on both stagings, KSplit, Pair7, TPair, k_conv7,
    the FVP_REG_INSTANCES, k_pool2): an instance added later fails here until it gets a row."""
    launched = set()
    for res in runs.values():
        for v in res.values():
            launched.update(v.get("insts", []))
            launched.update(v.get("alt_insts", []))
    for k in T.UNREACHABLE:
        assert k not in launched, f"{k} is launched but listed as unreachable"
    missing = sorted(set(T.ALL_INSTANTIATIONS) - launched - set(T.UNREACHABLE))
    assert not missing, f"instantiations no row launches: {missing}"
    unknown = sorted(k for k in launched - set(T.ALL_INSTANTIATIONS) if not k.startswith("k_conv_wino"))
    assert not unknown, f"launched instantiations the list does not know: {unknown}"
