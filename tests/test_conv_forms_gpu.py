"""The non-Winograd forms of the conv interpreter on the MI355X, one op per case: the table of tests/conv_form_cases.py on the
shipped library in-process - checks (a) the fp64 bound, (b) plane-count independence (for the Reg rows: k_conv_reg at
>= 1024 / 200 tiles against k_conv_dma below, the bit-equality csrc/fvp_conv.hip claims), (c) person masks, (d) poison guards,
and the profiler class FVP_K_CONV (FVP_K_OTHER for k_pool2), never a Winograd class - and under every conv switch on the
diagnostics build, one fresh child process per switch set (tests/conv_form_child.py --gpu), each under its own timeout,
one after the other, none re-run.

Measured worst error / bound per form on the MI355X (bound: (cinp * taps + 3) * eps32, + 3 with split K; printed per row
with -s):
    Direct k_conv_dma 0.24   Direct k_conv 0.25 (both: 1x1, 4 channels)   KSplit 0.025   K7 0.015   Pair7 0.16   TPair 0.10
    Reg 0.087   k_pool2 exact;   under the switch sets of the diagnostics build 0.15 (reg set: 0.087)"""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

import conv_form_cases as T

pytestmark = pytest.mark.gpu
# tools/gpu_switch_matrix.sh runs the suite on the diagnostics build under conv switches: the bound, mask and guard checks hold
# there too; which kernel class a row takes, and the children (which set their own switches), are checked without it only
_DIAG = os.environ.get("FVP_TEST_DIAG_LIB") == "1"

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GPU_ROWS = [(i, r) for i, r in enumerate(T.ROWS) if "default" in r.sets or "reg" in r.sets]


@pytest.fixture(scope="module")
def lib():
    from faster_voxelpose_amd import _capi as capi
    return capi.load()


def _prof_counts(lib, run):
    """Launch counts per profiler class of ``run()`` (fvp_prof_enable(2): one record per launch)."""
    from faster_voxelpose_amd import _capi as capi
    lib.fvp_prof_reset()
    lib.fvp_prof_enable(2)
    try:
        out = run()
        torch.cuda.synchronize()
        counts = {}
        for name, cls in (("conv", capi.K_CONV), ("other", capi.K_OTHER), ("wino", capi.K_CONV_WINO), ("wino_small", capi.K_CONV_WINO_SMALL)):
            ms, n, fl = C.c_double(), C.c_int64(), C.c_double()
            lib.fvp_prof_read(cls, C.byref(ms), C.byref(n), C.byref(fl))
            counts[name] = int(n.value)
    finally:
        lib.fvp_prof_enable(0)
        lib.fvp_prof_reset()
    return out, counts


@pytest.mark.parametrize("k", range(len(GPU_ROWS)), ids=[r.name for _, r in GPU_ROWS])
def test_conv_form_row_on_the_shipped_library(lib, k):
    index, row = GPU_ROWS[k]
    unfused = _DIAG and T.head_unfused(os.environ, row)
    r, counts = _prof_counts(lib, lambda: T.run_row(lib, "cuda", row, index, gpu=True, sample=3, head_fused=False if unfused else None))
    if _DIAG:
        return
    assert counts["wino"] == 0 and counts["wino_small"] == 0, f"{row.name}: Winograd launches {counts}"
    assert counts["other" if row.kind == "pool" else "conv"] >= 3, f"{row.name}: {counts}"     # the three runs of run_row
    print(f"{row.form} {row.name}: worst error / bound {r['ratio']:.4f} at {r['planes']} planes")


@pytest.mark.parametrize("case", range(len(T.REFUSALS)), ids=[c[0] for c in T.REFUSALS])
def test_conv_form_refusals_write_nothing(lib, case):
    T.run_refusal(lib, "cuda", T.REFUSALS[case])


@pytest.mark.parametrize("name", [n for n in T.SWITCH_SETS if n != "default" and n not in T.EMU_ONLY_SETS])
def test_conv_switch_set_on_the_diagnostics_build(diag_lib, tmp_path, name):
    """(a) and (d) ((b), (c) too for the reg set) under one switch set, in a fresh process that loads the diagnostics build
    under that environment."""
    out = tmp_path / f"{name}.pt"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "conv_form_child.py"), str(out), name, "--gpu"],
                       env=T.child_env(name, os.environ), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, f"{name}: exit {p.returncode}: {p.stderr[-2000:]}"
    res = torch.load(out)
    bad = {k: v["error"] for k, v in res.items() if "error" in v}
    assert not bad, bad
    rows = T.rows_of(name)
    assert rows and all(r.name in res for _, r in rows)
    print(f"{name}: worst error / bound {max(res[r.name]['ratio'] for _, r in rows):.4f}")
