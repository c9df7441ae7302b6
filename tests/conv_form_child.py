"""Runner of tests/conv_form_cases.py in a process of its own: the conv switches of csrc/fvp_conv.hip are `static const`,
read once when the library loads, so every switch set (and the default routing, which the session's emu_lib fixture
overrides with FVP_WINO_GENERIC=1 and FVP_CONV_REG_MIN_TILES=1) needs a fresh process.

    python tests/conv_form_child.py OUT.pt SET [--gpu] [--rows name,name,...] [--part I/N]

loads tests/hipemu/libfvp_emu.so (or, with --gpu, the diagnostics build tests/diag/libfvp_hip_diag.so) under the FVP_*
variables of its environment, keeps netspec.WINO_GENERIC consistent with them, runs the rows of set SET (or the named rows, or every N-th row of the set)
and, for SET 'default', the refusals, and saves per row: the worst error / bound, the launched instantiations, the first two
output planes, or the text of the failed assertion.  Not a test module."""
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import conv_form_cases as T  # noqa: E402


def main(argv):
    from faster_voxelpose_amd import netspec
    out, set_name = argv[0], argv[1]
    gpu = "--gpu" in argv
    names = argv[argv.index("--rows") + 1].split(",") if "--rows" in argv else None
    part, nparts = (int(v) for v in argv[argv.index("--part") + 1].split("/")) if "--part" in argv else (0, 1)
    netspec.WINO_GENERIC = os.environ.get("FVP_WINO_GENERIC") == "1"
    lib = T.load_lib(gpu)
    device = "cuda" if gpu else "cpu"
    res = {}
    env = os.environ
    todo = T.rows_of(set_name) if names is None else [(i, r) for i, r in enumerate(T.ROWS) if r.name in names]
    for index, row in todo[part::nparts]:                 # (every N-th row: the parts of a set cost about the same)
        unfused = T.head_unfused(env, row)
        t0 = time.time()
        try:
            # gpu=False also under --gpu: the diagnostics build honours FVP_CONV_REG_MIN_TILES, so the rows keep their small
            # plane counts (gpu=True selects the counts that cross the SHIPPED library's thresholds)
            r = T.run_row(lib, device, row, index, gpu=False, sample=3 if gpu else None, head_fused=False if unfused else None,
                          full=set_name in ("default", "reg"))
        except AssertionError as e:
            r = dict(error=str(e) or "assertion failed")
        except Exception as e:          # a refusal of the interpreter, a missing symbol: reported, the other rows still run
            r = dict(error=f"{type(e).__name__}: {e}")
            if gpu:                     # a failed GPU call: nothing more is started on the device
                res[row.name] = r
                break
        r["seconds"] = time.time() - t0
        res[row.name] = r
    if set_name == "default" and names is None and part == 0:
        for case in T.REFUSALS:
            try:
                res["refusal:" + case[0]] = dict(rc=T.run_refusal(lib, device, case))
            except AssertionError as e:
                res["refusal:" + case[0]] = dict(error=str(e) or "assertion failed")
    torch.save(res, out)


if __name__ == "__main__":
    main(sys.argv[1:])
