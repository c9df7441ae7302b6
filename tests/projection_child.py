"""Runner of one whole-space case of tests/projection_cases.py in a process of its own: the host reads FVP_WHOLE_NO_QUAD once
per process, so the lane-per-voxel form k_project_whole needs a fresh one.

    python tests/projection_child.py OUT.json CASE [--gpu]

loads tests/hipemu/libfvp_emu.so (or, with --gpu, the diagnostics build) under the environment it was given, runs
check_whole and writes the figures, the emulator's launch log, or the text of the failed assertion.  Not a test module."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    if _p not in sys.path:
        sys.path.insert(0, _p)


def main(argv):
    import torch  # noqa: F401  (its HIP runtime first)
    from faster_voxelpose_amd import _capi as capi
    import projection_cases as P
    out, name, gpu = argv[0], argv[1], "--gpu" in argv
    path = os.path.join(ROOT, "tests", "diag", "libfvp_hip_diag.so") if gpu else os.path.join(ROOT, "tests", "hipemu", "libfvp_emu.so")
    lib = capi.bind(C.CDLL(path))
    res = {}
    if not gpu:
        lib.hipemu_launch_log.restype = C.c_char_p
        lib.hipemu_launch_log_reset()
    try:
        res["figures"] = P.check_whole(P.Ctx(lib, "cuda:0" if gpu else "cpu"), name, lane_form=True)
    except AssertionError as e:
        res["error"] = str(e) or "assertion failed"
    if not gpu:
        res["log"] = lib.hipemu_launch_log().decode()
    with open(out, "w") as f:
        json.dump(res, f)


if __name__ == "__main__":
    main(sys.argv[1:])
