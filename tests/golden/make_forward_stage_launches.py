#!/usr/bin/env python
"""Writes tests/golden/forward_stage_launches.json: the kernel-name sequence of one warm forward of the scenario of
tests/forward_stage_cases.py - every optional stage set, the tiny configuration on the CPU emulation of the kernels, a stub
torch backbone, B = 2 - first with uint8 RGB frames as views, then with an NV12 surface and PoseOverlay(nv12=True).  Run it
on the commit whose launches are to be pinned (a refactor of the forward: its parent); tests/test_forward_stages.py holds
every later tree to the list.  CPU only."""
import ctypes
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
for p in (os.path.dirname(TESTS), TESTS, HERE):
    sys.path.insert(0, p)


def emu_lib():
    """As the tests' emu_lib fixture (tests/conftest.py)."""
    from faster_voxelpose_amd import _capi as capi
    from faster_voxelpose_amd import netspec
    os.environ.setdefault("FVP_WINO_GENERIC", "1")
    os.environ.setdefault("FVP_CONV_REG_MIN_TILES", "1")
    netspec.WINO_GENERIC = True
    here = os.path.join(TESTS, "hipemu")
    subprocess.run([os.path.join(here, "build_emu.sh")], check=True, capture_output=True)
    return capi.bind(ctypes.CDLL(os.path.join(here, "libfvp_emu.so")))


def main():
    lib = emu_lib()
    import forward_stage_cases as SC
    out = {}
    for kind in SC.KINDS:
        out[kind] = SC.Scenario(lib, kind).warm_launches()[1]
        print(kind, len(out[kind]), "launches")
    with open(SC.GOLDEN, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
