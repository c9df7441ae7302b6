"""Runner of single Winograd layers on the CPU emulation of the kernels (tests/hipemu), shared by tests/test_wino_emu.py and
run as a child process by it:

    python tests/wino_emu_child.py OUT.pt

runs FORM_CASES on tests/hipemu/libfvp_emu.so under the FVP_* switches of its environment (the emulated library reads them
once when it loads, hence one process per switch set) and saves every output buffer, the worst error-to-bound ratio and the
launched k_conv_wino instantiations to OUT.pt.  Not a test module."""
import ctypes as C
import os
import re
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import common as CM  # noqa: E402

EMU_LIB = os.path.join(ROOT, "tests", "hipemu", "libfvp_emu.so")
_INST = re.compile(r"k_conv_winoILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELb([01])ELb([01])ELi(\d+)EE")

# (cin, cout, (h, w), planes, layer options): layers whose form the switches move (full / half / quarter units, resident /
# streamed weights, 32-cout blocks, the 16-wave form) - every one of them is claimed to give the same bits
FORM_CASES = [
    (8, 32, (16, 16), 1, dict(res=True)),
    (8, 32, (16, 16), 7, dict(bn=True)),
    (16, 64, (8, 8), 5, dict(bn=True, res=True)),
    (32, 128, (16, 16), 2, dict(bn=True, pool=True)),
    (12, 32, (40, 40), 1, dict(bn=True, res=True)),
    (64, 64, (20, 64), 3, dict(res=True, res_after=True)),
    (12, 64, (2, 16), 9, dict(relu=False)),
]


def instantiations(log):
    """k_conv_wino template arguments (WC, WT, CC, NI, HAS_RES, RESW, CW) of every launch in an emulator launch log."""
    return [tuple(int(v) for v in m) for m in _INST.findall(log)]


def load_emu():
    from faster_voxelpose_amd import _capi as capi
    lib = capi.bind(C.CDLL(EMU_LIB))
    lib.hipemu_launch_log.restype = C.c_char_p
    lib.hipemu_launch_log.argtypes = []
    lib.hipemu_launch_log_reset.argtypes = []
    return lib


def run_layer(lib, cin, cout, hw, planes, opts, seed=0, plane_valid=None, valid_div=1, x=None):
    """One layer through the emulated interpreter with poisoned buffers.  Asserts the poison check; returns dict(out, pool,
    ratio (worst error / bound over the conv output and the pooled output of the valid planes), insts (launched k_conv_wino
    instantiations), x)."""
    spec, w, ids = CM.wino_layer(cin, cout, hw, seed=seed, **opts)
    if x is None:
        g = torch.Generator().manual_seed(1000 + seed)
        x = torch.randn((planes,) + spec.bufs[0], generator=g)
    lib.hipemu_launch_log_reset()
    info = {}
    bufs, check = CM.run_custom_conv_stack(lib, "cpu", spec, w, x, plane_valid=plane_valid, valid_div=valid_div, poison=True,
                                           info=info)
    insts = instantiations(lib.hipemu_launch_log().decode())
    check()
    valid = torch.ones(planes, dtype=torch.bool)
    if plane_valid is not None:
        valid = plane_valid.bool()[torch.arange(planes) // valid_div]
    out = bufs[ids["out"]].clone()
    pool = bufs[ids["pool"]].clone() if ids["pool"] is not None else None
    ratio = 0.0
    if valid.any():
        sc, sh = CM.wino_packed_bn(spec, info["blob"], ids["op"])
        r = bufs[ids["res"]][valid] if ids["res"] is not None else None
        ref = CM.wino_reference(w, x[valid], r, sc, sh, relu=opts.get("relu", True), res_after=opts.get("res_after", False),
                                pool=ids["pool"] is not None)
        ratio = CM.wino_ratio(out[valid], ref["y"], ref["mag"])
        if pool is not None:
            ratio = max(ratio, CM.wino_ratio(pool[valid], ref["p"], ref["pmag"]))
    return dict(out=out, pool=pool, ratio=ratio, insts=insts, x=x)


def main(path):
    from faster_voxelpose_amd import netspec
    # the parent's emu_lib fixture set FVP_WINO_GENERIC=1 (every row width on Winograd); the host side mirrors it
    netspec.WINO_GENERIC = os.environ.get("FVP_WINO_GENERIC") == "1"
    lib = load_emu()
    res = []
    for i, (cin, cout, hw, planes, opts) in enumerate(FORM_CASES):
        r = run_layer(lib, cin, cout, hw, planes, opts, seed=i)
        res.append(dict(out=r["out"], pool=r["pool"], ratio=r["ratio"], insts=r["insts"]))
    torch.save(res, path)


if __name__ == "__main__":
    main(sys.argv[1])
