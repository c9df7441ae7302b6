"""Case table and runner of the live-row promise of fvp_conv_stack_run_rows (include/fvp.h, ABI 21) on the 7x7 front conv
k_conv7 (csrc/fvp_conv7.h), shared by tests/test_conv7_live_rows_emu.py (CPU emulation) and
tests/test_conv7_live_rows_gpu.py (MI355X).  Not a test module.

A stack whose only op is the 7x7 conv + BN + ReLU, 7 planes of W = 64.  Every plane has its own range {r0, r1}; the input is
random in [0, 1] inside the range (clamped to the image) and exactly +0.0 outside, so the promise holds.  check_case():
  (a) fvp_conv_stack_run == fvp_conv_stack_run_rows(NULL), bit for bit;
  (b) the run with the array == the run without it, bit for bit (numpy.array_equal on the bit patterns; masked planes keep
      their poison in both);
  (c) the run without the array against the fp64 conv + BN + ReLU under the bound tests/conv_form_cases.py uses for this form
      (tests/common.py conv_gamma: (cinp * 49 + 3) * eps32).

Run as a program it is the child process of the fallback check (the conv switches are read once when a library loads):

    FVP_CONV_NO_K7=1 python tests/conv7_live_rows_cases.py OUT.pt [--gpu]

runs the H = 64 cases through the pixel-pair form k_conv_dma<7,7,...> with and without the array and saves, per case,
whether the bits agree (that kernel must ignore the array) and, on the emulator, the instantiations launched."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import common as CM  # noqa: E402

W, COUT, PLANES = 64, 16, 7
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1


def ranges(H, which):
    """Seven {r0, r1} per set.  'a': nothing dead; all dead twice; one live row; on and across tile edges (tiles of 4 rows);
    touching the top border.  'b': touching the bottom border; one row that its own tile and the next reach, the tile at
    y0 = 0 only as a dead neighbour; wider than the image (clamped), also at the ends of int32; r0 > r1; a range ending inside
    the last tile; everything but the border rows."""
    if which == "a":
        return [(0, H), (0, 0), (5, 5), (5, 6), (4, 8), (3, 9), (0, 3)]
    return [(H - 2, H), (7, 8), (-5, H + 9), (9, 4), (H - 5, H - 1), (1, H - 1), (INT_MIN, INT_MAX)]


# (cin, H, range set, plane_valid): 15 / 17 channels = four / five channel groups; H = 62: the last tile has two rows
CASES = [(cin, H, which, masked) for cin in (15, 17) for H in (64, 62) for which in ("a", "b") for masked in (False, True)]
PLANE_VALID = [1, 0, 1, 1, 0, 1, 1]


def case_id(c):
    return f"c{c[0]}_h{c[1]}_{c[2]}" + ("_masked" if c[3] else "")


def make_input(cin, H, rr, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand((len(rr), cin, H, W), generator=g)
    for p, (r0, r1) in enumerate(rr):
        c0, c1 = min(max(r0, 0), H), min(max(r1, 0), H)
        if c0 >= c1:
            x[p] = 0.0
        else:
            x[p, :, :c0] = 0.0
            x[p, :, c1:] = 0.0
    return x


def run(lib, device, spec, blob, x, live=None, plane_valid=None, rows_export=True):
    """One run of the stack on x into a poisoned output; live: list of (r0, r1) or None."""
    import ctypes as C

    from faster_voxelpose_amd import _capi as capi
    planes = x.shape[0]
    xin = x.to(device).contiguous()
    out = torch.full((planes,) + tuple(spec.bufs[1]), CM.POISON_BITS, dtype=torch.int32, device=device).view(torch.float32)
    arr = (C.c_void_p * 2)(xin.data_ptr(), out.data_ptr())
    pv = None if plane_valid is None else torch.tensor(plane_valid, dtype=torch.uint8, device=device)
    lr = None if live is None else torch.tensor(live, dtype=torch.int64).to(torch.int32).to(device).contiguous()
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
    if rows_export:
        rc = lib.fvp_conv_stack_run_rows(spec.op_array, len(spec.ops), ptr(blob), arr, 2, planes, ptr(pv), 1, ptr(lr), None)
    else:
        assert live is None
        rc = lib.fvp_conv_stack_run(spec.op_array, len(spec.ops), ptr(blob), arr, 2, planes, ptr(pv), 1, None)
    capi.check(lib, rc, "fvp_conv_stack_run_rows" if rows_export else "fvp_conv_stack_run")
    if device != "cpu":
        torch.cuda.synchronize()
    return xin, out


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


def layer(cin, H, seed):
    spec, w, ids = CM.conv_layer("conv", cin, COUT, (H, W), k=7, bn=True, seed=seed)
    return spec, w


def check_case(lib, device, case, index):
    """(a) - (c) of one case; returns the worst error / bound of (c)."""
    cin, H, which, masked = case
    spec, w = layer(cin, H, index)
    blob = torch.zeros(max(spec.nparams, 4), device=device)
    CM.pack_custom_conv_stack(lib, device, spec, w, blob)
    rr = ranges(H, which)
    x = make_input(cin, H, rr, 100 + index)
    pv = PLANE_VALID if masked else None
    xin, y_old = run(lib, device, spec, blob, x, None, pv, rows_export=False)
    _, y_null = run(lib, device, spec, blob, x, None, pv)
    _, y_live = run(lib, device, spec, blob, x, rr, pv)
    assert np.array_equal(bits(y_old), bits(y_null)), "fvp_conv_stack_run differs from fvp_conv_stack_run_rows(NULL)"   # (a)
    diff = bits(y_live) != bits(y_null)
    assert np.array_equal(bits(y_live), bits(y_null)), \
        f"with live_rows: {int(diff.sum())} elements differ, planes {sorted(set(np.nonzero(diff)[0].tolist()))}"        # (b)
    valid = torch.tensor(pv if masked else [1] * PLANES).bool()
    assert bool((torch.from_numpy(bits(y_null))[~valid] == CM.POISON_BITS).all()), "a masked plane was written"
    assert bool(torch.isfinite(y_null.cpu()[valid]).all())
    sel = [p for p in range(PLANES) if valid[p]]
    ratio = CM.conv_stack_ratio(spec, w, blob, [xin, y_null], sel)                                                     # (c)
    assert ratio <= 1.0, f"error / bound {ratio:.3g}"
    return ratio


FALLBACK_CASES = [c for c in CASES if c[1] == 64 and c[2] == "b" and not c[3]]


def main(argv):
    import ctypes as C

    import conv_form_cases as T
    out, gpu = argv[0], "--gpu" in argv
    lib = T.load_lib(gpu)
    device = "cuda" if gpu else "cpu"
    res = {}
    for case in FALLBACK_CASES:
        index = CASES.index(case)
        cin, H, which, _ = case
        spec, w = layer(cin, H, index)
        blob = torch.zeros(max(spec.nparams, 4), device=device)
        CM.pack_custom_conv_stack(lib, device, spec, w, blob)
        rr = ranges(H, which)
        x = make_input(cin, H, rr, 100 + index)
        if not gpu:
            lib.hipemu_launch_log_reset()
        _, y_null = run(lib, device, spec, blob, x, None)
        _, y_live = run(lib, device, spec, blob, x, rr)
        insts = T.instantiations(lib.hipemu_launch_log().decode()) if not gpu else []
        res[case_id(case)] = dict(equal=bool(np.array_equal(bits(y_null), bits(y_live))),
                                  finite=bool(torch.isfinite(y_null.cpu()).all()), insts=insts)
    torch.save(res, out)


if __name__ == "__main__":
    main(sys.argv[1:])
