"""k_conv_wino (Winograd F(2x2,3x3)) layer by layer on the MI355X, shipped library (or the diagnostics build under
tools/gpu_switch_matrix.sh, FVP_TEST_DIAG_LIB=1), in-process.  Every Winograd layer shape of P2PNet (jln64 / jln128) and
CenterNet (80 x 80 / 128 x 128 and their 3x3 heads), derived from netspec, plus the off-product edge shapes of
tests/test_wino_emu.py, at plane counts on both sides of the full / half / quarter unit thresholds:
  (a) the fp64 error bound of tests/common.py on the first, a middle and the last plane;
  (b) a plane's bits do not depend on the plane count it is computed in;
  (c) person masks (plane_valid, valid_div = 3) leave the valid planes bit-identical;
  (d) poisoned buffers: guards intact, valid outputs finite;
  (e) the layer went through k_conv_wino (profiler classes FVP_K_CONV_WINO / FVP_K_CONV_WINO_SMALL)."""
import os

import pytest
import torch

import common as CM
from test_wino_emu import EMU_CASES

pytestmark = pytest.mark.gpu

PLANE_COUNTS = (1, 7, 33, 130, 240)
# (e) is void where a switch of the diagnostics build routes the layer away from the Winograd kernel
_NO_WINO = os.environ.get("FVP_TEST_DIAG_LIB") == "1" and os.environ.get("FVP_CONV_NO_WINO", "0") not in ("", "0")


def _product_shapes():
    from faster_voxelpose_amd import _capi as capi
    from faster_voxelpose_amd import netspec
    shapes = {}
    specs = (netspec.p2pnet_spec(15, 15, 64), netspec.p2pnet_spec(15, 15, 128), netspec.centernet_spec(15, 80, 80),
             netspec.centernet_spec(15, 128, 128))
    for s in specs:
        ops = s.op_array
        for i, o in enumerate(ops):
            if o.kind == capi.OP_CONV and o.wino_off > 0:
                pool = any(ops[j].kind == capi.OP_POOL2 and ops[j].src == o.dst for j in range(i + 1, len(ops)))
                opts = dict(res=o.res >= 0, pool=pool, bn=True, res_after=bool(o.flags & capi.EPI_RES_AFTER_RELU))
                shapes[(o.cin, o.cout, (o.h, o.w), tuple(sorted(opts.items())))] = opts
    return [(c, o, hw, opts) for (c, o, hw, _), opts in sorted(shapes.items())]


def _edge_shapes():
    return [(cin, cout, hw, opts) for cin, cout, hw, _, opts in EMU_CASES]


SHAPES = _product_shapes() + _edge_shapes()


def _ids(shapes):
    return [f"{c}-{o}-{hw[0]}x{hw[1]}-" + "".join(k[0] for k, v in sorted(opts.items()) if v) for c, o, hw, opts in shapes]


def _run(lib, spec, w, x, planes, plane_valid=None):
    info = {}
    out = {}

    def go():
        out["bufs"], out["check"] = CM.run_custom_conv_stack(lib, "cuda", spec, w, x[:planes], plane_valid=plane_valid,
                                                            valid_div=3, poison=True, info=info)
    launches = CM.wino_prof_launches(lib, go)
    out["check"]()                                    # (d)
    return out["bufs"], info["blob"], launches


@pytest.fixture(scope="module")
def lib():
    from faster_voxelpose_amd import _capi as capi
    return capi.load()


@pytest.mark.parametrize("shape", range(len(SHAPES)), ids=_ids(SHAPES))
def test_wino_layer_vs_fp64(lib, shape):
    cin, cout, hw, opts = SHAPES[shape]
    spec, w, ids = CM.wino_layer(cin, cout, hw, seed=shape, **opts)
    nmax = max(PLANE_COUNTS)
    g = torch.Generator(device="cuda").manual_seed(shape)
    x = torch.randn((nmax,) + spec.bufs[0], generator=g, device="cuda")
    relu, res_after = opts.get("relu", True), opts.get("res_after", False)
    seen = {}                                         # plane -> (output, pooled output) of its first computation
    worst = 0.0
    for n in PLANE_COUNTS:
        bufs, blob, launches = _run(lib, spec, w, x, n)
        if not _NO_WINO:
            assert sum(launches) == 1, f"{n} planes: Winograd launches {launches}"          # (e)
        sc, sh = CM.wino_packed_bn(spec, blob, ids["op"])
        pick = sorted({0, n // 2, n - 1})
        xs = x[pick].cpu()
        r = bufs[ids["res"]][pick].cpu() if ids["res"] is not None else None
        ref = CM.wino_reference(w, xs, r, sc, sh, relu=relu, res_after=res_after, pool=ids["pool"] is not None)
        y = bufs[ids["out"]][pick].cpu()
        ratio = CM.wino_ratio(y, ref["y"], ref["mag"])                                        # (a)
        p = bufs[ids["pool"]][pick].cpu() if ids["pool"] is not None else None
        if p is not None:
            ratio = max(ratio, CM.wino_ratio(p, ref["p"], ref["pmag"]))
        assert ratio <= 1.0, f"{n} planes: error / bound {ratio:.3g}"
        worst = max(worst, ratio)
        for k, pl in enumerate(pick):                                                         # (b)
            if pl in seen:
                assert torch.equal(seen[pl][0], y[k]), f"plane {pl}: bits differ between plane counts"
                if p is not None:
                    assert torch.equal(seen[pl][1], p[k]), f"plane {pl}: pooled bits differ between plane counts"
            else:
                seen[pl] = (y[k], None if p is None else p[k])
        if n == 33:                                                                           # (c)
            full = bufs[ids["out"]].cpu()
            for pattern in ([0] + [1] * 10, [1, 0] * 5 + [1], [0] * 10 + [1]):
                pv = torch.tensor(pattern, dtype=torch.uint8)
                mb, _, _ = _run(lib, spec, w, x, n, plane_valid=pv)
                valid = pv.bool()[torch.arange(n) // 3]
                assert torch.equal(mb[ids["out"]].cpu()[valid], full[valid]), f"mask {pattern}: valid planes differ"
    print(f"worst error / bound {worst:.4f}")


def test_wino_both_launch_classes_occur(lib):
    """(e) across the kinds of launch: a chip-filling one (FVP_K_CONV_WINO) and one with fewer units than workgroup slots
    (FVP_K_CONV_WINO_SMALL)."""
    if _NO_WINO:
        pytest.skip("FVP_CONV_NO_WINO: the diagnostics build routes 3x3 layers to the direct kernel")
    spec, w, ids = CM.wino_layer(32, 32, 64, seed=1, bn=True)
    x = torch.randn((240,) + spec.bufs[0], device="cuda")
    big = _run(lib, spec, w, x, 240)[2]
    small = _run(lib, spec, w, x, 1)[2]
    assert big[0] == 1 and small[1] == 1, (big, small)
