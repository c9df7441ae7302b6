"""The soft-argmax + WeightNet instance for the shipped shape (64 x 64 maps, 32 features: k_softargmax_wn_fast<64, 32>) against
the generic kernel k_softargmax_weightnet on the same inputs, through the C ABI.  The fast instance claims to alter no
rounding and no summation order, so the condition is equality of bits of `pose2d`, `pmax` and `wgt`, not a tolerance.

The generic kernel is selected by construction with FVP_SOFTARGMAX_GENERIC, honoured by the diagnostics build only (GPU:
tests/diag/libfvp_hip_diag.so; CPU: the emulated kernels, which are a diagnostics build too) and read per call.

Maps: uniform noise, single bumps on noise, and the edges of the bordered LDS map and of the window loop - an all-equal map,
an all-zero map, a single peak in each corner and in the middle of each border, a map whose maximum is its last element, a
map of negative values, and a checkerboard that makes every pooled window differ from its neighbours."""
import ctypes as C

import numpy as np
import pytest
import torch

CN, F, HD, J = 64, 32, 64, 5
BETA = 100.0


def _maps(rng, n_random):
    yy, xx = np.mgrid[0:CN, 0:CN]
    maps = []
    for _ in range(n_random):
        maps.append(rng.random((CN, CN)) * 0.2)                                        # flat softmax
        cx, cy = rng.uniform(0, CN - 1, 2)
        maps.append(0.3 * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / 8.0) + 0.02 * rng.random((CN, CN)))
    maps.append(np.full((CN, CN), 0.125))                                              # all equal
    maps.append(np.zeros((CN, CN)))
    e = CN - 1
    for y, x in ((0, 0), (0, e), (e, 0), (e, e), (0, CN // 2), (e, CN // 2), (CN // 2, 0), (CN // 2, e)):
        m = np.zeros((CN, CN))
        m[y, x] = 1.0                                                                  # corners, then border middles
        maps.append(m)
    m = rng.random((CN, CN)) * 0.2
    m[e, e] = 0.5                                                                      # the maximum is the last element
    maps.append(m)
    maps.append(-rng.random((CN, CN)))                                                 # negative values next to the zero border
    maps.append(((yy + xx) % 2).astype(np.float64) * 0.01 + 1e-3 * rng.random((CN, CN)))
    while len(maps) % (3 * J):
        maps.append(rng.random((CN, CN)) * rng.uniform(0.01, 1.0))
    return np.stack(maps).astype(np.float32)


def _weightnet_blob(rng):
    """conv_w[F][9] | conv_b[F] | bn_scale[F] | bn_shift[F] | fc1_w[Hd][F] | fc1_b[Hd] | fc2_w[Hd] | fc2_b (fvp_joint.hip)"""
    parts = [rng.normal(0, 0.5, F * 9), rng.normal(0, 0.1, F), rng.uniform(0.5, 1.5, F) * rng.choice([-1.0, 1.0], F),
             rng.normal(0, 0.1, F), rng.normal(0, 0.3, HD * F), rng.normal(0, 0.1, HD), rng.normal(0, 0.3, HD),
             rng.normal(0, 0.1, 1)]
    return np.concatenate(parts).astype(np.float32)


def _run(lib, dev, feat, grid, wn, valid):
    n_people = feat.shape[0] // (3 * J)
    outs = [torch.full((n_people * 3 * J * k,), -7.0, device=dev) for k in (2, 1, 1)]   # sentinel: skipped people stay
    ptr = lambda t: C.c_void_p(t.data_ptr())                                            # noqa: E731
    rc = lib.fvp_softargmax_weightnet(ptr(feat), ptr(grid), ptr(wn), BETA, n_people, J, CN, F, HD,
                                      ptr(valid) if valid is not None else None, *[ptr(o) for o in outs], None)
    assert rc == 0, rc
    if dev != "cpu":
        torch.cuda.synchronize()
    return [o.cpu() for o in outs]


def _fast_equals_generic(lib, dev, monkeypatch, n_random):
    assert lib.fvp_diag_build() == 1, "the generic kernel is selected through a diagnostics-build switch"
    rng = np.random.default_rng(11)
    feat = torch.from_numpy(_maps(rng, n_random)).to(dev).contiguous()
    n_people = feat.shape[0] // (3 * J)
    grid = torch.from_numpy(rng.uniform(-1000.0, 1000.0, (3, CN * CN, 2)).astype(np.float32)).to(dev)
    wn = torch.from_numpy(_weightnet_blob(rng)).to(dev)
    mask = torch.ones(n_people, dtype=torch.uint8)
    mask[1::2] = 0
    for valid in (None, mask.to(dev)):
        monkeypatch.delenv("FVP_SOFTARGMAX_GENERIC", raising=False)
        fast = _run(lib, dev, feat, grid, wn, valid)
        monkeypatch.setenv("FVP_SOFTARGMAX_GENERIC", "1")
        generic = _run(lib, dev, feat, grid, wn, valid)
        monkeypatch.delenv("FVP_SOFTARGMAX_GENERIC", raising=False)
        for name, a, b in zip(("pose2d", "pmax", "wgt"), fast, generic):
            assert torch.isfinite(a).all(), name
            differ = (a.view(torch.int32) != b.view(torch.int32)).nonzero().flatten()
            assert differ.numel() == 0, f"{name}: {differ.numel()} words differ, first at {int(differ[0])}: " \
                                        f"{float(a[differ[0]])!r} vs {float(b[differ[0]])!r}"
        pose, pmax, wgt = (o.reshape(n_people, -1) for o in fast)
        live = torch.ones(n_people, dtype=torch.bool) if valid is None else mask.bool()
        assert (pmax[live] > 0).all() and (pmax[live] <= 1).all() and (wgt[live] >= 0).all() and (wgt[live] <= 1).all()
        assert (pose[~live] == -7.0).all() and (pmax[~live] == -7.0).all() and (wgt[~live] == -7.0).all()


@pytest.mark.gpu
def test_fast_instance_is_bit_equal_to_the_generic_kernel(diag_lib, monkeypatch):
    _fast_equals_generic(diag_lib, "cuda:0", monkeypatch, n_random=60)


def test_emulated_fast_instance_is_bit_equal_to_the_generic_kernel(emu_lib, monkeypatch):
    _fast_equals_generic(emu_lib, "cpu", monkeypatch, n_random=6)
