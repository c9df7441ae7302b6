"""Shared comparison logic: product outputs (HIP on the GPU, or the emulated kernels on the
CPU) against the golden vectors captured from the reference."""
import os

import numpy as np
import torch

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# north_star bar: 3-D joints within 1e-3 mm of the reference.
#  * conditioned fixtures (flavour "c" in cases.py: trained-like single-mode joint maps; the
#    reference's own fp32-vs-fp64 floor is <= ~4e-4 mm): |build - reference| <= 1e-3 mm, no escape.
#  * stress fixtures (random weights -> multi-modal joint maps with near-ties, uniform-noise
#    heatmaps): the reference's fp32 result itself is only reproducible to its rounding-noise floor
#    (fp32 vs the same nets in fp64, stored per fixture as margins[5]: 3e-3 .. 9e-2 mm), and any other
#    summation order inside the convs lands anywhere within that floor.  There: pass at <= 1e-3 mm, or
#    when |build - ref32| <= FLOOR_FACTOR x floor AND the distance to the float64 evaluation
#    |build - ref64| is <= 1e-3 mm -- except for the cases listed in FP64_EXCEPTIONS.
BAR_MM = 1e-3
FLOOR_FACTOR = 3.0
# |build - ref64| bound (mm) where it is not <= 1e-3: the three uniform-noise heatmap fixtures.  Their
# joint maps are almost flat (softmax mass spread over the whole 2 m cube, mean absolute deviation
# ~500 mm), so the build's own fp32 conv rounding (|d feat| ~ 1e-7, times beta = 100, times 500 mm)
# moves the expectation by a few 1e-3 mm, exactly like the reference's (floors 5e-3 .. 5e-2 mm there).
FP64_EXCEPTIONS = {"tiny_u_b3_thr": 3e-3, "campus_u_b2_all": 4e-3, "panoptic_u_b1_all": 6e-3}


# Conditioned fixtures on which the REFERENCE's fp32 output is itself further than 1e-3 mm from its own float64 evaluation,
# so "within 1e-3 mm of the reference's fp32 result" is below what the reference reproduces.  Campus: 3 views, world
# coordinates of 4 .. 7.5 m (one fp32 ulp = 4.9e-4 mm), blurry 360 x 288 images -> every person of every seed has a
# reference fp32-vs-fp64 distance of 0.8e-3 .. 2.0e-3 mm (tests/golden/find_conditioned.py, cases.py).  The bar asserted
# there, per valid proposal p with pfloor_p = max_j |ref32 - ref64| (the reference's own error on that person):
#     max_j |build - ref64| <= K64 * pfloor_p     the build is at most 1.5x as far from the exact answer as the reference
#     max_j |build - ref32| <= K32 * pfloor_p     and within twice the reference's own error of the reference's fp32 result
# (tighter than the triangle inequality K64 + 1 = 2.5, and than the seed sweep's R2 factor 3).  Fixed before the first GPU
# run of this fixture; the CPU emulation of the kernels gave worst ratios 1.26 / 1.71 (9 proposals, pfloor 0.96e-3 .. 1.97e-3,
# |build - ref32| max 2.0e-3 mm: the literal 1e-3 mm bar is NOT met on Campus, by the reference's fp32 path either).
# Round 6: K32 is no longer only a chosen constant - the reference run against ITSELF with another conv summation order
# (tests/golden/reorder_distribution.json, make_reorder_distribution.py) lands up to 1.62 x a Campus proposal's own floor
# from its fp32 result (p95 1.38, 100 of 100 proposals within 2 x): K32 = 2.0 = 1.25 x that maximum, rounded.
FLOOR_RULE = {"campus_c_b2_thr": (1.5, 2.0)}
FLOOR_RULE_ABS_MM = 2.5e-3


def floor_rule_check(case, xyz, g, report=None):
    """Assert FLOOR_RULE[case] for joints ``xyz`` [B,N,J,3] (numpy) against the golden ``g``; returns the worst ratios."""
    k64, k32 = FLOOR_RULE[case]
    v = g["valid"]
    f3 = xyz.astype(np.float64)
    d32 = np.linalg.norm(f3 - g["fused_poses"][..., :3], axis=-1)            # [B,N,J]
    d64 = np.linalg.norm(f3 - g["floor_fused"], axis=-1)
    pfl = np.linalg.norm(g["fused_poses"][..., :3].astype(np.float64) - g["floor_fused"], axis=-1).max(axis=-1)   # [B,N]
    r64 = d64.max(axis=-1)[v] / pfl[v]
    r32 = d32.max(axis=-1)[v] / pfl[v]
    if report is not None:
        report.update(worst_ratio_vs_fp64=float(r64.max()), worst_ratio_vs_ref32=float(r32.max()),
                      proposal_floor_min_mm=float(pfl[v].min()), proposal_floor_max_mm=float(pfl[v].max()))
    assert pfl[v].min() > 5e-4, "fixture no longer needs the floor rule"
    # an absolute ceiling beside the ratio bars: a regression that scales with the proposals' own floors
    # cannot hide behind them (measured on the MI355X: 1.97e-3 mm)
    assert d32.max(axis=-1)[v].max() <= FLOOR_RULE_ABS_MM, f"{case}: |build-ref32| max {d32.max(axis=-1)[v].max():.2e} mm"
    assert r64.max() <= k64 and r32.max() <= k32, \
        f"{case}: |build-ref64| / pfloor max {r64.max():.2f} (bar {k64}), |build-ref32| / pfloor max {r32.max():.2f} (bar {k32})"
    return float(r64.max()), float(r32.max())


# ---- drift gate ---------------------------------------------------------------------------
# tests/golden/parity_baseline.json holds the float results of the HIP path on the MI355X as they are at the commit it names.
# The kernels are deterministic, so an unchanged build reproduces them exactly on any box; a change of a summation order
# moves them.  Nothing used to fail until the 1e-3 mm bar itself (Shelf went 3.1e-4 -> 4.3e-4 mm in round 5 unnoticed in the
# documents): now a fixture / sweep figure that GROWS past the tolerance below fails the GPU suite unless the baseline file
# is updated in the same commit (tools/update_parity_baseline.py) - the drift is then visible in the diff.
DRIFT_TOL = 1.10            # a tracked maximum may grow by 10 % before the baseline has to be re-pinned
DRIFT_FLOOR_FACTOR = 1.5    # conditioned Panoptic / Shelf fixtures: |build - ref32| max <= 1.5 x the reference's own fp32-vs-fp64 floor
DRIFT_FRAC_TOL = 0.003      # fraction of sweep joints within 1e-3 mm may drop by 0.3 points


def parity_baseline():
    import json
    with open(os.path.join(GOLDEN_DIR, "parity_baseline.json")) as f:
        return json.load(f)


def drift_check(kind, name, rep):
    """kind = 'fixtures' (rep of check_outputs) or 'sweeps' (summary of seed_sweep.replay).  Returns the findings; the
    callers assert that the list is empty."""
    if os.environ.get("FVP_TEST_DIAG_LIB") == "1":
        return []          # tools/gpu_switch_matrix.sh: alternative kernels (other summation orders) on purpose; the bars above still apply
    base = parity_baseline()[kind].get(name)
    if base is None:
        return [f"{name}: no entry in tests/golden/parity_baseline.json (run tools/update_parity_baseline.py)"]
    bad = []

    def grew(key, tol=DRIFT_TOL):
        if key in base and key in rep and rep[key] > tol * base[key] + 1e-12:
            bad.append(f"{name}: {key} {rep[key]:.4g} > {tol:.2f} x baseline {base[key]:.4g}")

    if kind == "fixtures":
        grew("max_mm_vs_fp64")
        if is_conditioned(name):
            grew("max_mm_vs_ref")
            if name not in FLOOR_RULE and rep["max_mm_vs_ref"] > DRIFT_FLOOR_FACTOR * rep["ref_floor_mm"] + 1e-12:
                bad.append(f"{name}: max_mm_vs_ref {rep['max_mm_vs_ref']:.3e} > {DRIFT_FLOOR_FACTOR} x the reference's own floor "
                           f"{rep['ref_floor_mm']:.3e}")
            for key in ("worst_ratio_vs_fp64", "worst_ratio_vs_ref32"):
                grew(key)
    else:
        for key in ("max_mm_r1q", "max_mm_where_floor_le_4e-4", "worst_err_over_proposal_floor", "worst_proposal_err_over_own_floor"):
            grew(key)
        if rep.get("violations_where_floor_le_4e-4", 0) > base.get("violations_where_floor_le_4e-4", 0):
            bad.append(f"{name}: literal-R1 violations {rep['violations_where_floor_le_4e-4']} > baseline {base['violations_where_floor_le_4e-4']}")
        if rep["frac_within_1e-3_mm"] < base["frac_within_1e-3_mm"] - DRIFT_FRAC_TOL:
            bad.append(f"{name}: fraction of joints within 1e-3 mm {rep['frac_within_1e-3_mm']:.4f} < baseline "
                       f"{base['frac_within_1e-3_mm']:.4f} - {DRIFT_FRAC_TOL}")
        if rep["joints"] != base["joints"] or rep["proposals"] != base["proposals"]:
            bad.append(f"{name}: compared {rep['joints']} joints / {rep['proposals']} proposals, baseline {base['joints']} / {base['proposals']}")
    return bad


def is_conditioned(case):
    from cases import CASES
    return CASES[case][1] == "c"


def load_golden(case):
    return np.load(os.path.join(GOLDEN_DIR, case + ".npz"))


def joint_errors(fused, g):
    v = g["valid"]
    f = fused[..., :3].detach().cpu().numpy()
    e32 = np.linalg.norm((f - g["fused_poses"][..., :3])[v], axis=-1)
    e64 = np.linalg.norm((f - g["floor_fused"])[v], axis=-1)
    return e32, e64, float(g["margins"][5])


def check_outputs(case, g, fused, planes, centers, engine, report=None):
    """Exact checks on integer / index work, tolerance checks on floating point."""
    v = g["valid"]
    last = engine.last
    # --- HDN: cubes are bit-exact by construction (same fp32 op order as the reference's CPU path).  The forward
    # materialises them only when engine.keep_hdn_cubes is set (the callers of this function run both ways).
    sx, sy = g["cubes_sub_stride"]
    if last["cubes"] is not None:
        cubes = last["cubes"].detach().cpu()
        assert np.array_equal(cubes[:, :, ::sx, ::sy, :].numpy(), g["cubes_sub"]), "HDN cubes differ"
        np.testing.assert_allclose(cubes.double().sum(dim=(1, 2, 3, 4)).numpy(), g["cubes_sum"], rtol=1e-12)
        np.testing.assert_allclose((cubes.double() ** 2).sum(dim=(1, 2, 3, 4)).numpy(), g["cubes_sq"], rtol=1e-12)
        assert torch.equal(last["zmax"].cpu(), cubes.max(dim=4)[0]), "fused z-max != max over the cubes"
        # the proposal columns (projected directly or gathered) are columns of these cubes
        Bc, Jc = cubes.shape[:2]
        cols = cubes.flatten(2, 3).permute(0, 2, 1, 3)                              # [B, XY, J, Z]
        fl = last["flat"].cpu()
        want = torch.stack([cols[b][fl[b]] for b in range(Bc)])                    # [B, N, J, Z]
        assert torch.equal(last["feat1d"].cpu().view(want.shape), want), "proposal z-columns != columns of the cubes"
    # --- HDN's public outputs (human_detection_net.py:76-104: hm2d, hm1d, proposal_centers, bbox_preds) against the
    # reference's: conv outputs in another summation order (same bar as the conv-stack tests), indices exact
    hm2d = last["hm2d"].detach().cpu().numpy()
    assert hm2d.shape[1] == 1
    np.testing.assert_allclose(hm2d[:, 0], g["hm2d"], rtol=1e-4, atol=2e-5, err_msg="hm2d (CenterNet heatmap head)")
    np.testing.assert_allclose(last["hm1d"].detach().cpu().numpy(), g["hm1d"], rtol=1e-4, atol=2e-5,
                               err_msg="hm1d (C2CNet output)")
    Bh, _, Xh, Yh = hm2d.shape
    bbox = last["bbox_flat"].detach().cpu().numpy()                                   # [B, X*Y, 2] (:88)
    assert bbox.shape == (Bh, Xh * Yh, 2)
    bmap = bbox.reshape(Bh, Xh, Yh, 2).transpose(0, 3, 1, 2)                          # back to [B,2,X,Y]
    np.testing.assert_allclose(bmap[:, :, ::sx, ::sy], g["bbox_map_sub"], rtol=1e-4, atol=2e-5,
                               err_msg="bbox_preds (CenterNet size head)")
    assert np.array_equal(bmap, last["bbox_map"].detach().cpu().numpy()), "bbox_preds is not the flattened size map"
    # topk_index [B,N,3] int64 (:98): (ix, iy) from the flat index with the reference's divisor quirk (get_index2D
    # divides by shape[1] = X), iz = the z arg-max that produced the bit-equal proposal centres
    ti = last["topk_index"].cpu().numpy()
    assert ti.dtype == np.int64
    assert np.array_equal(ti[..., 0], g["topk_flat"] // Xh) and np.array_equal(ti[..., 1], g["topk_flat"] % Xh)
    assert np.array_equal(ti[..., 2], np.argmax(g["hm1d"], axis=2)), "z arg-max index differs from the reference's hm1d"
    # --- proposals: indices exact
    assert np.array_equal(last["flat"].cpu().numpy(), g["topk_flat"]), "top-k flat indices differ"
    c = centers.detach().cpu().numpy()
    gc = g["proposal_centers"]
    # ABI 8: the mask of faster_voxelpose.py:45 comes out of fvp_proposals as uint8 flags
    if "valid" in last:
        assert last["valid"].dtype == torch.uint8 and np.array_equal(last["valid"].cpu().numpy().astype(bool), gc[..., 3] >= 0)
    assert np.array_equal(c[..., :3], gc[..., :3]), "proposal centres (mm) not bit-equal"
    assert np.array_equal(c[..., 3], gc[..., 3]), "valid flags differ"
    np.testing.assert_allclose(c[..., 5:7], gc[..., 5:7], rtol=0, atol=5e-5)
    np.testing.assert_allclose(c[..., 4], gc[..., 4], rtol=2e-4, atol=1e-6)
    np.testing.assert_allclose(last["conf2d"].cpu().numpy(), g["conf2d"], rtol=1e-4, atol=1e-5)
    # --- JLN integer window arithmetic: exact
    N = v.shape[1]
    boxes = engine.last_jln["boxes"].cpu().numpy().reshape(v.shape[0], N, 9)
    offset = engine.last_jln["offset"].cpu().numpy().reshape(v.shape[0], N, 3)
    for f in range(v.shape[0]):
        if f"jl{f}_tl" not in g:
            continue
        assert np.array_equal(boxes[f][v[f]][:, 0:3], g[f"jl{f}_tl"])
        assert np.array_equal(boxes[f][v[f]][:, 3:6], g[f"jl{f}_start"])
        assert np.array_equal(boxes[f][v[f]][:, 6:9], g[f"jl{f}_end"])
        assert np.array_equal(offset[f][v[f]], g[f"jl{f}_offset"])
        # tri-planes: bit-exact (max of bit-exact samples)
        P = int(v[f].sum())
        planes_f = engine.last_jln["planes"].cpu().reshape(v.shape[0], N, 3, *engine.last_jln["planes"].shape[2:])[f][
            torch.from_numpy(v[f])]                                   # [P,3,J,C,C]
        tri = torch.cat([planes_f[:, 0], planes_f[:, 1], planes_f[:, 2]])   # reference order [3P,J,C,C]
        np.testing.assert_allclose(tri.double().sum(dim=(1, 2, 3)).numpy(), g[f"jl{f}_tri_sum"], rtol=1e-12)
        cs = int(g[f"jl{f}_tri_cstride"])
        rows = g[f"jl{f}_tri_rows"]
        assert np.array_equal(tri[rows][:, ::cs].numpy(), g[f"jl{f}_tri"]), "tri-plane maxima differ"
        # P2PNet features / WeightNet weights: fp32 conv in a different summation order
        feat = engine.last_jln["feat"].cpu().reshape(v.shape[0], N, 3, *engine.last_jln["feat"].shape[1:])[f][
            torch.from_numpy(v[f])]
        ft = torch.cat([feat[:, 0], feat[:, 1], feat[:, 2]])
        np.testing.assert_allclose(ft[rows][:, ::cs].numpy(), g[f"jl{f}_feat"], rtol=0, atol=2e-5)
        w = engine.last_jln["wgt"].cpu().reshape(v.shape[0], N, 3, -1)[f][torch.from_numpy(v[f])]
        wt = torch.cat([w[:, 0], w[:, 1], w[:, 2]])
        np.testing.assert_allclose(wt.numpy(), g[f"jl{f}_weights"], rtol=0, atol=2e-5)
    # --- final joints
    e32, e64, floor = joint_errors(fused, g)
    if report is not None:
        report.update(case=case, max_mm_vs_ref=float(e32.max()) if e32.size else 0.0,
                      mean_mm_vs_ref=float(e32.mean()) if e32.size else 0.0,
                      max_mm_vs_fp64=float(e64.max()) if e64.size else 0.0, ref_floor_mm=floor)
    if case in FLOOR_RULE and e32.size:
        floor_rule_check(case, fused[..., :3].detach().cpu().numpy(), g, report)
    elif e32.size:
        if is_conditioned(case):
            ok = e32.max() <= BAR_MM                       # the north-star bar itself
        else:
            ok = e32.max() <= BAR_MM or (e32.max() <= FLOOR_FACTOR * floor and
                                         e64.max() <= FP64_EXCEPTIONS.get(case, BAR_MM))
        assert ok, f"{case}: |build-ref32| max {e32.max():.2e} mm, |build-ref64| max {e64.max():.2e} mm, " \
                   f"reference fp32 noise floor {floor:.2e} mm"
    f = fused.detach().cpu().numpy()
    assert np.array_equal(f[..., 3], g["fused_poses"][..., 3])
    assert np.all(f[..., :3][~v] == 0.0), "invalid proposals must have zero joints"
    np.testing.assert_allclose(f[..., 4], g["fused_poses"][..., 4], rtol=2e-4, atol=1e-6)
    pl = planes.detach().cpu().numpy()
    tol = BAR_MM if (is_conditioned(case) and case not in FLOOR_RULE) else max(BAR_MM, FLOOR_FACTOR * floor) * 2
    np.testing.assert_allclose(pl, g["plane_poses"], rtol=0, atol=tol)


# NaN bit pattern of the poisoned buffers (run_custom_conv_stack(poison=True)): a quiet NaN no float operation produces
POISON_BITS = 0x7FA5A5A5
POISON_GUARD = 4096            # floats of guard region before and after every poisoned buffer


def run_custom_conv_stack(lib, device, spec, weights, x, stream=None, plane_valid=None, valid_div=1, poison=False, eps=1e-5,
                          info=None, allow_rc=()):
    """Run a hand-made ``netspec.StackSpec`` (finalized) through fvp_pack_conv + fvp_conv_stack_run.
    ``weights``: {key + '.weight' / '.bias': tensor}, and for a conv with a BN key {bn + '.weight' / '.bias' /
    '.running_mean' / '.running_var'}; ``x``: [planes, C, H, W].  Returns every activation buffer.
    ``info`` (a dict, optional) receives the packed parameter blob (``info['blob']``: bias | scale | shift at each op's e_off).
    ``poison=True``: every buffer, the input included, is carved out of an allocation with POISON_GUARD floats of guard
    before and after it; guards and outputs are pre-filled with POISON_BITS.  Returns (buffers, check); check() asserts that
    every guard is bit-identical (else the stack wrote out of bounds) and that every output element of a valid plane
    (plane_valid[n // valid_div] != 0) is finite (a NaN there was read from memory the zero padding should have masked,
    or is an element nobody wrote).  On the CPU emulation (tests/hipemu) the guards are also read fences: check() asserts
    that no emulated buffer load read them, even a value the kernel then discarded.  check(unwritten=ids): those buffers
    must still hold POISON_BITS everywhere (a map a fused epilogue never stores, every buffer after a refusal) instead of
    finite values.  ``allow_rc``: error codes of fvp_conv_stack_run that do not raise (info['rc'] receives the code)."""
    import ctypes as C

    from faster_voxelpose_amd import _capi as capi
    blob = torch.zeros(max(spec.nparams, 4), device=device)
    s = stream
    pack_custom_conv_stack(lib, device, spec, weights, blob, s, eps)
    return _run_packed_conv_stack(lib, device, spec, blob, x, s, plane_valid, valid_div, poison, info, allow_rc)


def pack_custom_conv_stack(lib, device, spec, weights, blob, s=None, eps=1e-5):
    """fvp_pack_conv for every conv of a finalized spec into ``blob`` (see run_custom_conv_stack)."""
    import ctypes as C

    from faster_voxelpose_amd import _capi as capi
    keep = []
    for key, bn, transposed, oi in spec.param_keys:
        w = weights[key + ".weight"].to(device).contiguous()
        b = weights[key + ".bias"].to(device).contiguous()
        bnp = [None] * 4
        if bn is not None:
            bnt = [weights[bn + k].to(device=device, dtype=torch.float32).contiguous()
                   for k in (".weight", ".bias", ".running_mean", ".running_var")]
            keep += bnt
            bnp = [C.c_void_p(t.data_ptr()) for t in bnt]
        capi.check(lib, lib.fvp_pack_conv(C.c_void_p(w.data_ptr()), C.c_void_p(b.data_ptr()), *bnp, eps,
                                          1 if transposed else 0, C.byref(spec.op_array[oi]), C.c_void_p(blob.data_ptr()), s),
                   "fvp_pack_conv")
    return blob


def _run_packed_conv_stack(lib, device, spec, blob, x, s, plane_valid, valid_div, poison, info, allow_rc):
    import ctypes as C

    from faster_voxelpose_amd import _capi as capi
    planes = x.shape[0]
    shapes = [(planes,) + tuple(b) for b in spec.bufs]
    if not poison:
        bufs = [x.to(device).contiguous()] + [torch.empty(sh, device=device) for sh in shapes[1:]]
    else:
        G = POISON_GUARD
        flats, bufs = [], []
        for i, sh in enumerate(shapes):
            n = int(np.prod(sh))
            f = torch.full((n + 2 * G,), POISON_BITS, dtype=torch.int32, device=device).view(torch.float32)
            v = f[G:G + n].view(sh)
            if i == 0:
                v.copy_(x.to(device))
            flats.append(f)
            bufs.append(v)
    fence = poison and device == "cpu" and hasattr(lib, "hipemu_fence")
    if fence:                     # the CPU emulation also counts reads of the guards (tests/hipemu: read fences)
        lib.hipemu_fence.argtypes = [C.c_void_p, C.c_size_t]
        lib.hipemu_fenced_reads.restype = C.c_long
        lib.hipemu_fences_clear()
        for f in flats:
            n = f.numel() - 2 * G
            lib.hipemu_fence(C.c_void_p(f.data_ptr()), 4 * G)
            lib.hipemu_fence(C.c_void_p(f.data_ptr() + 4 * (G + n)), 4 * G)
    arr = (C.c_void_p * len(bufs))(*[t.data_ptr() for t in bufs])
    pv = None if plane_valid is None else plane_valid.to(device=device, dtype=torch.uint8).contiguous()
    rc = lib.fvp_conv_stack_run(spec.op_array, len(spec.ops), C.c_void_p(blob.data_ptr()), arr, len(bufs), planes,
                                None if pv is None else C.c_void_p(pv.data_ptr()), valid_div, s)
    if info is not None:
        info["rc"] = rc
    if rc not in allow_rc:
        capi.check(lib, rc, "fvp_conv_stack_run")
    reads = 0
    if fence:
        reads = int(lib.hipemu_fenced_reads())
        lib.hipemu_fences_clear()
    if info is not None:
        info["blob"] = blob
    if not poison:
        return bufs

    def check(unwritten=()):
        # (on the device: the buffers of a 240-plane layer are gigabytes)
        valid = torch.ones(planes, dtype=torch.bool)
        if plane_valid is not None:
            valid = plane_valid.cpu().bool()[torch.arange(planes) // valid_div]
        valid = valid.to(device)
        assert reads == 0, f"{reads} reads of guard words (memory the kernel's masking should have kept it from)"
        for i, f in enumerate(flats):
            bits = f.view(torch.int32)
            n = bits.numel() - 2 * G
            bad = int((bits[:G] != POISON_BITS).sum()) + int((bits[G + n:] != POISON_BITS).sum())
            assert bad == 0, f"buffer {i}: {bad} guard words changed (out-of-bounds write)"
            if i in unwritten:
                nw = int((bits[G:G + n] != POISON_BITS).sum())
                assert nw == 0, f"buffer {i}: {nw} elements written (it must stay untouched)"
            elif i > 0:
                nf = int((~torch.isfinite(bufs[i][valid])).sum())
                assert nf == 0, f"buffer {i}: {nf} non-finite elements in valid planes (unwritten, or read unmasked memory)"
    return bufs, check


# ---- Winograd F(2x2,3x3) layer tests (tests/test_wino_*.py) ---------------------------------------------------------------
# A-priori error bound of one k_conv_wino layer against its float64 evaluation, per output element:
#
#     |y - y64| <= gamma * ( |s| * (conv(|x|, |w|) + |b|) + |t| + |r| ),   gamma = WINO_K * eps32
#
# (s, t: the BN scale / shift the layer packed, b: bias, r: the residual; ReLU and max-pool are 1-Lipschitz, so the same
# bound - max-pooled - covers the ReLU'd and the pooled outputs).  WINO_K counts the fp32 roundings on the longest path of one
# output and scales them by the magnitude growth of the transforms:
#   * outside the channel sum: input transform B^T d B 2 (row pass, column pass; every V is a +-1 combination), weight
#     transform G g G^T 4 (two adds per pass, the halving is exact), output transform A^T M A 4 (two adds per pass), the
#     epilogue 3 (acc + bias, the BN fma, + residual): WINO_ROUNDINGS = 13;
#   * the channel sum: one fma per channel in one chain (v_mfma_f32_16x16x4_f32 accumulates 4 channels per instruction,
#     chunk after chunk): at most WINO_CIN_MAX = 128 (the widest layer of P2PNet / CenterNet);
#   * the standard bound of a length-n fp32 evaluation is n * eps32 relative to the same sum of magnitudes.  The Winograd
#     form sums magnitudes of the transformed operands, |A^T| ( sum_ci |G g G^T| .* |B^T d B| ) |A|, which is a few times
#     conv(|x|, |w|): every U = G g G^T entry mixes up to 9 taps with weights <= 1/4 .. 1, every V up to 4 inputs, and
#     A^T sums 3 of the 16 products per output and pass.  For data with more than a handful of taps x channels per output the
#     ratio concentrates near 2 .. 3; WINO_SPREAD = 4 covers it (pointwise it is unbounded - an output whose own taps see
#     zeros while the rest of its 4x4 patch does not - which is why this is a bound for the random operands of these tests,
#     not for every possible input).
#   WINO_K = WINO_SPREAD * (WINO_ROUNDINGS + WINO_CIN_MAX) = 564.
# Measured (worst error / bound over every case): see tests/test_wino_emu.py (emulator) and tests/test_wino_conv.py (MI355X);
# both far below 1/2.  tests/test_wino_emu.py::test_wino_bound_rejects_mutated_references shows the bound is still sharp enough
# to reject a dropped channel, a missing tap, a wrong halo, a wrong residual, a shifted BN block or a misplaced ReLU.
WINO_ROUNDINGS = 13
WINO_CIN_MAX = 128
WINO_SPREAD = 4
WINO_K = WINO_SPREAD * (WINO_ROUNDINGS + WINO_CIN_MAX)
EPS32 = float(np.finfo(np.float32).eps)


def wino_layer(cin, cout, hw, *, relu=True, res=False, res_after=False, bn=False, pool=False, seed=0):
    """One 3x3 conv (+ BN, residual, ReLU, fused 2x2 max-pool) as a finalized ``netspec.StackSpec``.  The residual is the
    input when cin == cout, else a 1x1 projection of the input earlier in the same stack (the product's res blocks);
    ``pool`` adds spec.pool() on the conv output, which the interpreter fuses into the Winograd epilogue.
    Returns (spec, weights, ids) with ids = {'out', 'res' (buffer id or None), 'pool' (or None), 'op' (the conv's op index)}."""
    from faster_voxelpose_amd import netspec
    h, w_ = (hw, hw) if isinstance(hw, int) else hw
    spec = netspec.StackSpec(2, cin, (h, w_))
    spec._conv_entries("c", cin, cout, 3)
    if bn:
        spec._bn_entries("n", cout)
    rid = None
    if res:
        if cin == cout:
            rid = 0
        else:
            spec._conv_entries("p", cin, cout, 1)
            rid = spec.conv("p", None, 0, cout, 1, relu=False)
    o = spec.conv("c", "n" if bn else None, 0, cout, 3, relu=relu, res=rid, res_after_relu=res_after)
    op = len(spec.ops) - 1
    pid = spec.pool(o) if pool else None
    spec.outputs["out"] = o
    spec.finalize()
    g = torch.Generator().manual_seed(seed)
    wt = {"c.weight": torch.randn(cout, cin, 3, 3, generator=g) / (cin * 9) ** 0.5, "c.bias": torch.randn(cout, generator=g) * 0.1}
    if res and cin != cout:
        wt["p.weight"] = torch.randn(cout, cin, 1, 1, generator=g) / cin ** 0.5
        wt["p.bias"] = torch.randn(cout, generator=g) * 0.1
    if bn:
        # scales of both signs and per-cout shifts that differ from one 32-cout block to the next
        blk = (torch.arange(cout) // 32).float()
        wt["n.weight"] = (0.5 + torch.rand(cout, generator=g)) * torch.where(torch.rand(cout, generator=g) < 0.3, -1.0, 1.0) * (1 + 0.25 * blk)
        wt["n.bias"] = torch.randn(cout, generator=g) * 0.2 + 0.1 * blk
        wt["n.running_mean"] = torch.randn(cout, generator=g) * 0.1 - 0.05 * blk
        wt["n.running_var"] = 0.5 + torch.rand(cout, generator=g) + 0.1 * blk
    return spec, wt, dict(out=o, res=rid, pool=pid, op=op)


def wino_reference(weights, x, r, scale, shift, relu=True, res_after=False, pool=False):
    """float64 evaluation of the layer and the magnitude term of the error bound (see WINO_K).  x [P, cin, H, W];
    r: the residual buffer as the device holds it (or None); scale / shift: the packed per-cout BN vectors (float32 values,
    as the kernel reads them).  Returns dict(y, mag[, p, pmag]) in float64."""
    import torch.nn.functional as F
    w = weights["c.weight"].double()
    b = weights["c.bias"].double()
    x = x.double()
    s = scale.double().view(1, -1, 1, 1)
    t = shift.double().view(1, -1, 1, 1)
    z = F.conv2d(x, w, None, padding=1) + b.view(1, -1, 1, 1)
    y = z * s + t
    if r is not None and not res_after:
        y = y + r.double()
    if relu:
        y = torch.relu(y)
    if r is not None and res_after:
        y = y + r.double()
    mag = s.abs() * (F.conv2d(x.abs(), w.abs(), None, padding=1) + b.abs().view(1, -1, 1, 1)) + t.abs()
    if r is not None:
        mag = mag + r.double().abs()
    out = dict(y=y, mag=mag)
    if pool:
        out["p"] = F.max_pool2d(y, 2)
        out["pmag"] = F.max_pool2d(mag, 2)
    return out


def wino_ratio(y, y64, mag, gamma=None):
    """max |y - y64| / (gamma * mag) (gamma defaults to WINO_K * eps32); > 1 = the bound is violated.  NaN counts as a violation."""
    gamma = WINO_K * EPS32 if gamma is None else gamma
    err = (y.double() - y64).abs()
    if not torch.isfinite(err).all():
        return float("inf")
    return float((err / (gamma * mag + 1e-300)).max())


def wino_packed_bn(spec, blob, op):
    """(scale, shift) of op ``op`` as packed in the parameter blob (float32, on the CPU)."""
    o = spec.op_array[op]
    e = blob[o.e_off:o.e_off + 3 * o.coutp].cpu()
    return e[o.coutp:o.coutp + o.cout], e[2 * o.coutp:2 * o.coutp + o.cout]


def wino_prof_launches(lib, run):
    """Winograd launches made by ``run()`` on the GPU: (FVP_K_CONV_WINO, FVP_K_CONV_WINO_SMALL) counts of the per-launch
    profiler (fvp_prof_enable(2)); the profiler is reset and switched off again afterwards."""
    import ctypes as C

    from faster_voxelpose_amd import _capi as capi
    lib.fvp_prof_reset()
    lib.fvp_prof_enable(2)
    try:
        run()
        torch.cuda.synchronize()
        counts = []
        for cls in (capi.K_CONV_WINO, capi.K_CONV_WINO_SMALL):
            ms, n, fl = C.c_double(), C.c_int64(), C.c_double()
            lib.fvp_prof_read(cls, C.byref(ms), C.byref(n), C.byref(fl))
            counts.append(int(n.value))
    finally:
        lib.fvp_prof_enable(0)
        lib.fvp_prof_reset()
    return tuple(counts)


def split_k_stack(cin, cmid, hw, seed=0):
    """conv3x3 cin->cmid (ReLU) then conv3x3 cmid->cmid + residual (ReLU) on a map that is NOT a power of two
    (so the direct kernel runs, and with >= 64 channels on <= 40x40 its split-K form): spec, weights, torch reference."""
    import torch.nn.functional as F

    from faster_voxelpose_amd import netspec
    spec = netspec.StackSpec(2, cin, hw)
    spec._conv_entries("a", cin, cmid, 3)
    spec._conv_entries("b", cmid, cmid, 3)
    h = spec.conv("a", None, 0, cmid, 3, relu=True)
    o = spec.conv("b", None, h, cmid, 3, relu=True, res=h)
    spec.outputs["out"] = o
    spec.finalize()
    g = torch.Generator().manual_seed(seed)
    w = {"a.weight": torch.randn(cmid, cin, 3, 3, generator=g) / (cin * 9) ** 0.5, "a.bias": torch.randn(cmid, generator=g) * 0.1,
         "b.weight": torch.randn(cmid, cmid, 3, 3, generator=g) / (cmid * 9) ** 0.5, "b.bias": torch.randn(cmid, generator=g) * 0.1}

    def ref(x):
        x = x.double()
        h1 = F.relu(F.conv2d(x, w["a.weight"].double(), w["a.bias"].double(), padding=1))
        return F.relu(F.conv2d(h1, w["b.weight"].double(), w["b.bias"].double(), padding=1) + h1)
    return spec, w, ref, o


def front7_stack(cin, hw, seed=0):
    """The 7x7 front conv of P2PNet / CenterNet (cnns_2d.py:119-121: cin = joints -> 16, BN folded away here, ReLU) on a map
    whose width k_conv7 takes (64 / 80 / 128): spec, weights, float64 torch reference, output buffer id."""
    import torch.nn.functional as F

    from faster_voxelpose_amd import netspec
    spec = netspec.StackSpec(2, cin, hw)
    spec._conv_entries("f", cin, 16, 7)
    o = spec.conv("f", None, 0, 16, 7, relu=True)
    spec.outputs["out"] = o
    spec.finalize()
    g = torch.Generator().manual_seed(seed)
    w = {"f.weight": torch.randn(16, cin, 7, 7, generator=g) / (cin * 49) ** 0.5, "f.bias": torch.randn(16, generator=g) * 0.1}

    def ref(x):
        return F.relu(F.conv2d(x.double(), w["f.weight"].double(), w["f.bias"].double(), padding=3))
    return spec, w, ref, o


def reg_stack(seed=0, fused_head=True, head_cout=15):
    """1x1 convs and transposed convs with P2PNet's channel counts on 16x16 / 8x8 maps (whole 32-pixel tiles): the layers
    k_conv_reg takes.  x [planes, 32, 16, 16] -> 1x1 32->64, pool, 1x1 64->128, up 128->64 (+ skip), up 64->32 (+ skip),
    1x1 32->15 (fused into the second transposed conv when it is that conv's only consumer), 1x1 16->32 on a slice-free
    side branch.  Returns spec, weights, float64 torch reference (dict of outputs), output buffer ids."""
    import torch.nn.functional as F

    from faster_voxelpose_amd import netspec
    spec = netspec.StackSpec(2, 32, (16, 16))
    spec._conv_entries("s64", 32, 64, 1)
    spec._conv_entries("t128", 64, 128, 1)
    spec._conv_entries("u64", 128, 64, 2, transposed=True)
    spec._conv_entries("u32", 64, 32, 2, transposed=True)
    spec._conv_entries("head", 32, head_cout, 1)
    spec._conv_entries("d16", 32, 16, 3)
    spec._conv_entries("s32", 16, 32, 1)
    s64 = spec.conv("s64", None, 0, 64, 1, relu=False)
    p = spec.pool(s64)
    t128 = spec.conv("t128", None, p, 128, 1, relu=True)
    u64 = spec.up("u64", None, t128, 64, s64)
    u32 = spec.up("u32", None, p, 32, 0)
    head = spec.conv("head", None, u32, head_cout, 1, relu=False)
    d16 = spec.conv("d16", None, u32 if not fused_head else 0, 16, 3, relu=True)
    s32 = spec.conv("s32", None, d16, 32, 1, relu=False, res=0)
    spec.outputs.update(u64=u64, head=head, s32=s32)
    spec.finalize()
    g = torch.Generator().manual_seed(seed)

    def wb(key, cout, cin, k, transposed=False):
        shape = (cin, cout, k, k) if transposed else (cout, cin, k, k)
        return {key + ".weight": torch.randn(shape, generator=g) / (cin * k * k) ** 0.5, key + ".bias": torch.randn(cout, generator=g) * 0.1}
    w = {}
    for args in (("s64", 64, 32, 1), ("t128", 128, 64, 1), ("u64", 64, 128, 2, True), ("u32", 32, 64, 2, True),
                 ("head", head_cout, 32, 1), ("d16", 16, 32, 3), ("s32", 32, 16, 1)):
        w.update(wb(*args))

    def ref(x):
        x = x.double()
        W = {k: v.double() for k, v in w.items()}
        a = F.conv2d(x, W["s64.weight"], W["s64.bias"])
        pp = F.max_pool2d(a, 2)
        t = F.relu(F.conv2d(pp, W["t128.weight"], W["t128.bias"]))
        o_u64 = F.relu(F.conv_transpose2d(t, W["u64.weight"], W["u64.bias"], stride=2)) + a
        o_u32 = F.relu(F.conv_transpose2d(pp, W["u32.weight"], W["u32.bias"], stride=2)) + x
        o_head = F.conv2d(o_u32, W["head.weight"], W["head.bias"])
        d = F.relu(F.conv2d(o_u32 if not fused_head else x, W["d16.weight"], W["d16.bias"], padding=1))
        o_s32 = F.conv2d(d, W["s32.weight"], W["s32.bias"]) + x
        return dict(u64=o_u64, head=o_head, s32=o_s32)
    return spec, w, ref, dict(u64=u64, head=head, s32=s32)


# ---- non-Winograd conv forms, layer by layer (tests/conv_form_cases.py, tests/conv1d_fused_cases.py) ----------------------
# A-priori error bound of one direct conv / transposed conv op against its float64 evaluation, per output element:
#
#     |y - y64| <= gamma * ( |s| * (conv(|x|, |w|) + |b|) + |t| + |r| ),   gamma = (cinp * taps + c) * eps32
#
# (b: bias, s / t: the packed BN scale / shift, r: the residual; ReLU and max-pool are 1-Lipschitz).  Every direct form
# (k_conv, k_conv_dma and its pixel-pair / paired-transposed forms, k_conv7, k_conv_reg) sums an output's cinp * taps products
# in ONE chain of fused multiply-adds on the fp32 matrix cores (v_mfma_f32_32x32x2_f32 / 16x16x4: one rounding per product
# added; padded channels and the pixel-pair form's eighth tap column are zero products, which round nothing).  The standard
# bound of an n-term fp32 chain is n * u relative to the sum of magnitudes, u = eps32 / 2; eps32 is used, which also covers
# a matrix core that rounds the products of one instruction separately.  taps = kh * kw, and 1 for ConvTranspose(k2,s2):
# kernel = stride, so each output pixel sees exactly one tap.  c counts the roundings outside the chain, from the code:
#   * the epilogue, bn_affine() in csrc/fvp_common.h: acc + bias (1), fmaf(., scale, shift) (1), and + residual (1):
#     CONV_EPI_ROUNDINGS = 3;
#   * split K: k_conv_dma<..., KS> (four waves) and k_conv1d_fused (kKS = 4 slices) add four partial chains in the fixed
#     order 0, 1, 2, 3: three more adds, CONV_SPLIT_ROUNDINGS = 3 (pass split=True).
# A fused chain of ops without stored intermediates (the 1x1 head in a transposed conv's epilogue, the whole 1-D stack in
# k_conv1d_fused) is bounded by propagation (conv_chain_reference): an op's input error e enters its output as
# |s| * conv(e, |w|) (+ the residual's own error), max-pooled by a pool; the magnitudes are taken at |x64| + e.
CONV_EPI_ROUNDINGS = 3
CONV_SPLIT_ROUNDINGS = 3


def conv_gamma(op, split=False):
    """gamma of the bound above for a finalized op (capi.FvpConvOp or the dict of spec.ops with cinp)."""
    from faster_voxelpose_amd import _capi as capi
    taps = 1 if op.kind == capi.OP_CONVT2 else op.kh * op.kw
    return (op.cinp * taps + CONV_EPI_ROUNDINGS + (CONV_SPLIT_ROUNDINGS if split else 0)) * EPS32


def conv_layer(kind, cin, cout, hw, *, k=1, dim=2, relu=True, res=False, res_after=False, bn=False, pool=False, head=None, tail=None,
               seed=0):
    """One op of the conv interpreter as a finalized ``netspec.StackSpec`` (generalises wino_layer):
      kind 'conv': a k x k (dim 2) / 1 x k (dim 1) conv cin -> cout on hw (+ BN of both signs, residual before / after the
                   ReLU - the input when cin == cout, else a 1x1 projection of it earlier in the stack -, ``pool``: a max-pool
                   behind it);
      kind 'up':   ConvTranspose(k2,s2) cin -> cout from hw to 2 x hw with its skip (ReLU, then + skip).  The stack's input is
                   the skip [cout, 2h, 2w]; the transposed conv reads its max-pool (through a 1x1 conv cout -> cin when
                   cin != cout); ``head``: a 1x1 conv cout -> head behind it (P2PNet's output layer);
      kind 'pool': a 2x2 / 1x2 max-pool of the input.
    ``tail``: a 1x1 conv to that many channels behind the op (behind the pool where there is one; 'head' for kind 'up'), so
    that the op is a middle op whose result is observed through it.
    hw: (h, w), h = 1 when dim == 1.  Returns (spec, weights, ids): ids = {'op' (index of the op under test), 'out', 'pool',
    'head' (buffer ids or None), 'head_op'}."""
    from faster_voxelpose_amd import netspec
    h, w_ = (hw, hw) if isinstance(hw, int) else hw
    assert dim == 2 or h == 1
    g = torch.Generator().manual_seed(seed)
    wt = {}

    def params(key, ci, co, kk, transposed=False):
        ks = (kk,) * dim
        wt[key + ".weight"] = torch.randn(((ci, co) if transposed else (co, ci)) + ks, generator=g) / (ci * (1 if transposed else kk ** dim)) ** 0.5
        wt[key + ".bias"] = torch.randn(co, generator=g) * 0.1

    def bn_params(key, co):
        # scales of both signs and per-cout shifts that differ from one 32-cout block to the next (as wino_layer)
        blk = (torch.arange(co) // 32).float()
        wt[key + ".weight"] = (0.5 + torch.rand(co, generator=g)) * torch.where(torch.rand(co, generator=g) < 0.3, -1.0, 1.0) * (1 + 0.25 * blk)
        wt[key + ".bias"] = torch.randn(co, generator=g) * 0.2 + 0.1 * blk
        wt[key + ".running_mean"] = torch.randn(co, generator=g) * 0.1 - 0.05 * blk
        wt[key + ".running_var"] = 0.5 + torch.rand(co, generator=g) + 0.1 * blk

    ids = dict(pool=None, head=None, head_op=None)
    if kind == "conv":
        spec = netspec.StackSpec(dim, cin, (h, w_))
        spec._conv_entries("c", cin, cout, k)
        params("c", cin, cout, k)
        if bn:
            spec._bn_entries("n", cout)
            bn_params("n", cout)
        rid = None
        if res:
            rid = 0
            if cin != cout:
                spec._conv_entries("p", cin, cout, 1)
                params("p", cin, cout, 1)
                rid = spec.conv("p", None, 0, cout, 1, relu=False)
        o = spec.conv("c", "n" if bn else None, 0, cout, k, relu=relu, res=rid, res_after_relu=res_after)
        ids["op"] = len(spec.ops) - 1
        if pool:
            ids["pool"] = spec.pool(o)
    elif kind == "up":
        spec = netspec.StackSpec(dim, cout, (2 * h if dim == 2 else 1, 2 * w_))
        src = spec.pool(0)
        if cin != cout:
            spec._conv_entries("q", cout, cin, 1)
            params("q", cout, cin, 1)
            src = spec.conv("q", None, src, cin, 1, relu=False)
        spec._conv_entries("u", cin, cout, 2, transposed=True)
        params("u", cin, cout, 2, transposed=True)
        if bn:
            spec._bn_entries("n", cout)
            bn_params("n", cout)
        o = spec.up("u", "n" if bn else None, src, cout, 0)
        ids["op"] = len(spec.ops) - 1
        if head is not None:
            spec._conv_entries("h", cout, head, 1)
            params("h", cout, head, 1)
            ids["head"] = spec.conv("h", None, o, head, 1, relu=False)
            ids["head_op"] = len(spec.ops) - 1
    else:
        assert kind == "pool"
        spec = netspec.StackSpec(dim, cin, (h, w_))
        o = spec.pool(0)
        ids["op"] = 0
    ids["out"] = o
    ids["tail"] = None
    if tail is not None:
        last = ids["pool"] if ids["pool"] is not None else o
        spec._conv_entries("t", spec.bufs[last][0], tail, 1)
        params("t", spec.bufs[last][0], tail, 1)
        ids["tail"] = spec.conv("t", None, last, tail, 1, relu=False)
    spec.outputs["out"] = o
    spec.finalize()
    return spec, wt, ids


def conv_packed_epi(spec, blob, i):
    """(bias, scale, shift) of op i as packed in the parameter blob (float32 values as the kernel reads them, float64 dtype)."""
    o = spec.op_array[i]
    e = blob[o.e_off:o.e_off + 3 * o.coutp].cpu().double()
    return e[:o.cout], e[o.coutp:o.coutp + o.cout], e[2 * o.coutp:2 * o.coutp + o.cout]


def _conv_lin(spec, weights, i, x, absw=False):
    """float64 conv / transposed conv of op i without bias: x [P, cin, H, W] -> [P, cout, H', W']."""
    import torch.nn.functional as F

    from faster_voxelpose_amd import _capi as capi
    o = spec.op_array[i]
    key = [k for k, _, _, oi in spec.param_keys if oi == i][0]
    w = weights[key + ".weight"].double()
    if absw:
        w = w.abs()
    if o.kind == capi.OP_CONVT2:
        w = w.reshape(o.cin, o.cout, o.kh, o.kw)
        return F.conv_transpose2d(x, w, None, stride=(o.kh, o.kw))
    w = w.reshape(o.cout, o.cin, o.kh, o.kw)
    return F.conv2d(x, w, None, padding=(o.kh // 2, o.kw // 2))


def conv_op_reference(spec, weights, blob, i, x, r=None, xerr=None, rerr=None):
    """float64 evaluation of op i of a finalized spec on the input x (and residual r) and the magnitude term of the bound
    above: (y, mag, lin) in float64; mag is to be multiplied by conv_gamma().  A pool op returns (max-pool, None, None).
    With xerr / rerr (error bounds of x / r, chains of fused ops) the magnitudes are taken at |x| + xerr and ``lin`` is the
    propagated input error |s| * conv(xerr, |w|) + rerr (else None)."""
    import torch.nn.functional as F

    from faster_voxelpose_amd import _capi as capi
    o = spec.op_array[i]
    x = x.double()
    if o.kind == capi.OP_POOL2:
        kk = (2, 2) if o.h > 1 else (1, 2)
        return F.max_pool2d(x, kk), None, (None if xerr is None else F.max_pool2d(xerr, kk))
    b, s, t = (v.view(1, -1, 1, 1) for v in conv_packed_epi(spec, blob, i))
    y = (_conv_lin(spec, weights, i, x) + b) * s + t
    xa = x.abs() if xerr is None else x.abs() + xerr
    mag = s.abs() * (_conv_lin(spec, weights, i, xa, absw=True) + b.abs()) + t.abs()
    lin = None if xerr is None else s.abs() * _conv_lin(spec, weights, i, xerr, absw=True)
    relu, after = bool(o.flags & capi.EPI_RELU), bool(o.flags & capi.EPI_RES_AFTER_RELU)
    if r is not None:
        r = r.double()
        mag = mag + r.abs() + (0.0 if rerr is None else rerr)
        if lin is not None and rerr is not None:
            lin = lin + rerr
    if r is not None and not after:
        y = y + r
    if relu:
        y = torch.relu(y)
    if r is not None and after:
        y = y + r
    return y, mag, lin


def conv_chain_reference(spec, weights, blob, x, split=False, known=None, only=None):
    """float64 evaluation of the ops of a finalized spec (``only``: those op indices, in order) with the propagated error
    bound of every buffer they write.  ``known``: {buffer id: tensor} of buffers taken as exact inputs (default: the stack
    input x as buffer 0).  Returns ({buffer id: y64}, {buffer id: error bound})."""
    from faster_voxelpose_amd import _capi as capi
    val = {0: x.double()} if known is None else {b: v.double() for b, v in known.items()}
    err = {b: torch.zeros_like(v) for b, v in val.items()}
    for i in (range(len(spec.ops)) if only is None else only):
        o = spec.op_array[i]
        r = val[o.res] if (o.kind != capi.OP_POOL2 and o.res >= 0) else None
        y, mag, lin = conv_op_reference(spec, weights, blob, i, val[o.src], r, xerr=err[o.src], rerr=None if r is None else err[o.res])
        val[o.dst] = y
        err[o.dst] = lin if mag is None else conv_gamma(o, split) * mag + lin
    return val, err


def conv_ratio(y, y64, bound):
    """max |y - y64| / bound; > 1 = the bound is violated.  NaN counts as a violation."""
    e = (y.double() - y64).abs()
    if not torch.isfinite(e).all():
        return float("inf")
    return float((e / (bound + 1e-300)).max()) if e.numel() else 0.0


def conv_check_packed_epi(spec, weights, blob, eps=1e-5):
    """The epilogue vectors fvp_pack_conv wrote against the values folded from ``weights`` in float64: the bias bit for bit,
    scale = gamma / sqrt(var + eps) and shift = beta - mean * scale to 4 ulp of their terms (1 and 0 without a BN).  The
    references below read bias | scale | shift from the blob, as the kernels do: this keeps them independent of the packing."""
    for key, bn, _, oi in spec.param_keys:
        b, s, t = conv_packed_epi(spec, blob, oi)
        assert torch.equal(b, weights[key + ".bias"].double()), f"{key}: packed bias differs"
        if bn is None:
            assert bool((s == 1).all()) and bool((t == 0).all()), f"{key}: packed scale / shift without a BN are not 1 / 0"
            continue
        g, beta, mean, var = (weights[bn + k].double() for k in (".weight", ".bias", ".running_mean", ".running_var"))
        s64 = g / torch.sqrt(var + eps)
        assert bool(((s - s64).abs() <= 4 * EPS32 * s64.abs()).all()), f"{bn}: packed scale differs"
        assert bool(((t - (beta - mean * s64)).abs() <= 4 * EPS32 * (beta.abs() + (mean * s64).abs())).all()), f"{bn}: packed shift differs"


def conv_stack_ratio(spec, weights, blob, bufs, sel=slice(None), split=False, unstored=()):
    """Worst error / bound over every op of a stack that ran with stored intermediates ``bufs`` (planes ``sel``): each op
    against the float64 evaluation of its own stored inputs (conv_gamma, or WINO_K for an op with a Winograd weight copy); a
    max-pool must be exact (else inf).  ``unstored``: buffers a fused epilogue never wrote - their producer is skipped and
    their readers are checked through the propagated chain bound from the producer's inputs."""
    from faster_voxelpose_amd import _capi as capi
    conv_check_packed_epi(spec, weights, blob)
    cpu = [b[sel].cpu() for b in bufs]
    ops = spec.op_array
    worst = 0.0
    for i in range(len(spec.ops)):
        o = ops[i]
        if o.dst in unstored:
            continue
        if o.src in unstored:
            j = max(k for k in range(i) if ops[k].dst == o.src)
            known = {b: cpu[b] for b in (ops[j].src, ops[j].res, o.res) if b >= 0 and b not in unstored}
            val, err = conv_chain_reference(spec, weights, blob, None, split=split, known=known, only=(j, i))
            worst = max(worst, conv_ratio(cpu[o.dst], val[o.dst], err[o.dst]))
            continue
        r = cpu[o.res] if (o.kind != capi.OP_POOL2 and o.res >= 0) else None
        y, mag, _ = conv_op_reference(spec, weights, blob, i, cpu[o.src], r)
        if mag is None:
            if not torch.equal(cpu[o.dst].contiguous().view(torch.int32), y.float().contiguous().view(torch.int32)):
                return float("inf")
        else:
            gamma = WINO_K * EPS32 if o.wino_off > 0 else conv_gamma(o, split)
            worst = max(worst, conv_ratio(cpu[o.dst], y, gamma * mag))
    return worst
