"""The JLN tail (csrc/fvp_joint.hip: k_softargmax_weightnet, k_softargmax_wn_fast<64,32>, k_fuse, k_pack_weightnet) against a
float64 restatement with an a-priori error bound, through the C ABI.  Shared by tests/test_jln_tail_emu.py (CPU emulation)
and tests/test_jln_tail_gpu.py (MI355X).  The restatement is plain numpy on the exact fp32 inputs and shares no code with
oracle/fvp_oracle.py, so the two can be compared with each other.

Bounds (u = 2^-24; every test asserts error / bound <= 1, the bounds are not fitted to what a kernel gives):

soft-argmax   p_i = exp(beta x_i - M) / S, pose = sum p_i g_i, pmax = 1 / S.  The kernel rounds beta x_i and beta x_i - m to
              fp32: an absolute error of u (|beta x_i| + |beta x_i - M|) in the exponent, the dominant term.
              d_i = u (|beta x_i| + |beta x_i - M| + 2)   (+2: expf's 1 ulp, the fp32 division, the fp32 cast of S)
              dbar = sum p_i d_i
              bound_pose = 2 [ sum p_i |g_i - pose| (d_i + dbar) + 4 u sum p_i |g_i| ]
              bound_pmax = 2 pmax (dbar + 2 u)
              (the leading 2 is the allowance for second-order terms)
WeightNet     a running forward error in fp64 next to the values: the 9-term fma chain (9 u sum |w x|), bias, BN scale, BN
              shift (one rounding each, from the magnitudes); max-pool and ReLU pass the error on (1-Lipschitz); the fp32 sum
              over NWIN windows at depth ceil(NWIN / 256) + 8, the division; fc1 as an F-term fma chain; fc2 as a
              ceil(Hd / 64)-term chain + 6 shuffle steps + the bias; the sigmoid, 1/4-Lipschitz plus 3 ulp (6 u).
fusion        planes = fp32(pose) + fp32(offset), bit for bit; fused x / y / z within 6 u (|w_a / s a| + |w_b / s b|) of fp64;
              conf within (3 J + 1) u mean(pmax); flag copied; an invalid person gives zeros with flag and centers[:, 4]
              passed through; centers[:, 4] updated in place for valid people, every other column untouched.
pack          every word of the blob equals the fp32 restatement, one rounding per operation as in k_pack_weightnet.

Worst error / bound measured over the kernel cases of this module (KERNEL_CASES, BETA_CASES, FUSE_CASES):

                          pose      pmax      wgt       fused     conf
  CPU emulation           0.154     0.454     0.086     0.428     0.057
  MI355X                  0.154     0.454     0.086     0.428     0.057
  fp32 oracle (torch)     3.36      0.701     0.086     -         -

The emulation and the GPU agree to the digits shown: the fp64 sums leave little room for the order of operations to matter.
No ratio is near 1 and none is tiny, so no term of the derivation
is missing; the sharpness of the bounds is shown by test_bound_rejects_mutated_references (tests/test_jln_tail_emu.py): each
of 14 subtly wrong restatements leaves them on some case.  The oracle's fp32 softmax carries no fp64 sums: on nearly flat
128 x 128 maps its expectation is 3.4 bounds away, which is why tests/test_gpu_parity.py compares flat maps with the oracle's
float64 variant; the oracle's float64 variant is within the bounds on every case (asserted).
Wall time: tests/test_jln_tail_emu.py 17 s (8 s of it the mutation test), tests/test_jln_tail_gpu.py 8.5 s on an MI355X (4.8 s
of it the two fresh processes of the large-LDS orderings)."""
import ctypes as C
import functools

import numpy as np
import torch

U = 2.0 ** -24
SENTINEL = -7.0
POISON_BITS = 0x7FA5A5A5           # tests/common.py: a quiet NaN no float operation produces
GUARD = 1024                       # floats of guard behind and in front of every output buffer
BN_EPS = 1e-5
EINVAL, ELIMIT = 10001, 10002

# name -> (C, F, Hd, J, nP): what each exercises is in the name and in the comment
KERNEL_CASES = {
    "every_minimum": (2, 1, 1, 1, 1),                  # one pooled window, one feature, one hidden unit
    "three_idle_waves": (6, 7, 9, 3, 2),               # 36 cells: partial maxima of -inf and partial sums of 0; F < 32, Hd < 64
    "tiny_one_cell_per_thread": (16, 32, 64, 5, 3),
    "ragged_second_trip": (18, 31, 63, 4, 2),          # 324 cells, 81 windows, F and Hd one under their usual values
    "hd_one_over_a_wave": (50, 32, 65, 2, 2),          # 2500 cells
    "below_the_fast_instance": (62, 32, 64, 2, 1),
    "above_the_fast_instance": (66, 32, 64, 2, 1),
    "fast_instance": (64, 32, 64, 15, 2),              # also run with FVP_SOFTARGMAX_GENERIC (diagnostics builds)
    "c64_but_f16_is_generic": (64, 16, 64, 2, 1),
    "lds_65540_opt_in": (126, 8, 325, 1, 1),           # in front of its 65 536-byte neighbour: the opt-in comes first here
    "lds_65536_no_opt_in": (126, 8, 324, 1, 1),
    "jln128": (128, 32, 64, 2, 1),
    "every_upper_limit": (192, 32, 1024, 1, 1),        # Hd: four trips of the 256-stride loop
    "j32_ragged_hd": (8, 32, 300, 32, 1),
}
# the second ordering of the large-LDS opt-in state: a 128-case first, a small case last
ORDER_325_FIRST = ["lds_65540_opt_in", "lds_65536_no_opt_in"]
ORDER_128_FIRST = ["jln128", "lds_65536_no_opt_in", "lds_65540_opt_in", "three_idle_waves"]
ALONE_CASES = ["three_idle_waves", "ragged_second_trip", "fast_instance"]       # person p alone = person p in the batch
# beta = 1 (a nearly flat softmax) and beta = 1000 with values up to 1.0 (exponentials underflow to 0: the arg-max grid point)
BETA_CASES = {"beta_1": ("ragged_second_trip", 1.0), "beta_1000": ("tiny_one_cell_per_thread", 1000.0)}
FUSE_CASES = [(1, 1), (9, 32), (17, 17)]               # 288 and 289 threads: a ragged second block
PACK_CASES = [(1, 1), (32, 64), (7, 5), (32, 1024)]    # (7, 5): Hd F < 9 F, the launch is sized by the conv weights
ENGINE_GRID_CASES = ("tiny_one_cell_per_thread", "fast_instance", "jln128", "three_idle_waves")


def lds_bytes(Cn, Hd):
    """Dynamic LDS of the generic kernel (fvp_softargmax_weightnet)."""
    return ((Cn * Cn + 1) & ~1) * 4 + 12 * 8 + (5 * 32 + Hd) * 4


assert lds_bytes(126, 324) == 65536 and lds_bytes(126, 325) == 65540


# ---- inputs --------------------------------------------------------------------------------------------------------------
def edge_maps(Cn, rng, n_random=2):
    """The maps of tests/test_softargmax_fast_path.py::_maps scaled to C: flat noise, single bumps, all equal, all zero, a
    peak in each corner and in the middle of each border, the maximum in the last element, negative values, a checkerboard."""
    yy, xx = np.mgrid[0:Cn, 0:Cn]
    e, h = Cn - 1, Cn // 2
    maps = []
    for y, x in ((0, 0), (0, e), (e, 0), (e, e), (0, h), (e, h), (h, 0), (h, e)):
        m = np.zeros((Cn, Cn))
        m[y, x] = 1.0
        maps.append(m)
    m = rng.random((Cn, Cn)) * 0.2
    m[e, e] = 0.5
    maps.append(m)                                                                    # the maximum is the last element
    maps.append(np.full((Cn, Cn), 0.125))
    maps.append(np.zeros((Cn, Cn)))
    maps.append(-rng.random((Cn, Cn)))
    maps.append(((yy + xx) % 2).astype(np.float64) * 0.01 + 1e-3 * rng.random((Cn, Cn)))
    for _ in range(n_random):
        maps.append(rng.random((Cn, Cn)) * 0.2)
        cx, cy = rng.uniform(0, Cn - 1, 2)
        maps.append(0.3 * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / 8.0) + 0.02 * rng.random((Cn, Cn)))
    return np.stack(maps).astype(np.float32)


def fill_maps(Cn, n, rng):
    """n maps: the edge maps in order (as many as fit, starting at a case-dependent one), then scaled noise."""
    e = edge_maps(Cn, rng)
    start = (Cn // 2) % len(e) if n < len(e) else 0
    out = [e[(start + i) % len(e)] for i in range(min(n, len(e)))]
    while len(out) < n:
        out.append((rng.random((Cn, Cn)) * rng.uniform(0.01, 1.0)).astype(np.float32))
    return np.stack(out)


def uniform_grid(Cn, rng):
    return rng.uniform(-1000.0, 1000.0, (3, Cn * Cn, 2)).astype(np.float32)


def engine_grid(Cn, size=(2000.0, 2000.0, 2000.0), centre=(0.0, -500.0, 800.0)):
    """engine.HotPath.center_grid for a C^3 individual space: xy at z0, xz at y0, yz at x0 (checked against the engine's own
    tensor in tests/test_jln_tail_emu.py)."""
    ax = [torch.linspace(-size[a] / 2, size[a] / 2, Cn) + centre[a] for a in range(3)]
    pair = lambda a, b: torch.stack([ax[a].view(Cn, 1).expand(Cn, Cn), ax[b].view(1, Cn).expand(Cn, Cn)], 2).reshape(-1, 2)   # noqa: E731
    return torch.stack([pair(0, 1), pair(0, 2), pair(1, 2)]).numpy().astype(np.float32)


def weightnet_params(F, Hd, rng):
    """Raw WeightNet parameters (fp32), BatchNorm weights of both signs; fc weights scaled by fan-in so the sigmoid stays
    away from saturation at every Hd."""
    f32 = lambda a: np.asarray(a, dtype=np.float32)                                                # noqa: E731
    return dict(conv_w=f32(rng.normal(0, 0.5, (F, 9))), conv_b=f32(rng.normal(0, 0.1, F)),
                gamma=f32(rng.uniform(0.5, 1.5, F) * np.where(np.arange(F) % 2 == 0, 1.0, -1.0)), beta=f32(rng.normal(0, 0.1, F)),
                mean=f32(rng.normal(0, 0.1, F)), var=f32(rng.uniform(0.5, 1.5, F)),
                fc1_w=f32(rng.normal(0, 2.0 / np.sqrt(F), (Hd, F))), fc1_b=f32(rng.normal(0, 0.1, Hd)),
                fc2_w=f32(rng.normal(0, 2.0 / np.sqrt(Hd), Hd)), fc2_b=f32(rng.normal(0, 0.3, 1)))


PARAM_ORDER = ("conv_w", "conv_b", "gamma", "beta", "mean", "var", "fc1_w", "fc1_b", "fc2_w", "fc2_b")


def blob_len(F, Hd):
    """conv_w[F][9] | conv_b[F] | bn_scale[F] | bn_shift[F] | fc1_w[Hd][F] | fc1_b[Hd] | fc2_w[Hd] | fc2_b (fvp_joint.hip)"""
    return 9 * F + 3 * F + Hd * F + 2 * Hd + 1


def pack_ref(p, eps=BN_EPS):
    """k_pack_weightnet in fp32, one rounding per operation: scale = gamma / sqrt(var + eps), shift = beta - mean * scale."""
    f = np.float32
    scale = (p["gamma"] / np.sqrt((p["var"] + f(eps)).astype(f)).astype(f)).astype(f)
    shift = (p["beta"] - (p["mean"] * scale).astype(f)).astype(f)
    blob = np.concatenate([p["conv_w"].ravel(), p["conv_b"], scale, shift, p["fc1_w"].ravel(), p["fc1_b"], p["fc2_w"],
                           p["fc2_b"]]).astype(f)
    assert blob.size == blob_len(p["conv_w"].shape[0], p["fc1_w"].shape[0])
    return blob


# ---- float64 restatement ---------------------------------------------------------------------------------------------------
def ref_softargmax(feat, grid, beta, mut=None):
    """feat [P,3,J,C*C] fp32, grid [3,C*C,2] fp32 -> dict(pose [P,3,J,2], pmax [P,3,J], bound_pose, bound_pmax), float64."""
    x = feat.astype(np.float64)
    CC = x.shape[-1]
    bx = np.float64(np.float32(beta)) * x                           # 24 x 24 bits: exact
    M = bx.max(-1, keepdims=True)
    e = np.exp(bx - M)
    if mut == "last cell left out":
        e[..., -1] = 0.0
    if mut == "last row left out":
        e[..., CC - int(round(CC ** 0.5)):] = 0.0
    p = e / e.sum(-1, keepdims=True)
    g = grid.astype(np.float64)[None, :, None]                      # [1,3,1,CC,2]
    if mut == "plane 1 with the grid of plane 0":
        g = g.copy()
        g[:, 1] = g[:, 0]
    pose = (p[..., None] * g).sum(-2)
    pmax = p.max(-1)
    if mut == "pmax of the neighbouring joint":
        pmax = np.roll(pmax, 1, axis=2)
    d = U * (np.abs(bx) + np.abs(bx - M) + 2.0)
    dbar = (p * d).sum(-1)
    spread = (p[..., None] * np.abs(g - pose[..., None, :]) * (d + dbar[..., None])[..., None]).sum(-2)
    bound_pose = 2.0 * (spread + 4.0 * U * (p[..., None] * np.abs(g)).sum(-2))
    bound_pmax = 2.0 * pmax * (dbar + 2.0 * U)
    return dict(pose=pose, pmax=pmax, bound_pose=bound_pose, bound_pmax=bound_pmax)


def _weightnet_chunk(x, blob, F, Hd, mut):
    M, Cn = x.shape[0], x.shape[-1]
    b = blob.astype(np.float64)
    o = np.cumsum([0, 9 * F, F, F, F, Hd * F, Hd, Hd])
    cw, cb, bs, bh = b[:o[1]].reshape(F, 9), b[o[1]:o[2]], b[o[2]:o[3]], b[o[3]:o[4]]
    w1, b1, w2, b2 = b[o[4]:o[5]].reshape(Hd, F), b[o[5]:o[6]], b[o[6]:o[7]], b[o[7]]
    if mut == "fc1 with row stride Hd":
        idx = o[4] + np.arange(Hd)[:, None] * Hd + np.arange(F)[None, :]
        w1 = np.where(idx < b.size, b[np.minimum(idx, b.size - 1)], 0.0)
    xp = np.pad(x, ((0, 0), (1, 1), (1, 1)), mode="edge" if mut == "edge-replicate padding" else "constant")
    bc = lambda v: v[None, :, None, None]                                                         # noqa: E731
    a = np.zeros((M, F, Cn, Cn))
    mag = np.zeros_like(a)
    for ky in range(3):
        for kx in range(3):
            t = xp[:, None, ky:ky + Cn, kx:kx + Cn] * bc(cw[:, ky * 3 + kx])
            a += t
            mag += np.abs(t)
    err = 9.0 * U * mag                                              # nine fmas from 0
    pool = lambda v: v.reshape(M, F, Cn // 2, 2, Cn // 2, 2).max(axis=(3, 5))                     # noqa: E731
    v = a + bc(cb)
    err = err + U * (np.abs(v) + err)
    if mut == "max-pool before BN":
        v, err = pool(v), pool(err)
    v = v * bc(bs)
    err = np.abs(bc(bs)) * err
    err = err + U * (np.abs(v) + err)
    v = v + bc(bh)
    err = err + U * (np.abs(v) + err)
    if mut == "pooling windows shifted by one cell":
        v = np.roll(v, -1, axis=3)
    if mut != "max-pool before BN":
        v, err = pool(v), pool(err)                                  # |max a - max b| <= max |a - b|
    v = np.maximum(v, 0.0)
    NWIN = (Cn // 2) ** 2
    depth = -(-NWIN // 256) + 8
    s, es = v.sum((2, 3)), err.sum((2, 3))
    es = es + depth * U * (s + es)
    avg = s / (Cn * Cn if mut == "average divided by C^2" else NWIN)
    ea = es / NWIN
    ea = ea + U * (avg + ea)
    if mut == "feature F-1 dropped":
        avg = avg.copy()
        avg[:, F - 1] = 0.0
    h = b1[None] + avg @ w1.T
    eh = ea @ np.abs(w1).T
    eh = eh + F * U * (np.abs(b1)[None] + np.abs(avg) @ np.abs(w1).T + eh)
    h = np.maximum(h, 0.0)
    z = h @ w2 + (0.0 if mut == "b2 omitted" else b2)
    ez = eh @ np.abs(w2)
    ez = ez + (-(-Hd // 64) + 7) * U * (h @ np.abs(w2) + abs(b2) + ez)
    wgt = 1.0 / (1.0 + np.exp(-z))
    return wgt, 0.25 * ez + 6.0 * U * wgt


def ref_weightnet(feat, blob, F, Hd, mut=None):
    """feat [P,3,J,C,C] fp32, blob fp32 -> (wgt [P,3,J], bound_wgt) float64, in chunks of maps."""
    Cn = feat.shape[-1]
    x = feat.astype(np.float64).reshape(-1, Cn, Cn)
    step = max(1, (1 << 22) // (F * Cn * Cn))
    parts = [_weightnet_chunk(x[i:i + step], blob, F, Hd, mut) for i in range(0, len(x), step)]
    return tuple(np.concatenate([q[k] for q in parts]).reshape(feat.shape[:3]) for k in (0, 1))


def ref_fuse(pose2d, pmax, wgt, offset, valid, centers, mut=None):
    """fp32 inputs as k_fuse reads them -> dict(planes fp32 [3,nP,J,2] (exact), fused [nP,J,5] f64, bound [nP,J,5],
    centers [nP,7]).  fused[..., 3] (flag) and every word of an invalid person are exact (bound 0)."""
    f = np.float32
    nP, _, J = pmax.shape
    ok = np.ones(nP, bool) if valid is None else valid.astype(bool)
    ox, oy, oz = (offset[:, k][:, None] for k in range(3))
    second = oy if mut == "oy for the xz plane" else oz
    pl = np.stack([np.stack([pose2d[:, 0, :, 0] + ox, pose2d[:, 0, :, 1] + oy], -1),
                   np.stack([pose2d[:, 1, :, 0] + ox, pose2d[:, 1, :, 1] + second], -1),
                   np.stack([pose2d[:, 2, :, 0] + oy, pose2d[:, 2, :, 1] + oz], -1)]).astype(f)      # one fp32 add each
    assert pl.dtype == f and pose2d.dtype == f and offset.dtype == f
    d, w = pl.astype(np.float64), wgt.astype(np.float64)
    wxy, wxz, wyz = w[:, 0], w[:, 1], w[:, 2]

    def blend(wa, a, wb, b):
        s = wa + wb
        ta, tb = wa / s * a, wb / s * b
        return ta + tb, 6.0 * U * (np.abs(ta) + np.abs(tb))
    x, bx = blend(wxy, d[0, :, :, 0], wxz, d[1, :, :, 0])
    y, by = blend(wxy, d[0, :, :, 1], wyz, d[2, :, :, 0])
    if mut == "xz / yz weights swapped in z":
        z, bz = blend(wyz, d[1, :, :, 1], wxz, d[2, :, :, 1])
    else:
        z, bz = blend(wxz, d[1, :, :, 1], wyz, d[2, :, :, 1])
    conf = pmax.astype(np.float64).sum((1, 2)) / (J if mut == "confidence averaged over J" else 3 * J)
    bconf = (3 * J + 1) * U * pmax.astype(np.float64).mean((1, 2))
    c64 = centers.astype(np.float64)
    flag = np.broadcast_to(c64[:, 3:4], (nP, J))
    fused = np.stack([x, y, z, flag, np.broadcast_to(conf[:, None], (nP, J))], -1)
    bound = np.stack([bx, by, bz, np.zeros_like(bx), np.broadcast_to(bconf[:, None], (nP, J))], -1)
    dead = ~ok
    fused[dead, :, :3] = 0.0
    fused[dead, :, 4] = c64[dead, 4:5]
    bound[dead] = 0.0
    pl[:, dead] = 0.0
    cen = c64.copy()
    cen[ok, 4] = conf[ok]
    return dict(planes=pl, fused=fused, bound=bound, centers=cen, bound_conf=np.where(ok, bconf, 0.0))


def ratio(got, want, bound):
    """max |got - want| / bound; a zero bound demands equality (0 / 0 counts as 0, x / 0 as inf)."""
    err = np.abs(np.asarray(got, np.float64) - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    return float(np.nanmax(np.where(np.isnan(r), np.inf, r))) if r.size else 0.0


# ---- cases ---------------------------------------------------------------------------------------------------------------
def case_data(name, beta=100.0, grid_kind=None):
    """Inputs and the float64 reference of one kernel case, computed once per session and left unchanged.  The maps hold
    values up to 1.0 (the one-hot peaks), so at beta = 1000 the exponent reaches -1000."""
    return _case_data(name, float(beta), grid_kind)


@functools.lru_cache(maxsize=None)
def _case_data(name, beta, grid_kind):
    if name in KERNEL_CASES:
        Cn, F, Hd, J, nP = KERNEL_CASES[name]
        rng = np.random.default_rng(1000 + sorted(KERNEL_CASES).index(name))
    else:                                                           # "mutation C F Hd": every edge map, for the CPU bound test
        Cn, F, Hd = (int(v) for v in name.split()[1:])
        J, nP = 6, 1
        rng = np.random.default_rng(Cn)
    feat = fill_maps(Cn, nP * 3 * J, rng).reshape(nP, 3, J, Cn, Cn)
    kind = grid_kind or ("engine" if name in ENGINE_GRID_CASES else "uniform")
    grid = engine_grid(Cn) if kind == "engine" else uniform_grid(Cn, rng)
    params = weightnet_params(F, Hd, rng)
    blob = pack_ref(params)
    ref = ref_softargmax(feat.reshape(nP, 3, J, Cn * Cn), grid, beta)
    ref["wgt"], ref["bound_wgt"] = ref_weightnet(feat, blob, F, Hd)
    for v in (feat, grid, blob, *ref.values()):
        v.setflags(write=False)
    return dict(name=name, dims=(Cn, F, Hd, J, nP), beta=beta, feat=feat, grid=grid, params=params, blob=blob, ref=ref)


def oracle_ratios(case):
    """error / bound of oracle/fvp_oracle.py's fp32 restatement (torch ops) on the inputs of a case: reported, not asserted."""
    import fvp_oracle as O
    Cn, F, Hd, J, nP = case["dims"]
    x = _t(case["feat"]).permute(1, 0, 2, 3, 4).contiguous()          # reference layout [3,P,J,C,C]
    ref = case["ref"]
    pose, _ = O.soft_argmax(x, _t(case["grid"]).view(3, Cn, Cn, 2), case["beta"])
    pm = torch.softmax(case["beta"] * x.reshape(3, nP, J, -1), dim=3).max(dim=3)[0]
    w = O.weight_net(oracle_state_dict(case["params"]), "wn", x, Cn).view(3, nP, J)
    return dict(pose=ratio(pose.permute(1, 0, 2, 3).numpy(), ref["pose"], ref["bound_pose"]),
                pmax=ratio(pm.permute(1, 0, 2).numpy(), ref["pmax"], ref["bound_pmax"]),
                wgt=ratio(w.permute(1, 0, 2).numpy(), ref["wgt"], ref["bound_wgt"]))


def oracle_state_dict(p, pre="wn"):
    F, Hd = p["conv_w"].shape[0], p["fc1_w"].shape[0]
    t = torch.from_numpy
    return {pre + ".heatmap_feature_net.0.weight": t(p["conv_w"]).view(F, 1, 3, 3), pre + ".heatmap_feature_net.0.bias": t(p["conv_b"]),
            pre + ".heatmap_feature_net.1.weight": t(p["gamma"]), pre + ".heatmap_feature_net.1.bias": t(p["beta"]),
            pre + ".heatmap_feature_net.1.running_mean": t(p["mean"]), pre + ".heatmap_feature_net.1.running_var": t(p["var"]),
            pre + ".output.0.weight": t(p["fc1_w"]), pre + ".output.0.bias": t(p["fc1_b"]),
            pre + ".output.2.weight": t(p["fc2_w"]).view(1, Hd), pre + ".output.2.bias": t(p["fc2_b"])}


# ---- running the kernels ---------------------------------------------------------------------------------------------------
_t = lambda a: torch.from_numpy(np.array(a, copy=True))                                           # noqa: E731
_ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())                                   # noqa: E731


class Guarded:
    """A device buffer of n floats pre-filled with `fill`, between two guard regions of POISON_BITS."""

    def __init__(self, n, dev, fill=SENTINEL, src=None):
        self.flat = torch.full((n + 2 * GUARD,), POISON_BITS, dtype=torch.int32, device=dev).view(torch.float32)
        self.t = self.flat[GUARD:GUARD + n]
        if src is not None:
            self.t.copy_(_t(src).reshape(-1))
        else:
            self.t.fill_(fill)
        self.n = n

    def result(self, what):
        bits = self.flat.view(torch.int32).cpu()
        bad = int((bits[:GUARD] != POISON_BITS).sum()) + int((bits[GUARD + self.n:] != POISON_BITS).sum())
        assert bad == 0, f"{what}: {bad} guard words changed (out-of-bounds write)"
        return self.t.cpu().numpy().copy()


def sync(dev):
    if dev != "cpu":
        torch.cuda.synchronize()


def run_softargmax(lib, dev, case, valid=None, people=None):
    """fvp_softargmax_weightnet on a case (or on the people listed) -> pose [P,3,J,2], pmax [P,3,J], wgt [P,3,J] (numpy);
    outputs start as SENTINEL between poisoned guards."""
    Cn, F, Hd, J, nP = case["dims"]
    feat = case["feat"] if people is None else case["feat"][people]
    nP = feat.shape[0]
    d_feat, d_grid, d_wn = (_t(a).to(dev) for a in (feat, case["grid"], case["blob"]))
    d_valid = None if valid is None else torch.from_numpy(valid.astype(np.uint8)).to(dev)
    outs = [Guarded(nP * 3 * J * k, dev) for k in (2, 1, 1)]
    rc = lib.fvp_softargmax_weightnet(_ptr(d_feat), _ptr(d_grid), _ptr(d_wn), case["beta"], nP, J, Cn, F, Hd, _ptr(d_valid),
                                      *[_ptr(o.t) for o in outs], None)
    assert rc == 0, rc
    sync(dev)
    return [o.result(n).reshape(s) for o, n, s in zip(outs, ("pose2d", "pmax", "wgt"), ((nP, 3, J, 2), (nP, 3, J), (nP, 3, J)))]


def check_softargmax(got, case, valid=None, worst=None):
    """Valid people finite and within the bounds, skipped people still the sentinel.  Returns / updates the worst ratios."""
    ref, nP = case["ref"], case["dims"][4]
    ok = np.ones(nP, bool) if valid is None else valid.astype(bool)
    worst = {} if worst is None else worst
    for a, key, bkey in zip(got, ("pose", "pmax", "wgt"), ("bound_pose", "bound_pmax", "bound_wgt")):
        assert np.isfinite(a[ok]).all(), f"{case['name']}: {key} not finite"
        assert (a[~ok] == np.float32(SENTINEL)).all(), f"{case['name']}: {key} of a skipped person was written"
        r = ratio(a[ok], ref[key][ok], ref[bkey][ok])
        worst[key] = max(worst.get(key, 0.0), r)
        print(f"{case['name']} beta={case['beta']:g} {key}: error / bound = {r:.4f}")
    for key in ("pose", "pmax", "wgt"):
        assert worst[key] <= 1.0, f"{case['name']}: {key} error / bound = {worst[key]:.3f}"
    return worst


def alternate(nP):
    v = np.ones(nP, np.uint8)
    v[1::2] = 0
    return v


def run_and_check_case(lib, dev, name, beta=100.0, masks=True, worst=None):
    case = case_data(name, beta)
    nP = case["dims"][4]
    got = run_softargmax(lib, dev, case)
    worst = check_softargmax(got, case, None, worst)
    if masks and nP > 1:
        v = alternate(nP)
        masked = run_softargmax(lib, dev, case, v)
        check_softargmax(masked, case, v, worst)
        for a, b in zip(masked, got):                               # a person's result does not depend on the mask of others
            assert np.array_equal(a[v.astype(bool)].view(np.int32), b[v.astype(bool)].view(np.int32))
    return got, worst


def check_one_hot_gives_the_grid_point(got, case):
    """beta = 1000: every other exponential of a one-hot map underflows to 0, the result is the arg-max cell's grid point."""
    Cn, F, Hd, J, nP = case["dims"]
    x = case["feat"].reshape(nP, 3, J, -1)
    one_hot = ((x == 1.0).sum(-1) == 1) & ((x == 0.0).sum(-1) == Cn * Cn - 1)
    assert one_hot.sum() >= 8
    point = case["grid"][np.arange(3)[None, :, None], x.argmax(-1)]                 # [P,3,J,2]
    assert (np.abs(got[0].astype(np.float64) - point)[one_hot] <= case["ref"]["bound_pose"][one_hot]).all()
    assert (got[1][one_hot] == 1.0).all()


def check_person_alone(lib, dev, name):
    case = case_data(name)
    batch = run_softargmax(lib, dev, case)
    p = case["dims"][4] - 1
    alone = run_softargmax(lib, dev, case, people=[p])
    for a, b, what in zip(alone, batch, ("pose2d", "pmax", "wgt")):
        assert np.array_equal(a[0].view(np.int32), b[p].view(np.int32)), f"{name}: {what} of person {p} depends on the batch"


# fusion
@functools.lru_cache(maxsize=None)
def fuse_inputs(nP, J):
    rng = np.random.default_rng(nP * 100 + J)
    f = np.float32
    return dict(pose2d=rng.uniform(-1000, 1000, (nP, 3, J, 2)).astype(f), pmax=rng.uniform(1e-4, 1.0, (nP, 3, J)).astype(f),
                wgt=rng.uniform(0.01, 1.0, (nP, 3, J)).astype(f), offset=rng.uniform(-3000, 3000, (nP, 3)).astype(f),
                centers=np.concatenate([rng.uniform(-3000, 3000, (nP, 3)), rng.integers(-1, 2, (nP, 1)).astype(float),
                                        rng.uniform(0, 1, (nP, 3))], 1).astype(f))


def fuse_masks(nP):
    return {"NULL": None, "all invalid": np.zeros(nP, np.uint8), "alternating": alternate(nP)}


def run_fuse(lib, dev, inp, valid):
    nP, _, J = inp["pmax"].shape
    dv = {k: torch.from_numpy(inp[k]).to(dev) for k in ("pose2d", "pmax", "wgt", "offset")}
    d_valid = None if valid is None else torch.from_numpy(valid).to(dev)
    cen = Guarded(nP * 7, dev, src=inp["centers"])                  # a clone: updated in place
    fused, planes = Guarded(nP * J * 5, dev), Guarded(3 * nP * J * 2, dev)
    rc = lib.fvp_fuse_poses(_ptr(dv["pose2d"]), _ptr(dv["pmax"]), _ptr(dv["wgt"]), _ptr(dv["offset"]), _ptr(d_valid), nP, J,
                            _ptr(cen.t), _ptr(fused.t), _ptr(planes.t), None)
    assert rc == 0, rc
    sync(dev)
    return fused.result("fused").reshape(nP, J, 5), planes.result("planes").reshape(3, nP, J, 2), cen.result("centers").reshape(nP, 7)


def check_fuse(lib, dev, nP, J, worst=None):
    inp = fuse_inputs(nP, J)
    worst = {} if worst is None else worst
    for what, valid in fuse_masks(nP).items():
        ref = ref_fuse(inp["pose2d"], inp["pmax"], inp["wgt"], inp["offset"], valid, inp["centers"])
        fused, planes, cen = run_fuse(lib, dev, inp, valid)
        tag = f"fuse ({nP}, {J}) {what}"
        assert np.isfinite(fused).all() and np.isfinite(planes).all(), tag
        assert np.array_equal(planes.view(np.int32), ref["planes"].view(np.int32)), f"{tag}: planes are one fp32 add each"
        rf = ratio(fused[..., :3], ref["fused"][..., :3], ref["bound"][..., :3])
        rc = ratio(fused[..., 4], ref["fused"][..., 4], ref["bound"][..., 4])
        print(f"{tag}: fused error / bound = {rf:.4f}, conf error / bound = {rc:.4f}")
        worst["fused"], worst["conf"] = max(worst.get("fused", 0.0), rf), max(worst.get("conf", 0.0), rc)
        assert rf <= 1.0 and rc <= 1.0, tag
        assert np.array_equal(fused[..., 3], ref["fused"][..., 3].astype(np.float32)), f"{tag}: the flag is copied"
        other = [0, 1, 2, 3, 5, 6]
        assert np.array_equal(cen[:, other].view(np.int32), inp["centers"][:, other].view(np.int32)), f"{tag}: centers outside column 4"
        assert ratio(cen[:, 4], ref["centers"][:, 4], ref["bound_conf"]) <= 1.0, f"{tag}: centers[:, 4]"
        assert np.array_equal(cen[:, 4].view(np.int32), fused[:, 0, 4].view(np.int32)), f"{tag}: centers[:, 4] is the fused confidence"
    return worst


# pack
def run_pack(lib, dev, p, eps=BN_EPS):
    F, Hd = p["conv_w"].shape[0], p["fc1_w"].shape[0]
    dv = [_t(p[k]).to(dev) for k in PARAM_ORDER]
    out = Guarded(blob_len(F, Hd), dev)
    rc = lib.fvp_pack_weightnet(*[_ptr(t) for t in dv[:6]], eps, *[_ptr(t) for t in dv[6:]], F, Hd, _ptr(out.t), None)
    assert rc == 0, rc
    sync(dev)
    return out.result("wn blob")


def check_pack(lib, dev, F, Hd):
    p = weightnet_params(F, Hd, np.random.default_rng(F * 31 + Hd))
    got, want = run_pack(lib, dev, p), pack_ref(p)
    differ = np.flatnonzero(got.view(np.int32) != want.view(np.int32))
    assert differ.size == 0, f"pack ({F}, {Hd}): {differ.size} words differ, first at {differ[0]}: {got[differ[0]]!r} vs {want[differ[0]]!r}"


# argument errors
def check_argument_errors(lib, dev):
    """Every refused call returns the library's code and leaves sentinel-filled outputs untouched."""
    Cn, F, Hd, J, nP = 6, 7, 9, 3, 2
    case = case_data("three_idle_waves")
    d_feat, d_grid, d_wn = (_t(a).to(dev) for a in (case["feat"], case["grid"], case["blob"]))
    outs = [Guarded(nP * 3 * J * k, dev) for k in (2, 1, 1)]

    def call(nP=nP, J=J, Cn=Cn, F=F, Hd=Hd, null=None):
        ptrs = [_ptr(d_feat), _ptr(d_grid), _ptr(d_wn)] + [_ptr(o.t) for o in outs]
        if null is not None:
            ptrs[null] = None
        return lib.fvp_softargmax_weightnet(*ptrs[:3], 100.0, nP, J, Cn, F, Hd, None, *ptrs[3:], None)
    refused = {"C odd": (dict(Cn=7), ELIMIT), "C = 0": (dict(Cn=0), ELIMIT), "C = 194": (dict(Cn=194), ELIMIT),
               "F = 0": (dict(F=0), ELIMIT), "F = 33": (dict(F=33), ELIMIT), "Hd = 0": (dict(Hd=0), ELIMIT),
               "Hd = 1025": (dict(Hd=1025), ELIMIT), "J = 0": (dict(J=0), EINVAL), "nP < 0": (dict(nP=-1), EINVAL)}
    refused.update({f"NULL pointer {i}": (dict(null=i), EINVAL) for i in range(6)})
    for what, (kw, code) in refused.items():
        assert call(**kw) == code, f"fvp_softargmax_weightnet with {what}: {call(**kw)}, expected {code}"
    sync(dev)
    for o in outs:
        assert (o.result("refused call") == np.float32(SENTINEL)).all(), "a refused fvp_softargmax_weightnet wrote its output"
    assert lib.fvp_error_string(EINVAL) and lib.fvp_error_string(ELIMIT)
    # fvp_fuse_poses
    inp = fuse_inputs(9, 32)
    dv = [torch.from_numpy(inp[k]).to(dev) for k in ("pose2d", "pmax", "wgt", "offset")]
    cen, fused, planes = Guarded(9 * 7, dev), Guarded(9 * 32 * 5, dev), Guarded(3 * 9 * 32 * 2, dev)
    for i in range(7):
        ptrs = [_ptr(t) for t in dv] + [_ptr(cen.t), _ptr(fused.t), _ptr(planes.t)]
        ptrs[i] = None
        assert lib.fvp_fuse_poses(*ptrs[:4], None, 9, 32, *ptrs[4:], None) == EINVAL, f"fvp_fuse_poses with NULL pointer {i}"
    full = [_ptr(t) for t in dv] + [_ptr(cen.t), _ptr(fused.t), _ptr(planes.t)]
    assert lib.fvp_fuse_poses(*full[:4], None, -1, 32, *full[4:], None) == EINVAL
    assert lib.fvp_fuse_poses(*full[:4], None, 9, 0, *full[4:], None) == EINVAL
    sync(dev)
    for o in (cen, fused, planes):
        assert (o.result("refused call") == np.float32(SENTINEL)).all(), "a refused fvp_fuse_poses wrote its output"
    # fvp_pack_weightnet
    p = weightnet_params(7, 5, np.random.default_rng(5))
    dp = [_t(p[k]).to(dev) for k in PARAM_ORDER]
    out = Guarded(blob_len(7, 5), dev)
    for i in range(11):
        ptrs = [_ptr(t) for t in dp] + [_ptr(out.t)]
        ptrs[i] = None
        rc = lib.fvp_pack_weightnet(*ptrs[:6], BN_EPS, *ptrs[6:10], 7, 5, ptrs[10], None)
        assert rc == EINVAL, f"fvp_pack_weightnet with NULL pointer {i}: {rc}"
    full = [_ptr(t) for t in dp]
    for F_, Hd_ in ((0, 5), (33, 5), (7, 0)):
        assert lib.fvp_pack_weightnet(*full[:6], BN_EPS, *full[6:], F_, Hd_, _ptr(out.t), None) == ELIMIT, (F_, Hd_)
    sync(dev)
    assert (out.result("refused call") == np.float32(SENTINEL)).all(), "a refused fvp_pack_weightnet wrote its output"


def report(where, worst):
    print(f"worst error / bound on {where}: " + ", ".join(f"{k} {v:.4f}" for k, v in sorted(worst.items())))
