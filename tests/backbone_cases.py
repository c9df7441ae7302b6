"""Per-layer cases of the bf16 Pose-ResNet backbone (fvp_backbone.hip, fvp_backbone_fused.h), shared by the emulator suite
(test_backbone_layers_emu.py) and the GPU suite (test_backbone_layers_gpu.py).  Nothing here touches a GPU at import.

Every op of a plan is run ALONE through ``fvp_bb_run`` on random bf16 activations and compared with the same operation in
float64.  The criterion is derived, not tuned (``check``):

* The reference evaluates the op exactly: bf16 weights and bf16 activations widened to fp64, ``F.conv2d`` /
  ``F.conv_transpose2d`` in fp64, the scale / shift CONSTANTS of ``k_bb_pack_epi`` (fp32 ``gamma / sqrtf(var + eps)`` and
  ``beta + (bias - mean) * scale``, evaluated in fp32 and then widened: the constants are part of the operation), residual.
  That is ``y``, the value before ReLU and before the one rounding to bf16.
* Any fp32 evaluation of the K-term sum in any order (hardware MFMA, the emulator's chain, split over waves), followed by the
  epilogue's few fp32 operations (scale, shift, residual; the fp32 evaluation of the constants themselves), lies within
  ``e = (K + 8) * 2^-24 * mag`` of ``y``, with ``mag = conv(|x|, |w|) * |scale| + |shift| + |res|`` and ``K = taps * cin``.
* bf16 output: ``bf16(y - e) <= got <= bf16(y + e)`` (round to nearest even, straight from fp64; both ends clamped at 0 under
  ReLU).  In addition fewer than ``FLIP_CAP`` = 1 % of the elements may differ from ``bf16(y)``: rounding flips inside the
  interval are legitimate but rare (measured over the passes of the two suites: 0.0036 - 0.0069 % of a pass's elements on the
  emulator, 0.0039 - 0.0050 % on the MI355X; at most 0.13 % of a single op's elements - 5 of 4 096 - on the emulator and
  0.033 % on the MI355X), while truncation or rounding twice gives tens of per cent.  The cap guards a systematic rounding
  error; it is not a budget.
* fp32 output (heatmap layer): ``|got - y| <= e + 2^-23 * |y|``.
* The max-pool is exact.

Fixture sanity (``CANCEL_CAP``): at an element with ``mag * 2^-7 > |y|`` the terms cancel so far that a 1-ulp error of the
output hides inside ``e``.  The share of such elements per op must stay under 50 %.  Measured on the emulator: 4.5 - 7.7 % of a
whole pass's elements (5.0 % for the ResNet-50 pass at 32 x 32), at most 23.3 % of one op's (a transposed conv with 2 048
input channels); on the MI355X 4.9 - 8.0 % of a pass, at most 29.1 % of one op's (3 x 160 x 224).  The fp32 heatmap layer
reaches at most 0.033 of its bound on the emulator (a 32-filter deconv head) and 0.020 on the MI355X.
"""
import ctypes as C

import numpy as np
import torch
import torch.nn.functional as F

import fvp_synthetic as S
from faster_voxelpose_amd import _capi as capi

CFG_SHIFT = 8                  # FVP_BB_CFG_SHIFT: bits 8-9 of FvpBbOp.flags hold the tile configuration (0 = heuristic)
FLIP_CAP = 0.01                # share of elements that may differ from bf16(y) (measured: see the module docstring)
CANCEL_CAP = 0.5               # share of elements with mag * 2^-7 > |y| (measured: see the module docstring)

CONFIGS = {
    "r50": dict(),
    "r18": dict(layers=18),
    "r34": dict(layers=34),
    "r101": dict(layers=101),
    "r50_bias_f256_128_64_j17": dict(deconv_bias=True, deconv_filters=(256, 128, 64), joints=17),
    "r50_two_deconvs": dict(deconv_filters=(256, 256)),
}


# ---- fixture ---------------------------------------------------------------------------------------------------------------
def make_cfg(device, layers=50, deconv_bias=False, deconv_filters=(256, 256, 256), joints=15):
    from faster_voxelpose_amd.core import config as CFG
    cfg = CFG.default_config()
    cfg.DEVICE = str(device)
    cfg.RESNET.NUM_LAYERS = int(layers)
    cfg.RESNET.DECONV_WITH_BIAS = bool(deconv_bias)
    cfg.RESNET.NUM_DECONV_LAYERS = len(deconv_filters)
    cfg.RESNET.NUM_DECONV_FILTERS = [int(f) for f in deconv_filters]
    cfg.RESNET.NUM_DECONV_KERNELS = [4] * len(deconv_filters)
    cfg.DATASET.NUM_JOINTS = int(joints)
    return cfg


def build(lib, device, seed=11, **cfg):
    """``(model, sd)``: a PoseResNet for ``layers`` / ``deconv_bias`` / ``deconv_filters`` / ``joints`` on ``lib`` (None = the
    shipped library) with ``fill_backbone_state_dict`` weights, plus: non-zero random deconv biases (the filler leaves conv
    biases at zero, which would hide a dropped bias), a non-zero ``running_mean`` and a ``running_var`` spread over 0.25 .. 4
    for every BatchNorm, so that scale != 1 and shift != 0 in every layer."""
    from faster_voxelpose_amd.models import resnet as RN
    c = make_cfg(device, **cfg)
    m = RN.PoseResNet(c, _lib=lib) if lib is not None else RN.get(c)
    if torch.device(device).type != "cpu":
        m = m.to(device)
    sd = S.fill_backbone_state_dict(m.state_dict(), seed=seed)
    rng = np.random.default_rng(seed + 1000)
    for k in sorted(sd):
        n = tuple(sd[k].shape)
        if k.endswith(".running_mean"):
            sd[k] = torch.from_numpy((rng.uniform(0.05, 0.3, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32))
        elif k.endswith(".running_var"):
            sd[k] = torch.from_numpy(np.exp(rng.uniform(np.log(0.25), np.log(4.0), n)).astype(np.float32))
        elif k.startswith("deconv_layers.") and k.endswith(".bias") and (k[:-5] + ".running_mean") not in sd and \
                (k[:-5] + ".weight") in sd and sd[k[:-5] + ".weight"].dim() == 4:
            sd[k] = torch.from_numpy((rng.uniform(0.2, 0.6, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32))
    m.load_state_dict(sd)
    # the fixture itself: no layer with scale == 1 or shift == 0, no zero deconv bias
    for o in m._convs:
        if o["kind"] == capi.BB_MAXPOOL:
            continue
        sc, sh = epilogue_constants(sd, o)
        assert bool((sh != 0).all()), o["key"]
        if o.get("bn"):
            assert bool((sc != 1).all()) and bool((sd[o["bn"] + ".running_mean"] != 0).all()), o["key"]
        if o["kind"] == capi.BB_DECONV and cfg.get("deconv_bias"):
            assert bool((sd[o["key"] + ".bias"] != 0).all()), o["key"]
    return m, sd


def epilogue_constants(sd, o):
    """scale, shift as k_bb_pack_epi evaluates them: in fp32."""
    cout = o["cout"]
    b = sd[o["key"] + ".bias"].float() if o.get("bias") else torch.zeros(cout, dtype=torch.float32)
    if o.get("bn"):
        g, beta, mean, var = [sd[o["bn"] + s].float() for s in (".weight", ".bias", ".running_mean", ".running_var")]
        sc = g / torch.sqrt(var + torch.tensor(1e-5, dtype=torch.float32))
        sh = beta + (b - mean) * sc
    else:
        sc, sh = torch.ones(cout, dtype=torch.float32), b
    return sc, sh


def prepare(model, H, W):
    plan = model._plan(H, W)
    model.ensure_packed(plan)
    return plan


class Bufs:
    """Random bf16 activations (rand - 0.5) for every buffer of a plan; channel 3 of the pixel-pair input is zero."""

    def __init__(self, plan, N, device, seed=3):
        g = torch.Generator()
        g.manual_seed(seed)
        self.t = []
        for name in plan["names"]:
            c, h, w = plan["shapes"][name]
            if name == "x":
                v = torch.rand((N, h, w // 2, 2, 4), generator=g) - 0.5
                v[..., 3] = 0
                v = v.reshape(N, h, w // 2, 8)
            else:
                v = torch.rand((N, h, w, c), generator=g) - 0.5
            self.t.append(v.bfloat16().to(device))
        self.arr = (C.c_void_p * len(self.t))(*[t.data_ptr() for t in self.t])
        self.N = N

    def __getitem__(self, i):
        return self.t[i]

    def __len__(self):
        return len(self.t)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def run_op(model, plan, i, bufs, cfg=None, heat_cl=None, heat_nchw=None, nops=1):
    """Ops ``i .. i + nops - 1`` of the plan through one fvp_bb_run call on the current stream.  The destination of every op is
    pre-filled with bf16 NaNs (an element the kernel never writes stays visible), read back, and then restored to its
    random content, so that the buffers serve the next op unchanged.  Returns the destinations' contents (a list, None for
    an op without one).  Nothing is synchronised here."""
    ops = (capi.FvpBbOp * nops)(*[plan["ops"][i + k] for k in range(nops)])
    if cfg:
        ops[0].flags = (ops[0].flags & ~(3 << CFG_SHIFT)) | (int(cfg) << CFG_SHIFT)
    saved = {}
    for k in range(nops):
        d = ops[k].dst
        if d >= 0:
            saved[d] = bufs[d].clone()
            bufs[d].fill_(float("nan"))
    jp = int(heat_cl.shape[-1]) if heat_cl is not None else 0
    rc = model.lib.fvp_bb_run(ops, nops, _ptr(model._wblob), _ptr(model._eblob), bufs.arr, len(bufs), bufs.N,
                              _ptr(heat_cl), jp, _ptr(heat_nchw), model._stream())
    capi.check(model.lib, rc, "fvp_bb_run")
    out = []
    for k in range(nops):
        d = ops[k].dst
        out.append(bufs[d].clone() if d >= 0 else None)
    for d, t in saved.items():
        bufs[d].copy_(t)
    return out


def heat_outputs(model, plan, N, device, cl=True, nchw=True):
    """NaN-filled fp32 heatmap tensors: channels-last [N, oh*ow, JP] and / or NCHW [N, J, oh, ow]."""
    oh, ow = plan["out_hw"]
    J = model.num_joints
    JP = (J + 3) // 4 * 4
    hc = torch.full((N, oh * ow, JP), float("nan"), dtype=torch.float32, device=device) if cl else None
    hn = torch.full((N, J, oh, ow), float("nan"), dtype=torch.float32, device=device) if nchw else None
    return hc, hn


# ---- reference -------------------------------------------------------------------------------------------------------------
def _nchw64(t):
    return t.detach().cpu().double().permute(0, 3, 1, 2).contiguous()


def op_input(o, op, bufs):
    """The op's input as fp64 NCHW (the stem's pixel-pair buffer [N,H,W/2,8] unfolded to [N,3,H,W])."""
    x = bufs[op.src].detach().cpu()
    if o.get("stem"):
        n, h, w2, _ = x.shape
        return x.double().reshape(n, h, w2 * 2, 4)[..., :3].permute(0, 3, 1, 2).contiguous()
    return _nchw64(x)


def reference(model, sd, plan, i, bufs, x=None):
    """Op ``i`` in float64: ``(y, mag, K)`` with ``y`` the exact value before ReLU and before rounding, NHWC."""
    o, op = model._convs[i], plan["ops"][i]
    assert op.kind != capi.BB_MAXPOOL
    x = op_input(o, op, bufs) if x is None else x
    w = sd[o["key"] + ".weight"].bfloat16().double()
    if op.kind == capi.BB_DECONV:
        conv = lambda a, b: F.conv_transpose2d(a, b, None, stride=2, padding=1)     # noqa: E731
        K = 4 * o["cin"]                        # an output pixel gathers 2 x 2 of the 4 x 4 taps
    else:
        conv = lambda a, b: F.conv2d(a, b, None, stride=o["stride"], padding=o["pad"])   # noqa: E731
        K = o["k"] * o["k"] * o["cin"]
    sc, sh = [t.double().view(1, -1, 1, 1) for t in epilogue_constants(sd, o)]
    y = conv(x, w) * sc + sh
    mag = conv(x.abs(), w.abs()) * sc.abs() + sh.abs()
    if op.res >= 0:
        r = _nchw64(bufs[op.res])
        y, mag = y + r, mag + r.abs()
    return y.permute(0, 2, 3, 1).contiguous(), mag.permute(0, 2, 3, 1).contiguous(), K


def bf16_rne(v):
    """fp64 tensor -> the nearest bf16 value (ties to even), as fp64.  The significand is rounded to 8 bits directly
    (frexp / rint / ldexp); going through fp32 would round twice."""
    m, e = np.frexp(v.numpy())
    return torch.from_numpy(np.ldexp(np.rint(m * 256.0) / 256.0, e))


def check(got, y, mag, K, relu, fp32_out, key="", stats=None):
    """The derived criterion of the module docstring.  ``got``: the kernel's output (NHWC; bf16 or fp32), ``y`` / ``mag``:
    ``reference``.  Raises AssertionError with layer key, element index, got, y and e; returns the op's figures."""
    g = got.detach().cpu().double()
    assert g.shape == y.shape, (key, tuple(g.shape), tuple(y.shape))
    e = (K + 8) * 2.0 ** -24 * mag
    if fp32_out:
        assert not relu
        bad = ~((g - y).abs() <= e + 2.0 ** -23 * y.abs())               # a NaN (unwritten) element is bad
        exact = y
    else:
        lo, hi, exact = bf16_rne(y - e), bf16_rne(y + e), bf16_rne(y)
        if relu:
            lo, hi, exact = lo.clamp(min=0), hi.clamp(min=0), exact.clamp(min=0)
        bad = ~((lo <= g) & (g <= hi))
    if bool(bad.any()):
        idx = tuple(int(v) for v in torch.nonzero(bad)[0])
        raise AssertionError(f"{key}: {int(bad.sum())} of {bad.numel()} elements outside the interval; first at {idx}: "
                             f"got {float(g[idx])!r}, y {float(y[idx])!r}, e {float(e[idx])!r}")
    assert bool((g != 0).any()), f"{key}: all-zero output"
    flips = 0 if fp32_out else int((g != exact).sum())
    cancel = float((mag * 2.0 ** -7 > y.abs()).double().mean())
    rel = float(((g - y).abs() / (e + 2.0 ** -23 * y.abs())).max()) if fp32_out else 0.0
    assert flips < FLIP_CAP * g.numel(), f"{key}: {flips} of {g.numel()} elements differ from bf16(y)"
    assert cancel < CANCEL_CAP, f"{key}: {cancel:.3f} of the elements cancel below one bf16 ulp of the summed magnitudes"
    out = dict(key=key, flips=flips, n=g.numel(), cancel=cancel, heat_rel=rel, fp32=fp32_out)
    if stats is not None:
        stats.append(out)
    return out


def check_maxpool(got, src, key="maxpool"):
    x = src.detach().cpu().float().permute(0, 3, 1, 2)
    assert bool((x < 0).any())                                          # the -inf padding matters only with negative inputs
    want = F.max_pool2d(x, 3, 2, 1).permute(0, 2, 3, 1).bfloat16()
    g = got.detach().cpu()
    assert bool((g.float() != 0).any()), key
    assert torch.equal(g.view(torch.int16), want.contiguous().view(torch.int16)), key


def check_heat(model, hc, hn, y, mag, K, key, stats=None):
    """fp32 heatmaps in either layout against ``reference`` (NHWC ``y``); padding channels of the channels-last layout zero,
    its first J channels bit-equal to the NCHW output when both were written."""
    J = model.num_joints
    n, oh, ow, _ = y.shape
    if hn is not None:
        check(hn.detach().cpu().permute(0, 2, 3, 1), y, mag, K, False, True, key + " nchw", stats)
    if hc is not None:
        c = hc.detach().cpu()
        assert bool((c[..., J:] == 0).all()), key + ": padding channels of the channels-last heatmaps"
        check(c[..., :J].reshape(n, oh, ow, J), y, mag, K, False, True, key + " cl", stats)
        if hn is not None:
            assert torch.equal(c[..., :J].reshape(n, oh, ow, J).contiguous().view(torch.int32),
                               hn.detach().cpu().permute(0, 2, 3, 1).contiguous().view(torch.int32)), key + ": cl != nchw"


# ---- passes ----------------------------------------------------------------------------------------------------------------
def tunable(op):
    return op.kind != capi.BB_MAXPOOL and op.dst >= 0 and op.cinp % 64 == 0 and op.coutp % 128 == 0 and \
        not (op.flags & (capi.BB_STEM | capi.BB_OUT_HEAT))


def per_op_pass(model, sd, N, H, W, device, seed=3, all_cfgs=False, only=None):
    """Every op of the plan alone against ``reference`` (``only``: a predicate on (template, op)).  ``all_cfgs``: each
    tunable op with tile configurations 1, 2, 3 (1 only where coutp % 256 == 0), bit-equal to each other, the others
    skipped.  All launches go to the current stream first; one synchronisation, then the comparisons.  Returns the figures."""
    plan = prepare(model, H, W)
    bufs = Bufs(plan, N, device, seed)
    runs = []
    for i, o in enumerate(model._convs):
        op = plan["ops"][i]
        if only is not None and not only(o, op):
            continue
        if all_cfgs:
            if not tunable(op):
                continue
            cfgs = (1, 2, 3) if op.coutp % 256 == 0 else (2, 3)
            runs.append((i, [run_op(model, plan, i, bufs, cfg=c)[0] for c in cfgs], None, None))
        elif op.flags & capi.BB_OUT_HEAT:
            hc, hn = heat_outputs(model, plan, N, device)
            run_op(model, plan, i, bufs, heat_cl=hc, heat_nchw=hn)
            runs.append((i, [], hc, hn))
        else:
            runs.append((i, run_op(model, plan, i, bufs), None, None))
    if torch.device(device).type == "cuda":
        torch.cuda.current_stream(device).synchronize()
    stats = []
    for i, outs, hc, hn in runs:
        o, op = model._convs[i], plan["ops"][i]
        key = o.get("key", "maxpool") + f" [{op.cin}->{op.cout} k{op.kh} s{op.stride} {op.h}x{op.w}]"
        if op.kind == capi.BB_MAXPOOL:
            check_maxpool(outs[0], bufs[op.src], key)
            continue
        y, mag, K = reference(model, sd, plan, i, bufs)
        if op.flags & capi.BB_OUT_HEAT:
            check_heat(model, hc, hn, y, mag, K, key, stats)
            continue
        check(outs[0], y, mag, K, bool(o.get("relu")), False, key, stats)
        for other in outs[1:]:
            assert torch.equal(outs[0].view(torch.int16), other.view(torch.int16)), key + ": tile configurations differ"
    assert runs
    return stats


def summary(stats):
    """Figures of a pass: rounding flips over the bf16 outputs, cancellation share, the fp32 outputs' largest share of their bound."""
    n = sum(s["n"] for s in stats)
    return dict(checks=len(stats), flips=sum(s["flips"] for s in stats), bf16_elements=sum(s["n"] for s in stats if not s["fp32"]),
                worst_flip_share=max((s["flips"] / s["n"] for s in stats), default=0.0),
                cancel_share=sum(s["cancel"] * s["n"] for s in stats) / max(n, 1),
                worst_cancel=max((s["cancel"] for s in stats), default=0.0),
                worst_heat_rel=max((s["heat_rel"] for s in stats), default=0.0))


def op_shape(o, op):
    return (op.kind, op.cin, op.cout, op.kh, op.stride, op.h, op.w, op.res >= 0)


def plan_shapes(model, H, W):
    plan = model._plan(H, W)
    return {op_shape(o, plan["ops"][i]) for i, o in enumerate(model._convs)}


def stage1(model, N, H, W, device, seed=1):
    """The stem, the pooling and layer1 (the ops the fused kernels k_bb_stem_pool / k_bb_bottleneck64 replace) in one
    fvp_bb_run call on an image with negative values; returns layer1's output tensor."""
    plan = prepare(model, H, W)
    nops = 1 + max(i for i, o in enumerate(model._convs) if str(o.get("key", "")).startswith("layer1."))
    last = plan["ops"][nops - 1].dst
    x = (torch.from_numpy(np.random.default_rng(seed).random((N, 3, H, W), dtype=np.float32)) - 0.5).to(device)
    bufs = []
    for name in plan["names"]:
        c, h, w = plan["shapes"][name]
        shape = (N, h, w // 2, c) if name == "x" else (N, h, w, c)
        bufs.append(torch.full(shape, float("nan"), dtype=torch.bfloat16, device=device))
    s = model._stream()
    capi.check(model.lib, model.lib.fvp_bb_input(_ptr(x), _ptr(bufs[0]), N, 3, H, W, s), "fvp_bb_input")
    arr = (C.c_void_p * len(bufs))(*[t.data_ptr() for t in bufs])
    capi.check(model.lib, model.lib.fvp_bb_run(plan["ops"], nops, _ptr(model._wblob), _ptr(model._eblob), arr, len(bufs), N,
                                               None, 0, None, s), "fvp_bb_run")
    return bufs[last].clone()


def stage1_forms(model, N, H, W, device, setenv, log=None):
    """Fused stem + pooling and fused bottlenecks against the separate launches (diagnostics switches), bit-equal.
    ``log``: a callable returning the kernels launched since its last call (emulator), to assert which form ran."""
    names = []
    fused = stage1(model, N, H, W, device)
    names.append(log() if log else None)
    setenv("FVP_BB_NO_FUSE_STEM", "1")
    no_stem = stage1(model, N, H, W, device)
    names.append(log() if log else None)
    setenv("FVP_BB_NO_FUSE_BLOCK", "1")
    plain = stage1(model, N, H, W, device)
    names.append(log() if log else None)
    f = fused.cpu()
    for name, t in (("fused", f), ("fused bottlenecks, separate stem", no_stem.cpu()), ("separate", plain.cpu())):
        assert not bool(t.float().isnan().any()), f"{name}: elements of layer1's output that no kernel wrote (NaN pre-fill)"
    assert float(f.float().abs().max()) > 0
    assert torch.equal(f.view(torch.int16), no_stem.cpu().view(torch.int16)), "stem"
    assert torch.equal(f.view(torch.int16), plain.cpu().view(torch.int16)), "bottleneck"
    if log:
        has = lambda txt, k: any(k in line for line in txt)                 # noqa: E731
        assert has(names[0], "k_bb_stem_pool") and has(names[0], "k_bb_bottleneck64"), names[0]
        assert not has(names[1], "k_bb_stem_pool") and has(names[1], "k_bb_bottleneck64"), names[1]
        assert not has(names[2], "k_bb_stem_pool") and not has(names[2], "k_bb_bottleneck64"), names[2]


def heat_matrix(model, sd, N, H, W, device, setenv, delenv, log=None, seed=5):
    """The last transposed conv and the heatmap layer run together, fused (where eligible) and as two launches
    (FVP_BB_NO_FUSE_FINAL), with heat_cl only, heat_nchw only and both.  The separate run's bf16 deconv output is the
    intermediate (the fused form rounds the same values in registers); both forms are held to the fp32 bound against the
    fp64 1 x 1 conv of it.  Returns the figures."""
    plan = prepare(model, H, W)
    bufs = Bufs(plan, N, device, seed)
    i = len(model._convs) - 2
    od, of_ = plan["ops"][i], plan["ops"][i + 1]
    assert od.kind == capi.BB_DECONV and (of_.flags & capi.BB_OUT_HEAT)
    eligible = of_.cout <= 32 and of_.cinp == 256 and od.coutp == 256
    before = bufs[od.dst].clone()
    stats, ref = [], None
    for cl, nchw in ((True, False), (False, True), (True, True)):
        setenv("FVP_BB_NO_FUSE_FINAL", "1")
        hc_s, hn_s = heat_outputs(model, plan, N, device, cl, nchw)
        if log:
            log()
        mid = run_op(model, plan, i, bufs, heat_cl=hc_s, heat_nchw=hn_s, nops=2)[0]
        n_sep = len(log()) if log else 2
        delenv("FVP_BB_NO_FUSE_FINAL")
        hc_f, hn_f = heat_outputs(model, plan, N, device, cl, nchw)
        ops = (capi.FvpBbOp * 2)(od, of_)                    # not through run_op: the deconv's destination keeps its content
        rc = model.lib.fvp_bb_run(ops, 2, _ptr(model._wblob), _ptr(model._eblob), bufs.arr, len(bufs), N, _ptr(hc_f),
                                  int(hc_f.shape[-1]) if cl else 0, _ptr(hn_f), model._stream())
        capi.check(model.lib, rc, "fvp_bb_run")
        n_fused = len(log()) if log else (1 if eligible else 2)
        after = bufs[od.dst].clone()
        if torch.device(device).type == "cuda":
            torch.cuda.current_stream(device).synchronize()
        assert n_sep == 2 and n_fused == (1 if eligible else 2), (n_sep, n_fused)
        if eligible:       # the fused form's contract: the deconv's output tensor is never written
            assert torch.equal(after.cpu().view(torch.int16), before.cpu().view(torch.int16)), "fused form wrote the deconv output"
        else:
            assert torch.equal(after.cpu().view(torch.int16), mid.cpu().view(torch.int16))
            bufs[od.dst].copy_(before)
        assert not bool(mid.float().isnan().any())
        if ref is None:     # the intermediate does not depend on which heatmap layouts were asked for
            ref = (mid.cpu(), reference(model, sd, plan, i + 1, bufs, x=_nchw64(mid)))
        assert torch.equal(mid.cpu().view(torch.int16), ref[0].view(torch.int16))
        y, mag, K = ref[1]
        tag = f"J={model.num_joints} cl={int(cl)} nchw={int(nchw)}"
        check_heat(model, hc_s, hn_s, y, mag, K, "separate " + tag, stats)
        check_heat(model, hc_f, hn_f, y, mag, K, "fused " + tag, stats)
    return stats


def whole_network(model, sd, x, layers, ndeconv, one_pass=False):
    """m(x) against the oracle's bf16-emulating evaluation with the suite's whole-network criterion; NCHW and channels-last
    outputs identical.  ``one_pass``: both layouts from one run (the emulator is slow) instead of forward +
    forward_channels_last."""
    import fvp_oracle as O
    with torch.no_grad():
        if one_pass:
            y, cl = model._run(x.to(model._device()), True, True)
        else:
            y = model(x.to(model._device()))
            cl = model.forward_channels_last(x.to(model._device()))
    y, cl = y.cpu(), cl.cpu()
    o32 = O.pose_resnet(sd, x, num_layers=layers, num_deconv=ndeconv)
    o16 = O.pose_resnet(sd, x, num_layers=layers, num_deconv=ndeconv, bf16=True)
    e_prod = float((y - o32).norm() / o32.norm())
    e_orc = float((o16 - o32).norm() / o32.norm())
    print(f"whole network: e_prod {e_prod:.5f} e_orc {e_orc:.5f}")
    assert e_prod < 1.5 * e_orc + 1e-3, (e_prod, e_orc)
    J = model.num_joints
    assert y.shape[1] == J and torch.equal(cl[..., :J], y.reshape(y.shape[0], J, -1).permute(0, 2, 1)) and not cl[..., J:].any()
    return e_prod, e_orc
