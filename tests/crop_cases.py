"""Cases and the yardsticks of fvp_person_rois, fvp_crop_rois and fvp_crop_rois_nv12 (include/fvp.h, ABI 16), shared by
tests/test_crop_emu.py (CPU emulator) and tests/test_crop_gpu.py (the shipped library on the card): an independent numpy
restatement of both definitions - fp32 emulated operation by operation with numpy float32 scalars and arrays, which round
every result to float32 - the NV12 source pixel in int64, seeded frames and pitched surfaces whose padding is random, the
wrong readings of the definitions (mutants) the case set must tell apart, and runners that call the entry points on torch
memory (CPU for the emulator, the card otherwise).  Everything is compared bit for bit: no tolerance anywhere."""
import ctypes as C

import numpy as np
import torch

from ingest_cases import pack_nhwc8

f32 = np.float32
NAN, INF = float("nan"), float("inf")
IMAGENET = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
OTHER_NORM = ((0.5, 0.25, 0.125), (0.25, 0.5, 2.0))
EINVAL, ELIMIT = 10001, 10002
MAX_JOINTS, MAX_VIEWS = 32, 8


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _dev(a, device):
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a).copy())
    return t if str(device) == "cpu" else t.to(device)


def _ptr(t, off=0):
    return None if t is None else C.c_void_p(t.data_ptr() + off)


def _stream(device):
    return C.c_void_p(torch.cuda.current_stream().cuda_stream) if str(device).startswith("cuda") else None


def _sync(device):
    if str(device).startswith("cuda"):
        torch.cuda.synchronize()


def _fa(v):
    v = [float(x) for x in v]
    return (C.c_float * len(v))(*v)


# ======================================================================================================================
# fvp_person_rois
# ======================================================================================================================
ROI_MUTANTS = ("minmax_all", "aspect_reversed")
B, V, N = 2, 2, 3


def roi_reference(case, mutant=None):
    """(rois [B,V,N,4] f32, count [B,V,N] i32, score [B,V,N] f32, branches taken) by the definition in include/fvp.h."""
    views, ids, conf = case["views"], case["ids"], case["conf"]
    nb, nv, nn, J, _ = views.shape
    scale, pad, aspect, conf_min = f32(case["scale"]), f32(case["pad_px"]), f32(case["aspect"]), f32(case["conf_min"])
    rois = np.zeros((nb, nv, nn, 4), f32)
    count = np.zeros((nb, nv, nn), np.int32)
    score = np.zeros((nb, nv, nn), f32)
    branches = set()
    with np.errstate(invalid="ignore"):
        for b in range(nb):
            for v in range(nv):
                for n in range(nn):
                    if ids is not None and not ids[b, n] >= 0:
                        continue
                    xs, ys, k, tot = [], [], 0, f32(0)
                    for j in range(J):
                        if not (case["mask"] >> j) & 1:
                            continue
                        px, py, depth, s = (f32(t) for t in views[b, v, n, j])
                        ok = bool(depth > 0) and bool(abs(px) <= f32(32768)) and bool(abs(py) <= f32(32768))
                        if conf is not None:
                            ok = ok and bool(conf[b, n, j] >= conf_min)
                        if ok:
                            k += 1
                            tot = f32(tot + s)
                        if ok or (mutant == "minmax_all" and not (np.isnan(px) or np.isnan(py))):
                            xs.append(px)
                            ys.append(py)
                    if k < case["min_joints"]:
                        continue
                    xmin, xmax, ymin, ymax = min(xs), max(xs), min(ys), max(ys)
                    cx, cy = f32(f32(xmin + xmax) * f32(0.5)), f32(f32(ymin + ymax) * f32(0.5))
                    hw = f32(f32(f32(f32(xmax - xmin) * f32(0.5)) * scale) + pad)
                    hh = f32(f32(f32(f32(ymax - ymin) * f32(0.5)) * scale) + pad)
                    widen = bool(hw < f32(hh * aspect))
                    branches.add(widen)
                    if widen != (mutant == "aspect_reversed"):
                        hw = f32(hh * aspect)
                    else:
                        hh = f32(hw / aspect)
                    rois[b, v, n] = (f32(cx - hw), f32(cy - hh), f32(cx + hw), f32(cy + hh))
                    count[b, v, n] = k
                    score[b, v, n] = f32(tot / f32(k))
    return rois, count, score, branches


def _base_views(J, seed):
    rng = np.random.default_rng([seed, J])
    v = np.empty((B, V, N, J, 4), f32)
    v[..., 0] = rng.uniform(-20.0, 200.0, v.shape[:-1])
    v[..., 1] = rng.uniform(-30.0, 120.0, v.shape[:-1])
    v[..., 2] = rng.uniform(1.0, 5.0, v.shape[:-1])
    v[..., 3] = rng.uniform(0.0, 1.0, v.shape[:-1])
    return v


def _roi(J, seed, **kw):
    c = dict(views=_base_views(J, seed), ids=None, conf=None, mask=(1 << J) - 1, min_joints=2, scale=1.25, pad_px=0.0,
             aspect=0.75, conf_min=0.0)
    c.update(kw)
    return c


def _roi_all_usable(J):
    return _roi(J, 1, pad_px=6.5, scale=1.0)


def _roi_behind_camera(J):
    c = _roi(J, 2)
    c["views"][0, 0, 0, 1, :3] = (5000.0, -4000.0, -1.0)         # behind the camera, far from the others
    c["views"][1, 1, 2, 0, :3] = (-3000.0, 2500.0, 0.0)          # depth 0 is not > 0
    return c


def _roi_nan_pixel(J):
    c = _roi(J, 3)
    c["views"][0, 1, 1, 2, 0] = NAN
    c["views"][0, 1, 2, 3, 1] = INF
    c["views"][1, 0, 0, 4, 0] = 40000.0                          # |px| > 32768
    c["views"][1, 0, 1, 0, 1] = -32768.0                         # exactly on the bound: usable
    c["views"][1, 1, 1, 1, 2] = NAN
    return c


def _roi_conf(J, on):
    c = _roi(J, 4, conf_min=0.5)
    rng = np.random.default_rng([44, J])
    conf = rng.uniform(0.0, 1.0, (B, N, J)).astype(f32)
    conf[0, 0, 0] = 0.5                                          # exactly conf_min: usable
    conf[0, 1, 1] = NAN
    c["conf"] = conf if on else None
    return c


def _roi_ids(J):
    return _roi(J, 5, ids=np.array([[3, -1, 7], [-1, 0, 2]], np.int32))


def _roi_mask_two(J):
    return _roi(J, 6, mask=(1 << 1) | (1 << 3))


def _roi_mask_none(J):
    return _roi(J, 7, mask=0)


def _roi_k_at_min(J):
    c = _roi(J, 8, min_joints=3)
    c["views"][0, 0, 0, 3:, 2] = 0.0                             # k == 3 == min_joints: valid
    c["views"][0, 0, 1, 2:, 2] = 0.0                             # k == 2 == min_joints - 1: invalid
    return c


def _roi_single_joint(J):
    c = _roi(J, 9, min_joints=1, pad_px=0.0)
    c["views"][:, :, 0, 1:, 2] = -2.0                            # person 0: joint 0 alone -> x1 == x0, y1 == y0
    return c


def _roi_tall_and_wide(J):
    c = _roi(J, 10)
    rng = np.random.default_rng([10, J])
    shape = (B, V, J)
    c["views"][:, :, 0, :, 0] = rng.uniform(100.0, 110.0, shape)  # tall: widened to the aspect
    c["views"][:, :, 0, :, 1] = rng.uniform(0.0, 200.0, shape)
    c["views"][:, :, 1, :, 0] = rng.uniform(0.0, 300.0, shape)    # wide: heightened
    c["views"][:, :, 1, :, 1] = rng.uniform(50.0, 60.0, shape)
    return c


ROI_BUILDERS = {
    "all_usable": _roi_all_usable, "behind_camera": _roi_behind_camera, "nan_pixel": _roi_nan_pixel,
    "conf_on": lambda J: _roi_conf(J, True), "conf_off": lambda J: _roi_conf(J, False), "ids_minus1": _roi_ids,
    "mask_two": _roi_mask_two, "mask_none": _roi_mask_none, "k_at_min": _roi_k_at_min, "single_joint": _roi_single_joint,
    "tall_and_wide": _roi_tall_and_wide,
}
ROI_CASES = [(name, J) for name in ROI_BUILDERS for J in (5, 17)]
_roi_cache = {}


def roi_case(name, J):
    """(case, (rois, count, score, branches)) - computed once, shared, never modified."""
    if (name, J) not in _roi_cache:
        case = ROI_BUILDERS[name](J)
        _roi_cache[name, J] = (case, roi_reference(case))
    return _roi_cache[name, J]


def roi_call(lib, device, case, outs=(True, True, True), **over):
    """fvp_person_rois on ``device``; returns (rc, [rois, count, score] as numpy or None).  Outputs start poisoned."""
    a = dict(case)
    a.update(over)
    views = _dev(a["views"], device)
    nb, nv, nn, J = a.get("B", views.shape[0]), a.get("V", views.shape[1]), a.get("N", views.shape[2]), a.get("J", views.shape[3])
    ids, conf = _dev(a["ids"], device), _dev(a["conf"], device)
    shp = a["views"].shape[:3]
    o = [_dev(np.full(shp + (4,), NAN, f32), device) if outs[0] else None,
         _dev(np.full(shp, -77, np.int32), device) if outs[1] else None,
         _dev(np.full(shp, NAN, f32), device) if outs[2] else None]
    rc = lib.fvp_person_rois(None if a.get("null_views") else _ptr(views), _ptr(ids), _ptr(conf), nb, nv, nn, J, a["mask"],
                             a["min_joints"], a["scale"], a["pad_px"], a["aspect"], a["conf_min"], _ptr(o[0]), _ptr(o[1]),
                             _ptr(o[2]), _stream(device))
    _sync(device)
    return rc, [None if t is None else t.cpu().numpy() for t in o]


def roi_check(lib, device, name, J):
    case, (rois, count, score, _) = roi_case(name, J)
    rc, (r, c, s) = roi_call(lib, device, case)
    assert rc == 0, rc
    assert np.array_equal(c, count), (name, J)
    assert np.array_equal(bits(r), bits(rois)), (name, J, r, rois)
    assert np.array_equal(bits(s), bits(score)), (name, J)


def roi_check_null_outputs(lib, device):
    """Each output may be NULL, not all three; the others keep their bits."""
    case, (rois, count, score, _) = roi_case("conf_on", 17)
    for outs in ((True, False, False), (False, True, False), (False, False, True), (True, False, True)):
        rc, (r, c, s) = roi_call(lib, device, case, outs=outs)
        assert rc == 0
        assert r is None or np.array_equal(bits(r), bits(rois))
        assert c is None or np.array_equal(c, count)
        assert s is None or np.array_equal(bits(s), bits(score))
    assert roi_call(lib, device, case, outs=(False, False, False))[0] == EINVAL


def roi_argument_errors(lib, device):
    case, _ = roi_case("all_usable", 5)
    bad = [dict(null_views=True), dict(B=-1), dict(V=-1), dict(N=0), dict(J=0), dict(min_joints=0), dict(scale=0.0),
           dict(scale=-1.0), dict(scale=NAN), dict(scale=INF), dict(pad_px=-0.5), dict(pad_px=NAN), dict(pad_px=INF),
           dict(aspect=0.0), dict(aspect=NAN), dict(aspect=INF), dict(conf_min=NAN)]
    for over in bad:
        rc, (r, c, s) = roi_call(lib, device, case, **over)
        assert rc == EINVAL, (over, rc)
        assert np.isnan(r).all() and (c == -77).all() and np.isnan(s).all(), over         # nothing written
    for over in (dict(N=33), dict(J=MAX_JOINTS + 1), dict(V=MAX_VIEWS + 1)):
        rc, (r, c, s) = roi_call(lib, device, case, **over)
        assert rc == ELIMIT, (over, rc)
        assert np.isnan(r).all() and (c == -77).all() and np.isnan(s).all(), over
    for over in (dict(B=0), dict(V=0)):                                                 # no launch: nothing written
        rc, (r, c, s) = roi_call(lib, device, case, **over)
        assert rc == 0 and np.isnan(r).all() and (c == -77).all() and np.isnan(s).all(), over


# ======================================================================================================================
# fvp_crop_rois / fvp_crop_rois_nv12
# ======================================================================================================================
CROP_MUTANTS = ("no_half", "wh_swapped", "clip", "frame_index")
# standard -> (yoff, CY, CRV, CGU, CGV, CBU): the table of include/fvp.h
YUV = {0: (16, 1220945, 1673555, -410793, -852458, 2115221), 1: (16, 1220945, 1879825, -223607, -558796, 2215014),
       2: (0, 1048576, 1470104, -360853, -748826, 1858077), 3: (0, 1048576, 1651297, -196424, -490864, 1945738)}


def roi_list(hs, ws):
    """The boxes every crop case cuts, for a frame of hs x ws: (name, (x0, y0, x1, y1))."""
    return [
        ("inside_up", (10.3, 5.2, 14.9, 9.7)),                   # a few source pixels over the whole patch
        ("inside_down", (2.0, 1.0, 37.5, 22.0)),                 # most of the frame into the patch
        ("over_left", (-6.5, 4.0, 9.0, 15.0)),
        ("over_right", (30.0, 3.0, 47.25, 20.0)),
        ("over_top", (5.0, -7.3, 25.0, 8.0)),
        ("over_bottom", (8.0, 15.0, 30.0, hs + 6.5)),
        ("over_all", (-3.0, -2.0, ws + 4.0, hs + 1.5)),
        ("outside_right", (ws + 10.0, 3.0, ws + 20.0, 14.0)),
        ("outside_above", (4.0, -40.0, 20.0, -21.0)),
        ("outside_far", (1.0e6, -1.0e6, 1.0001e6, -0.9999e6)),
        ("x1_eq_x0", (5.0, 5.0, 5.0, 9.0)),
        ("x1_lt_x0", (9.0, 5.0, 5.0, 9.0)),
        ("y1_eq_y0", (5.0, 7.0, 9.0, 7.0)),
        ("nan", (NAN, 1.0, 5.0, 9.0)),
        ("nan_y1", (1.0, 1.0, 5.0, NAN)),
        ("inf", (1.0, 1.0, INF, 9.0)),
        ("minus_inf", (1.0, -INF, 5.0, 9.0)),
        ("zeros", (0.0, 0.0, 0.0, 0.0)),                         # an invalid box of fvp_person_rois
    ]


def _crop(kind, hs, ws, size, rpf, seed, swap=False, norm=IMAGENET, standard=0, y_pitch=None, uv_pitch=None, split=False,
          gap=0, rois=None):
    boxes = [b for _, b in roi_list(hs, ws)] if rois is None else list(rois)
    while len(boxes) % rpf:
        boxes.append((3.5, 2.25, 21.0, 19.5))
    c = dict(kind=kind, hs=hs, ws=ws, h=size[0], w=size[1], rpf=rpf, F=len(boxes) // rpf, rois=np.array(boxes, f32),
             swap=swap, mean=norm[0], std=norm[1], standard=standard, seed=seed)
    rng = np.random.default_rng([seed, hs, ws])
    F = c["F"]
    if kind == "rgb":
        fr = rng.integers(0, 256, size=(F, hs, ws, 3), dtype=np.uint8)
        fr.reshape(-1)[:2] = (0, 255)
        c["bufs"] = [fr.reshape(-1)]
        return c
    c["y_pitch"], c["uv_pitch"] = y_pitch or ws, uv_pitch or ws
    ylen, uvlen = hs * c["y_pitch"], (hs // 2) * c["uv_pitch"]
    if split:                                                  # planes in allocations of their own
        c["y_fs"], c["uv_fs"] = ylen + gap + 1, uvlen + gap     # an odd luma frame stride
        c["bufs"] = [rng.integers(1, 256, size=F * c["y_fs"], dtype=np.uint8), rng.integers(1, 256, size=F * c["uv_fs"], dtype=np.uint8)]
        c["y"], c["uv"] = (0, 0), (1, 0)                        # (buffer, byte offset)
    else:                                                      # the decoder's contiguous buffer: uv = y + hs * pitch
        assert c["y_pitch"] == c["uv_pitch"] and gap % 2 == 0
        c["y_fs"] = c["uv_fs"] = ylen + uvlen + gap
        c["bufs"] = [rng.integers(1, 256, size=F * c["y_fs"], dtype=np.uint8)]
        c["y"], c["uv"] = (0, 0), (0, ylen)
    y, uv = nv12_planes(c, c["bufs"])
    y[...] = rng.integers(0, 256, size=y.shape, dtype=np.uint8)
    uv[...] = rng.integers(0, 256, size=uv.shape, dtype=np.uint8)
    ey, eu = rng.random(y.shape), rng.random(uv.shape[:-1])
    y[ey < 1 / 16], y[ey > 15 / 16] = 0, 255                     # extremes all over: the conversion clips
    uv[eu < 1 / 16], uv[eu > 15 / 16] = (0, 0), (255, 255)
    return c


def nv12_planes(c, bufs):
    """Strided numpy views [F,hs,ws] and [F,hs/2,ws/2,2] of the allocations (writable)."""
    st = np.lib.stride_tricks.as_strided
    y = st(bufs[c["y"][0]][c["y"][1]:], (c["F"], c["hs"], c["ws"]), (c["y_fs"], c["y_pitch"], 1))
    uv = st(bufs[c["uv"][0]][c["uv"][1]:], (c["F"], c["hs"] // 2, c["ws"] // 2, 2), (c["uv_fs"], c["uv_pitch"], 2, 1))
    return y, uv


def nv12_padding(c):
    """Per buffer, the [begin, end) byte ranges that belong to no pixel: pitch padding, frame gaps, both ends."""
    used = [np.zeros(len(b), bool) for b in c["bufs"]]
    for f in range(c["F"]):
        for r in range(c["hs"]):
            a = c["y"][1] + f * c["y_fs"] + r * c["y_pitch"]
            used[c["y"][0]][a:a + c["ws"]] = True
        for r in range(c["hs"] // 2):
            a = c["uv"][1] + f * c["uv_fs"] + r * c["uv_pitch"]
            used[c["uv"][0]][a:a + c["ws"]] = True
    out = []
    for u in used:
        edges = np.flatnonzero(np.diff(np.concatenate([[True], u, [True]]).astype(np.int8)))
        out.append([(int(a), int(e)) for a, e in zip(edges[::2], edges[1::2])])
    return out


def source_rgb(c):
    """The frames as [F,hs,ws,3] uint8 in SOURCE channel order; an NV12 pixel through the integer formula of include/fvp.h."""
    if c["kind"] == "rgb":
        return c["bufs"][0].reshape(c["F"], c["hs"], c["ws"], 3)
    y, uv = nv12_planes(c, c["bufs"])
    yoff, cy, crv, cgu, cgv, cbu = YUV[c["standard"]]
    yi, xi = np.arange(c["hs"])[:, None] >> 1, np.arange(c["ws"])[None, :] >> 1
    lum = np.maximum(0, y.astype(np.int64) - yoff)
    d, e = uv[:, yi, xi, 0].astype(np.int64) - 128, uv[:, yi, xi, 1].astype(np.int64) - 128
    half = 1 << 19
    rgb = np.stack([(cy * lum + crv * e + half) >> 20, (cy * lum + cgu * d + cgv * e + half) >> 20,
                    (cy * lum + cbu * d + half) >> 20], axis=-1)
    return np.clip(rgb, 0, 255).astype(np.uint8)


def croppable(roi):
    x0, y0, x1, y1 = (f32(t) for t in roi)
    with np.errstate(invalid="ignore"):
        return bool(np.all(np.abs(np.array([x0, y0, x1, y1], f32)) <= np.finfo(f32).max)) and bool(x1 > x0) and bool(y1 > y0)


def crop_matrix(roi, h, w, mutant=None, hs=None, ws=None):
    """inv[6] of a croppable ROI, fp32, operation by operation."""
    x0, y0, x1, y1 = (f32(t) for t in roi)
    if mutant == "clip":
        x0, y0, x1, y1 = max(x0, f32(0)), max(y0, f32(0)), min(x1, f32(ws)), min(y1, f32(hs))
    dw, dh = (f32(h), f32(w)) if mutant == "wh_swapped" else (f32(w), f32(h))
    ax, ay = f32(f32(x1 - x0) / dw), f32(f32(y1 - y0) / dh)
    if mutant == "no_half":
        return np.array([ax, 0, x0, 0, ay, y0], f32)
    bx = f32(f32(x0 + f32(f32(0.5) * ax)) - f32(0.5))
    by = f32(f32(y0 + f32(f32(0.5) * ay)) - f32(0.5))
    return np.array([ax, 0, bx, 0, ay, by], f32)


def warp_f32(frame, inv, h, w, swap, mean, std):
    """One frame [hs,ws,3] uint8 through the ingest arithmetic of include/fvp.h -> ([3,h,w] f32, taps inside the frame)."""
    hs, ws = frame.shape[:2]
    mean, std = np.asarray(mean, f32), np.asarray(std, f32)
    x, y = np.arange(w, dtype=f32)[None, :], np.arange(h, dtype=f32)[:, None]
    sx = ((inv[0] * x) + (inv[1] * y)) + inv[2]
    sy = ((inv[3] * x) + (inv[4] * y)) + inv[5]
    assert sx.dtype == f32 and sx.shape == (h, w) and sy.shape == (h, w)
    flx, fly = np.floor(sx), np.floor(sy)
    fx, fy = sx - flx, sy - fly
    gx, gy = f32(1) - fx, f32(1) - fy
    ix, iy = np.clip(flx, -2, ws).astype(np.int64), np.clip(fly, -2, hs).astype(np.int64)
    taps, vals = 0, []
    for dy in (0, 1):
        for dx in (0, 1):
            yy, xx = iy + dy, ix + dx
            ok = (yy >= 0) & (yy < hs) & (xx >= 0) & (xx < ws)
            taps += int(ok.sum())
            px = frame[np.clip(yy, 0, hs - 1), np.clip(xx, 0, ws - 1)]          # [h,w,3]
            vals.append(np.where(ok[..., None], px, 0).astype(f32))
    out = np.empty((3, h, w), f32)
    for c in range(3):
        sc = 2 - c if swap else c
        p00, p01, p10, p11 = (t[..., sc] for t in vals)
        v = (gy * ((gx * p00) + (fx * p01))) + (fy * ((gx * p10) + (fx * p11)))
        o = ((v / f32(255)) - mean[c]) / std[c]
        assert o.dtype == f32
        out[c] = o
    return out, taps


def crop_reference(c, mutant=None):
    """(nchw [R,3,h,w] f32, number of in-frame taps) of a case by the definition."""
    src = source_rgb(c)
    R = len(c["rois"])
    out = np.zeros((R, 3, c["h"], c["w"]), f32)
    taps = 0
    for r in range(R):
        if not croppable(c["rois"][r]):
            continue
        f = r % c["F"] if mutant == "frame_index" else r // c["rpf"]
        inv = crop_matrix(c["rois"][r], c["h"], c["w"], mutant, c["hs"], c["ws"])
        out[r], t = warp_f32(src[f], inv, c["h"], c["w"], c["swap"], c["mean"], c["std"])
        taps += t
    return out, taps


CROP_BUILDERS = {
    "rgb_6x4": lambda: _crop("rgb", 24, 40, (6, 4), 1, 11),
    "rgb_8x8_per3_swap": lambda: _crop("rgb", 24, 40, (8, 8), 3, 12, swap=True),
    "rgb_5x2_per3_norm": lambda: _crop("rgb", 24, 40, (5, 2), 3, 13, norm=OTHER_NORM),
    # the whole frame at the frame's own size: the identity ingest; 480 pixel pairs = one full block and a part of a second
    "rgb_identity": lambda: _crop("rgb", 24, 40, (24, 40), 1, 14, swap=True, rois=[(0.0, 0.0, 40.0, 24.0)] * 2),
    "nv12_601l_6x4": lambda: _crop("nv12", 26, 40, (6, 4), 1, 21, standard=0, y_pitch=48, uv_pitch=48, gap=6),
    # planes in separate allocations, an odd luma pitch, another chroma pitch, frames further apart than a plane is long
    "nv12_709l_8x8_per3_planes": lambda: _crop("nv12", 26, 40, (8, 8), 3, 22, standard=1, y_pitch=47, uv_pitch=48, split=True, gap=38),
    "nv12_601f_5x2_per3": lambda: _crop("nv12", 26, 40, (5, 2), 3, 23, standard=2, norm=OTHER_NORM),
    "nv12_709f_identity_planes": lambda: _crop("nv12", 26, 40, (26, 40), 1, 24, standard=3, y_pitch=45, uv_pitch=44, split=True,
                                              rois=[(0.0, 0.0, 40.0, 26.0)] * 2),
    # nothing to load: every box is non-croppable or wholly outside the frame
    "rgb_nothing": lambda: _crop("rgb", 24, 40, (6, 4), 1, 15, rois=[b for n, b in roi_list(24, 40) if not croppable(b) or n.startswith("outside")]),
    "nv12_nothing": lambda: _crop("nv12", 26, 40, (6, 4), 1, 25, standard=1, y_pitch=47, uv_pitch=48, split=True, gap=10,
                                  rois=[b for n, b in roi_list(26, 40) if not croppable(b) or n.startswith("outside")]),
}
CROP_CASES = list(CROP_BUILDERS)
_crop_cache = {}


def crop_case(name):
    """(case, (nchw, taps)) - computed once, shared, never modified."""
    if name not in _crop_cache:
        c = CROP_BUILDERS[name]()
        _crop_cache[name] = (c, crop_reference(c))
    return _crop_cache[name]


def _fence(lib, ranges_per_buf, bufs):
    lib.hipemu_fence.argtypes = [C.c_void_p, C.c_size_t]
    lib.hipemu_fenced_reads.restype = C.c_long
    lib.hipemu_fences_clear()
    for t, ranges in zip(bufs, ranges_per_buf):
        for a, e in ranges:
            lib.hipemu_fence(C.c_void_p(t.data_ptr() + a), e - a)


def crop_call(lib, device, c, want=(True, True), fences=None, **over):
    """fvp_crop_rois / fvp_crop_rois_nv12 on ``device``: (rc, nhwc8 uint16 [R,h,w/2,8] or None, nchw f32 or None[, fenced
    reads]).  Outputs start poisoned.  ``over`` replaces arguments (the error tests)."""
    a = dict(c)
    a.update(over)
    bufs = [_dev(b, device) for b in c["bufs"]]
    rois = _dev(c["rois"], device)
    R = len(c["rois"])
    o16 = _dev(np.full((R, c["h"], c["w"] // 2, 8), 0xDEAD, np.uint16).view(np.int16), device) if want[0] else None
    o32 = _dev(np.full((R, 3, c["h"], c["w"]), NAN, f32), device) if want[1] else None
    tail = (None if a.get("null_rois") else _ptr(rois), a.get("R", R), a["rpf"], None if a.get("null_mean") else _fa(a["mean"]),
            None if a.get("null_std") else _fa(a["std"]), a["h"], a["w"])
    if fences is not None:
        _fence(lib, fences, bufs)
    if c["kind"] == "rgb":
        rc = lib.fvp_crop_rois(None if a.get("null_frames") else _ptr(bufs[0]), a["F"], a["hs"], a["ws"], *tail,
                               a.get("flags", 1 if a["swap"] else 0), _ptr(o16), _ptr(o32), _stream(device))
    else:
        rc = lib.fvp_crop_rois_nv12(None if a.get("null_frames") else _ptr(bufs[c["y"][0]], c["y"][1]),
                                    None if a.get("null_uv") else _ptr(bufs[c["uv"][0]], c["uv"][1] + a.get("uv_shift", 0)),
                                    a["F"], a["hs"], a["ws"], a["y_pitch"], a["uv_pitch"], a["y_fs"], a["uv_fs"], a["standard"],
                                    *tail, _ptr(o16), _ptr(o32), _stream(device))
    _sync(device)
    res = (rc, None if o16 is None else o16.cpu().numpy().view(np.uint16), None if o32 is None else o32.cpu().numpy())
    if fences is not None:
        res += (int(lib.hipemu_fenced_reads()),)
        lib.hipemu_fences_clear()
    return res


def crop_check(lib, device, name):
    """Bit equality with the restatement; the bf16 layout equal to pack_nhwc8 of the fp32 output; each output alone."""
    c, (want, _) = crop_case(name)
    rc, o16, o32 = crop_call(lib, device, c)
    assert rc == 0, rc
    assert np.array_equal(bits(o32), bits(want)), name
    assert np.array_equal(o16, pack_nhwc8(o32)), name
    for r, roi in enumerate(c["rois"]):
        if not croppable(roi):
            assert not bits(o32[r]).any() and not o16[r].any(), (name, r)             # fp32 +0, bf16 0
    rc, a16, a32 = crop_call(lib, device, c, want=(True, False))
    assert rc == 0 and a32 is None and np.array_equal(a16, o16)
    rc, a16, a32 = crop_call(lib, device, c, want=(False, True))
    assert rc == 0 and a16 is None and np.array_equal(bits(a32), bits(o32))


def crop_check_tie(lib, device, name):
    """THE TIE: crop r equals fvp_ingest_frames / fvp_ingest_nv12 called on frame r / rois_per_frame alone with the derived
    matrix, H = h, W = w - both outputs, bit for bit."""
    c, _ = crop_case(name)
    rc, o16, o32 = crop_call(lib, device, c)
    assert rc == 0
    bufs = [_dev(b, device) for b in c["bufs"]]
    h, w = c["h"], c["w"]
    tied = 0
    for r, roi in enumerate(c["rois"]):
        if not croppable(roi):
            continue
        f = r // c["rpf"]
        inv = crop_matrix(roi, h, w)
        i16 = _dev(np.full((1, h, w // 2, 8), 0xDEAD, np.uint16).view(np.int16), device)
        i32 = _dev(np.full((1, 3, h, w), NAN, f32), device)
        if c["kind"] == "rgb":
            rc = lib.fvp_ingest_frames(_ptr(bufs[0], f * c["hs"] * c["ws"] * 3), 1, c["hs"], c["ws"], _fa(inv), _fa(c["mean"]),
                                       _fa(c["std"]), h, w, 1 if c["swap"] else 0, _ptr(i16), _ptr(i32), _stream(device))
        else:
            rc = lib.fvp_ingest_nv12(_ptr(bufs[c["y"][0]], c["y"][1] + f * c["y_fs"]), _ptr(bufs[c["uv"][0]], c["uv"][1] + f * c["uv_fs"]),
                                     1, c["hs"], c["ws"], c["y_pitch"], c["uv_pitch"], c["y_fs"], c["uv_fs"], c["standard"],
                                     _fa(inv), _fa(c["mean"]), _fa(c["std"]), h, w, _ptr(i16), _ptr(i32), _stream(device))
        assert rc == 0, rc
        _sync(device)
        assert np.array_equal(bits(i32.cpu().numpy()[0]), bits(o32[r])), (name, r)
        assert np.array_equal(i16.cpu().numpy().view(np.uint16)[0], o16[r]), (name, r)
        tied += 1
    return tied


def crop_check_identity(lib, device, name):
    """An ROI equal to the whole frame at the frame's size: the matrix is the identity exactly and the crop is the identity
    ingest of every frame in one call."""
    c, _ = crop_case(name)
    assert (c["h"], c["w"]) == (c["hs"], c["ws"]) and c["rpf"] == 1
    assert np.array_equal(crop_matrix(c["rois"][0], c["h"], c["w"]), np.array([1, 0, 0, 0, 1, 0], f32))
    rc, o16, o32 = crop_call(lib, device, c)
    bufs = [_dev(b, device) for b in c["bufs"]]
    F, h, w = c["F"], c["h"], c["w"]
    i16 = _dev(np.zeros((F, h, w // 2, 8), np.int16), device)
    i32 = _dev(np.zeros((F, 3, h, w), f32), device)
    ident = _fa([1, 0, 0, 0, 1, 0])
    if c["kind"] == "rgb":
        rc2 = lib.fvp_ingest_frames(_ptr(bufs[0]), F, h, w, ident, _fa(c["mean"]), _fa(c["std"]), h, w, 1 if c["swap"] else 0,
                                    _ptr(i16), _ptr(i32), _stream(device))
    else:
        rc2 = lib.fvp_ingest_nv12(_ptr(bufs[c["y"][0]], c["y"][1]), _ptr(bufs[c["uv"][0]], c["uv"][1]), F, h, w, c["y_pitch"],
                                  c["uv_pitch"], c["y_fs"], c["uv_fs"], c["standard"], ident, _fa(c["mean"]), _fa(c["std"]), h, w,
                                  _ptr(i16), _ptr(i32), _stream(device))
    _sync(device)
    assert rc == 0 and rc2 == 0
    assert np.array_equal(bits(i32.cpu().numpy()), bits(o32)) and np.array_equal(i16.cpu().numpy().view(np.uint16), o16)


def crop_argument_errors(lib, device):
    """Every refusal of the two crop calls; nothing is written when an error is returned."""
    def untouched(o16, o32):
        return (o16 == 0xDEAD).all() and np.isnan(o32).all()

    for name in ("rgb_8x8_per3_swap", "nv12_709l_8x8_per3_planes"):
        c, _ = crop_case(name)
        R = len(c["rois"])
        bad = [dict(null_frames=True), dict(null_rois=True), dict(null_mean=True), dict(null_std=True), dict(F=-1), dict(R=-1),
               dict(hs=0), dict(ws=0), dict(h=0), dict(w=0), dict(w=7), dict(rpf=0), dict(rpf=-3), dict(R=R - 1), dict(F=c["F"] + 1),
               dict(rpf=2), dict(mean=(NAN, 0, 0)), dict(std=(1, INF, 1)), dict(std=(1, 1, 0))]
        if c["kind"] == "rgb":
            bad += [dict(flags=2), dict(flags=4), dict(flags=-1)]
        else:
            bad += [dict(null_uv=True), dict(hs=25), dict(ws=39), dict(y_pitch=39), dict(uv_pitch=38), dict(uv_pitch=49),
                    dict(uv_fs=c["uv_fs"] + 1), dict(uv_shift=1), dict(standard=4), dict(standard=-1)]
        for over in bad:
            rc, o16, o32 = crop_call(lib, device, c, **over)
            assert rc == EINVAL, (name, over, rc)
            assert untouched(o16, o32), (name, over)
        rc, o16, o32 = crop_call(lib, device, c, want=(False, False))
        assert rc == EINVAL
        for over in (dict(hs=1 << 24), dict(ws=1 << 24), dict(h=1 << 24), dict(w=1 << 24), dict(h=65536, w=512)):
            if c["kind"] == "nv12" and "ws" in over:
                over = dict(ws=1 << 24, y_pitch=1 << 24, uv_pitch=1 << 24)
            rc, o16, o32 = crop_call(lib, device, c, **over)
            assert rc == ELIMIT, (name, over, rc)
            assert untouched(o16, o32), (name, over)
        rc, o16, o32 = crop_call(lib, device, c, F=0, R=0)                             # no launch: nothing written
        assert rc == 0 and untouched(o16, o32)


# ======================================================================================================================
# host side: frames for PersonCrops and model.crops
# ======================================================================================================================
def nv12_frames(c, bufs, lead):
    """dataset.images.Nv12Frames over torch allocations laid out as ``c`` describes, leading dimensions ``lead``."""
    from faster_voxelpose_amd.dataset.images import Nv12Frames
    y = torch.as_strided(bufs[c["y"][0]], (c["F"], c["hs"], c["ws"]), (c["y_fs"], c["y_pitch"], 1), c["y"][1])
    uv = torch.as_strided(bufs[c["uv"][0]], (c["F"], c["hs"] // 2, c["ws"] // 2, 2), (c["uv_fs"], c["uv_pitch"], 2, 1), c["uv"][1])
    std = {0: ("bt601", False), 1: ("bt709", False), 2: ("bt601", True), 3: ("bt709", True)}[c["standard"]]
    return Nv12Frames(y.unflatten(0, lead), uv.unflatten(0, lead), standard=std[0], full_range=std[1])


def person_scene(J, hs, ws, seed):
    """views [B,V,N,J,4], ids, conf for figures that lie partly inside a frame of hs x ws."""
    rng = np.random.default_rng([seed, J, hs, ws])
    v = np.empty((B, V, N, J, 4), f32)
    cx = rng.uniform(0.1 * ws, 0.9 * ws, (B, V, N, 1))
    cy = rng.uniform(0.1 * hs, 0.9 * hs, (B, V, N, 1))
    v[..., 0] = cx + rng.uniform(-0.15 * ws, 0.15 * ws, (B, V, N, J))
    v[..., 1] = cy + rng.uniform(-0.3 * hs, 0.3 * hs, (B, V, N, J))
    v[..., 2] = rng.uniform(1.0, 5.0, (B, V, N, J))
    v[..., 3] = rng.uniform(0.0, 1.0, (B, V, N, J))
    v[0, 1, 2, :, 2] = -1.0                                      # one person behind one camera: an invalid box there
    ids = np.array([[4, -1, 9], [0, 1, 2]], np.int32)
    conf = rng.uniform(0.0, 1.0, (B, N, J)).astype(f32)
    return v, ids, conf
