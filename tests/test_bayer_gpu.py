"""fvp_demosaic_bayer and fvp_ingest_bayer on the MI355X through the shipped library: the value checks of
tests/test_bayer_emu.py again (shared cases and references: tests/bayer_cases.py), one 1080p shape, and the Python
surface end to end - ``model(views=BayerFrames)`` with the HIP backbone (``bayer_rgb`` False and True, an overlay on
``last_frames``) and with a plain torch module, ``PoseResNet.forward_frames`` under hipGraph capture."""
import numpy as np
import pytest
import torch

import bayer_cases as BC
import fvp_synthetic as S
import ingest_cases as IC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def lib():
    from faster_voxelpose_amd import _capi as capi
    return capi.load()


def test_version(lib):
    assert lib.fvp_version() == 24


@pytest.mark.parametrize("name", list(BC.CASES))
def test_bit_equal_to_the_restatement_and_to_ingest_frames(lib, name):
    """The demosaic == the numpy int64 restatement, every byte, guards intact; both ingest outputs == the restatement + the
    float32 restatement of fvp_ingest_frames, each requested alone too, and == fvp_ingest_frames of the shipped library on
    the demosaiced frame (the defining property of include/fvp.h)."""
    m = BC.Mosaic(name)
    c = m.case
    W, H = c["dst"]
    rgb = m.rgb()
    ref = BC.reference_f32(rgb, BC.invert_affine(c["fwd"]), W, H, False)
    frame, guards = BC.run_demosaic(lib, m, device=DEV)
    assert guards, "bytes outside the RGB output were written"
    bad = int((frame != rgb).sum())
    assert bad == 0, f"{bad} of {rgb.size} demosaiced bytes differ from the restatement"
    o16, o32 = BC.run_ingest(lib, m, device=DEV)
    bad = int((BC.bits(o32) != BC.bits(ref)).sum())
    assert bad == 0, f"{bad} of {ref.size} fp32 values differ from the restatement"
    assert np.array_equal(o16, BC.pack_nhwc8(ref))
    only16, _ = BC.run_ingest(lib, m, device=DEV, want_nchw=False)
    _, only32 = BC.run_ingest(lib, m, device=DEV, want_bf16=False)
    assert np.array_equal(only16, o16) and np.array_equal(BC.bits(only32), BC.bits(o32))
    r16, r32 = IC.run(lib, frame, c["fwd"], W, H, False, False, device=DEV)
    assert np.array_equal(o16, r16) and np.array_equal(BC.bits(o32), BC.bits(r32))


@pytest.mark.parametrize("size", BC.DEMOSAIC_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_demosaic_around_the_tile(lib, size):
    for pattern, extra, tone in ((BC.GRBG, 0, False), (BC.BGGR, 5, True)):
        m = BC.sized(*size, pattern=pattern, pitch=size[0] + extra, gap=3 * bool(extra), tone=tone)
        got, guards = BC.run_demosaic(lib, m, device=DEV)
        assert guards and np.array_equal(got, m.rgb())


def test_argument_errors_write_nothing(lib):
    raw = torch.full((2 * 8 * 16 + 8,), 90, dtype=torch.uint8, device=DEV)
    rgb = torch.full((2, 8, 8, 3), 7, dtype=torch.uint8, device=DEV)
    o32 = torch.full((2, 3, 4, 4), 7.0, dtype=torch.float32, device=DEV)
    inv = BC.invert_affine(BC.IDENTITY)
    st = BC._stream()

    def dem(n=2, hs=8, ws=8, pitch=16, pattern=0, flags=0, out=rgb.data_ptr()):
        return BC.call_demosaic(lib, raw.data_ptr(), n, hs, ws, pitch, 128, pattern, None, flags, out, stream=st)

    def ing(n=2, hs=8, ws=8, pitch=16, pattern=0, H=4, W=4, out=o32.data_ptr(), sd=BC.STD32):
        return BC.call_ingest(lib, raw.data_ptr(), n, hs, ws, pitch, 128, pattern, None, inv, H, W, None, out, std=sd, stream=st)

    for f in (dem, ing):
        assert f(n=-1) == 10001 and f(hs=6 + 1) == 10001 and f(ws=2) == 10001 and f(pitch=7) == 10001 and f(pattern=4) == 10001
    assert dem(flags=2) == 10001 and dem(out=None) == 10001 and dem(hs=16386) == 10002
    assert ing(W=3) == 10001 and ing(out=None) == 10001 and ing(sd=(1, 0, 1)) == 10001 and ing(W=1 << 24) == 10002
    assert dem(n=0) == 0 and ing(n=0) == 0
    torch.cuda.synchronize()
    assert bool((rgb == 7).all()) and bool((o32 == 7).all())


def test_panoptic_1080p_shape(lib):
    """2 frames 1080 x 1920 at pitch 2048 -> 512 x 960, both kernels == the numpy reference, every byte and every pixel of
    both ingest outputs."""
    from faster_voxelpose_amd.dataset import images as IMG
    from faster_voxelpose_amd.utils.transforms import get_resize_transform
    hs, ws, pitch = 1080, 1920, 2048
    fwd = get_resize_transform((ws, hs), (960, 512))
    assert BC.lds_plan(BC.invert_affine(fwd), 512, 960, hs, ws)[0]
    rng = np.random.default_rng(1080)
    buf = rng.integers(0, 256, size=(2, hs, pitch), dtype=np.uint8)
    rgb = BC.demosaic(buf[:, :, :ws], BC.GBRG)
    ref = BC.reference_f32(rgb, BC.invert_affine(fwd), 960, 512, False)
    fr = IMG.BayerFrames(torch.from_numpy(buf).to(DEV)[:, :, :ws], "gbrg")
    assert (fr.pitch, fr.frame_stride) == (pitch, hs * pitch)
    got = fr.to_rgb()
    o32 = IMG.ingest_bayer(fr, fwd, (960, 512))
    o16 = torch.full((2, 512, 480, 8), -8531, dtype=torch.int16, device=DEV)
    IMG.launch_bayer(lib, fr, fwd, (960, 512), IMG.IMAGENET_MEAN, IMG.IMAGENET_STD, o16, None)
    torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy(), rgb)
    assert np.array_equal(BC.bits(o32.cpu().numpy()), BC.bits(ref))
    assert np.array_equal(o16.cpu().numpy().view(np.uint16), BC.pack_nhwc8(ref))


def _setup(name, seed, backbone):
    """A synthetic configuration, its model (and the HIP backbone), Bayer frames [B=1,V] at the camera's size on a pitched
    buffer with a tone table, the numpy demosaic of them (RGB) and its BGR copy on the device."""
    from faster_voxelpose_amd.core import config as CFG
    from faster_voxelpose_amd.dataset.images import BayerFrames
    from faster_voxelpose_amd.models import faster_voxelpose as FV, resnet as RN
    cfg = S.make_cfg(name, device=DEV, min_score=-1.0)
    cams, seq = S.load_cameras(name)
    rt = S.resize_transform(cfg).to(DEV)
    model = FV.get(cfg).to(DEV)
    model.load_state_dict(S.fill_state_dict(model.state_dict(), seed=7))
    bb = None
    if backbone:
        bb = RN.get(CFG.default_config()).to(DEV)
        bb.load_state_dict(S.fill_backbone_state_dict(bb.state_dict(), seed=3))
    ws, hs = cfg.DATASET.ORI_IMAGE_SIZE
    V = cfg.DATASET.CAMERA_NUM
    pitch = ws + 61                                           # odd
    rng = np.random.default_rng(seed)
    buf = rng.integers(0, 256, size=(1, V, hs, pitch), dtype=np.uint8)
    tone = BC.tone_formula(**BC.TONE_ARGS)
    rgb = BC.demosaic(buf[0, :, :, :ws], BC.GRBG, tone)[None]
    frames = BayerFrames(torch.from_numpy(buf).to(DEV)[..., :ws], "grbg", torch.from_numpy(tone).to(DEV))
    bgr = torch.from_numpy(np.ascontiguousarray(rgb[..., ::-1])).to(DEV)
    return cfg, model, bb, cams, rt, frames, rgb, bgr, {"seq": [seq]}


def test_model_takes_bayer_views_end_to_end():
    """model(views=BayerFrames [B,V]) == model(views=uint8 BGR of the numpy demosaic) bit for bit - heat-maps, poses,
    centres - with the HIP backbone; equal again with model.bayer_rgb = True, where last_frames is the numpy demosaic and
    an overlay runs on it; with bayer_rgb False and an overlay set the new error is raised."""
    from faster_voxelpose_amd import _capi as capi
    from faster_voxelpose_amd.utils.overlay import PoseOverlay
    cfg, model, bb, cams, rt, frames, rgb, bgr, meta = _setup("panoptic", 5, True)
    kw = dict(backbone=bb, meta=meta, cameras=cams, resize_transform=rt)
    with torch.no_grad():
        want = [t.clone() for t in model(views=bgr, **kw)[:4]]
        assert torch.isfinite(want[0]).all() and want[3].abs().max() > 0
        got = [t.clone() for t in model(views=frames, **kw)[:4]]
        assert model.last_frames is None
        for a, b in zip(got, want):
            assert torch.equal(a, b)
        model.bayer_rgb = True
        got = [t.clone() for t in model(views=frames, **kw)[:4]]
        for a, b in zip(got, want):
            assert torch.equal(a, b)
        assert model.last_frames.shape == rgb.shape and np.array_equal(model.last_frames.cpu().numpy(), rgb)
        model.evidence = True
        model.overlay = PoseOverlay(cfg, alpha=0.5)
        got = [t.clone() for t in model(views=frames, **kw)[:4]]
        for a, b in zip(got, want):
            assert torch.equal(a, b)
        painted = model.overlay.draw(torch.from_numpy(rgb).to(DEV), model.last_evidence[0], joint_conf=model.last_evidence[1])
        torch.cuda.synchronize()
        assert torch.equal(model.last_frames, painted)
        model.bayer_rgb = False
        with pytest.raises(capi.FvpError, match="set model.bayer_rgb = True"):
            model(views=frames, **kw)
        model.overlay = None
        with pytest.raises(capi.FvpError):                       # Bayer views cannot be resized without the matrix
            model(backbone=bb, views=frames, meta=meta, cameras=cams)
        with pytest.raises(capi.FvpError):                       # swap_rb has no meaning for Bayer frames
            bb.forward_frames(frames, rt, swap_rb=True)


def test_torch_module_backbone_takes_the_fp32_route():
    """The smallest synthetic configuration: a plain torch module as backbone gets the fp32 tensor of ingest_bayer, view by
    view; poses and heat-maps equal those of the uint8 BGR frames through the same module, bit for bit, and again with
    model.bayer_rgb = True."""
    from faster_voxelpose_amd.dataset.images import ingest_bayer
    cfg, model, _, cams, rt, frames, rgb, bgr, meta = _setup("tiny", 13, False)
    W, H = cfg.DATASET.IMAGE_SIZE
    want = ingest_bayer(frames, rt, (W, H))
    seen = []

    class Stub(torch.nn.Module):
        def forward(self, x):
            seen.append(x.clone())
            pooled = torch.nn.functional.avg_pool2d(x, 4).mean(dim=1, keepdim=True)
            return pooled.expand(-1, cfg.DATASET.NUM_JOINTS, -1, -1).contiguous()

    V = cfg.DATASET.CAMERA_NUM
    with torch.no_grad():
        fb, _, _, hb, _ = [t.clone() if isinstance(t, torch.Tensor) else t
                           for t in model(backbone=Stub(), views=bgr, meta=meta, cameras=cams, resize_transform=rt)]
        ref_seen = list(seen)
        for flag in (False, True):
            del seen[:]
            model.bayer_rgb = flag
            fn, _, _, hn, _ = model(backbone=Stub(), views=frames, meta=meta, cameras=cams, resize_transform=rt)
            assert len(seen) == V and len(ref_seen) == V
            for v in range(V):
                assert seen[v].shape == (1, 3, H, W) and seen[v].dtype == torch.float32
                assert torch.equal(seen[v], want[:, v]) and torch.equal(seen[v], ref_seen[v])
            assert torch.equal(hn, hb) and torch.equal(fn, fb)
    assert np.array_equal(model.last_frames.cpu().numpy(), rgb)


def test_forward_frames_under_graph_capture():
    """forward_frames(BayerFrames) on a small image (224 x 160 from 4 frames of 360 x 288 at pitch 384), captured once and
    replayed with other contents in the same buffer: each replay equals the eager call.  The inverse is computed once per
    resize_transform tensor and reused: no host read in steady state (one under capture would fail it)."""
    from faster_voxelpose_amd.core import config as CFG
    from faster_voxelpose_amd.dataset import images as IMG
    from faster_voxelpose_amd.dataset.images import BayerFrames
    from faster_voxelpose_amd.models import resnet as RN
    from faster_voxelpose_amd.utils.transforms import get_resize_transform
    cfg = CFG.default_config()
    cfg.DATASET.IMAGE_SIZE = np.array([224, 160])
    bb = RN.get(cfg).to(DEV)
    bb.load_state_dict(S.fill_backbone_state_dict(bb.state_dict(), seed=3))
    hs, ws, pitch = 288, 360, 384
    rt = torch.as_tensor(get_resize_transform((ws, hs), (224, 160)), dtype=torch.float32).to(DEV)
    g = torch.Generator().manual_seed(11)
    a = torch.randint(0, 256, (4, hs, pitch), dtype=torch.uint8, generator=g).to(DEV)
    b = torch.flip(a, dims=[0]).contiguous()                 # other contents: frames reversed
    assert not torch.equal(a, b)
    tone = BayerFrames.tone_table(**BC.TONE_ARGS, device=DEV)
    with torch.no_grad():
        eager_a = bb.forward_frames(BayerFrames(a[..., :ws], "bggr", tone), rt).clone()
        eager_b = bb.forward_frames(BayerFrames(b[..., :ws], "bggr", tone), rt).clone()
        assert eager_a.shape == (4, 15, 40, 56) and not torch.equal(eager_a, eager_b)
        static = a.clone()
        sframes = BayerFrames(static[..., :ws], "bggr", tone)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            bb.forward_frames(sframes, rt)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        cached = IMG._inverse.inv
        assert IMG._inverse.ref is rt
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = bb.forward_frames(sframes, rt)
        assert IMG._inverse.inv is cached
        for src, want in ((b, eager_b), (a, eager_a)):
            static.copy_(src)
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, want)
