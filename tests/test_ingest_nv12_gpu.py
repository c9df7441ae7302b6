"""fvp_ingest_nv12 on the MI355X through the shipped library: the value checks of tests/test_ingest_nv12_emu.py again
(shared cases and references: tests/ingest_nv12_cases.py), one 1080p shape, and the Python surface end to end -
``model(views=Nv12Frames)`` with the HIP backbone and with a plain torch module, ``PoseResNet.forward_frames`` under
hipGraph capture."""
import numpy as np
import pytest
import torch

import fvp_synthetic as S
import ingest_cases as IC
import ingest_nv12_cases as NC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def lib():
    from faster_voxelpose_amd import _capi as capi
    return capi.load()


@pytest.mark.parametrize("name", list(NC.CASES))
def test_bit_equal_to_the_restatement_and_to_ingest_frames(lib, name):
    """Every pixel of both outputs == nv12_to_rgb (numpy int64) + the float32 restatement, and == fvp_ingest_frames of the
    shipped library on the converted RGB frame (the defining property of include/fvp.h)."""
    s = NC.Surface(name)
    c = s.case
    W, H = c["dst"]
    rgb = s.rgb()
    ref = NC.reference_f32(rgb, NC.invert_affine(c["fwd"]), W, H, False)
    o16, o32 = NC.run(lib, s, device=DEV)
    bad = int((NC.bits(o32) != NC.bits(ref)).sum())
    assert bad == 0, f"{bad} of {ref.size} fp32 values differ from the restatement"
    assert np.array_equal(o16, NC.pack_nhwc8(ref))
    only16, _ = NC.run(lib, s, device=DEV, want_nchw=False)
    assert np.array_equal(only16, o16)
    r16, r32 = IC.run(lib, rgb, c["fwd"], W, H, False, False, device=DEV)
    assert np.array_equal(o16, r16) and np.array_equal(NC.bits(o32), NC.bits(r32))


def test_panoptic_1080p_shape(lib):
    """2 frames 1080 x 1920 at pitch 2048 (one contiguous NV12 buffer each, through Nv12Frames.from_buffer) -> 512 x 960:
    == the numpy reference, every pixel, both outputs."""
    from faster_voxelpose_amd.dataset import images as IMG
    from faster_voxelpose_amd.utils.transforms import get_resize_transform
    hs, ws, pitch = 1080, 1920, 2048
    fwd = get_resize_transform((ws, hs), (960, 512))
    rng = np.random.default_rng(1080)
    buf = rng.integers(0, 256, size=(2, hs * 3 // 2, pitch), dtype=np.uint8)
    y = buf[:, :hs, :ws]
    uv = buf[:, hs:, :ws].reshape(2, hs // 2, ws // 2, 2)
    ref = NC.reference_f32(NC.nv12_to_rgb(y, uv, NC.BT709_LIMITED), NC.invert_affine(fwd), 960, 512, False)
    fr = IMG.Nv12Frames.from_buffer(torch.from_numpy(buf).to(DEV), hs, ws, standard="bt709")
    assert (fr.y_pitch, fr.uv_pitch, fr.y_frame_stride) == (pitch, pitch, hs * 3 // 2 * pitch)
    o32 = IMG.ingest_nv12(fr, fwd, (960, 512))
    o16 = torch.full((2, 512, 480, 8), -8531, dtype=torch.int16, device=DEV)
    IMG.launch_nv12(lib, fr, fwd, (960, 512), IMG.IMAGENET_MEAN, IMG.IMAGENET_STD, o16, None)
    torch.cuda.synchronize()
    assert np.array_equal(NC.bits(o32.cpu().numpy()), NC.bits(ref))
    assert np.array_equal(o16.cpu().numpy().view(np.uint16), NC.pack_nhwc8(ref))


def _setup(name, seed, backbone):
    """A synthetic configuration, its model (and the HIP backbone), NV12 frames [B=1,V] at the camera's size on a pitched
    surface, and the BGR uint8 frames they convert to."""
    from faster_voxelpose_amd.core import config as CFG
    from faster_voxelpose_amd.dataset.images import Nv12Frames
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
    pitch = ws + 64
    rng = np.random.default_rng(seed)
    buf = rng.integers(0, 256, size=(1, V, hs * 3 // 2, pitch), dtype=np.uint8)
    y = buf[0, :, :hs, :ws]
    uv = buf[0, :, hs:, :ws].reshape(V, hs // 2, ws // 2, 2)
    bgr = np.ascontiguousarray(NC.nv12_to_rgb(y, uv, NC.BT601_LIMITED)[..., ::-1])[None]
    frames = Nv12Frames.from_buffer(torch.from_numpy(buf).to(DEV), hs, ws)
    return cfg, model, bb, cams, rt, frames, torch.from_numpy(bgr).to(DEV), {"seq": [seq]}


def test_model_takes_nv12_views_end_to_end():
    """model(views=Nv12Frames [B,V]) == model(views=uint8 BGR of nv12_to_rgb) bit for bit, heatmaps and fused poses, with
    the HIP backbone (direct bf16 route).  The Panoptic shape: the smallest synthetic configuration whose image size the
    bf16 backbone takes (multiples of 32) and its 15 joints; the miniature one runs in the torch-module test below."""
    from faster_voxelpose_amd import _capi as capi
    cfg, model, bb, cams, rt, frames, bgr, meta = _setup("panoptic", 5, True)
    with torch.no_grad():
        fn, pn, cn, hn, _ = [t.clone() if isinstance(t, torch.Tensor) else t
                             for t in model(backbone=bb, views=frames, meta=meta, cameras=cams, resize_transform=rt)]
        fb, pb, cb, hb, _ = model(backbone=bb, views=bgr, meta=meta, cameras=cams, resize_transform=rt)
    assert torch.isfinite(fn).all() and hn.abs().max() > 0
    assert torch.equal(hn, hb) and torch.equal(fn, fb) and torch.equal(pn, pb) and torch.equal(cn, cb)
    with pytest.raises(capi.FvpError):                       # NV12 views cannot be resized without the matrix
        model(backbone=bb, views=frames, meta=meta, cameras=cams)
    with pytest.raises(capi.FvpError):                       # swap_rb has no meaning for NV12
        bb.forward_frames(frames, rt, swap_rb=True)


def test_torch_module_backbone_takes_the_fp32_route():
    """The smallest synthetic configuration: a plain torch module as backbone gets the fp32 tensor of ingest_nv12, view by
    view; poses and heatmaps equal those of the uint8 BGR frames through the same module, bit for bit."""
    from faster_voxelpose_amd.dataset.images import ingest_nv12
    cfg, model, _, cams, rt, frames, bgr, meta = _setup("tiny", 13, False)
    W, H = cfg.DATASET.IMAGE_SIZE
    want = ingest_nv12(frames, rt, (W, H))
    seen = []

    class Stub(torch.nn.Module):
        def forward(self, x):
            seen.append(x.clone())
            pooled = torch.nn.functional.avg_pool2d(x, 4).mean(dim=1, keepdim=True)
            return pooled.expand(-1, cfg.DATASET.NUM_JOINTS, -1, -1).contiguous()

    with torch.no_grad():
        fn, _, _, hn, _ = [t.clone() if isinstance(t, torch.Tensor) else t
                           for t in model(backbone=Stub(), views=frames, meta=meta, cameras=cams, resize_transform=rt)]
        nv = list(seen)
        del seen[:]
        fb, _, _, hb, _ = model(backbone=Stub(), views=bgr, meta=meta, cameras=cams, resize_transform=rt)
    V = cfg.DATASET.CAMERA_NUM
    assert len(nv) == V and len(seen) == V
    for v in range(V):
        assert nv[v].shape == (1, 3, H, W) and nv[v].dtype == torch.float32
        assert torch.equal(nv[v], want[:, v]) and torch.equal(nv[v], seen[v])
    assert torch.equal(hn, hb) and torch.equal(fn, fb)


def test_forward_frames_under_graph_capture():
    """forward_frames(Nv12Frames) on a small image (224 x 160 from 4 frames of 360 x 288 at pitch 384), captured once and
    replayed with other surface contents in the same buffer: each replay equals the eager call.  The inverse is computed
    once per resize_transform tensor and reused: no host read in steady state (one under capture would fail it)."""
    from faster_voxelpose_amd.core import config as CFG
    from faster_voxelpose_amd.dataset import images as IMG
    from faster_voxelpose_amd.dataset.images import Nv12Frames
    from faster_voxelpose_amd.models import resnet as RN
    from faster_voxelpose_amd.utils.transforms import get_resize_transform
    cfg = CFG.default_config()
    cfg.DATASET.IMAGE_SIZE = np.array([224, 160])
    bb = RN.get(cfg).to(DEV)
    bb.load_state_dict(S.fill_backbone_state_dict(bb.state_dict(), seed=3))
    hs, ws, pitch = 288, 360, 384
    rt = torch.as_tensor(get_resize_transform((ws, hs), (224, 160)), dtype=torch.float32).to(DEV)
    g = torch.Generator().manual_seed(11)
    a = torch.randint(0, 256, (4, hs * 3 // 2, pitch), dtype=torch.uint8, generator=g).to(DEV)
    b = torch.flip(a, dims=[0]).contiguous()                 # other contents: frames reversed
    assert not torch.equal(a, b)
    with torch.no_grad():
        eager_a = bb.forward_frames(Nv12Frames.from_buffer(a, hs, ws), rt).clone()
        eager_b = bb.forward_frames(Nv12Frames.from_buffer(b, hs, ws), rt).clone()
        assert eager_a.shape == (4, 15, 40, 56) and not torch.equal(eager_a, eager_b)
        static = a.clone()
        sframes = Nv12Frames.from_buffer(static, hs, ws)
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
