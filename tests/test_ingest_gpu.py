"""fvp_ingest_frames on the MI355X through the shipped library: the value checks of tests/test_ingest_emu.py again
(shared cases and references: tests/ingest_cases.py) plus the 1080p shape, and the Python surface end to end -
``model(views=<uint8 frames>)``, ``PoseResNet.forward_frames`` under hipGraph capture, a plain torch module as
backbone, ``core.function.validate`` on the image source."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import fvp_synthetic as S
import ingest_cases as IC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def lib():
    from faster_voxelpose_amd import _capi as capi
    return capi.load()


def _case(name):
    (ws, hs), (W, H), fwd, n, swap = IC.CASES[name]
    return IC.make_frames(name), fwd, W, H, swap


@pytest.mark.parametrize("name", list(IC.CASES))
def test_bit_equal_to_the_float32_restatement(lib, name):
    """With and without FVP_INGEST_GENERAL (one form ships; the flag changes nothing)."""
    frames, fwd, W, H, swap = _case(name)
    ref = IC.reference_f32(frames, IC.invert_affine(fwd), W, H, swap)
    for general in (False, True):
        o16, o32 = IC.run(lib, frames, fwd, W, H, swap, general, device=DEV)
        bad = int((IC.bits(o32) != IC.bits(ref)).sum())
        assert bad == 0, f"general={general}: {bad} of {ref.size} fp32 values differ from the float32 restatement"
        assert np.array_equal(o16, IC.pack_nhwc8(ref)), f"general={general}"
        only16, _ = IC.run(lib, frames, fwd, W, H, swap, general, device=DEV, want_nchw=False)
        assert np.array_equal(only16, o16)


def test_panoptic_1080p_shape(lib):
    """10 frames 1080 x 1920 -> 512 x 960 through get_resize_transform: == the float32 restatement, every pixel (with and without FVP_INGEST_GENERAL),
    and within the derived bound of the exact float64 bilinear."""
    from faster_voxelpose_amd.utils.transforms import get_resize_transform
    fwd = get_resize_transform((1920, 1080), (960, 512))
    rng = np.random.default_rng(1080)
    frames = rng.integers(0, 256, size=(10, 1080, 1920, 3), dtype=np.uint8)
    ref = IC.reference_f32(frames, IC.invert_affine(fwd), 960, 512, True)
    want16 = IC.pack_nhwc8(ref)
    for general in (False, True):
        o16, o32 = IC.run(lib, frames, fwd, 960, 512, True, general, device=DEV)
        assert np.array_equal(IC.bits(o32), IC.bits(ref)), f"general={general}"
        assert np.array_equal(o16, want16), f"general={general}"
    exact = IC.reference_f64(frames[:2], fwd, 960, 512, True)
    err = float(np.abs(o32[:2].astype(np.float64) - exact).max())
    bound = IC.f64_bound(fwd, 1080, 1920, 960, 512)
    print(f"1080p: max |fp32 - exact| = {err:.3e}, bound {bound:.3e}")
    assert err <= bound


@pytest.mark.parametrize("name", ["identity", "identity_noswap"])
def test_identity_equals_the_loader_path(lib, name):
    """Identity transform: nchw == ToTensor + Normalize in fp32 (computed by torch where the reference's loader computes
    it, on the host), nhwc8 == fvp_bb_input of that tensor - today's float path - bit for bit."""
    frames, fwd, W, H, swap = _case(name)
    t = IC.torch_loader_f32(frames[..., ::-1] if swap else frames)
    n = frames.shape[0]
    today = torch.zeros((n, H, W // 2, 8), dtype=torch.int16, device=DEV)
    tg = t.to(DEV)
    rc = lib.fvp_bb_input(C.c_void_p(tg.data_ptr()), C.c_void_p(today.data_ptr()), n, 3, H, W,
                          C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    for general in (False, True):
        o16, o32 = IC.run(lib, frames, fwd, W, H, swap, general, device=DEV)
        assert np.array_equal(IC.bits(o32), IC.bits(t.numpy()))
        assert np.array_equal(o16, today.cpu().numpy().view(np.uint16))


def _panoptic(batch=1, seed=5):
    from faster_voxelpose_amd.core import config as CFG
    from faster_voxelpose_amd.models import faster_voxelpose as FV, resnet as RN
    cfg = S.make_cfg("panoptic", device=DEV, min_score=-1.0)
    cams, seq = S.load_cameras("panoptic")
    rt = S.resize_transform(cfg).to(DEV)
    model = FV.get(cfg).to(DEV)
    model.load_state_dict(S.fill_state_dict(model.state_dict(), seed=7))
    bb = RN.get(CFG.default_config()).to(DEV)
    bb.load_state_dict(S.fill_backbone_state_dict(bb.state_dict(), seed=3))
    ws, hs = cfg.DATASET.ORI_IMAGE_SIZE
    g = torch.Generator().manual_seed(seed)
    frames = torch.randint(0, 256, (batch, cfg.DATASET.CAMERA_NUM, hs, ws, 3), dtype=torch.uint8, generator=g).to(DEV)
    meta = {"seq": [seq] * batch}
    return cfg, model, bb, cams, rt, frames, meta


def test_model_takes_uint8_frames_end_to_end():
    """model(views=uint8 [B,V,Hs,Ws,3]) == model(views=ingest_frames(...)) bit for bit: heatmaps and fused poses (same fp32
    values, same bf16 rounding, same kernels after the input stage)."""
    from faster_voxelpose_amd import _capi as capi
    from faster_voxelpose_amd.dataset.images import ingest_frames
    cfg, model, bb, cams, rt, frames, meta = _panoptic()
    with torch.no_grad():
        f8, p8, c8, h8, _ = model(backbone=bb, views=frames, meta=meta, cameras=cams, resize_transform=rt)
        views = ingest_frames(frames, rt, cfg.DATASET.IMAGE_SIZE)
        W, H = cfg.DATASET.IMAGE_SIZE
        assert views.shape == (1, cfg.DATASET.CAMERA_NUM, 3, H, W) and views.dtype == torch.float32
        f32_, p32, c32, h32, _ = model(backbone=bb, views=views, meta=meta, cameras=cams, resize_transform=rt)
    assert torch.isfinite(f8).all() and h8.abs().max() > 0
    assert torch.equal(h8, h32) and torch.equal(f8, f32_) and torch.equal(p8, p32) and torch.equal(c8, c32)
    with pytest.raises(capi.FvpError):                       # uint8 views cannot be resized without the matrix
        model(backbone=bb, views=frames, meta=meta, cameras=cams)
    with pytest.raises(capi.FvpError):                       # CHW uint8 is not the accepted form
        model(backbone=bb, views=frames.permute(0, 1, 4, 2, 3).contiguous(), meta=meta, cameras=cams, resize_transform=rt)


def test_forward_frames_under_graph_capture():
    """forward_frames captured once (the by-value matrix is baked into the launch), replayed with two different frame
    contents in the static buffer: each replay equals the eager call on the same frames."""
    cfg, model, bb, cams, rt, frames, meta = _panoptic(seed=11)
    a = frames[0]
    b = torch.flip(a, dims=[0, 2]).contiguous()              # other contents: views reversed and mirrored
    assert not torch.equal(a, b)
    with torch.no_grad():
        eager_a = bb.forward_frames(a, rt).clone()
        eager_b = bb.forward_frames(b, rt).clone()
        assert not torch.equal(eager_a, eager_b)
        static = a.clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            bb.forward_frames(static, rt)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = bb.forward_frames(static, rt)
        for src, want in ((b, eager_b), (a, eager_a)):
            static.copy_(src)
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, want)


def test_torch_module_backbone_takes_the_fp32_route():
    from faster_voxelpose_amd.dataset.images import ingest_frames
    cfg, model, _, cams, rt, frames, meta = _panoptic(seed=13)
    W, H = cfg.DATASET.IMAGE_SIZE
    want = ingest_frames(frames, rt, (W, H))
    seen = []

    class Stub(torch.nn.Module):
        def forward(self, x):
            seen.append(x.clone())
            pooled = torch.nn.functional.avg_pool2d(x, 4).mean(dim=1, keepdim=True)
            return pooled.expand(-1, cfg.DATASET.NUM_JOINTS, -1, -1).contiguous()

    with torch.no_grad():
        fused, _, _, heat, _ = model(backbone=Stub(), views=frames, meta=meta, cameras=cams, resize_transform=rt)
    assert len(seen) == cfg.DATASET.CAMERA_NUM
    for v, x in enumerate(seen):
        assert x.shape == (1, 3, H, W) and x.dtype == torch.float32 and torch.equal(x, want[:, v])
    assert heat.shape == (1, cfg.DATASET.CAMERA_NUM, cfg.DATASET.NUM_JOINTS, H // 4, W // 4)
    assert torch.isfinite(fused).all()


def test_validate_on_the_image_source_with_uint8_inputs(tmp_path):
    """core.function.validate with TEST_HEATMAP_SRC == 'image', a stub loader that yields uint8 frames on the host and the
    HIP backbone: the poses equal a direct call of the model."""
    from faster_voxelpose_amd.core import function as FN
    cfg, model, bb, cams, rt, frames, meta = _panoptic(seed=17)
    with torch.no_grad():
        want, _, _, _, _ = model(backbone=bb, views=frames, meta=meta, cameras=cams, resize_transform=rt)
        want = want.clone()
    host = frames.cpu()
    seen = {}

    class Dataset:
        cameras = cams
        resize_transform = rt.cpu().numpy()

        def evaluate(self, all_fused_poses):
            seen["poses"] = all_fused_poses.clone()
            return 3.5, "stub"

    class Loader:
        dataset = Dataset()

        def __len__(self):
            return 2

        def __iter__(self):
            for _ in range(2):
                yield host, None, meta, None

    cfg.DATASET.TEST_HEATMAP_SRC = "image"
    cfg.TEST = types.SimpleNamespace(VISUALIZATION=False)
    cfg.PRINT_FREQ = 1
    assert FN.validate(cfg, bb, model, Loader(), str(tmp_path), has_evaluate_function=True) == 3.5
    n = want.shape[0]
    assert seen["poses"].shape[0] == 2 * n
    assert torch.equal(seen["poses"][:n], want) and torch.equal(seen["poses"][n:], want)
