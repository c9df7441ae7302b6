"""fvp_anonymise_rois and fvp_anonymise_rois_nv12 of the shipped library on the MI355X: every case of
tests/anonymise_cases.py against the independent numpy restatement of include/fvp.h, whole allocations byte for byte (guards,
pitch padding and frame gaps included); ROI order; the privacy property; every argument error; FaceAnonymiser eager and
captured once into a hipGraph, replayed on other frames and other boxes."""
import numpy as np
import pytest
import torch

import anonymise_cases as AC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def lib():
    from faster_voxelpose_amd import _capi as capi
    return capi.load()


def test_library_holds_the_two_exports(lib):
    from faster_voxelpose_amd import _capi as capi
    assert capi.ABI_VERSION >= 23 and lib.fvp_version() == capi.ABI_VERSION
    for name in ("fvp_anonymise_rois", "fvp_anonymise_rois_nv12"):
        assert name in capi.SIGNATURES and hasattr(lib, name)


@pytest.mark.parametrize("name", AC.CASES)
def test_frames_equal_the_yardstick(lib, name):
    AC.check(lib, DEV, name)


@pytest.mark.parametrize("name", ["rgb_c8_rect_r64", "rgb_c32_ellipse_r64", "nv12_c8_ellipse_r64_planes", "rgb_c4_ellipse_r3",
                                  "nv12_fill_601f"])
def test_roi_order_does_not_matter(lib, name):
    AC.check_reversed(lib, DEV, name)


def test_privacy_property(lib):
    """Shuffling the source pixels inside every cell leaves every covered output pixel unchanged."""
    c, (want, _, _) = AC.case("rgb_c8_ellipse_r3")
    p = AC.permuted_within_cells(c)
    rc, got = AC.call(lib, DEV, p)
    cov = AC.coverage(c)
    assert rc == 0 and cov.any() and np.array_equal(AC.rgb_view(c, got)[cov], AC.rgb_view(c, want)[cov])
    assert np.array_equal(AC.rgb_view(c, got)[~cov], AC.rgb_view(p, p["bufs"])[~cov])


def test_argument_errors(lib):
    AC.argument_errors(lib, DEV)


@pytest.mark.parametrize("kind,J", [("rgb", 17), ("nv12", 15)])
def test_face_anonymiser_class(kind, J):
    """__call__ with the head preset equals the yardsticks of its two launches; captured once into a hipGraph (one stream, no
    parallel branches) and replayed on other frames and other poses in the same memory, the replay's bytes are the yardstick's
    for those; the refusals."""
    from faster_voxelpose_amd import _capi as capi
    from faster_voxelpose_amd.utils.anonymise import FaceAnonymiser
    B, V, N = 2, 2, 3
    fa = FaceAnonymiser(J, scale=2.0, pad_px=1.5, min_joints=2, aspect=0.8, conf_min=0.3, cell=4)
    assert fa.joints == ([0, 1, 2, 3, 4] if J == 17 else [0, 1])

    def scene(seed):
        views, ids, conf = AC.head_scene(J, list(fa.joints), 38, 70, seed)
        rois = AC.head_rois(views, ids, conf, fa.joints, 2.0, 1.5, 2, 0.8, 0.3)[0]
        per_frame = [[tuple(b) for b in rois[b, v]] for b in range(B) for v in range(V)]
        c = AC._case(kind, 4, AC.ELLIPSE, AC.MOSAIC, N, per_frame, 41 + seed, standard=3, y_pitch=75, uv_pitch=72, split=True, gap=6)
        want, loads, _ = AC.reference(c)
        assert loads > 0
        return (views, ids, conf), c, want

    def check(bufs, want):
        torch.cuda.synchronize()
        assert AC.same([t.cpu().numpy() for t in bufs], want)

    (views, ids, conf), c, want = scene(5)
    bufs = [torch.from_numpy(b.copy()).to(DEV) for b in c["bufs"]]
    frames = AC.torch_frames(c, bufs, (B, V))
    tv, ti, tc = (torch.from_numpy(a).to(DEV) for a in (views, ids, conf))
    assert fa(frames, tv, ids=ti, joint_conf=tc) is frames
    check(bufs, want)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fa(frames, tv, ids=ti, joint_conf=tc)
    (views2, ids2, conf2), c2, want2 = scene(6)
    for t, b in zip(bufs, c2["bufs"]):
        t.copy_(torch.from_numpy(b))
    tv.copy_(torch.from_numpy(views2))
    ti.copy_(torch.from_numpy(ids2))
    tc.copy_(torch.from_numpy(conf2))
    graph.replay()
    check(bufs, want2)
    assert not AC.same(want2, want)
    rois = fa.rois(tv, ids=ti, joint_conf=tc)[0]
    with pytest.raises(capi.FvpError):
        fa.rois(tv.cpu())                                                        # host memory
    with pytest.raises(capi.FvpError):
        fa.apply(frames, rois.cpu())                                             # frames and rois on different devices
    with pytest.raises(capi.FvpError):
        fa.apply(frames, rois[:, :1].contiguous())                               # V differs
    with pytest.raises(capi.FvpError):
        fa.apply(frames, torch.zeros(B, V, 65, 4, device=DEV))                   # more than 64 boxes per frame
    check(bufs, want2)                                                           # a refusal writes nothing
