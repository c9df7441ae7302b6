"""fvp_person_signature and fvp_track_reid on the CPU emulation of the kernels (tests/hipemu): every case of tests/reid_cases.py
against the independent numpy restatement, bit for bit - outputs and every state array after every call; the read fence (no
byte of a sample that does not count is read, nothing outside the frames); every edge of the state machine on hand-made
streams; chunk invariance; the stated invariants; every argument error; PersonReId; the closed loop with painted people, the
evidence kernel's pixels and a real PoseTracker."""
import numpy as np
import pytest
import torch

import reid_cases as RC
from faster_voxelpose_amd import _capi as capi
from faster_voxelpose_amd.core.reid import PersonReId
from faster_voxelpose_amd.dataset.images import Nv12Frames

f32 = np.float32


def test_header_and_binding_hold_the_two_exports(emu_lib):
    assert capi.ABI_VERSION >= 20 and emu_lib.fvp_version() == capi.ABI_VERSION
    header = open(RC.__file__.replace("tests/reid_cases.py", "include/fvp.h")).read()
    for name in ("fvp_person_signature", "fvp_track_reid"):
        assert name in capi.SIGNATURES and hasattr(emu_lib, name) and f"int {name}(" in header
    for name, value in (("FVP_SIG_MAX_PARTS", RC.MAX_PARTS), ("FVP_SIG_BINS", RC.BINS), ("FVP_REID_MAX_GALLERY", RC.MAX_GALLERY),
                        ("FVP_REID_MAX_WINDOW", RC.MAX_WINDOW), ("FVP_SIG_MAX_SAMPLES", 8 * 64 * 32)):
        assert getattr(capi, name) == value and f"#define {name} {value} " in header


# ---- fvp_person_signature ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", RC.SIG_CASES)
def test_signatures_equal_the_yardstick(emu_lib, name):
    RC.sig_check(emu_lib, "cpu", name)


def test_signature_cases_hold_what_their_names_say():
    for name in RC.SIG_CASES:
        c, (sig, cnt, taken) = RC.sig_case(name)
        assert int(sig.sum()) == int(cnt.sum()) == taken and (taken == 0) == (name == "all_invalid")
        assert cnt.sum(axis=2).max() <= capi.FVP_SIG_MAX_SAMPLES
    shapes = {(c["views"].shape[0], c["views"].shape[1], c["views"].shape[2], c["views"].shape[3], c["K"], c["P"])
              for c in (RC.sig_case(n)[0] for n in RC.SIG_CASES)}
    for axis, want in ((0, {1, 3, 8}), (1, {1, 3, 5}), (2, {4, 10}), (3, {15, 17}), (4, {1, 8, 32}), (5, {1, 2, 4})):
        assert {s[axis] for s in shapes} == want
    assert {RC.sig_case(n)[0]["frames"].shape[2:4] for n in RC.SIG_CASES} == {(96, 128), (50, 67)}
    # the border: the last column counts, half a pixel beyond it goes to the even neighbour - out at 128, in at 67
    for name, (hs, ws), beyond_in in (("edges_128x96", (96, 128), False), ("edges_67x50", (50, 67), True)):
        c, (sig, cnt, _) = RC.sig_case(name)
        one = dict(c, limbs=[[6, 6]], parts=[0], ids=np.array([[0, -1, -1, -1]], np.int32))
        assert RC.sig_reference(one)[2] == 8                                          # x = ws - 1
        one["limbs"] = [[7, 7]]
        assert RC.sig_reference(one)[2] == (8 if beyond_in else 0)                    # x = ws - 0.5
        one["limbs"] = [[1, 1]]
        assert RC.sig_reference(one)[2] == 8                                          # x = -0.5 rounds to -0: inside
        one["limbs"] = [[2, 2]]
        assert RC.sig_reference(one)[2] == 0
    on, off = RC.sig_case("conf_on")[1], RC.sig_case("conf_off")[1]
    assert 0 < on[2] < off[2]
    c, (sig, cnt, _) = RC.sig_case("ids_minus1")
    assert not cnt[0, 1].any() and not cnt[1, 0].any() and not cnt[2, 3].any() and cnt[0, 0].any()
    c, (sig, cnt, taken) = RC.sig_case("occluder_one_view")
    assert taken < RC.sig_reference(dict(c, occ=None))[2]
    c, (sig, cnt, _) = RC.sig_case("limb_ends_coincide_k32")
    frame_bins = [(int(p[0]) >> 6) * 16 + (int(p[1]) >> 6) * 4 + (int(p[2]) >> 6) for p in c["frames"][0, :, 31, 20]]
    assert all(sig[0, 0, 3 % 2, b] >= 32 for b in frame_bins)                       # (20.25, 30.75) -> pixel (20, 31), K times
    c, (_, _, taken) = RC.sig_case("behind_camera")
    assert taken < RC.sig_reference(dict(c, views=np.abs(c["views"]) + f32(1e-3)))[2]
    c, (_, cnt, _) = RC.sig_case("nan_pixel")
    assert cnt.any()


def test_signature_outputs_may_be_null(emu_lib):
    RC.sig_check_null_outputs(emu_lib, "cpu")


def test_signature_argument_errors(emu_lib):
    RC.sig_argument_errors(emu_lib, "cpu")


@pytest.mark.parametrize("name", ["rand_b3_v3_k8_p2_j17", "edges_67x50", "edges_128x96", "nan_pixel", "all_invalid"])
def test_reads_exactly_the_counting_samples(emu_lib, name):
    """The emulator's read fence: over the frames, one load per counting sample; over the guard band, none."""
    c, (want, _, taken) = RC.sig_case(name)
    rc, sig, _, reads = RC.sig_call(emu_lib, "cpu", c, fence="frames")
    assert rc == 0 and np.array_equal(sig, want) and reads == taken
    rc, sig, _, reads = RC.sig_call(emu_lib, "cpu", c, fence="guard")
    assert rc == 0 and np.array_equal(sig, want) and reads == 0


# ---- fvp_track_reid ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(RC.SCENARIOS))
def test_state_machine_edge(emu_lib, name):
    """Hand-made id / slot / signature streams: the kernel against the restatement after every call (outputs, every state
    array, the invariants), and the restatement against what the scenario's name says."""
    RC.SCENARIOS[name](emu_lib, "cpu")


def test_scenarios_cover_the_list():
    assert len(RC.SCENARIOS) == 11 and {s[3] for s in RC.RANDOM_STREAMS} == {1, 2, 4}          # G
    assert {s[4] for s in RC.RANDOM_STREAMS} == {1, 2, 4} and {s[1] for s in RC.RANDOM_STREAMS} == {4, 10}     # P, N
    assert {s[2] // s[1] for s in RC.RANDOM_STREAMS} == {1, 2}                                    # T = N and 2 N


@pytest.mark.parametrize("seed,n,t,g,p,nseq", RC.RANDOM_STREAMS)
def test_random_streams_and_chunk_invariance(emu_lib, seed, n, t, g, p, nseq):
    RC.random_stream_check(emu_lib, "cpu", seed, n, t, g, p, nseq)


def bits_(a):
    return np.ascontiguousarray(a).view(np.int32)


def test_reid_argument_errors(emu_lib):
    RC.reid_argument_errors(emu_lib, "cpu")


# ---- host side -------------------------------------------------------------------------------------------------------------
def test_person_reid_class(emu_lib):
    """signature(), update() and __call__ equal the C calls (the yardstick's bits); defaults; reset / state / load_state; the
    constructor's and the methods' refusals."""
    c, (want_sig, want_cnt, _) = RC.sig_case("rand_b1_v5_k8_p4_j17")
    B, V, n, J = c["views"].shape[:4]
    kw = dict(nseq=2, gallery=4, max_age=3, min_samples=4, min_frames=2, window=8, sim_min=0.6, margin=0.1, device="cpu", _lib=emu_lib)
    r = PersonReId((n, J), limbs=c["limbs"], limb_part=c["parts"], parts=c["P"], samples=c["K"], conf_min=c["conf_min"], **kw)
    assert (r.T, r.G, r.P, r.K) == (2 * n, 4, 4, 8)
    tf, tv, tc, to = (torch.from_numpy(c[k]) for k in ("frames", "views", "conf", "occ"))
    sig, cnt = r.signature(tf, tv, joint_conf=tc, occluder=to)
    assert np.array_equal(sig.numpy(), want_sig) and np.array_equal(cnt.numpy(), want_cnt)
    # the default tables: the overlay's limbs; legs are part 1
    d17, d15 = PersonReId((4, 17), device="cpu", _lib=emu_lib), PersonReId((4, 15), device="cpu", _lib=emu_lib)
    assert d17.limbs == [tuple(l) for l in RC.LIMBS17] and d15.limbs == [tuple(l) for l in RC.LIMBS15]
    assert [l for l, p in zip(d17.limbs, d17.limb_part) if p] == [(11, 13), (13, 15), (12, 14), (14, 16), (11, 12)]
    assert [l for l, p in zip(d15.limbs, d15.limb_part) if p] == [(2, 6), (2, 12), (6, 7), (7, 8), (12, 13), (13, 14)]
    assert set(PersonReId((4, 14), parts=1, device="cpu", _lib=emu_lib).limb_part) == {0}
    # update() against the restatement over two calls, sequences by name, then __call__
    call = RC.random_stream(7, 12, n, 2 * n, 4, nseq=1)
    st = RC.reid_init(2, 2 * n, 4, 4)
    prm = dict(RC.PRM)
    for part in RC.chunks(call, [5]):
        ids, slots, s, k, _ = part
        fs = np.ones(len(ids), np.int32)                                              # "b" is row 1: "a" was seen first
        want = RC.reid_reference(st, ids, slots, s, k, fs, prm)
        r.frame_sets(["a"])
        got = r.update(*(torch.from_numpy(x) for x in (ids, slots, s, k)), meta={"seq": ["b"] * len(ids)})
        assert all(np.array_equal(bits_(g.numpy()), bits_(w)) for g, w in zip(got, want))
        assert RC.same_state({k2: v.numpy() for k2, v in r.state().items()}, st)
    saved = r.state()
    r.reset("b")
    assert RC.same_state({k2: v.numpy() for k2, v in r.state().items()}, RC.reid_init(2, 2 * n, 4, 4))
    r.load_state(saved)
    assert RC.same_state({k2: v.numpy() for k2, v in r.state().items()}, st)
    r.reset()
    ids = torch.zeros((B, n), dtype=torch.int32)
    slots = torch.arange(n, dtype=torch.int32).repeat(B, 1)
    both = r(tf, tv, ids, slots, joint_conf=tc, occluder=to)
    st0 = RC.reid_init(2, 2 * n, 4, 4)
    want_sig_ids = RC.sig_reference(dict(c, ids=ids.numpy()))
    want = RC.reid_reference(st0, ids.numpy(), slots.numpy(), want_sig_ids[0], want_sig_ids[1], None, prm)
    assert all(np.array_equal(bits_(g.numpy()), bits_(w)) for g, w in zip(both, want))
    # refusals
    with pytest.raises(capi.FvpError, match="NV12 is not built"):
        r.signature(Nv12Frames.__new__(Nv12Frames), tv)
    for bad in (tf[:, :, :, :, :2], tf.float(), tf[:, :3].contiguous()):
        with pytest.raises(capi.FvpError):
            r.signature(bad.contiguous(), tv)
    with pytest.raises(capi.FvpError):
        r.signature(tf, tv, ids=ids.long())
    with pytest.raises(capi.FvpError):
        r.signature(tf, tv, occluder=to.float())
    with pytest.raises(capi.FvpError):
        r.update(ids, slots, sig[:, :, :2].contiguous(), cnt)
    with pytest.raises(capi.FvpError):
        r.update(ids, slots.long(), sig, cnt)
    with pytest.raises(capi.FvpError):
        r.update(ids, slots, sig, cnt, meta={"seq": ["a", "b", "c"][:B] * 2})
    with pytest.raises(capi.FvpError):
        r.reset(5)
    with pytest.raises(capi.FvpError):
        PersonReId((n, J), device="cpu")                                              # the product: no CPU fallback
    for bad in (dict(gallery=0), dict(gallery=65), dict(parts=5), dict(parts=0), dict(samples=0), dict(samples=33),
                dict(min_frames=0), dict(window=1), dict(window=1025), dict(sim_min=float("nan")), dict(margin=float("nan")),
                dict(conf_min=float("nan")), dict(max_age=-1), dict(min_samples=-1), dict(gallery_max_age=-1),
                dict(max_tracks=n - 1), dict(max_tracks=65), dict(limbs=[(0, J)]), dict(limb_part=[0]),
                dict(limb_part=[2] * len(RC.LIMBS17))):
        with pytest.raises(capi.FvpError):
            PersonReId((n, J), **{**kw, **bad})
    with pytest.raises(capi.FvpError, match="limb_part"):
        PersonReId((n, 14), device="cpu", _lib=emu_lib)                                             # a skeleton, but no default parts
    with pytest.raises(capi.FvpError, match="limbs"):
        PersonReId((n, 5), device="cpu", _lib=emu_lib)


@pytest.mark.parametrize("variant", ["return", "twins"])
def test_closed_loop(emu_lib, variant):
    RC.closed_loop_check(emu_lib, "cpu", variant)
