"""The argument layer of the stream-side wrappers (faster-voxelpose_amd/_args.py): the tensor check, the loose device
comparison, the sequence rows and the camera tables.  Host code only: no library, no GPU."""
import numpy as np
import pytest
import torch

from faster_voxelpose_amd import _args as A
from faster_voxelpose_amd import _capi as capi

CPU = torch.device("cpu")
GOOD = torch.zeros(2, 3, 5, 4)
PATTERN = ("B", 3, None, 4)                               # printed as [B,3,*,4]


@pytest.mark.parametrize("name,bad,kw", [
    ("wrong dtype", GOOD.double(), {}),
    ("wrong rank", GOOD[0], {}),
    ("wrong fixed extent", torch.zeros(2, 4, 5, 4), {}),
    ("not contiguous", torch.zeros(2, 3, 4, 5).transpose(2, 3), {}),
    ("wrong device", GOOD.to("meta"), dict(device=CPU)),
    ("no tensor", [[1.0]], {}),
    ("None, not optional", None, {}),
])
def test_tensor_arg_refuses(name, bad, kw):
    with pytest.raises(capi.FvpError) as e:
        A.tensor_arg("poses", bad, torch.float32, PATTERN, hint="what the forward returns", **kw)
    msg = str(e.value)
    assert "poses" in msg and "contiguous" in msg and "torch.float32" in msg and "[B,3,*,4]" in msg, msg
    assert "(what the forward returns)" in msg and ("[B,3,*,4] on cpu" in msg) == ("device" in kw)
    if torch.is_tensor(bad):
        assert str(tuple(bad.shape)) in msg and str(bad.dtype) in msg, msg      # what arrived
    else:
        assert type(bad).__name__ in msg, msg


def test_tensor_arg_accepts():
    assert A.tensor_arg("poses", GOOD, torch.float32, PATTERN) is GOOD
    assert A.tensor_arg("poses", GOOD, torch.float32, PATTERN, device=CPU, hint="x", optional=True) is GOOD
    assert A.tensor_arg("poses", None, torch.float32, PATTERN, device=CPU, optional=True) is None
    empty = torch.zeros(0, 3, 7, 4)
    assert A.tensor_arg("poses", empty, torch.float32, PATTERN) is empty
    ids = torch.zeros(2, 3, dtype=torch.int32)
    assert A.tensor_arg("ids", ids, torch.int32, (2, 3), CPU) is ids


def test_device_matches():
    cuda, cuda0, cuda1 = torch.device("cuda"), torch.device("cuda:0"), torch.device("cuda:1")
    assert A.device_matches(cuda0, cuda) and A.device_matches(cuda1, cuda)      # no index: any cuda:N
    assert A.device_matches(cuda0, cuda0) and not A.device_matches(cuda0, cuda1)
    assert not A.device_matches(CPU, cuda) and not A.device_matches(cuda0, CPU) and A.device_matches(CPU, CPU)


def test_require_gpu_and_f3():
    A.require_gpu("the tracker", CPU, True)                                     # an injected library runs anywhere
    A.require_gpu("the tracker", torch.device("cuda:0"), False)
    with pytest.raises(capi.FvpError, match="the tracker.*no CPU fallback"):
        A.require_gpu("the tracker", CPU, False)
    assert list(A.f3((1, 2.5, 3))) == [1.0, 2.5, 3.0] and A.ptr(None) is None and A.stream_ptr(CPU) is None
    assert A.ptr(GOOD).value == GOOD.data_ptr() and A.load_lib("lib") == ("lib", True)


def test_sequence_rows():
    rows = A.SequenceRows()
    fs = rows.rows(["b", "a", "b"], CPU)
    assert rows.ids == {"b": 0, "a": 1} and list(rows.ids) == ["b", "a"]        # numbered by first appearance
    assert fs.dtype == torch.int32 and fs.tolist() == [0, 1, 0]
    assert rows.rows(("b", "a", "b"), CPU) is fs                                # one upload per distinct list
    assert rows.rows(["a", "c"], CPU).tolist() == [1, 2]
    # the cache is bounded at 256 lists: the 257th drops the oldest, which is then built again
    rows = A.SequenceRows()
    first = rows.rows(["s0"], CPU)
    for i in range(1, 256):
        rows.rows([f"s{i}"], CPU)
    assert len(rows._cache) == 256 and rows.rows(["s0"], CPU) is first
    rows.rows(["s256"], CPU)
    assert len(rows._cache) == 256 and ("s0",) not in rows._cache
    again = rows.rows(["s0"], CPU)
    assert again is not first and again.tolist() == [0] and len(rows._cache) == 256 and len(rows.ids) == 257
    # limit: the state rows an object was built for
    rows = A.SequenceRows(limit=2)
    assert rows.rows(["x", "y", "x"], CPU).tolist() == [0, 1, 0]
    with pytest.raises(capi.FvpError, match="one more than the nseq = 2"):
        rows.rows(["x", "z"], CPU)
    assert rows.ids == {"x": 0, "y": 1}


def _camera(seed):
    r = np.random.default_rng(seed)
    return dict(R=r.normal(size=(3, 3)), T=r.normal(size=(3, 1)), fx=float(r.uniform(900, 1100)), fy=float(r.uniform(900, 1100)),
                cx=float(r.uniform(400, 600)), cy=float(r.uniform(200, 400)), k=r.normal(size=(3, 1)), p=r.normal(size=(2, 1)))


def test_camera_tables():
    from faster_voxelpose_amd.engine import HotPath
    cameras = {"hall": [_camera(1), _camera(2)], "yard": [_camera(3), _camera(4)]}
    tab = A.CameraTables()
    cams, fs = tab.tables(cameras, ["hall", "hall"], 2, CPU)
    assert cams.shape == (1, 2, capi.FVP_CAM_FLOATS) and cams.dtype == torch.float32 and fs.tolist() == [0, 0]
    assert np.array_equal(cams[0, 1].numpy().view(np.int32), HotPath._cam_row(cameras["hall"][1]).view(np.int32))
    assert tab.tables(cameras, ["hall", "hall"], 2, CPU)[1] is fs and tab.cams is cams      # nothing new: nothing uploaded
    row0 = cams[0].clone()
    cams2, fs2 = tab.tables(cameras, ["yard", "hall"], 2, CPU)
    assert cams2.shape == (2, 2, capi.FVP_CAM_FLOATS) and fs2.tolist() == [1, 0] and tab.ids == {"hall": 0, "yard": 1}
    assert torch.equal(cams2[0].view(torch.int32), row0.view(torch.int32))      # a second sequence appends: row 0 keeps its bits
    assert ("hall", "hall") not in tab._cache and list(tab._cache) == [("yard", "hall")]    # ... and clears the list cache
    with pytest.raises(capi.FvpError):
        tab.tables(cameras, ["attic"], 2, CPU)
    with pytest.raises(capi.FvpError):
        A.CameraTables().tables(cameras, ["hall"], 3, CPU)                      # the dict holds 2 cameras, not 3


def test_resolve_cameras():
    cameras = {"hall": [_camera(1), _camera(2)]}
    tab = A.CameraTables()
    cams, fs, V = A.resolve_cameras(tab, cameras, {"seq": ["hall"] * 3}, 3, None, CPU)
    assert V == 2 and cams is tab.cams and fs.tolist() == [0, 0, 0]
    assert A.resolve_cameras(tab, cameras, ["hall"] * 3, 3, 2, CPU)[1] is fs
    got = A.resolve_cameras(tab, cams, fs, 3, None, CPU)
    assert got[0] is cams and got[1] is fs and got[2] == 2
    for bad in ((cameras, ["hall"] * 2, 3, None), (cams, fs, 3, 5), (cams, fs[:2], 3, None), (cams, fs.long(), 3, None),
                (cams[:0], fs, 3, None), (cams.double(), fs, 3, None), (cams, ["hall"] * 3, 3, None)):
        with pytest.raises(capi.FvpError):
            A.resolve_cameras(tab, bad[0], bad[1], bad[2], bad[3], CPU)
