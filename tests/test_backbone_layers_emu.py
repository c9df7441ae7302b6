"""The bf16 Pose-ResNet backbone layer by layer on the CPU emulator: every op of every plan alone against float64 with the
derived interval of tests/backbone_cases.py, every kernel form (register-staged, LDS-DMA with each tile configuration, fused
stem + pooling, fused bottleneck, fused heatmap epilogue) and every configuration cfg.RESNET.* accepts."""
import ctypes as C

import numpy as np
import pytest
import torch

import backbone_cases as B


@pytest.fixture()
def launch_log(emu_lib):
    """A callable: the kernels launched since its last call (mangled symbols, one per launch)."""
    emu_lib.hipemu_launch_log.restype = C.c_char_p
    emu_lib.hipemu_launch_log.argtypes = []
    emu_lib.hipemu_launch_log_reset.argtypes = []

    def read():
        lines = emu_lib.hipemu_launch_log().decode().split()
        emu_lib.hipemu_launch_log_reset()
        return lines
    read()
    return read


def _clear_switches(monkeypatch):
    for k in ("FVP_BB_NO_BIG", "FVP_BB_DMA_BN", "FVP_BB_NO_FUSE_FINAL", "FVP_BB_NO_FUSE_STEM", "FVP_BB_NO_FUSE_BLOCK"):
        monkeypatch.delenv(k, raising=False)


# (configuration, N, H, W): at 32 x 32 layer4 is a 1 x 1 map - a 3 x 3 conv that reads only padding around one pixel, M = 2
PER_OP = [("r50", 2, 32, 32), ("r18", 2, 32, 32), ("r34", 2, 64, 96), ("r50_bias_f256_128_64_j17", 2, 32, 32),
          ("r50_two_deconvs", 2, 32, 32)]


@pytest.mark.parametrize("name,N,H,W", PER_OP, ids=[p[0] for p in PER_OP])
def test_every_op_alone_vs_fp64(emu_lib, monkeypatch, name, N, H, W):
    _clear_switches(monkeypatch)
    m, sd = B.build(emu_lib, "cpu", **B.CONFIGS[name])
    stats = B.per_op_pass(m, sd, N, H, W, "cpu")
    assert len(stats) == len(m._convs)            # every conv once, the heatmap layer in both layouts; the max-pool is exact
    print(name, B.summary(stats))


def test_resnet101_adds_no_op_shape():
    """The 101 / 152 plans repeat layer3 / layer2 blocks: every distinct (kind, cin, cout, k, stride, h, w, residual?) of
    the ResNet-101 plan at 32 x 32 occurs in the ResNet-50 plan that is run above (152 differs from 101 in block counts only)."""
    from faster_voxelpose_amd.models import resnet as RN

    class NoLib:                                          # a plan needs no library
        pass
    shapes = {}
    for name in ("r50", "r101"):
        shapes[name] =B.plan_shapes(RN.PoseResNet(B.make_cfg("cpu", **B.CONFIGS[name]), _lib=NoLib()), 32, 32)
    assert shapes["r101"] <= shapes["r50"], shapes["r101"] - shapes["r50"]
    m152 = RN.PoseResNet(B.make_cfg("cpu", layers=152), _lib=NoLib())
    assert B.plan_shapes(m152, 32, 32) <= shapes["r50"]


@pytest.mark.parametrize("switch,value,N,H,W", [("FVP_BB_NO_BIG", "1", 2, 32, 32), ("FVP_BB_DMA_BN", "128", 2, 32, 32)])
def test_every_op_alone_under_the_kernel_switches(emu_lib, monkeypatch, launch_log, switch, value, N, H, W):
    """FVP_BB_NO_BIG: the register-staged k_bb_conv<64|128> for every layer; FVP_BB_DMA_BN=128: 128-cout tiles only."""
    _clear_switches(monkeypatch)
    monkeypatch.setenv(switch, value)
    m, sd = B.build(emu_lib, "cpu", **B.CONFIGS["r50"])
    launch_log()
    stats = B.per_op_pass(m, sd, N, H, W, "cpu")
    log = launch_log()
    if switch == "FVP_BB_NO_BIG":
        assert not any("k_bb_conv_dma" in line for line in log)
    else:
        assert any("k_bb_conv_dma" in line for line in log) and not any("k_bb_conv_dmaILi256" in line for line in log), set(log)
    print(switch, B.summary(stats))


@pytest.mark.parametrize("stage", ["layer1", "layer2", "layer3", "layer4", "deconv_layers"])
def test_every_tile_configuration_of_every_tunable_op(emu_lib, monkeypatch, stage):
    """Tile configurations 1, 2, 3 (bits 8-9 of the flags, what fvp_bb_tune chooses among) at 3 x 64 x 96 - N = 3 leaves
    partial pixel tiles and partial XCD groups: bit-equal to each other and within the interval.  (One case per stage to
    keep each short.)"""
    _clear_switches(monkeypatch)
    m, sd = B.build(emu_lib, "cpu", **B.CONFIGS["r50"])
    stats = B.per_op_pass(m, sd, 3, 64, 96, "cpu", all_cfgs=True,
                          only=lambda o, op: o.get("key", "").startswith(stage + "."))
    want = sum(1 for i, o in enumerate(m._convs) if o.get("key", "").startswith(stage + ".") and B.tunable(m._plan(64, 96)["ops"][i]))
    assert len(stats) == want >= 3
    print("tile configurations", stage, B.summary(stats))


@pytest.mark.parametrize("hw", [(32, 32), (64, 160)])
def test_stem_alone_vs_fp64(emu_lib, monkeypatch, hw):
    """Alone the stem takes the pixel-pair k_bb_conv form: against F.conv2d(x[:, :3], w, stride 2, padding 3) on an input
    with negative values (a skipped ReLU would otherwise go unseen)."""
    _clear_switches(monkeypatch)
    m, sd = B.build(emu_lib, "cpu", **B.CONFIGS["r50"])
    stats = B.per_op_pass(m, sd, 2, hw[0], hw[1], "cpu", only=lambda o, op: bool(o.get("stem")))
    assert len(stats) == 1


@pytest.mark.parametrize("N,H,W", [(2, 32, 32), (2, 64, 160), (1, 64, 64), (3, 128, 128), (2, 32, 256)])
def test_fused_stem_and_bottlenecks_equal_the_separate_launches(emu_lib, monkeypatch, launch_log, N, H, W):
    """k_bb_stem_pool and k_bb_bottleneck64 against the launches they replace, bit-equal.  The stage-1 map at 64 x 64 is 16
    columns (a 15-column pooling tile and a one-column one), at 128 x 128 32 columns (a 30-column bottleneck tile and a
    2-column one).  The launch log shows which form ran."""
    _clear_switches(monkeypatch)
    m, _ = B.build(emu_lib, "cpu", seed=5, **B.CONFIGS["r50"])
    B.stage1_forms(m, N, H, W, "cpu", monkeypatch.setenv, launch_log)


@pytest.mark.parametrize("J", [1, 15, 17, 20, 32, 33])
def test_heatmap_layer_fused_and_separate(emu_lib, monkeypatch, launch_log, J):
    _clear_switches(monkeypatch)
    m, sd = B.build(emu_lib, "cpu", joints=J)
    stats = B.heat_matrix(m, sd, 2, 32, 32, "cpu", monkeypatch.setenv, monkeypatch.delenv, launch_log)
    print("J", J, B.summary(stats))


def test_heatmap_layer_behind_a_64_filter_deconv_is_not_fused(emu_lib, monkeypatch, launch_log):
    _clear_switches(monkeypatch)
    m, sd = B.build(emu_lib, "cpu", **B.CONFIGS["r50_bias_f256_128_64_j17"])
    B.heat_matrix(m, sd, 2, 32, 32, "cpu", monkeypatch.setenv, monkeypatch.delenv, launch_log)


@pytest.mark.parametrize("filters", [(256, 64, 32), (16,), ()])
def test_narrow_deconv_heads_vs_fp64(emu_lib, monkeypatch, filters):
    """Deconv heads narrower than a 64-channel tile (32 / 16 stored channels: masked channel groups, K below one k chunk in the
    heatmap layer) and no deconv at all (the heatmap layer reads layer4): every op behind layer4 alone against fp64."""
    _clear_switches(monkeypatch)
    m, sd = B.build(emu_lib, "cpu", deconv_filters=filters)
    stats = B.per_op_pass(m, sd, 2, 32, 32, "cpu", only=lambda o, op: not o.get("key", "layer").startswith("layer")
                          and not o.get("stem"))
    assert len(stats) == len(filters) + 2


@pytest.mark.parametrize("filters", [(96,), (256, 256, 100), (256, 4)])
def test_unsupported_deconv_filters_are_refused(filters):
    """A channel count the conv kernels cannot decode (not a power of two >= 8) is refused when the model is built, not
    when it first runs; so is a filter list that does not match NUM_DECONV_LAYERS."""
    from faster_voxelpose_amd import _capi as capi
    from faster_voxelpose_amd.models import resnet as RN
    with pytest.raises(capi.FvpError):
        RN.PoseResNet(B.make_cfg("cpu", deconv_filters=filters), _lib=object())
    cfg = B.make_cfg("cpu")
    cfg.RESNET.NUM_DECONV_FILTERS = [256, 256]
    with pytest.raises(capi.FvpError):
        RN.PoseResNet(cfg, _lib=object())


@pytest.mark.parametrize("name", ["r18", "r50_bias_f256_128_64_j17"])
def test_whole_network_non_default_configurations(emu_lib, monkeypatch, name):
    _clear_switches(monkeypatch)
    cfg = B.CONFIGS[name]
    m, sd = B.build(emu_lib, "cpu", seed=3, **cfg)
    x = torch.from_numpy(np.random.default_rng(0).random((1, 3, 32, 32), dtype=np.float32))
    B.whole_network(m, sd, x, cfg.get("layers", 50), len(cfg.get("deconv_filters", (1, 2, 3))), one_pass=True)
